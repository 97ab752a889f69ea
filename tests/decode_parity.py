"""References, emulations, case tables and input builders of the decode-step kernel tests (a plain module, no pytest in
it): zk_dec_cross / zk_dec_self (zero_amd/csrc/zk_decfuse.hip), the row-local LayerNorm forms of zk_lndec_dev.h,
zk_gemm_parts, zk_dec_embed, zk_cache_rows.  tests/test_decode_parity_checker.py (CPU) measures the tolerances on these
tables and shows that planted defects fail; tests/test_gpu_decode_elementwise.py runs the kernels on the same tensors.

``dec_attn_math``  one decode attention sub-layer at Lq = 1 from the bf16 input VALUES.  emulate = False: float64, nothing
                   rounded (the reference).  emulate = True: float32 with bf16 rounding at the sites the header of
                   zk_decfuse.hip names -- q, k, v, P, ctx -- used only to measure the tolerances.  A fully masked
                   sentence attends uniformly (fp32 semantics: -mask_inf absorbs every score).
``ln_math``        y (from ybuf / partial sums / the gate) -> LayerNorm(x + y), the sum unrounded -> the running sum and
                   [out | average].  y of the partial-sum forms is exactly reproducible (fp32 sums in the order p = 0, 1,
                   .., then the bias, one rounding to bf16: ``parts_y``) and is taken as such by reference and emulation.
``row_ratio``      ||got_row - ref_row|| / max(||ref_row||, rms row norm of the tensor) on [rows, H] rows.
Every ``defect`` argument plants ONE defect of the kind the kernels could have; None = correct.
"""
import functools

import torch

from tests import parity as P

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
D = 64                                   # head width of the fused kernels


def _bf(x):
    return x.to(BF).to(x.dtype)


def row_ratio(got, ref64):
    """got / ref [..., H] -> worst row ratio (rows = the leading dimensions flattened)."""
    Hd = ref64.shape[-1]
    return float(P.attn_row_ratio(got.reshape(-1, Hd), ref64.reshape(-1, Hd), Hd).max())


def parts_ratio(got, ref64):
    """out_parts [nh, rows, H]: each head's part is a tensor of its own (its own rms row norm)."""
    return max(row_ratio(got[h], ref64[h]) for h in range(ref64.shape[0]))


def rel_index(pos, n, max_rel, defect=None):
    """modules/rpr.py at Lq = 1: key j of a query at position pos reads table row clip(pos - j) + max_rel."""
    dlt = pos - torch.arange(n)
    if defect == "sign_flip":
        dlt = -dlt
    hi = max_rel - 1 if defect == "clip_off1" else max_rel
    return dlt.clamp(-max_rel, hi) + max_rel


def dec_attn_math(x, wqt, bq, wot, keys, vals, B, R, nh, scale, t=None, kmask=None, mask_inf=0.0, rk=None, rv=None,
                  max_rel=0, pos=0, emulate=False, defect=None, defect_row=0, defect_head=0):
    """x [B*R, H]; wqt [H | 3H, H] and wot [H, H] TRANSPOSED as the kernels take them (row = output channel); bq [H | 3H].
    Cross (t None): keys / vals [B, Lk, H], kmask [B, Lk] or None, the query at position pos.
    Self (t = the step): keys / vals = the caches [B*R, Tmax, H]; slots < t are attended, slot t is this step's.
    -> dict parts [nh, rows, H], sum [rows, H], smax (largest |score| before the mask) and, self, knew / vnew [rows, H]."""
    dt = F32 if emulate else F64
    rnd = _bf if emulate else (lambda v: v)
    c = lambda v: None if v is None else v.detach().to("cpu").to(dt)
    x, wqt, bq, wot, keys, vals, kmask, rk, rv = (c(v) for v in (x, wqt, bq, wot, keys, vals, kmask, rk, rv))
    rows, H = B * R, nh * D
    proj = x @ wqt.t() + bq
    q = rnd(proj[:, :H])
    res = {}
    if t is not None:
        knew, vnew = rnd(proj[:, H:2 * H]), rnd(proj[:, 2 * H:])
        res["knew"], res["vnew"] = knew.double(), vnew.double()
        n = t + 1
        if defect == "skip_t":
            n = t
        elif defect == "past_t":
            n = t + 2
        Kr, Vr = keys[:, :n].clone(), vals[:, :n].clone()
        if defect not in ("stale_slot", "skip_t"):
            Kr[:, t], Vr[:, t] = knew, vnew
        pos, mrow = t, None
    else:
        sent = lambda tag: torch.tensor([(r // R) if not (defect == tag and r == defect_row)
                                         else ((r // R + 1) if r // R + 1 < B else r // R - 1) for r in range(rows)])
        Kr, Vr = keys[sent("neighbour_k")], vals[sent("neighbour_v")]
        mrow = None if kmask is None else kmask[sent("neighbour_mask")]
        n = Kr.shape[1]
    qh = q.view(rows, nh, D)
    sc = torch.einsum("rhd,rjhd->rhj", qh, Kr.reshape(rows, n, nh, D))
    if rk is not None:
        idx = rel_index(pos, n, max_rel, defect)
        sc = sc + torch.einsum("rhd,jd->rhj", qh, rk[idx])
    sc = sc * scale
    res["smax"] = float(sc.abs().max())
    if mrow is not None:
        sc = sc + ((1 - mrow) * -mask_inf)[:, None, :]
        sc = torch.where((mrow.sum(1) == 0)[:, None, None], torch.zeros_like(sc), sc)      # fully masked: uniform
    p = rnd(torch.softmax(sc, -1))
    Vh = Vr.reshape(rows, n, nh, D)
    if rv is not None and defect != "no_rpr_v":
        Vh = Vh + rv[idx][None, :, None, :]
    ctx = rnd(torch.einsum("rhj,rjhd->rhd", p, Vh))
    parts = torch.einsum("rhd,hdo->hro", ctx, wot.t().reshape(nh, D, H))
    if defect == "zero_head":
        parts[defect_head] = 0
    res["parts"], res["sum"] = parts.double(), parts.sum(0).double()
    return res


# ---------------------------------------------------------------------------------------------- LayerNorm forms
def parts_y(parts, bias, defect=None):
    """bf16(sum_p parts[p] + bias) exactly as the kernel forms it: fp32, p = 0, 1, .., then the bias, one rounding."""
    parts = parts.detach().to("cpu").float()
    n = parts.shape[0] - (1 if defect == "drop_last_part" else 0)
    s = torch.zeros_like(parts[0])
    for p_ in range(n):
        s = s + parts[p_]
    if bias is not None and defect != "no_bias":
        s = s + bias.detach().to("cpu").float()
    return s.to(BF)


def ln_math(x, gamma, beta, eps, ybuf=None, parts=None, bias=None, z=None, cat_in=None, cache=None, inv_count=1.0,
            emulate=False, defect=None):
    """-> dict out [rows, H] (and cache, cat [rows, 2H] with a running sum).  The form is chosen as the kernel chooses it:
    cat_in -> the gate (z given, or z = bf16(sum of parts + bias)); parts -> y = bf16(sum of parts + bias); else ybuf."""
    dt = F32 if emulate else F64
    rnd = _bf if emulate else (lambda v: v)
    c = lambda v: None if v is None else v.detach().to("cpu").to(dt)
    H = x.shape[1]
    if cat_in is not None:
        zz = c(z) if z is not None else c(parts_y(parts, bias, defect))
        ci = c(cat_in)
        y = rnd(torch.sigmoid(zz[:, :H]) * ci[:, :H] + torch.sigmoid(zz[:, H:]) * ci[:, H:])
    elif parts is not None:
        y = c(parts_y(parts, bias, defect))
    else:
        y = c(ybuf)
    v = c(x) + y
    mean = v.mean(1, keepdim=True)
    var = ((v - mean) ** 2).mean(1, keepdim=True)
    out = rnd(c(gamma) * (v - mean) * torch.rsqrt(var + eps) + c(beta))
    res = {"out": out.double(), "y": y.double()}
    if cache is not None:
        new = c(cache) + out * (2 if defect == "cache_twice" else 1)
        res["cache"] = new.double()
        res["cat"] = torch.cat([out, rnd(new * inv_count)], 1).double()
    return res


def running_sum_expected(old, xout):
    """fp32: old + float(xout), the kernel's own output row added ONCE."""
    return old.detach().cpu().float() + xout.detach().cpu().float()


def assert_running_sum(old, xout, new, what):
    want, new = running_sum_expected(old, xout), new.detach().cpu().float()
    bad = int((want.view(torch.int32) != new.view(torch.int32)).sum())
    assert bad == 0, "%s: %d elements of the running sum are not old + xout in fp32 (max diff %.3e)" % (
        what, bad, float((want - new).abs().max()))


def cat_bound(new_cache, inv_count):
    """The average half of cat_out = bf16(cache * inv_count): one bf16 rounding (half an ulp of 8 bits: 2^-8) of an fp32
    product of the kernel's own running sum with an inv_count that may have been formed on the device (2^-23 each; 2^-21
    is four times their sum)."""
    ref = new_cache.detach().cpu().double() * inv_count
    return ref, (2.0 ** -8 + 2.0 ** -21) * ref.abs()


def ln32(v, gamma, beta, eps, order):
    """LayerNorm of fp32 rows v with the two sums taken in a given order, output NOT rounded -> float64 tensor.
    forward / reversed: one running sum; pairwise: a binary tree; strided: the kernel's (lane l owns the 8-column chunks
    l, l + 64, ..: a running sum per lane, then a butterfly over the 64 lanes)."""
    v = v.float()
    H = v.shape[1]

    def tree(cols):                     # cols: list of [rows] tensors
        while len(cols) > 1:
            cols = [cols[i] + cols[i + 1] if i + 1 < len(cols) else cols[i] for i in range(0, len(cols), 2)]
        return cols[0]

    def total(m):
        cols = list(m.unbind(1))
        if order == "pairwise":
            return tree(cols)
        if order == "strided":
            lanes = []
            for l in range(64):
                s = torch.zeros_like(cols[0])
                for i in range((H + 511) // 512):
                    for j in range(8):
                        cidx = (i * 64 + l) * 8 + j
                        if cidx < H:
                            s = s + cols[cidx]
                lanes.append(s)
            return tree(lanes)
        if order == "reversed":
            cols = cols[::-1]
        s = torch.zeros_like(cols[0])
        for col in cols:
            s = s + col
        return s

    inv = torch.tensor(1.0 / H, dtype=F32)
    mean = (total(v) * inv)[:, None]
    dlt = v - mean
    var = (total(dlt * dlt) * inv)[:, None]
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))
    return (gamma.float() * dlt * rstd + beta.float()).double()


LN_ORDERS = ("forward", "reversed", "pairwise", "strided")


def ln_elem(x, y, gamma, beta, eps, c_ln):
    """Element-wise reference and bound of LayerNorm(x + y) stored as bf16, y exact:
    bound = 2^-8 |ref| + c_ln 2^-23 (|gamma| |xhat| + |beta|)."""
    v = x.detach().cpu().double() + y.detach().cpu().double()
    mean = v.mean(1, keepdim=True)
    xhat = (v - mean) * torch.rsqrt(((v - mean) ** 2).mean(1, keepdim=True) + eps)
    g, b = gamma.detach().cpu().double(), beta.detach().cpu().double()
    ref = g * xhat + b
    return ref, 2.0 ** -8 * ref.abs() + c_ln * 2.0 ** -23 * (g.abs() * xhat.abs() + b.abs())


def ln_unit(x, y, gamma, beta, eps):
    """The unit of c_ln per element: 2^-23 (|gamma| |xhat| + |beta|)."""
    ref, b1 = ln_elem(x, y, gamma, beta, eps, 1.0)
    return ref, b1 - 2.0 ** -8 * ref.abs()


# ---------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def _randn(g, *shape, scale=1.0, dtype=BF):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


@functools.lru_cache(maxsize=None)
def attn_weights(H, self_attn):
    """Projection weights shared by every case of one H (transposed: row = output channel) and the biases.  q and k
    come out with std 0.7, so that scores (std ~0.5, ~0.6 with relative positions) stay below 4 in magnitude."""
    g = _gen(7000 + H + (1 if self_attn else 0))
    n = 3 if self_attn else 1
    wqt = _randn(g, n * H, H, scale=0.7 * H ** -0.5)
    if self_attn:
        wqt[2 * H:] = (wqt[2 * H:].float() / 0.7).to(BF)          # values of std 1
    return {"wqt": wqt, "bq": _randn(g, n * H, scale=0.1, dtype=F32), "wot": _randn(g, H, H, scale=H ** -0.5)}


MASK_INF = 1e9
SCALE = D ** -0.5
EPS = 1e-6

# rel: None or (max_rel, pos, "val" | "dev"); "dev": the position comes from pos_dev, the by-value argument is wrong
REL_LEVELS = [None, (4, 0, "val"), (4, 3, "dev"), (4, 9, "val"), (4, 9, "dev"), (0, 2, "val"), (31, 40, "dev")]
CROSS_FACTORS = {
    "H": [128, 512, 1024, 2048],
    "BR": [(3, 4), (5, 1), (2, 8), (3, 5)],
    "group": [0, 1, 3, 16],
    "Lk": [1, 3, 31, 32, 33, 65, 130],
    "mask": [None, "ragged", "key0", "ldmask"],
    "layout": ["halves", "separate"],
    "rel": REL_LEVELS,
}


@functools.lru_cache(maxsize=None)
def cross_cases():
    """The pairwise covering of CROSS_FACTORS with exactly ONE H = 2048 row (the pairs of H = 2048 with the other factors
    are not all covered: one case of that size per entry point), then the cases the covering does not force:
    group 16 on 12 and on 20 rows (NR < gr in the first / the last group), group 3 on R = 4 (a sentence split across
    groups) with different masks per sentence, Lk = 130 on 16 rows (four passes of the 512-pair loop) and on 4 rows
    (two), and a fully masked sentence."""
    small = dict(CROSS_FACTORS, H=[128, 512, 1024])
    rows = P.pairwise(small)
    rows.append(dict(H=2048, BR=(3, 5), group=16, Lk=33, mask="ragged", layout="halves", rel=(4, 9, "dev")))
    extra = [
        dict(H=128, BR=(3, 4), group=16, Lk=33, mask="ragged", layout="halves", rel=None),
        dict(H=128, BR=(5, 4), group=16, Lk=31, mask="ragged", layout="separate", rel=(4, 3, "dev")),
        dict(H=128, BR=(3, 4), group=3, Lk=9, mask="ragged", layout="halves", rel=(4, 3, "val")),
        dict(H=512, BR=(2, 8), group=16, Lk=130, mask="ragged", layout="halves", rel=(31, 40, "dev")),
        dict(H=128, BR=(3, 4), group=0, Lk=130, mask="key0", layout="separate", rel=(4, 9, "val")),
        dict(H=128, BR=(3, 4), group=16, Lk=33, mask="allmasked", layout="halves", rel=None),
    ]
    return tuple(rows + extra)


def make_mask(kind, B, Lk):
    """[B, Lk] fp32 (1 = valid) or None.  ragged: every sentence loses a different number of trailing keys (neighbouring
    sentences differ); key0: sentence 1 (0 when B = 1) keeps key 0 only; allmasked: that sentence keeps nothing."""
    if kind is None:
        return None
    km = torch.ones(B, Lk)
    b1 = 1 if B > 1 else 0
    if kind in ("ragged", "ldmask"):
        for b in range(B):
            km[b, Lk - (2 * b + 1) % Lk:] = 0
        km[:, 0] = 1
    elif kind == "key0":
        km[b1, 1:] = 0
    elif kind == "allmasked":
        for b in range(B):
            km[b, Lk - (2 * b + 1) % Lk:] = 0
        km[:, 0] = 1
        km[b1] = 0
    return km


def _case_seed(case):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(repr(sorted(case.items())))) % 100003


def cross_inputs(case, rel_scale=0.5):
    """CPU operands of one cross case (dict of CROSS_FACTORS levels)."""
    H, (B, R), Lk = case["H"], case["BR"], case["Lk"]
    g = _gen(20000 + _case_seed(case))
    w = attn_weights(H, False)
    x = dict(w, x=_randn(g, B * R, H), keys=_randn(g, B, Lk, H, scale=0.7), vals=_randn(g, B, Lk, H),
             kmask=make_mask(case["mask"], B, Lk), rk=None, rv=None, max_rel=0, pos=0)
    if case["rel"] is not None:
        x["max_rel"], x["pos"] = case["rel"][0], case["rel"][1]
        x["rk"] = _randn(g, 2 * x["max_rel"] + 1, D, scale=rel_scale)
        x["rv"] = _randn(g, 2 * x["max_rel"] + 1, D, scale=rel_scale)
    return x


def cross_math(case, x, emulate=False, defect=None, **kw):
    B, R = case["BR"]
    return dec_attn_math(x["x"], x["wqt"], x["bq"], x["wot"], x["keys"], x["vals"], B, R, case["H"] // D, SCALE,
                         kmask=x["kmask"], mask_inf=MASK_INF, rk=x["rk"], rv=x["rv"], max_rel=x["max_rel"], pos=x["pos"],
                         emulate=emulate, defect=defect, **kw)


# self: H, (B, R), Tmax, time, how the time is given, group, rel (max_rel or None)
SELF_CASES = tuple(
    [dict(H=128, BR=(3, 4), Tmax=40, time=t, tdev=(i % 2 == 1), group=0, rel=None)
     for i, t in enumerate((0, 1, 31, 32, 33, 39))] +
    [dict(H=512, BR=(2, 3), Tmax=132, time=t, tdev=(i % 2 == 0), group=0, rel=None)
     for i, t in enumerate((0, 1, 31, 32, 33, 131))] +
    [dict(H=128, BR=(5, 4), Tmax=40, time=33, tdev=True, group=16, rel=None),       # 16 x 34 = 544 pairs; 20 rows
     dict(H=128, BR=(3, 4), Tmax=40, time=9, tdev=False, group=0, rel=4),
     dict(H=512, BR=(2, 3), Tmax=40, time=9, tdev=True, group=3, rel=4),
     dict(H=1024, BR=(2, 3), Tmax=40, time=33, tdev=False, group=16, rel=None),
     dict(H=2048, BR=(3, 2), Tmax=40, time=32, tdev=True, group=0, rel=4)])


def self_inputs(case, rel_scale=0.5, stale=False):
    """CPU operands of one self case.  The caches hold data in the slots < time; the slots >= time hold NaN (the GPU
    test: nothing there may be read into a result) or, stale = True, other finite data (the CPU defect cases)."""
    H, (B, R), Tmax, t = case["H"], case["BR"], case["Tmax"], case["time"]
    g = _gen(40000 + _case_seed(case))
    w = attn_weights(H, True)
    x = dict(w, x=_randn(g, B * R, H), keys=_randn(g, B * R, Tmax, H, scale=0.7), vals=_randn(g, B * R, Tmax, H),
             rk=None, rv=None, max_rel=0)
    if not stale:
        x["keys"][:, t:] = float("nan")
        x["vals"][:, t:] = float("nan")
    if case["rel"] is not None:
        x["max_rel"] = case["rel"]
        x["rk"] = _randn(g, 2 * case["rel"] + 1, D, scale=rel_scale)
        x["rv"] = _randn(g, 2 * case["rel"] + 1, D, scale=rel_scale)
    return x


def self_math(case, x, emulate=False, defect=None, **kw):
    B, R = case["BR"]
    return dec_attn_math(x["x"], x["wqt"], x["bq"], x["wot"], x["keys"], x["vals"], B, R, case["H"] // D, SCALE,
                         t=case["time"], rk=x["rk"], rv=x["rv"], max_rel=x["max_rel"], emulate=emulate, defect=defect, **kw)


# LayerNorm forms: name -> (gate, nparts or None (ybuf / z given))
LN_FORMS = {"ybuf": (False, None), "parts1": (False, 1), "parts4": (False, 4), "parts9": (False, 9),
            "gate_z": (True, None), "gate_parts5": (True, 5)}
LN_FACTORS = {"H": [8, 72, 512, 520, 1024, 1032, 2048], "rows": [1, 3, 5, 130], "form": list(LN_FORMS),
              "cache": [False, True], "tdev": [False, True]}


@functools.lru_cache(maxsize=None)
def ln_cases():
    return tuple(P.pairwise(LN_FACTORS))


def ln_inputs(rows, H, form, cache, seed=0, nparts=None):
    """CPU operands of one row-local LayerNorm: x, gamma, beta and the operands of the form (the partial sums carry
    partial products of mixed signs ~3 each, so that a dropped one is far outside any rounding), the running sum of
    `time` = 6 earlier rows.  nparts overrides the count of the form (the prologue's nparts = nh)."""
    gate, npf = LN_FORMS[form]
    npf = nparts if (nparts is not None and npf is not None) else npf
    g = _gen(60000 + 7 * rows + 13 * H + 101 * list(LN_FORMS).index(form) + seed)
    a = {"x": _randn(g, rows, H), "gamma": 1 + 0.1 * torch.randn(H, generator=g), "beta": 0.1 * torch.randn(H, generator=g),
         "ybuf": None, "parts": None, "bias": None, "z": None, "cat_in": None, "cache": None, "time": 6,
         "inv_count": 1.0 / 7}
    W = 2 * H if gate else H
    if npf is not None:
        a["parts"] = _randn(g, npf, rows, W, scale=3.0, dtype=F32)
        a["bias"] = _randn(g, W, scale=1.0, dtype=F32)
    if gate:
        a["cat_in"] = _randn(g, rows, 2 * H)
        if npf is None:
            a["z"] = _randn(g, rows, 2 * H, scale=2.0)
    elif npf is None:
        a["ybuf"] = _randn(g, rows, H)
    if cache:
        a["cache"] = _randn(g, rows, H, scale=2.5, dtype=F32)
    return a


def ln_run(a, emulate=False, defect=None):
    return ln_math(a["x"], a["gamma"], a["beta"], EPS, ybuf=a["ybuf"], parts=a["parts"], bias=a["bias"], z=a["z"],
                   cat_in=a["cat_in"], cache=a["cache"], inv_count=a["inv_count"], emulate=emulate, defect=defect)


def ln_exact_y(a):
    """y where it is exactly reproducible (ybuf and the partial-sum form), else None (the gate: an exp)."""
    if a["cat_in"] is not None:
        return None
    return a["ybuf"] if a["parts"] is None else parts_y(a["parts"], a["bias"])


# prologue: (form, cache, tdev) per entry point on a small attention case
PROLOGUE_CASES = tuple((f, c, (i + c) % 2 == 1) for i, f in enumerate(LN_FORMS) for c in (False, True))
PRO_CROSS = dict(H=128, BR=(3, 4), group=3, Lk=9, mask="ragged", layout="halves", rel=(4, 3, "val"))
PRO_SELF = dict(H=128, BR=(3, 4), Tmax=40, time=6, tdev=True, group=3, rel=None)

GEMM_PARTS_CASES = [(1, 128, 192, 4), (20, 128, 64, 4), (128, 512, 2048, 4), (130, 256, 512, 3)]


def gemm_parts_ranges(K, splits):
    """The K ranges of zk_gemm_parts: ceil(K / splits) rounded up to a multiple of 64."""
    kchunk = ((K + splits - 1) // splits + 63) // 64 * 64
    return [(k0, min(K, k0 + kchunk)) for k0 in range(0, K, kchunk)]


# ---------------------------------------------------------------------------------------------- planted defects
# defect -> (kind, case): the case built for it.  Cross cases use group 3 on R = 4: rows 3 .. 5 are one group over two
# sentences; row 3 (sentence 0, the group's other rows belong to sentence 1) gets the neighbour's operands.
_DC = dict(H=128, BR=(3, 4), group=3, Lk=9, mask="ragged", layout="halves", rel=None)
_DR = dict(H=128, BR=(3, 4), group=3, Lk=33, mask="ragged", layout="halves", rel=(4, 9, "val"))
_DS = dict(H=128, BR=(3, 4), Tmax=40, time=33, tdev=False, group=16, rel=None)
ATTN_DEFECTS = {
    "neighbour_k": ("cross", _DC), "neighbour_v": ("cross", _DC), "neighbour_mask": ("cross", _DC),
    "stale_slot": ("self", _DS), "skip_t": ("self", _DS), "past_t": ("self", _DS),
    "clip_off1": ("cross", _DR), "sign_flip": ("cross", _DR), "no_rpr_v": ("cross", _DR), "zero_head": ("cross", _DC),
}
LN_DEFECTS = {"drop_last_part": ("parts9", False), "no_bias": ("parts4", False), "cache_twice": ("ybuf", True)}


def attn_defect_ratios(name):
    """-> (worst head-part ratio, head-sum ratio) of the emulation with the defect planted, against the reference."""
    kind, case = ATTN_DEFECTS[name]
    if kind == "cross":
        x = cross_inputs(case)
        ref = cross_math(case, x)
        bad = cross_math(case, x, emulate=True, defect=name, defect_row=3, defect_head=1)
    else:
        x = self_inputs(case, stale=True)
        ref = self_math(case, x)
        bad = self_math(case, x, emulate=True, defect=name)
    return parts_ratio(bad["parts"], ref["parts"]), row_ratio(bad["sum"], ref["sum"])
