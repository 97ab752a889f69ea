"""The kernels of the decode hot path called directly and compared with a float64 reference (tests/decode_parity.py):
zk_dec_cross / zk_dec_self with and without the LayerNorm prologue, zk_ln_decode in every form, zk_gemm_parts,
zk_dec_embed, zk_cache_rows.  Every operand and output is a parity.guarded buffer: outputs are prefilled with NaN and
nothing outside their windows may change, inputs (ybuf included: the kernels only read it) must be bit-identical after
the call.

Row check of the attention outputs and of the LayerNorm output: ||got_row - ref_row|| <= c max(||ref_row||, rms row norm
of the tensor), each out_parts[h] a tensor of its own.  The constants are not chosen: each is twice the worst ratio of
the CPU emulation (float32, bf16 rounding of q, k, v, P, ctx -- and of y and the output for the LayerNorm) over every
case of the tables; tests/test_decode_parity_checker.py re-measures them on every CPU run, requires the constants below
to lie within [1x, 2x] of the measurement and shows that each planted defect fails with a ratio >= 4 c.

    output              emulation, worst row ratio and the case that gives it                               c
    head part           4.91e-03  zk_dec_self H 512, time 1 (two keys); cross: 4.51e-03 (H 1024, Lk 3)      9.8e-03
    head sum            3.54e-03  zk_dec_self H 128, time 1; cross: 3.52e-03 (the fully masked sentence)    7.0e-03
    LayerNorm output    3.57e-03  over the 41 cases of zk_ln_decode alone and the 24 prologues              7.1e-03

    emulation by entry point and H (worst head part / head sum over the cases; the checker prints every case with -s)
    zk_dec_cross   H 128, 39 cases  3.67e-03 / 3.52e-03      zk_dec_self   H 128, 8 cases  4.07e-03 / 3.54e-03
                   H 512, 10 cases  3.45e-03 / 2.83e-03                    H 512, 7 cases  4.91e-03 / 3.09e-03
                   H 1024, 9 cases  4.51e-03 / 2.82e-03                    H 1024, 1 case  3.76e-03 / 2.60e-03
                   H 2048, 1 case   2.74e-03 / 2.09e-03                    H 2048, 1 case  2.61e-03 / 1.93e-03
    many keys sit lower than few: Lk = 130 on 16 rows (group 16, H 512) 2.61e-03 / 1.98e-03, time 131 (H 512)
    3.24e-03 / 2.76e-03, 544 pairs (20 rows, time 33, group 16) 3.58e-03 / 3.03e-03

Where y is exactly reproducible (ybuf, and the partial-sum form: fp32 sums in the order p = 0, 1, .., the bias, one
rounding) the LayerNorm output is checked element by element: bound = 2^-8 |ref| + C_LN_ELEM 2^-23 (|gamma| |xhat| +
|beta|), C_LN_ELEM twice the worst ratio of float32 LayerNorms that sum in forward, reversed, pairwise and 64-strided
order against float64 (same CPU file): 33.9 units at worst -- an element with xhat and beta both near zero, where the
unit is small and the error of the row mean is not -- 7.2 on every other case; C_LN_ELEM = 67.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng  # noqa: E402
from tests import parity as P  # noqa: E402
from tests import decode_parity as DP  # noqa: E402

# twice the worst emulation ratio (tests/test_decode_parity_checker.py asserts that they still are)
C_PART = 9.8e-3
C_SUM = 7.0e-3
C_LN = 7.1e-3
C_LN_ELEM = 67.0

BF, F32 = torch.bfloat16, torch.float32
WORST = {"part": 0.0, "sum": 0.0, "ln": 0.0, "ln_elem": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst ratios on this device: head part %.3e (c %.3e), head sum %.3e (c %.3e), LayerNorm rows %.3e (c %.3e), "
          "LayerNorm elements %.3g x 2^-23 unit (c %.3g)" % (WORST["part"], C_PART, WORST["sum"], C_SUM, WORST["ln"], C_LN,
                                                             WORST["ln_elem"], C_LN_ELEM))


def G(rows, cols, ld=None, off=0, dtype=BF, prefill=None):
    return P.guarded(rows, cols, ld, off, dtype, prefill, "cuda")


def ptr(g):
    return None if g is None else g.mat.ptr


def dev_int(v):
    return torch.tensor([int(v)], dtype=torch.int32, device="cuda")


class Group(object):
    """zk_dec_group for the duration of a block; the previous value comes back whatever happens."""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.old = eng().lib.raw("zk_dec_group")(self.n)

    def __exit__(self, *exc):
        eng().lib.raw("zk_dec_group")(self.old)


# ---------------------------------------------------------------------------------------------- LayerNorm forms
class LnBuffers(object):
    """The guarded operands of one row-local LayerNorm (DP.ln_inputs) and the argument tuples of the entry points."""

    def __init__(self, a, tdev):
        self.a = a
        rows, H = a["x"].shape
        self.rows, self.H = rows, H
        g = torch.Generator(); g.manual_seed(5)
        self.x = G(rows, H, prefill=a["x"])
        self.ybuf = G(rows, H, prefill=a["ybuf"] if a["ybuf"] is not None else torch.randn(rows, H, generator=g))
        self.gamma = G(1, H, dtype=F32, prefill=a["gamma"])
        self.beta = G(1, H, dtype=F32, prefill=a["beta"])
        self.z = G(rows, 2 * H, prefill=a["z"]) if a["z"] is not None else None
        self.cat_in = G(rows, 2 * H, prefill=a["cat_in"]) if a["cat_in"] is not None else None
        self.parts = self.bias = None
        self.nparts, self.stride = 0, 0
        if a["parts"] is not None:
            self.nparts, _, W = a["parts"].shape
            self.stride = rows * W + 16
            self.parts = G(self.nparts, rows * W, self.stride, 0, F32, a["parts"].reshape(self.nparts, rows * W))
            self.bias = G(1, W, dtype=F32, prefill=a["bias"])
        self.tdev = dev_int(a["time"]) if tdev else None
        self.inv_arg = 0.5 if tdev else a["inv_count"]          # with time_dev the by-value argument is wrong on purpose
        self.fresh_outputs()

    def fresh_outputs(self):
        a, rows, H = self.a, self.rows, self.H
        self.out = G(rows, H)
        self.cache = G(rows, H, dtype=F32, prefill=a["cache"]) if a["cache"] is not None else None
        self.cat_out = G(rows, 2 * H) if a["cache"] is not None else None

    def head(self):
        return (ptr(self.x), ptr(self.ybuf), ptr(self.gamma), ptr(self.beta), ptr(self.out))

    def tail(self):
        return (self.H, DP.EPS, ptr(self.z), ptr(self.cat_in), ptr(self.parts), self.nparts, self.stride, ptr(self.bias),
                ptr(self.cache), ptr(self.cat_out), self.inv_arg, None if self.tdev is None else self.tdev.data_ptr())

    def check(self, what):
        """-> xout (bf16, CPU).  Inputs intact, guards intact, xout against the reference, the running sum exact."""
        a = self.a
        for g in (self.x, self.ybuf, self.gamma, self.beta, self.z, self.cat_in, self.parts, self.bias):
            if g is not None:
                g.check_intact(what + ": LayerNorm operand")
        self.out.check_guard(what + ": xout")
        xout = self.out.value()
        ref = DP.ln_run(a)
        r = DP.row_ratio(xout, ref["out"])
        WORST["ln"] = max(WORST["ln"], r)
        msg = "%s: LayerNorm rows %.3e (c %.3e)" % (what, r, C_LN)
        y = DP.ln_exact_y(a)
        if y is not None:
            ref_e, unit = DP.ln_unit(a["x"], y, a["gamma"], a["beta"], DP.EPS)
            err = (xout.double() - ref_e).abs() - 2.0 ** -8 * ref_e.abs()
            ru = float((err / unit.clamp_min(1e-300)).max())
            WORST["ln_elem"] = max(WORST["ln_elem"], ru)
            msg += ", elements %.3g units beyond 2^-8 |ref| (c %.3g)" % (ru, C_LN_ELEM)
        print(msg)
        assert r <= C_LN, msg
        if y is not None:
            ref_e, bound = DP.ln_elem(a["x"], y, a["gamma"], a["beta"], DP.EPS, C_LN_ELEM)
            P.assert_elementwise(xout, ref_e, bound, what + ": xout")
        if self.cache is not None:
            self.cache.check_guard(what + ": running sum")
            self.cat_out.check_guard(what + ": cat_out")
            new = self.cache.value()
            DP.assert_running_sum(a["cache"], xout, new, what)
            cat = self.cat_out.value()
            assert torch.equal(cat[:, :self.H].view(torch.int16), xout.view(torch.int16)), what + ": cat_out[:, :H] != xout"
            ref_c, bound_c = DP.cat_bound(new, a["inv_count"])
            P.assert_elementwise(cat[:, self.H:], ref_c, bound_c, what + ": cat_out average")
        return xout


def run_ln_alone(buf):
    e = eng()
    e.lib.call("zk_ln_decode", *buf.head(), buf.rows, *buf.tail(), e.stream)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", DP.ln_cases(), ids=lambda c: "H%d-r%d-%s-c%d-t%d" % (c["H"], c["rows"], c["form"], c["cache"], c["tdev"]))
def test_ln_decode_forms(case):
    a = DP.ln_inputs(case["rows"], case["H"], case["form"], case["cache"])
    buf = LnBuffers(a, case["tdev"])
    run_ln_alone(buf)
    buf.check("zk_ln_decode %s" % (case,))


# ---------------------------------------------------------------------------------------------- attention
_WEIGHTS = {}


def weights(H, self_attn):
    """The guarded projection weights of one H on the device (read-only: shared, compared whole after every call)."""
    key = (H, self_attn)
    if key not in _WEIGHTS:
        w = DP.attn_weights(H, self_attn)
        n = 3 if self_attn else 1
        _WEIGHTS[key] = {"wqt": G(n * H, H, H + 8, 0, prefill=w["wqt"]), "bq": G(1, n * H, dtype=F32, prefill=w["bq"]),
                         "wot": G(H, H, H + 16, 8, prefill=w["wot"])}
    return _WEIGHTS[key]


def rel_tables(x):
    if x["rk"] is None:
        return None, None
    n = 2 * x["max_rel"] + 1
    return G(n, DP.D, prefill=x["rk"]), G(n, DP.D, prefill=x["rv"])


def check_attn(what, parts_buf, ref, nh, rows, H):
    parts_buf.check_guard(what + ": out_parts")
    got = parts_buf.value().view(nh, rows, H)
    rp = DP.parts_ratio(got, ref["parts"])
    rs = DP.row_ratio(got.double().sum(0), ref["sum"])
    WORST["part"], WORST["sum"] = max(WORST["part"], rp), max(WORST["sum"], rs)
    msg = "%s: head parts %.3e (c %.3e), head sum %.3e (c %.3e)" % (what, rp, C_PART, rs, C_SUM)
    print(msg)
    assert rp <= C_PART and rs <= C_SUM, msg


def run_cross(case, x, pro=None):
    """One zk_dec_cross call on guarded operands -> (out_parts buffer, the read-only operands)."""
    e = eng()
    H, (B, R), Lk = case["H"], case["BR"], case["Lk"]
    nh, rows = H // DP.D, B * R
    w = weights(H, False)
    if case["layout"] == "halves":                 # column halves of one [B*Lk, 2H] buffer, as production passes them
        ld = 2 * H + 16
        kv = G(B * Lk, 2 * H, ld, 8, prefill=torch.cat([x["keys"].reshape(B * Lk, H), x["vals"].reshape(B * Lk, H)], 1))
        kp, vp, ldk, bsk, kvs = kv.mat.ptr, kv.mat.cols_slice(H, 2 * H).ptr, ld, Lk * ld, [kv]
    else:                                          # separate buffers, two NaN rows behind every sentence (padded bsk)
        ldk = H + 8
        pad = lambda t: torch.cat([t, torch.full((B, 2, H), float("nan"), dtype=t.dtype)], 1).reshape(B * (Lk + 2), H)
        kb, vb = G(B * (Lk + 2), H, ldk, 0, prefill=pad(x["keys"])), G(B * (Lk + 2), H, ldk, 0, prefill=pad(x["vals"]))
        kp, vp, bsk, kvs = kb.mat.ptr, vb.mat.ptr, (Lk + 2) * ldk, [kb, vb]
    mask = None
    if x["kmask"] is not None:
        mask = G(B, Lk, Lk + (5 if case["mask"] == "ldmask" else 0), 0, F32, x["kmask"])
    rk, rv = rel_tables(x)
    pos, pos_dev = x["pos"], None
    if case["rel"] is not None and case["rel"][2] == "dev":
        pos, pos_dev = x["pos"] + 7, dev_int(x["pos"])           # the device value wins
    out = G(nh * rows, H, dtype=F32)
    if pro is None:
        xin = G(rows, H, prefill=x["x"])
        lead = (ptr(xin), None, None, None, None, H, DP.EPS, None, None, None, 0, 0, None, None, None, 1.0, None)
    else:
        xin, lead = None, pro.head() + pro.tail()
    with Group(case["group"]):
        e.lib.call("zk_dec_cross", *lead, ptr(w["wqt"]), w["wqt"].ld, ptr(w["bq"]), kp, vp, ldk, ldk, bsk, bsk, ptr(mask),
                   0 if mask is None else mask.ld, ptr(w["wot"]), w["wot"].ld, ptr(out), B, R, nh, Lk, DP.SCALE, DP.MASK_INF,
                   ptr(rk), ptr(rv), x["max_rel"], pos, None if pos_dev is None else pos_dev.data_ptr(), e.stream)
        torch.cuda.synchronize()
    for g in [w["wqt"], w["bq"], w["wot"], xin, mask, rk, rv] + kvs:
        if g is not None:
            g.check_intact("zk_dec_cross operand")
    return out


def _cross_id(c):
    return "H%d-B%dR%d-g%d-L%d-%s-%s-%s" % (c["H"], c["BR"][0], c["BR"][1], c["group"], c["Lk"], c["mask"], c["layout"],
                                           "norel" if c["rel"] is None else "rel%d_%d_%s" % c["rel"])


@pytest.mark.parametrize("case", DP.cross_cases(), ids=_cross_id)
def test_dec_cross(case):
    x = DP.cross_inputs(case)
    ref = DP.cross_math(case, x)
    assert ref["smax"] < 4.0
    out = run_cross(case, x)
    (B, R), H = case["BR"], case["H"]
    check_attn("zk_dec_cross %s" % _cross_id(case), out, ref, H // DP.D, B * R, H)


def run_self(case, x, pro=None):
    """One zk_dec_self call -> (out_parts buffer, key cache, value cache)."""
    e = eng()
    H, (B, R), Tmax, t = case["H"], case["BR"], case["Tmax"], case["time"]
    nh, rows = H // DP.D, B * R
    w = weights(H, True)
    kc = G(rows * Tmax, H, prefill=x["keys"].reshape(rows * Tmax, H))
    vc = G(rows * Tmax, H, prefill=x["vals"].reshape(rows * Tmax, H))
    rk, rv = rel_tables(x)
    time, time_dev = t, None
    if case["tdev"]:
        time, time_dev = (t + 3) % Tmax, dev_int(t)              # the device value wins
    out = G(nh * rows, H, dtype=F32)
    if pro is None:
        xin = G(rows, H, prefill=x["x"])
        lead = (ptr(xin), None, None, None, None, H, DP.EPS, None, None, None, 0, 0, None, None, None, 1.0, None)
    else:
        xin, lead = None, pro.head() + pro.tail()
    with Group(case["group"]):
        e.lib.call("zk_dec_self", *lead, ptr(w["wqt"]), w["wqt"].ld, ptr(w["bq"]), ptr(kc), ptr(vc), Tmax, time,
                   None if time_dev is None else time_dev.data_ptr(), ptr(w["wot"]), w["wot"].ld, ptr(out), B, R, nh,
                   DP.SCALE, ptr(rk), ptr(rv), x["max_rel"], e.stream)
        torch.cuda.synchronize()
    for g in (w["wqt"], w["bq"], w["wot"], xin, rk, rv):
        if g is not None:
            g.check_intact("zk_dec_self operand")
    return out, kc, vc


def check_caches(what, case, x, xin, kc, vc):
    """Slot t = bf16(x W + b) element by element (parity.gemm_bound, K = H); every other slot and the guards bit-identical."""
    H, (B, R), Tmax, t = case["H"], case["BR"], case["Tmax"], case["time"]
    rows = B * R
    for name, g, blk in (("key", kc, 1), ("value", vc, 2)):
        now = g.t.detach().cpu().view(torch.int16)
        slot = torch.zeros(now.numel(), dtype=torch.bool)
        idx = (P.LEAD + (torch.arange(rows)[:, None] * Tmax + t) * H + torch.arange(H)[None, :]).reshape(-1)
        slot[idx] = True
        changed = (now != g.before) & ~slot
        assert int(changed.sum()) == 0, "%s: %d elements of the %s cache outside slot %d changed" % (
            what, int(changed.sum()), name, t)
        got = g.value().view(rows, Tmax, H)[:, t]
        ref, bound = P.gemm_bound(xin, x["wqt"][blk * H:(blk + 1) * H].t(), H, BF, bias=x["bq"][blk * H:(blk + 1) * H])
        P.assert_elementwise(got, ref, bound, "%s: %s cache slot %d" % (what, name, t))


def _self_id(c):
    return "H%d-B%dR%d-T%d-t%d-%s-g%d-%s" % (c["H"], c["BR"][0], c["BR"][1], c["Tmax"], c["time"],
                                            "dev" if c["tdev"] else "val", c["group"], "rel%d" % c["rel"] if c["rel"] else "norel")


@pytest.mark.parametrize("case", DP.SELF_CASES, ids=_self_id)
def test_dec_self(case):
    x = DP.self_inputs(case)
    ref = DP.self_math(case, x)
    assert ref["smax"] < 4.0
    out, kc, vc = run_self(case, x)
    (B, R), H = case["BR"], case["H"]
    what = "zk_dec_self %s" % _self_id(case)
    check_caches(what, case, x, x["x"], kc, vc)
    check_attn(what, out, ref, H // DP.D, B * R, H)


# ---------------------------------------------------------------------------------------------- prologue
def _prologue(entry, form, cache, tdev):
    case = DP.PRO_CROSS if entry == "cross" else DP.PRO_SELF
    (B, R), H = case["BR"], case["H"]
    nh, rows = H // DP.D, B * R
    a = DP.ln_inputs(rows, H, form, cache, seed=1, nparts=nh if form == "parts4" else None)
    buf = LnBuffers(a, tdev)
    what = "%s prologue %s cache=%d time_dev=%d" % (entry, form, cache, tdev)
    if entry == "cross":
        x = DP.cross_inputs(case)
        out = run_cross(case, x, pro=buf)
    else:
        x = DP.self_inputs(case)
        out, kc, vc = run_self(case, x, pro=buf)
    xout = buf.check(what)
    x["x"] = xout                                  # the attention stage alone: the reference is fed the kernel's own xout
    ref = DP.cross_math(case, x) if entry == "cross" else DP.self_math(case, x)
    if entry == "self":
        check_caches(what, case, x, xout, kc, vc)
    check_attn(what, out, ref, nh, rows, H)
    # the same LayerNorm by zk_ln_decode on the same arguments (reported, not asserted)
    buf.fresh_outputs()
    run_ln_alone(buf)
    same = torch.equal(buf.out.value().view(torch.int16), xout.view(torch.int16))
    print("%s: xout %s zk_ln_decode's" % (what, "bit-identical to" if same else "DIFFERS in bits from"))


@pytest.mark.parametrize("form,cache,tdev", DP.PROLOGUE_CASES)
def test_dec_cross_prologue(form, cache, tdev):
    _prologue("cross", form, cache, tdev)


@pytest.mark.parametrize("form,cache,tdev", DP.PROLOGUE_CASES)
def test_dec_self_prologue(form, cache, tdev):
    _prologue("self", form, cache, tdev)


# ---------------------------------------------------------------------------------------------- zk_gemm_parts
@pytest.mark.parametrize("M,N,K,splits", DP.GEMM_PARTS_CASES)
def test_gemm_parts(M, N, K, splits):
    e = eng()
    g = torch.Generator(); g.manual_seed(M + N + K)
    A = (torch.randn(M, K, generator=g)).to(BF)
    Bm = (torch.randn(K, N, generator=g) * K ** -0.5).to(BF)
    ga, gb = G(M, K, K + 8, 0, prefill=A), G(K, N, N + 16, 8, prefill=Bm)
    parts = G(splits, M * N, dtype=F32)
    n_out = ctypes.c_int(-1)
    e.lib.call("zk_gemm_parts", ptr(ga), ptr(gb), ptr(parts), M, N, K, ga.ld, gb.ld, 0, 0, splits, ctypes.byref(n_out),
               e.stream)
    torch.cuda.synchronize()
    ranges = DP.gemm_parts_ranges(K, splits)
    assert n_out.value == len(ranges), (n_out.value, ranges)
    ga.check_intact("A"); gb.check_intact("B")
    parts.check_guard("parts")
    got = parts.value().view(splits, M, N)
    for z, (k0, k1) in enumerate(ranges):
        ref, bound = P.gemm_bound(A[:, k0:k1], Bm[k0:k1], k1 - k0, F32)
        P.assert_elementwise(got[z], ref, bound, "part %d = K[%d, %d)" % (z, k0, k1))
    nan_bits = parts.before[P.LEAD:P.LEAD + splits * M * N].view(splits, M * N)
    now_bits = parts.t.detach().cpu().view(torch.int32)[P.LEAD:P.LEAD + splits * M * N].view(splits, M * N)
    assert torch.equal(now_bits[len(ranges):], nan_bits[len(ranges):]), "the space of parts >= nparts was written"
    # the consumer: zk_ln_decode adds the parts in the order z = 0, 1, .., the bias and the residual
    n = len(ranges)
    a = DP.ln_inputs(M, N, "ybuf", False, seed=2)
    a.update(ybuf=None, parts=got[:n].clone(), bias=torch.randn(N, generator=g))
    buf = LnBuffers(a, False)
    run_ln_alone(buf)
    buf.check("zk_ln_decode fed by zk_gemm_parts (%d, %d, %d, %d)" % (M, N, K, splits))


# ---------------------------------------------------------------------------------------------- zk_dec_embed
# rows, H, all ids pad, position from pos_dev, cache / cat, ride-along reorder (nl = 3)
EMBED_CASES = [(1, 128, True, False, False, False), (5, 128, False, True, False, False), (5, 520, False, False, True, False),
               (130, 520, False, True, True, True), (5, 128, True, True, True, True), (130, 128, False, False, True, True),
               (1, 520, False, True, True, False)]


@pytest.mark.parametrize("rows,H,allpad,posdev,cache,reorder", EMBED_CASES)
def test_dec_embed(rows, H, allpad, posdev, cache, reorder):
    e = eng()
    V, pad_id, pos, nl, Tpos = 11, 0, 4, 3, 8
    g = torch.Generator(); g.manual_seed(rows + H)
    ids = torch.zeros(rows, dtype=torch.int32) if allpad else torch.randint(0, V, (rows,), generator=g, dtype=torch.int32)
    if not allpad:
        ids[0] = 3                                  # at least one real id; pad ids among the others embed like any id
    table, bias, timing = torch.randn(V, H, generator=g).to(BF), 0.1 * torch.randn(H, generator=g), torch.randn(Tpos, H, generator=g)
    scale = float(H) ** 0.5
    gt, gb, gtim = G(V, H, prefill=table), G(1, H, dtype=F32, prefill=bias), G(Tpos, H, dtype=F32, prefill=timing)
    out = G(rows, H)
    nlay = nl if reorder else 1
    old = torch.randn(nlay, rows, H, generator=g) * 2.5
    idx = torch.randint(0, max(rows // 2, 1), (rows,), generator=g, dtype=torch.int32)      # parents repeat
    gcache = gsrc = gcat = None
    if cache:
        gcache = G(nlay * rows, H, dtype=F32, prefill=None if reorder else old.reshape(nlay * rows, H))
        gcat = G(rows, 2 * H)
        if reorder:
            gsrc = G(nlay * rows, H, dtype=F32, prefill=old.reshape(nlay * rows, H))
    ids_d, idx_d = ids.cuda(), idx.cuda()
    pos_dev = dev_int(pos) if posdev else None
    e.lib.call("zk_dec_embed", ids_d.data_ptr(), pad_id, ptr(gt), ptr(gb), ptr(gtim), ptr(out), rows, H, scale,
               pos + 2 if posdev else pos, None if pos_dev is None else pos_dev.data_ptr(), ptr(gcache), ptr(gcat),
               0.5 if posdev else 1.0 / (pos + 1), ptr(gsrc), idx_d.data_ptr() if reorder and cache else None, nlay, e.stream)
    torch.cuda.synchronize()
    for gg in (gt, gb, gtim, gsrc):
        if gg is not None:
            gg.check_intact("zk_dec_embed operand")
    assert torch.equal(ids_d.cpu(), ids) and torch.equal(idx_d.cpu(), idx)
    out.check_guard("out")
    got = out.value()
    tim = timing[pos].double()
    if allpad:
        assert torch.equal(got.view(torch.int16), timing[pos].to(BF).expand(rows, H).contiguous().view(torch.int16))
    else:
        # fp32: table * scale + bias (one or two roundings), + timing (one more), then one rounding to bf16
        emb = table[ids.long()].double() * scale
        ref = emb + bias.double() + tim
        mag = emb.abs() + bias.double().abs() + tim.abs()
        P.assert_elementwise(got, ref, 2.0 ** -8 * ref.abs() + 2 * 2.0 ** -23 * mag, "zk_dec_embed out")
    if cache:
        gcache.check_guard("running sums")
        gcat.check_guard("cat")
        new = gcache.value().view(nlay, rows, H)
        parent = old[0][idx.long()] if reorder else old[0]
        DP.assert_running_sum(parent, got, new[0], "zk_dec_embed layer 0")
        if reorder:
            assert torch.equal(new[1:].view(torch.int32), old[1:, idx.long()].contiguous().view(torch.int32)), \
                "layers 1 .. nl-1 are not byte copies of the parents' rows"
        cat = gcat.value()
        assert torch.equal(cat[:, :H].view(torch.int16), got.view(torch.int16))
        ref_c, bound_c = DP.cat_bound(new[0], 1.0 / (pos + 1))
        P.assert_elementwise(cat[:, H:], ref_c, bound_c, "zk_dec_embed cat average")


# ---------------------------------------------------------------------------------------------- zk_cache_rows
@pytest.mark.parametrize("rows,U,Tmax,t", [(5, 128, 7, 3), (130, 64, 5, 0), (12, 512, 6, 5)])
def test_cache_rows_append(rows, U, Tmax, t):
    """dst[r][*time_dev] <- src[r] (one unit of U bf16); src = a column slice of a wider matrix, as the qkv rows are."""
    e = eng()
    g = torch.Generator(); g.manual_seed(rows + U)
    src = G(rows, U, 3 * U, U, prefill=torch.randn(rows, U, generator=g))
    dst = G(rows, Tmax * U, Tmax * U + 8, 0, prefill=torch.randn(rows, Tmax * U, generator=g))
    want = dst.value().view(torch.int16).clone()
    want[:, t * U:(t + 1) * U] = src.value().view(torch.int16)
    td = dev_int(t)
    e.lib.call("zk_cache_rows", ptr(src), src.ld * 2, None, ptr(dst), dst.ld * 2, rows, U * 2, Tmax, td.data_ptr(), 0, 0,
               e.stream)
    torch.cuda.synchronize()
    src.check_intact("src")
    dst.check_guard("dst")
    assert torch.equal(dst.value().view(torch.int16), want)


@pytest.mark.parametrize("period,tables,U,Tmax,t", [(4, 3, 128, 6, 4), (130, 1, 64, 5, 2), (6, 2, 64, 4, 0), (5, 2, 64, 300, 299)])
def test_cache_rows_reorder(period, tables, U, Tmax, t):
    """dst[r][0 .. *time_dev) <- src[table(r) * period + index[r % period]][0 .. *time_dev); parents repeat."""
    e = eng()
    rows = period * tables
    g = torch.Generator(); g.manual_seed(rows + U)
    src = G(rows, Tmax * U, Tmax * U + 16, 8, prefill=torch.randn(rows, Tmax * U, generator=g))
    dst = G(rows, Tmax * U, Tmax * U + 8, 0, prefill=torch.randn(rows, Tmax * U, generator=g))
    idx = torch.randint(0, max(period // 2, 1), (period,), generator=g, dtype=torch.int32)
    parent = (torch.arange(rows) // period) * period + idx.long()[torch.arange(rows) % period]
    want = dst.value().view(torch.int16).clone()
    want[:, :t * U] = src.value().view(torch.int16)[parent][:, :t * U]
    td, idx_d = dev_int(t), idx.cuda()
    e.lib.call("zk_cache_rows", ptr(src), src.ld * 2, idx_d.data_ptr(), ptr(dst), dst.ld * 2, rows, U * 2, Tmax,
               td.data_ptr(), 1, period, e.stream)
    torch.cuda.synchronize()
    src.check_intact("src")
    dst.check_guard("dst")
    assert torch.equal(dst.value().view(torch.int16), want)
