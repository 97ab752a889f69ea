"""The in-launch LayerNorm (chain) kernels -- zk_gemm_add_ln, zk_gemm_ln_bwd, zk_attn_out_ln, zk_proj_attn_out_ln: cases,
inputs, STAGED float64 references with derived bounds, the CPU stand-in and the planted defects (a plain module, no pytest
in it; CPU only).  tests/test_chain_checker.py shows on the CPU that the check has teeth, tests/test_gpu_chain_elementwise.py
applies it to the kernels.

Staging.  Every stage is compared with float64 of what the kernel STORED for the stage before it, so no bound carries the
error of an earlier stage except where that stage is never stored (the product inside the sum, dout in the backward):

forward (zk_gemm_add_ln; the projection tail of the attention launches with A = the stored att)
    p   = bf16(A B + bias)         never stored: parity.gemm_bound (bias, bf16 output) -> (p_ref, bp)
    s   = R + m p                  parity.ln_fwd_bound's s line with y = p_ref, plus the propagated m bp (1 + 2^-8)
    s, exactly                     the product IS rounded to bf16 before the sum (the two-launch structure stored it), so the
                                   stored s must be bf16(R + m c) for a bf16 c that p can round to: c in {bf16(p_ref - a),
                                   bf16(p_ref + a)}, a = bp - 2^-8 |p_ref| (the accumulation part), the fp32 sum off by at most
                                   2 PER_TERM (|R| + |m c|).  This is what tells bf16(R + m p) from bf16(R + m bf16(p)).
    mean, rstd, y                  ln_fwd_bound(.., s_stored = the kernel's s)
    lean (nothing saved)           the kernel normalises the fp32 sum: ln_fwd_bound's inference branch with
                                   e = m bp + 2 PER_TERM (|R| + m (|p_ref| + bp)) in place of its 2 PER_TERM mag
backward (zk_gemm_ln_bwd)
    dout = bf16(dY W^T + R)        never stored: gemm_bound (tb = 1, residual, bf16 output) -> (dout_ref, delta)
    ds                             parity.ln_bwd_bound on dout_ref, plus (the backward is linear in dout)
                                   rstd (|gamma_j| delta_j + mean_row(|gamma| delta) + |xh_j| mean_row(|gamma| delta |xh|))
    dy                             from the STORED ds and the mask (ln_bwd_bound)
    partials [ceil(M/64)][3][N]    per 64-row block, before any reduction: ln_bwd_bound's column sums over the block's valid
                                   rows plus sum delta |xh| and sum delta; the third row from the STORED dy (ds without dropout)
attention launches
    q (k, v) tiles                 gemm_bound of x Wp + bp (zk_proj_attn_out_ln); the attention is conditioned on the stored tiles
    att, lse                       parity.attn_math, the row check under C_X["out"] and the 2e-2 lse bar of
                                   tests/test_gpu_attention_elementwise.py
    the tail                       as the forward, A = the stored att

Nothing here is measured on a device and no element is excused.
"""
import torch

from tests import parity as P
from zero_amd.utils import dtype as zdtype

BF, F32 = torch.bfloat16, torch.float32
EPS = float(zdtype.epsilon())
C_ATT = 7.9e-3          # C_X["out"] of tests/test_gpu_attention_elementwise.py (tests/test_chain_checker.py asserts the equality)
LSE_BAR = 2e-2          # its lse bar
SENTINEL = 12288.0      # (exact in bf16) the row behind row M of every [M, N] output: a full row of this, bit for bit afterwards
ATT_D = 64
S_STEPS = 8             # bf16 candidates of the product visited one by one in the exact check of s (fwd_bounds)


def nblocks(M):
    return (M + 63) // 64


def sy_local(M):
    """zk_gemm2.hip launch_dlds_sync_ln: the exchange stays in the XCD's L2 exactly when the number of 64-row blocks is a
    multiple of 8 (attention launches: B % 8 == 0)."""
    return 1 if nblocks(M) % 8 == 0 else 0


# ------------------------------------------------------------------------------------------------------------- cases
def _cover(factors, valid=lambda r: True):
    return P.pairwise(factors, valid)


# layout "win": A, B / W, R are column windows of wider guarded buffers (ld and offset multiples of 8).  The covering
# breaks ties towards the first level, so the more demanding level of every option comes first: the rows that only complete
# the M x K pairs are windows with dropout, a bias, saved statistics and a signed gamma.
FWD_FACTORS = {"M": [1, 5, 63, 64, 65, 130, 448, 500, 512, 513], "K": [8, 64, 72, 200, 264, 2048], "N": [512, 1024, 64, 128],
               "layout": ["win", "contig"], "drop": [0.25, 0.0], "bias": [True, False], "save": [True, False],
               "gamma": ["signed", "plain"]}
BWD_FACTORS = {"M": FWD_FACTORS["M"], "K": FWD_FACTORS["K"], "N": FWD_FACTORS["N"], "layout": ["win", "contig"],
               "drop": [0.25, 0.0], "res": [True, False], "gamma": ["signed", "plain"]}
FWD_CASES = _cover(FWD_FACTORS)
BWD_CASES = _cover(BWD_FACTORS)
# the exchange forced through memory (tuning key 15 = 1) on a shape whose grid would take the L2 route
MEM_ROUTE_CASE = dict(M=500, K=72, N=512, layout="win", drop=0.25, bias=True, save=True, gamma="signed", res=True)


def _attn_valid(r):
    if r["pro"] == 3 and (r["Lk"] != r["Lq"] or r["G"] != 1):
        return False                                    # merged qkv_map: self-attention
    if r["G"] == 2 and r["B"] != 8:
        return False                                    # two query sentences per key sentence
    if r["pro"] == 0 and r["Kp"] != 64:
        return False                                    # (no projection: Kp means nothing; keep one level)
    if r["mask"] == "key0" and r["Lk"] == 1:
        return False
    return True


# Lk has every level of Lq so that pro = 3 (Lk == Lq) can have each; mask: "ragged", "key0" (sentence 1 sees key 0 only), None
ATTN_FACTORS = {"Lk": [1, 13, 37, 64, 65, 150, 256], "Lq": [1, 13, 37, 64], "nh": [8, 2, 16], "B": [5, 8], "pro": [0, 1, 3],
                "Kp": [64, 192], "G": [1, 2], "causal": [True, False], "mask": ["ragged", "key0", None], "drop": [0.2, 0.0],
                "save": [True, False]}
ATTN_CASES = _cover(ATTN_FACTORS, _attn_valid)


def case_id(c):
    if "Lq" in c:
        return "B%d-nh%d-Lq%d-Lk%d-pro%d-Kp%d-G%d%s-%s-d%g-%s" % (c["B"], c["nh"], c["Lq"], c["Lk"], c["pro"], c["Kp"], c["G"],
                                                                "-causal" if c["causal"] else "", c["mask"], c["drop"],
                                                                "save" if c["save"] else "lean")
    tail = ("%s-%s" % ("bias" if c["bias"] else "nobias", "save" if c["save"] else "lean")) if "bias" in c else \
        ("res" if c["res"] else "nores")
    return "M%d-K%d-N%d-%s-d%g-%s-%s" % (c["M"], c["K"], c["N"], c["layout"], c["drop"], tail, c["gamma"])


# ------------------------------------------------------------------------------------------------------------ inputs
def _gen(c, seed):
    return torch.Generator().manual_seed(9000 + 131 * seed + sum(int(v) if isinstance(v, (int, bool)) else len(str(v))
                                                                 for v in c.values()))


def _ln_params(g, N, kind):
    gam = torch.randn(N, generator=g) if kind == "signed" else 1.0 + 0.2 * torch.randn(N, generator=g)
    return gam.float(), (0.1 * torch.randn(N, generator=g)).float()


def _residual(g, M, N, scale=1.0):
    """Rows with a mean of their own and 64-column groups with a level of their own: a wrong row's statistics, one
    workgroup's own statistics and a missing peer all move the result."""
    r = torch.randn(M, N, generator=g) + 0.7 * torch.randn(M, 1, generator=g)
    r = r + 0.5 * torch.randn(1, N // 64, generator=g).repeat_interleave(64, 1)
    return (scale * r).to(BF)


def fwd_inputs(c, seed=0):
    """bf16 A [M, K], B [K, N], R [M, N]; fp32 bias [N] or None, gamma, beta.  seed: the second, louder input of the
    stale-slot defect and of the repetition tests."""
    M, K, N = c["M"], c["K"], c["N"]
    g = _gen(c, seed)
    amp = 1.0 + 2.0 * seed
    x = {"A": (0.5 * amp * torch.randn(M, K, generator=g)).to(BF), "B": (torch.randn(K, N, generator=g) * K ** -0.5).to(BF),
         "R": _residual(g, M, N, amp)}
    x["bias"] = (0.1 * torch.randn(N, generator=g)).float() if c.get("bias", True) else None
    x["gamma"], x["beta"] = _ln_params(g, N, c["gamma"])
    return x


def bwd_inputs(c, seed=0):
    """bf16 dY [M, K], W [N, K], R [M, N] or None, s [M, N]; fp32 mean, rstd of s (as the forward leaves them), gamma."""
    M, K, N = c["M"], c["K"], c["N"]
    g = _gen(c, seed + 50)
    x = {"dY": (0.5 * torch.randn(M, K, generator=g)).to(BF), "W": (torch.randn(N, K, generator=g) * K ** -0.5).to(BF),
         "R": _residual(g, M, N, 0.3) if c["res"] else None, "s": _residual(g, M, N)}
    sf = x["s"].float()
    x["mean"] = sf.mean(1).contiguous()
    x["rstd"] = torch.rsqrt(sf.var(1, unbiased=False) + EPS).contiguous()
    x["gamma"], _ = _ln_params(g, N, c["gamma"])
    return x


def cpu_mask(rows, cols, p, seed):
    """A dropout scale per element as zk_dropout_mask gives it (0 or fp32 1 / keep) from torch's generator: the CPU tests'
    stand-in for the device's mask; None for p = 0."""
    if not p:
        return None
    g = torch.Generator().manual_seed(77000 + seed)
    keep = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))
    return (torch.rand(rows, cols, generator=g) >= p).float() * keep


def attn_inputs(c, seed=0):
    """q / k / v (or x, Wp, bp for the projected ones), kmask, Wo, bias, R, gamma, beta of an attention case."""
    B, nh, Lq, Lk, G, pro, Kp = (c[n] for n in ("B", "nh", "Lq", "Lk", "G", "pro", "Kp"))
    H, Tq, Tk = nh * ATT_D, B * Lq, (B // G) * Lk
    g = _gen(c, seed + 100)
    rnd = lambda *s, scale=1.0: (scale * torch.randn(*s, generator=g)).to(BF)
    x = {"q": None, "k": None, "v": None, "x": None, "Wp": None, "bp": None}
    if pro:
        x["x"], x["Wp"] = rnd(Tq, Kp), rnd(Kp, pro * H, scale=Kp ** -0.5)
        x["bp"] = (0.1 * torch.randn(pro * H, generator=g)).float()
    else:
        x["q"] = rnd(Tq, H)
    if pro != 3:
        x["k"], x["v"] = rnd(Tk, H), (torch.randn(Tk, H, generator=g) + torch.randn(B // G, 1, H, generator=g)
                                      .expand(-1, Lk, -1).reshape(Tk, H)).to(BF)
    km = None
    if c["mask"] is not None:
        km = torch.ones(B // G, Lk)
        if c["mask"] == "ragged":
            for b in range(1, B // G):
                km[b, Lk - (b * 3) % max(Lk - 1, 1):] = 0
        else:
            km[1, 1:] = 0
        km[:, 0] = 1
    x["kmask"] = km
    x["Wo"], x["R"] = rnd(H, H, scale=H ** -0.5), _residual(g, Tq, H)
    x["bias"] = (0.1 * torch.randn(H, generator=g)).float()
    x["gamma"], x["beta"] = _ln_params(g, H, "signed" if c["causal"] else "plain")
    return x


def tail_case(c):
    """The attention launch's projection tail as a forward case: M = B Lq rows, K = N = nh 64."""
    H = c["nh"] * ATT_D
    return dict(M=c["B"] * c["Lq"], K=H, N=H, layout="win", drop=c["drop"], bias=True, save=c["save"], gamma="plain")


# --------------------------------------------------------------------------------------------- references and bounds
def _d(x):
    return None if x is None else x.detach().to("cpu").double()


def _bf64(x):
    """float64 -> the nearest bf16 value, as float64."""
    return x.float().to(BF).double()


def fwd_bounds(x, mask, got):
    """x: fwd_inputs (A may be the stored att), mask: the dropout scale [M, N] or None, got: {"s", "mean", "rstd", "y"} the
    kernel's outputs (s None: the lean form).  -> ({name: (ref, bound)} in staged order, s_ok) with s_ok the boolean
    [M, N] tensor of the exact-membership check of s (None in the lean form)."""
    K = x["A"].shape[1]
    p_ref, bp = P.gemm_bound(x["A"], x["B"], K, BF, bias=x["bias"])
    R = _d(x["R"])
    m = torch.ones_like(R) if mask is None else _d(mask).reshape(R.shape)
    prop = m * bp
    if got.get("s") is None:
        e = prop + 2 * P.PER_TERM * (R.abs() + m * (p_ref.abs() + bp))
        b = P.ln_fwd_bound(x["R"], p_ref, mask, x["gamma"], x["beta"], EPS, s_stored=None, e=e)
        return {"y": b["out"]}, None
    b = P.ln_fwd_bound(x["R"], p_ref, mask, x["gamma"], x["beta"], EPS, s_stored=got["s"])
    s_ref, s_bound = b["s"]
    res = {"s": (s_ref, s_bound + prop * (1 + P.U_OUT[BF]) + 2 * P.PER_TERM * prop),
           "mean": b["mean"], "rstd": b["rstd"], "y": b["out"]}
    acc = bp - P.U_OUT[BF] * p_ref.abs()
    gs = _d(got["s"])
    lo, hi = (p_ref - acc).float().to(BF), (p_ref + acc).float().to(BF)
    s_of = lambda cnd, sign: _bf64(R + m * cnd + sign * 2 * P.PER_TERM * (R.abs() + (m * cnd).abs()))
    # more than S_STEPS bf16 values between lo and hi (a product that cancelled to nearly nothing): s is monotone in c
    ok = (gs >= s_of(lo.double(), -1)) & (gs <= s_of(hi.double(), 1))
    cnd, up, exhausted = lo, torch.full_like(lo, float("inf")), torch.ones_like(ok)
    for _ in range(S_STEPS):
        c64 = cnd.double()
        ok_here = (gs >= s_of(c64, -1)) & (gs <= s_of(c64, 1))          # (the two are equal or neighbours unless the sum cancels)
        exhausted &= ~ok_here
        nxt = torch.minimum(torch.nextafter(cnd, up), hi)
        done = nxt == cnd
        cnd = nxt
        if bool(done.all()):
            break
    # an element whose candidates were all visited must be one of them
    visited_all = cnd == hi
    last = (gs >= s_of(hi.double(), -1)) & (gs <= s_of(hi.double(), 1))
    ok = torch.where(visited_all, ~exhausted | last, ok)
    return res, ok


def check_fwd(x, mask, got, what):
    """Every stored tensor of a forward against its stage's bound, element by element.  -> name -> worst |err| / bound."""
    bounds, s_ok = fwd_bounds(x, mask, got)
    worst = P.check_all(got, bounds, what)
    if s_ok is not None:
        bad = int((~s_ok).sum())
        if bad:
            r, c = (int(v) for v in torch.nonzero(~s_ok)[0])
            raise AssertionError("%s [s, exactly]: %d of %d elements are no bf16(R + mask bf16(A B + bias)); the first at "
                                 "(row %d, col %d): got %r" % (what, bad, s_ok.numel(), r, c, float(got["s"][r, c])))
    return worst


def bwd_bounds(x, mask, got):
    """x: bwd_inputs, got: {"ds", "dy" (None without dropout), "part" [nblk, 3, N]}.  -> {name: (ref, bound)}; the
    partials as "part" [nblk, 3, N]."""
    M, K = x["dY"].shape
    dout, delta = P.gemm_bound(x["dY"], x["W"].t(), K, BF, res=x["R"])
    b = P.ln_bwd_bound(dout, x["s"], x["mean"], x["rstd"], x["gamma"], scale=mask, ds_stored=got["ds"], dy_stored=got.get("dy"))
    g = _d(x["gamma"]).abs()[None]
    mu, rs = _d(x["mean"]).reshape(M, 1), _d(x["rstd"]).reshape(M, 1)
    xh = (_d(x["s"]) - mu) * rs
    kd = dict(dim=1, keepdim=True)
    gd = g * delta
    prop = rs.abs() * (gd + gd.mean(**kd) + xh.abs() * (gd * xh.abs()).mean(**kd))
    res = {"ds": (b["ds"][0], b["ds"][1] + prop * (1 + P.U_OUT[BF]))}
    if mask is not None:
        res["dy"] = b["dy"]
    refs, bnds = [], []
    for blk in range(nblocks(M)):
        sl = slice(blk * 64, min(M, blk * 64 + 64))
        pb = P.ln_bwd_bound(dout[sl], x["s"][sl], x["mean"][sl], x["rstd"][sl], x["gamma"],
                            scale=None if mask is None else mask[sl], ds_stored=got["ds"][sl],
                            dy_stored=None if mask is None else got["dy"][sl])
        extra = [(delta[sl] * xh[sl].abs()).sum(0), delta[sl].sum(0), torch.zeros_like(delta[0])]
        refs.append(torch.stack([pb[k][0] for k in ("dgamma", "dbeta", "dbias_prev")]))
        bnds.append(torch.stack([pb[k][1] + ex * (1 + (sl.stop - sl.start + P.C_RED) * P.PER_TERM)
                                 for k, ex in zip(("dgamma", "dbeta", "dbias_prev"), extra)]))
    res["part"] = (torch.stack(refs), torch.stack(bnds))
    return res


def check_bwd(x, mask, got, what):
    bounds = bwd_bounds(x, mask, got)
    flat = dict(got)
    nb = nblocks(x["dY"].shape[0])
    flat["part"] = got["part"].reshape(nb * 3, -1)
    bounds["part"] = tuple(t.reshape(nb * 3, -1) for t in bounds["part"])
    return P.check_all(flat, bounds, what)


def expand_kv(c, t):
    """[B / G sentences of L rows, H] -> one sentence per query sentence (kv_group > 1: G query sentences share keys,
    values and mask row)."""
    if t is None or c["G"] == 1:
        return t
    nB = c["B"] // c["G"]
    return t.reshape(nB, -1).repeat_interleave(c["G"], 0).reshape(-1, t.shape[1])


def attn_reference(c, q, k, v, kmask, drop_mask, emulate=False):
    """parity.attn_math on the (stored) q / k / v: {"out" [B Lq, H], "lse" [B, nh, Lq]} float64."""
    B, nh, Lq, Lk = c["B"], c["nh"], c["Lq"], c["Lk"]
    H = nh * ATT_D
    kk, vv = expand_kv(c, k), expand_kv(c, v)
    km = None if kmask is None else kmask.repeat_interleave(c["G"], 0)
    r = P.attn_math(q, kk, vv, torch.zeros(B * Lq, H), B, nh, Lq, Lk, ATT_D, kmask=km, causal=c["causal"], drop_mask=drop_mask,
                    emulate=emulate)
    return {"out": r["out"], "lse": r["lse"]}


def check_attn(c, x, got, masks, what):
    """got: {"q", "k", "v" (the stored tiles with a projection; else the inputs), "att", "lse" [B nh Lq], "s", "mean", "rstd",
    "y"}; masks: {"attn": [B, nh, Lq, Lk] or None, "tail": [M, N] or None}.  -> name -> worst ratio."""
    B, nh, Lq = c["B"], c["nh"], c["Lq"]
    H = nh * ATT_D
    worst = {}
    if c["pro"]:
        ref, bound = P.gemm_bound(x["x"], x["Wp"], c["Kp"], BF, bias=x["bp"])
        names = ("q", "k", "v")[:c["pro"]]
        bounds = {n: (ref[:, i * H:(i + 1) * H], bound[:, i * H:(i + 1) * H]) for i, n in enumerate(names)}
        worst.update(P.check_all(got, bounds, what))
    ref = attn_reference(c, got["q"], got["k"], got["v"], x["kmask"], masks["attn"])
    worst["att"] = P.assert_attn_rows(got["att"], ref["out"], ATT_D, C_ATT, what + " [att]", heads=nh)
    lse_err = (_d(got["lse"]).reshape(B, nh, Lq) - ref["lse"]).abs()
    assert bool(torch.isfinite(lse_err).all()) and float(lse_err.max()) < LSE_BAR, (what, "lse", float(lse_err.max()))
    worst["lse"] = float(lse_err.max()) / LSE_BAR
    xt = {"A": got["att"], "B": x["Wo"], "R": x["R"], "bias": x["bias"], "gamma": x["gamma"], "beta": x["beta"]}
    worst.update(check_fwd(xt, masks["tail"], got, what))
    return worst


# ------------------------------------------------------------------------------- the CPU stand-in, the planted defects
FWD_DEFECTS = ("peer_missing", "stale_slot", "own_columns_only", "neighbour_row", "mask_other_site", "no_residual", "no_bias",
               "product_unrounded", "stale_chunk", "row_M_processed")
BWD_DEFECTS = ("bwd_peer_missing", "partial_next_row", "dy_unrounded", "bwd_stale_chunk", "bwd_row_M_processed")
ATTN_DEFECTS = ("next_sentence_row",)


def _f(x):
    return None if x is None else x.detach().to("cpu").float()


def fwd_applies(defect, c):
    M, N = c["M"], c["N"]
    return {"peer_missing": N > 64, "stale_slot": N > 64, "own_columns_only": N > 64, "neighbour_row": M > 1,
            "mask_other_site": c["drop"] > 0, "no_bias": c.get("bias", True), "product_unrounded": c["save"],
            "row_M_processed": M % 64 != 0}.get(defect, True)


def bwd_applies(defect, c):
    M, N = c["M"], c["N"]
    return {"bwd_peer_missing": N > 64, "partial_next_row": M > 64, "dy_unrounded": c["drop"] > 0,
            "bwd_row_M_processed": M % 64 != 0}.get(defect, True)


def _partials(r):
    """{sum, M2} of every row's 64-column groups, as a workgroup publishes them: [M, np] each."""
    M, N = r.shape
    t = r.view(M, N // 64, 64)
    s1 = t.sum(2)
    mt = s1 * (1.0 / 64.0)
    return s1, ((t - mt[:, :, None]) ** 2).sum(2)


def _chan(s1, s2, N, have=None):
    """Chan's combination of the per-group partials: (mean, rstd) per row."""
    invh = torch.tensor(1.0, dtype=F32) / torch.tensor(float(N), dtype=F32)
    if have is None:
        have = torch.ones_like(s1)
    mu = (s1 * have).sum(1) * invh
    d = s1 * (1.0 / 64.0) - mu[:, None]
    m2 = ((s2 + 64.0 * d * d) * have).sum(1)
    return mu, torch.rsqrt(m2 * invh + EPS)


def fwd_standin(x, mask, save, defect=None, other=None, other_mask=None, at=None):
    """What a correct zk_gemm_add_ln computes, on the CPU: fp32 product and epilogue, bf16 at the storage sites (the
    product ahead of the sum, the saved sum, y), the statistics as Chan's combination of per-64-column {sum, M2}.
    -> {"s", "mean", "rstd" (None in the lean form), "y"}, and "row_M" with the defect that writes one.

    defect (at = (row, peer / first column of the chunk); one at a time):
      peer_missing       row at[0]'s statistics lack the partial of column group at[1]
      stale_slot         that partial comes from ``other`` (the other input's run: a slot of the launch before)
      own_columns_only   every 64-column group normalised with the statistics of its own columns
      neighbour_row      row at[0] normalised with the statistics of the row below (above for the last row)
      mask_other_site    the dropout scale of ``other_mask``
      no_residual / no_bias
      product_unrounded  R + mask (A B + bias) without the bf16 rounding of the product
      stale_chunk        8 elements of y left at the NaN prefill
      row_M_processed    the ragged last block also stores row M (from the clamped loads of row M - 1)"""
    A, B, R = _f(x["A"]), _f(x["B"]), _f(x["R"])
    M, N = R.shape
    r0, q0 = at if at is not None else (M // 2, (N // 64) // 2)
    p = A @ B
    if x["bias"] is not None and defect != "no_bias":
        p = p + _f(x["bias"])[None]
    if defect != "product_unrounded":
        p = p.to(BF).float()
    mk = other_mask if defect == "mask_other_site" else mask
    if mk is not None:
        p = p * _f(mk).reshape(M, N)
    v = p if defect == "no_residual" else R + p
    s = v.to(BF) if save else None
    r = s.float() if save else v
    s1, s2 = _partials(r)
    if defect == "stale_slot":
        o = fwd_standin(other, None, save)
        o1, o2 = _partials(o["_r"])
        s1, s2 = s1.clone(), s2.clone()
        s1[r0, q0], s2[r0, q0] = o1[r0, q0], o2[r0, q0]
    have = torch.ones_like(s1)
    if defect == "peer_missing":
        have[r0, q0] = 0
    mu, rs = _chan(s1, s2, N, have)
    mu_u, rs_u = mu[:, None].expand(M, N), rs[:, None].expand(M, N)
    if defect == "own_columns_only":
        mu_u = (s1 * (1.0 / 64.0)).repeat_interleave(64, 1)
        rs_u = torch.rsqrt(s2 * (1.0 / 64.0) + EPS).repeat_interleave(64, 1)
    if defect == "neighbour_row":
        o = r0 + 1 if r0 + 1 < M else r0 - 1
        mu_u, rs_u = mu_u.clone(), rs_u.clone()
        mu_u[r0], rs_u[r0] = mu[o], rs[o]
    y = (_f(x["gamma"])[None] * (r - mu_u) * rs_u + _f(x["beta"])[None]).to(BF)
    if defect == "stale_chunk":
        y[r0, q0 * 64 + 8:q0 * 64 + 16] = float("nan")
    out = {"s": s, "mean": mu if save else None, "rstd": rs if save else None, "y": y, "_r": r, "_mu": mu, "_rs": rs}
    if defect == "row_M_processed":
        out["row_M"] = {"y": y[M - 1].clone(), "s": None if s is None else s[M - 1].clone()}
    return out


def bwd_standin(x, mask, defect=None, at=None):
    """What a correct zk_gemm_ln_bwd computes, on the CPU: dout rounded to bf16 as the dgrad launch stored it, the two row
    means as sums of per-64-column partial sums (eight of them at N = 512), ds and dy rounded to bf16, dy from the
    rounded ds, the partials per 64-row block.  -> {"ds", "dy" (None without dropout), "part" [nblk, 3, N]}.

    defect: bwd_peer_missing (row at[0]'s means lack column group at[1]; by default the largest partial), partial_next_row (block 0's partials include row
    64), dy_unrounded (dy from the fp32 ds), bwd_stale_chunk, bwd_row_M_processed (row M stored as well)."""
    dY, W, sv = _f(x["dY"]), _f(x["W"]), _f(x["s"])
    M, N = sv.shape
    r0, q0 = at if at is not None else (M // 2, (N // 64) // 2)
    v = dY @ W.t()
    if x["R"] is not None:
        v = v + _f(x["R"])
    d = v.to(BF).float()
    mu, rs = _f(x["mean"]).reshape(M, 1), _f(x["rstd"]).reshape(M, 1)
    xh = (sv - mu) * rs
    g = d * _f(x["gamma"])[None]
    invh = torch.tensor(1.0, dtype=F32) / torch.tensor(float(N), dtype=F32)
    sg, sgx = g.view(M, N // 64, 64).sum(2), (g * xh).view(M, N // 64, 64).sum(2)
    if defect == "bwd_peer_missing":
        if at is None:          # where it shows best: the row's largest partial (one that happens to be ~0 changes nothing)
            r0, q0 = divmod(int((sg.abs() * rs).reshape(-1).argmax()), N // 64)
        sg, sgx = sg.clone(), sgx.clone()
        sg[r0, q0] = 0
        sgx[r0, q0] = 0
    mg, mgx = (sg.sum(1) * invh)[:, None], (sgx.sum(1) * invh)[:, None]
    ds32 = rs * (g - mg - xh * mgx)
    ds = ds32.to(BF)
    dy = None
    src = ds.float()
    if mask is not None:
        dy = ((ds32 if defect == "dy_unrounded" else ds.float()) * _f(mask).reshape(M, N)).to(BF)
        src = dy.float()
    part = torch.zeros(nblocks(M), 3, N)
    for blk in range(nblocks(M)):
        hi = min(M, blk * 64 + 64 + (1 if defect == "partial_next_row" and blk == 0 else 0))
        sl = slice(blk * 64, hi)
        part[blk, 0], part[blk, 1], part[blk, 2] = (d[sl] * xh[sl]).sum(0), d[sl].sum(0), src[sl].sum(0)
    if defect == "bwd_stale_chunk":
        ds = ds.clone()
        ds[r0, q0 * 64 + 8:q0 * 64 + 16] = float("nan")
    out = {"ds": ds, "dy": dy, "part": part}
    if defect == "bwd_row_M_processed":
        out["row_M"] = {"ds": ds[M - 1].clone(), "dy": None if dy is None else dy[M - 1].clone()}
    return out


def attn_standin(c, x, masks, defect=None):
    """The attention launches on the CPU: the projection as parity.cpu_gemm_standin, the attention as parity.attn_math in
    its emulating form, the tail as fwd_standin with A = the rounded att.
    defect next_sentence_row (Lq < 64, B > 1): the row tile of sentence 0 reaches into sentence 1 and stores its first row,
    normalised with the statistics of its own last row."""
    B, nh, Lq, pro = c["B"], c["nh"], c["Lq"], c["pro"]
    H = nh * ATT_D
    got = {"q": x["q"], "k": x["k"], "v": x["v"]}
    if pro:
        pr = P.cpu_gemm_standin(x["x"], x["Wp"], BF, bias=x["bp"])
        for i, n in enumerate(("q", "k", "v")[:pro]):
            got[n] = pr[:, i * H:(i + 1) * H].contiguous()
    a = attn_reference(c, got["q"], got["k"], got["v"], x["kmask"], masks["attn"], emulate=True)
    got["att"], got["lse"] = a["out"].to(BF), a["lse"].float().reshape(-1)
    xt = {"A": got["att"], "B": x["Wo"], "R": x["R"], "bias": x["bias"], "gamma": x["gamma"], "beta": x["beta"]}
    got.update(fwd_standin(xt, masks["tail"], c["save"]))
    if defect == "next_sentence_row":
        assert Lq < 64 and B > 1
        r, mu, rs = got["_r"], got["_mu"], got["_rs"]
        y = got["y"].clone()
        y[Lq] = (_f(x["gamma"]) * (r[Lq] - mu[Lq - 1]) * rs[Lq - 1] + _f(x["beta"])).to(BF)
        got["y"] = y
    return got


# -------------------------------------------------------------------------------------------- guarded output buffers
def out_rows(M, N, ld=None, off=0, dtype=BF, device="cpu"):
    """An [M, N] output of a chain kernel: a guarded window of M + 1 rows, the M rows NaN (nobody wrote them yet), row M a
    full row of SENTINEL -- what a ragged block that also processed row M would overwrite (the 64 guard elements behind
    a window are fewer than a row)."""
    pre = torch.full((M + 1, N), float("nan"))
    pre[M] = SENTINEL
    return P.guarded(M + 1, N, ld, off, dtype, pre, device)


def out_value(gd, M, what):
    """Guard band and sentinel row intact -> the M rows as a CPU tensor."""
    gd.check_guard(what)
    v = gd.value()
    if not bool((v[M].float() == SENTINEL).all()):
        raise AssertionError("%s: row M = %d (behind the last row) was written" % (what, M))
    return v[:M].contiguous()


def deposit(gd, rows, row_M=None):
    """The CPU tests' store of a stand-in's tensor into an out_rows buffer."""
    M = rows.shape[0]
    w = gd.window()
    w[:M] = rows.to(w.dtype)
    if row_M is not None:
        w[M] = row_M.to(w.dtype)
