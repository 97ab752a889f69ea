"""Element-wise parity of the row kernels of the training step (zero_amd/csrc/zk_elem.hip: residual + LayerNorm forward
and backward, the fused cross entropy, the column sums, the loss tail) against float64 references with the derived
bounds of tests/parity.py (ln_fwd_bound, ln_bwd_bound, ce_bound, colsum_ref), on guarded operands: every output is a
NaN-prefilled window between two guard bands, every input is compared bit for bit after the call.

Column reductions run twice: on random values against the worst-case bound, and on small integers (|v| <= 8, every
partial sum below 2^24), where every summation order gives the bits of the float64 sum and one missing or doubled row
among thousands shows.  The integer runs use dropout 0.5 where the random ones use 0.25: the scale 2 keeps the terms
integers, 4/3 does not.

Which case reaches which kernel:
  k_add_ln_fwd<1> H <= 512, <2> H in {520, 1024}, <4> H in {1032, 2048}; the row loop repeats at 8200 rows (2048 blocks x 4)
  k_add_ln_bwd_wide H <= 512 (zk_tune(0, 1)), k_add_ln_bwd<1> the same H under zk_tune(0, 0), <2> H in {520, 1024},
  <4> H in {1032, 2048}; 4100 rows (H = 64 wide and narrow, H = 1032) run the block-stride loop (256 blocks x 16 rows)
  k_ce_fused ld <= 4096 and ld > 32768, k_ce_fused_reg<4> 4096 < ld <= 16384, k_ce_fused_reg<8> 16384 < ld <= 32768
  k_colsum with gy clamped to 64 at 16500 rows; k_colsum_pair; k_colsum_grouped + k_reduce_grouped
  k_loss_tail (B <= 4096, tuning key 16 = 0), k_per_sample + k_mean (key 16 = 1, and B = 4097 always)

The case lists and the operand builders are plain CPU code: tests/test_rowkernel_checker.py imports them.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng  # noqa: E402
from tests import parity as P  # noqa: E402
from tests.parity import guarded, pairwise  # noqa: E402
from zero_amd.utils import dtype as zdtype  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
EPS = float(torch.tensor(zdtype.epsilon(), dtype=F32))
SEED, SID = 4321, 11


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def _ints(g, *shape, lim=8):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def _G(rows, cols, dtype=BF, prefill=None, ld=None, off=0):
    return guarded(rows, cols, ld, off, dtype, prefill, "cuda")


def _vec(g):
    """A 1 x n fp32 window as the flat tensor the Engine takes."""
    return g.window().view(-1)


def _val(g):
    return None if g is None else (g.value().view(-1) if g.rows == 1 and g.dtype == F32 else g.value())


def _mask(e, rows, cols, p, sid=SID):
    """The dropout scale per element (0 or 1 / keep) the kernels apply for the engine's seed and this site."""
    msk = torch.zeros(rows * cols, device="cuda")
    e.lib.call("zk_dropout_mask", msk.data_ptr(), rows * cols, p, e.seed.data_ptr(), sid, e.stream)
    torch.cuda.synchronize()
    return msk.view(rows, cols).cpu()


def cpu_mask(rows, cols, p, seed=99):
    """The same kind of tensor without a GPU (the checker tests)."""
    return (torch.rand(rows, cols, generator=_gen(seed)) >= p).float() / (1 - p) if p > 0 else None


def _finish(outs, ins, what):
    for name, g in outs.items():
        if g is not None:
            g.check_guard("%s %s" % (what, name))
    for name, g in ins.items():
        if g is not None:
            g.check_intact("%s %s" % (what, name))


# ---------------------------------------------------------------------------------------------- LayerNorm forward
LN_H = [8, 64, 72, 504, 512, 520, 1024, 1032, 2048]      # one live lane; part-filled and full slabs of <1>, <2>, <4>
LN_FWD_CASES = pairwise(dict(H=LN_H, rows=[1, 5, 37], y=[0, 1], save=[0, 1], drop=[0.0, 0.25], gamma=["plain", "signed"]),
                        valid=lambda r: r["y"] or r["drop"] == 0.0)
LN_FWD_CASES.append(dict(H=64, rows=8200, y=1, save=1, drop=0.25, gamma="signed"))
ROW_CONST, ROW_TINY, ROW_SPIKE = 1, 2, 3                  # the special rows of a case with at least 5 rows


def _gamma_beta(g, H, kind):
    gamma = 1 + 0.1 * torch.randn(H, generator=g)
    if kind == "signed":
        gamma[::3] = -gamma[::3]
        gamma[1::5] = 0.0
    return gamma, 0.1 * torch.randn(H, generator=g)


def ln_fwd_inputs(case):
    """x, y (bf16), gamma, beta (fp32) on the CPU.  With 5 rows or more: row 1 is constant, row 2 holds +-2^-14 (a
    variance of 2^-28, of the order of eps = 1e-8: eps inside the root and eps outside it give different rows), row 3 has
    one entry 2^7 times the rest; y is 0 in these rows, so they are what the kernel normalises."""
    H, rows = case["H"], case["rows"]
    g = _gen(7 + H + rows)
    x = torch.randn(rows, H, generator=g)
    y = torch.randn(rows, H, generator=g) if case["y"] else None
    if rows >= 5:
        x[ROW_CONST] = 3.0
        x[ROW_TINY] = 2.0 ** -14
        x[ROW_TINY, ::2] = -2.0 ** -14
        x[ROW_SPIKE] = 0.25 * torch.randn(H, generator=g)
        x[ROW_SPIKE, H // 2] = 32.0
        if y is not None:
            y[ROW_CONST:ROW_SPIKE + 1] = 0.0
    gamma, beta = _gamma_beta(g, H, case["gamma"])
    return {"x": x.to(BF), "y": None if y is None else y.to(BF), "gamma": gamma, "beta": beta}


@pytest.mark.parametrize("case", LN_FWD_CASES, ids=lambda c: "H%d-r%d-y%d-s%d-d%g-%s" % tuple(c.values()))
def test_add_ln_fwd(case):
    e, inp = eng(), ln_fwd_inputs(case)
    H, rows, drop = case["H"], case["rows"], case["drop"]
    what = "add_ln_fwd %s" % (case,)
    ins = {"x": _G(rows, H, BF, inp["x"]), "y": _G(rows, H, BF, inp["y"]) if case["y"] else None,
           "gamma": _G(1, H, F32, inp["gamma"]), "beta": _G(1, H, F32, inp["beta"])}
    outs = {"out": _G(rows, H), "s": None, "mean": None, "rstd": None}
    if case["save"]:
        outs.update(s=_G(rows, H), mean=_G(1, rows, F32), rstd=_G(1, rows, F32))
    e.set_seed(SEED)
    e.add_ln_fwd(ins["x"].mat, ins["y"].mat if case["y"] else None, _vec(ins["gamma"]), _vec(ins["beta"]), outs["out"].mat,
                 outs["s"].mat if case["save"] else None, _vec(outs["mean"]) if case["save"] else None,
                 _vec(outs["rstd"]) if case["save"] else None, drop, SID)
    torch.cuda.synchronize()
    scale = _mask(e, rows, H, drop) if drop > 0 else None
    _finish(outs, ins, what)
    got = {k: _val(v) for k, v in outs.items()}
    bounds = P.ln_fwd_bound(inp["x"], inp["y"], scale, inp["gamma"], inp["beta"], EPS, s_stored=got["s"])
    print(what, "worst |err| / bound:", P.check_all(got, bounds, what))


# ---------------------------------------------------------------------------------------------- LayerNorm backward
LN_BWD_CASES = [dict(c, kind="random") for c in
                pairwise(dict(H=LN_H, rows=[1, 15, 16, 17, 37], drop=[0.0, 0.25], defer=[0, 1]))]
LN_BWD_CASES += [dict(H=H, rows=37, drop=(0.0, 0.5)[i % 2], defer=(i // 2) % 2, kind="exact") for i, H in enumerate(LN_H)]
LN_BWD_CASES += [dict(H=H, rows=4100, drop=d, defer=f, kind=k)
                 for H, f in ((64, 0), (1032, 1)) for k, d in (("random", 0.25), ("exact", 0.5))]
LN_BWD_EXACT = ("dgamma", "dbeta", "dbias_prev")


def ln_bwd_inputs(case):
    """dout, s (bf16), mean, rstd, gamma (fp32) on the CPU.  kind "random": mean and rstd are the float64 statistics of
    s, rounded to fp32.  kind "exact": every row of s holds +1 and -1 in equal numbers at random places, mean = 0 and
    rstd = 1 are given, so xh = s exactly; gamma = 1 and dout holds small integers in pairs (v, -v) within the columns
    of either sign, so mean(g) = mean(g xh) = 0, ds = dout exactly, and every term of the three column sums is an
    integer (dropout 0.5: twice one)."""
    H, rows = case["H"], case["rows"]
    g = _gen(11 + H + rows)
    if case["kind"] == "random":
        dout, s = torch.randn(rows, H, generator=g).to(BF), (0.5 + 1.5 * torch.randn(rows, H, generator=g)).to(BF)
        sd = s.double()
        mean = sd.mean(1)
        rstd = (((sd - mean[:, None]) ** 2).mean(1) + EPS) ** -0.5
        gamma, _ = _gamma_beta(g, H, "signed")
        return {"dout": dout, "s": s, "mean": mean.float(), "rstd": rstd.float(), "gamma": gamma}
    perm = torch.rand(rows, H, generator=g).argsort(1)
    v = _ints(g, rows, H // 4)
    half = torch.stack([v, -v], 2).reshape(rows, H // 2)            # (v, -v) pairs: H / 2 is even for every H of LN_H
    w = _ints(g, rows, H // 4)
    pat = torch.cat([half, torch.stack([w, -w], 2).reshape(rows, H // 2)], 1)
    sign = torch.cat([torch.ones(H // 2), -torch.ones(H // 2)])[None].expand(rows, H)
    dout, s = torch.zeros(rows, H), torch.zeros(rows, H)
    dout.scatter_(1, perm, pat)
    s.scatter_(1, perm, sign)
    return {"dout": dout.to(BF), "s": s.to(BF), "mean": torch.zeros(rows), "rstd": torch.ones(rows),
            "gamma": torch.ones(H)}


def _ln_bwd_once(e, case, inp, what):
    H, rows, drop = case["H"], case["rows"], case["drop"]
    ins = {"dout": _G(rows, H, BF, inp["dout"]), "s": _G(rows, H, BF, inp["s"]), "mean": _G(1, rows, F32, inp["mean"]),
           "rstd": _G(1, rows, F32, inp["rstd"]), "gamma": _G(1, H, F32, inp["gamma"])}
    outs = {"ds": _G(rows, H), "dy": _G(rows, H) if drop > 0 else None, "dgamma": _G(1, H, F32), "dbeta": _G(1, H, F32),
            "dbias_prev": _G(1, H, F32)}
    ws = None
    if case["defer"]:
        outs["ws"] = _G(1, e.lib.query("zk_add_ln_bwd_workspace", rows, H) // 4, F32)
        ws = _vec(outs["ws"])
    e.set_seed(SEED)
    red = (_vec(outs["dgamma"]), _vec(outs["dbeta"]), _vec(outs["dbias_prev"]))
    e.add_ln_bwd(ins["dout"].mat, ins["s"].mat, _vec(ins["mean"]), _vec(ins["rstd"]), _vec(ins["gamma"]), outs["ds"].mat,
                 outs["dy"].mat if drop > 0 else None, red[0], red[1], red[2], drop, SID, private_ws=ws)
    if case["defer"]:
        torch.cuda.synchronize()
        assert torch.isnan(outs["dgamma"].value()).all(), what + ": the deferred form wrote dgamma before the reduction"
        e.add_ln_bwd_reduce(ws, rows, H, *red)
    torch.cuda.synchronize()
    scale = _mask(e, rows, H, drop) if drop > 0 else None
    _finish(outs, ins, what)
    got = {k: _val(v) for k, v in outs.items() if k != "ws"}
    bounds = P.ln_bwd_bound(inp["dout"], inp["s"], inp["mean"], inp["rstd"], inp["gamma"], scale, got["ds"], got["dy"])
    print(what, "worst |err| / bound:",
          P.check_all(got, bounds, what, exact=LN_BWD_EXACT if case["kind"] == "exact" else ()))


@pytest.mark.parametrize("case", LN_BWD_CASES, ids=lambda c: "H%d-r%d-d%g-f%d-%s" % tuple(c.values()))
def test_add_ln_bwd(case):
    e, inp = eng(), ln_bwd_inputs(case)
    tune = e.lib.raw("zk_tune")
    old = tune(0, 1)
    try:
        for wide in ((1, 0) if case["H"] <= 512 else (old,)):      # H <= 512: k_add_ln_bwd_wide, then k_add_ln_bwd<1>
            tune(0, wide)
            _ln_bwd_once(e, case, inp, "add_ln_bwd %s tune0=%d" % (case, wide))
    finally:
        tune(0, old)


# ---------------------------------------------------------------------------------------------- cross entropy
CE_T = 6
CE_SHAPES = [(2, 4), (5, 8), (1021, 1024), (4093, 4096), (4096, 4096),              # streaming kernel up to its limit
             (4097, 4100), (16381, 16384), (16384, 16384),                          # reg<4>, first and last
             (16385, 16388), (32765, 32768), (32768, 32768),                        # reg<8>
             (32769, 32772), (70001, 70004)]                                        # streaming, many trips
CE_CASES = [(V, ld, ls) for (V, ld) in CE_SHAPES for ls in (0.0, 0.1)]
CE_ROW_W0, CE_ROW_SPAN, CE_ROW_EQUAL = 4, 2, 3


def ce_inputs(case):
    """logits [T, ld] fp32 (pad columns 777), ids, w on the CPU.  Gold ids are placed: row 0 column 0, row 1 column V - 1,
    row 2 the last column of the last full float4, row 3 the first column of the scalar tail (V % 4 != 0; column 1
    otherwise), row 4 repeats row 2's, row 5 the middle.  Row 2 spans +-30 with its maximum in the last column (in
    the scalar tail when there is one), row 3 is all-equal, row 4 has w = 0."""
    V, ld, ls = case
    g = _gen(13 + V)
    z = torch.full((CE_T, ld), 777.0)
    z[:, :V] = torch.randn(CE_T, V, generator=g) * 3
    span = torch.linspace(-30.0, 30.0, V)[torch.randperm(V, generator=g)]
    i = int(span.argmax())
    span[i], span[V - 1] = span[V - 1].clone(), span[i].clone()
    z[CE_ROW_SPAN, :V] = span
    z[CE_ROW_EQUAL, :V] = 0.5
    V4 = V & ~3
    last4 = max(V4 - 1, 0)
    ids = torch.tensor([0, V - 1, last4, V4 if V % 4 else min(1, V - 1), last4, V // 2], dtype=torch.int32)
    w = 0.1 + 0.9 * torch.rand(CE_T, generator=g)
    w[CE_ROW_W0] = 0.0
    return {"z": z, "ids": ids, "w": w}


@pytest.mark.parametrize("case", CE_CASES, ids=lambda c: "V%d-ld%d-ls%g" % c)
def test_ce_fused(case):
    e, inp = eng(), ce_inputs(case)
    V, ld, ls = case
    what = "ce_fused V=%d ld=%d ls=%g" % case
    ids = inp["ids"].cuda()
    ins = {"logits": _G(CE_T, ld, F32, inp["z"]), "w": _G(1, CE_T, F32, inp["w"])}
    outs = {"ce": _G(1, CE_T, F32), "dl": _G(CE_T, ld), "ce_fwd": _G(1, CE_T, F32)}
    e.ce_fused(ins["logits"].mat, ids, _vec(ins["w"]), _vec(outs["ce"]), outs["dl"].mat, CE_T, V, ls)
    e.ce_fused(ins["logits"].mat, ids, None, _vec(outs["ce_fwd"]), None, CE_T, V, ls)         # the forward-only form
    torch.cuda.synchronize()
    _finish(outs, ins, what)
    assert torch.equal(ids.cpu(), inp["ids"])
    got = {k: _val(v) for k, v in outs.items()}
    t = P.ce_terms(inp["z"], inp["ids"], inp["w"], V, ld, ls)
    print(what, "c_exp needed:", P.ce_c_exp_needed(t, got["ce"], got["dl"]))
    bounds = P.ce_bound(t)
    print(what, "worst |err| / bound:", P.check_all(got, bounds, what),
          P.check_all({"ce": got["ce_fwd"]}, {"ce": bounds["ce"]}, what + " forward only"))
    assert float(got["dl"][:, V:].float().abs().max() if ld > V else 0.0) == 0.0
    assert float(got["dl"][CE_ROW_W0].float().abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------- column sums
COLSUM_CASES = pairwise(dict(rows=[1, 31, 32, 33, 255, 256, 257, 16500], N=[8, 64, 72], strided=[0, 1], skip=[0, 7],
                             acc=[0, 1], drop=[0, 1]))
KINDS = (("random", 0.25), ("exact", 0.5))


def colsum_inputs(rows, N, kind, seed=0, acc=1):
    g = _gen(17 + rows + N + seed)
    if kind == "exact":
        return _ints(g, rows, N).to(BF), (_ints(g, N, lim=100) if acc else None)
    return torch.randn(rows, N, generator=g).to(BF), (torch.randn(N, generator=g) if acc else None)


@pytest.mark.parametrize("case", COLSUM_CASES, ids=lambda c: "r%d-N%d-st%d-sk%d-acc%d-d%d" % tuple(c.values()))
def test_colsum_ex(case):
    e = eng()
    rows, N = case["rows"], case["N"]
    ld, off = (N + 24, 8) if case["strided"] else (N, 0)
    for kind, p in KINDS:
        what = "colsum_ex %s %s" % (case, kind)
        drop = p if case["drop"] else 0.0
        a, prev = colsum_inputs(rows, N, kind, acc=case["acc"])
        A = _G(rows, N, BF, a, ld=ld, off=off)
        out = _G(1, N, F32, prev)
        e.set_seed(SEED)
        e.colsum(A.mat, _vec(out), skip_L=case["skip"], accumulate=bool(case["acc"]), drop_p=drop, sid=SID)
        torch.cuda.synchronize()
        scale = _mask(e, rows, N, drop) if drop > 0 else None
        _finish({"out": out}, {"a": A}, what)
        ref, bound = P.colsum_ref(a, case["skip"], scale, prev)
        print(what, P.check_all({"out": _val(out)}, {"out": (ref, bound)}, what, exact=("out",) if kind == "exact" else ()))


COLSUM_PAIR_CASES = [(300, 40, 7, 3, 64), (40, 300, 0, 7, 72), (300, 40, 7, 0, 8)]      # rows a, rows b, skip a, skip b, N


def colsum_pair_terms(a, ska, sa, b, skb, sb):
    """The terms of both sides as the rows of ONE float64 matrix: the pair is one sum of rows_a + rows_b terms."""
    t = []
    for m, skip, scale in ((a, ska, sa), (b, skb, sb)):
        m = m.double() * (1.0 if scale is None else scale.double())
        if skip > 0:
            m[::skip] = 0
        t.append(m)
    return torch.cat(t, 0)


@pytest.mark.parametrize("case", COLSUM_PAIR_CASES)
def test_colsum_pair(case):
    e = eng()
    ra, rb, ska, skb, N = case
    for kind, p in KINDS:
        for drop in (0.0, p):
            what = "colsum_pair %s %s drop=%g" % (case, kind, drop)
            a, _ = colsum_inputs(ra, N, kind, 1, acc=0)
            b, _ = colsum_inputs(rb, N, kind, 2, acc=0)
            A, B = _G(ra, N, BF, a, ld=N + 8, off=8), _G(rb, N, BF, b)
            out = _G(1, N, F32)
            e.set_seed(SEED)
            e.colsum_pair(A.mat, ska, SID, B.mat, skb, SID + 1, _vec(out), drop_p=drop)
            torch.cuda.synchronize()
            sa = _mask(e, ra, N, drop, SID) if drop > 0 else None
            sb = _mask(e, rb, N, drop, SID + 1) if drop > 0 else None
            _finish({"out": out}, {"a": A, "b": B}, what)
            print(what, P.check_all({"out": _val(out)}, {"out": P.colsum_ref(colsum_pair_terms(a, ska, sa, b, skb, sb))},
                                    what, exact=("out",) if kind == "exact" else ()))


@pytest.mark.parametrize("kind", ["random", "exact"])
def test_reductions_grouped(kind):
    """Three column sums of different rows / N and two sets of LayerNorm partials in the two grouped launches: one set
    written by add_ln_bwd(private_ws), one laid out as zk_gemm_ln_bwd leaves it (a partial row per 64-row block)."""
    e = eng()
    what = "reductions_grouped %s" % kind
    cs, ins, outs = [], {}, {}
    for i, (rows, N, ld, off) in enumerate([(300, 64, 64, 0), (33, 72, 96, 16), (1, 8, 8, 0)]):
        a, _ = colsum_inputs(rows, N, kind, 3 + i, acc=0)
        A, out = _G(rows, N, BF, a, ld=ld, off=off), _G(1, N, F32)
        pw = _G(1, e.lib.raw("zk_colsum_rowchunks")(rows) * N, F32)
        ins["a%d" % i], outs["out%d" % i], outs["pw%d" % i] = A, out, pw
        cs.append((A.mat, _vec(out), _vec(pw)))
    case = dict(H=72, rows=37, drop=0.0, defer=1, kind=kind)
    inp = ln_bwd_inputs(case)
    lin = {k: _G(37, 72, BF, inp[k]) for k in ("dout", "s")}
    lin.update({k: _G(1, inp[k].numel(), F32, inp[k]) for k in ("mean", "rstd", "gamma")})
    lout = {"ds": _G(37, 72), "dgamma": _G(1, 72, F32), "dbeta": _G(1, 72, F32), "dbias_prev": _G(1, 72, F32),
            "ws": _G(1, e.lib.query("zk_add_ln_bwd_workspace", 37, 72) // 4, F32)}
    e.add_ln_bwd(lin["dout"].mat, lin["s"].mat, _vec(lin["mean"]), _vec(lin["rstd"]), _vec(lin["gamma"]), lout["ds"].mat,
                 None, None, None, None, private_ws=_vec(lout["ws"]))
    rows2, H2 = 200, 520
    nblk = (rows2 + 63) // 64
    g = _gen(23)
    part = _ints(g, nblk * 3, H2) if kind == "exact" else torch.randn(nblk * 3, H2, generator=g)
    PT = _G(1, nblk * 3 * H2, F32, part.reshape(1, -1))
    o2 = {"dgamma": _G(1, H2, F32), "dbeta": _G(1, H2, F32)}
    torch.cuda.synchronize()
    lout["ws"].check_guard(what + " ws")
    lout["ws"].rebase()
    e.__dict__.pop("_red_cache", None)        # (keyed by addresses: the buffers of an earlier test may have had these)
    e.reductions_grouped(cs, [(_vec(lout["ws"]), 37, 72, _vec(lout["dgamma"]), _vec(lout["dbeta"]), _vec(lout["dbias_prev"])),
                              (_vec(PT), rows2, H2, _vec(o2["dgamma"]), _vec(o2["dbeta"]), None, True)])
    torch.cuda.synchronize()
    _finish(dict(outs, **{k: v for k, v in lout.items() if k != "ws"}, **{"2" + k: v for k, v in o2.items()}),
            dict(ins, **lin, ws=lout["ws"], partials2=PT), what)
    ex = lambda *names: names if kind == "exact" else ()
    for i in range(3):
        ref, bound = P.colsum_ref(ins["a%d" % i].value())
        P.check_all({"out": _val(outs["out%d" % i])}, {"out": (ref, bound)}, "%s colsum %d" % (what, i), exact=ex("out"))
    got = {k: _val(v) for k, v in lout.items() if k != "ws"}
    bounds = P.ln_bwd_bound(inp["dout"], inp["s"], inp["mean"], inp["rstd"], inp["gamma"], None, got["ds"], None)
    P.check_all(got, bounds, what + " ln partials", exact=ex(*LN_BWD_EXACT))
    p3 = part.double().view(nblk, 3, H2)
    b3 = (nblk + P.C_RED) * P.PER_TERM * p3.abs().sum(0)
    P.check_all({k: _val(v) for k, v in o2.items()}, {"dgamma": (p3[:, 0].sum(0), b3[0]), "dbeta": (p3[:, 1].sum(0), b3[1])},
                what + " gemm_ln_bwd partials", exact=ex("dgamma", "dbeta"))


@pytest.mark.parametrize("n", [1, 255, 100003])
def test_sum_slices(n):
    e = eng()
    for kind in ("random", "exact"):
        for nsl in (1, 3):
            for acc in (0, 1):
                what = "sum_slices n=%d nslices=%d acc=%d %s" % (n, nsl, acc, kind)
                g = _gen(29 + n + nsl)
                mk = (lambda *s: _ints(g, *s)) if kind == "exact" else (lambda *s: torch.randn(*s, generator=g))
                x, prev = mk(nsl, n), mk(1, n)
                X = _G(nsl, n, F32, x, ld=n + 5, off=3)                       # stride > n
                out = _G(1, n, F32, prev if acc else None)
                e.lib.call("zk_sum_slices", _vec(out).data_ptr(), X.mat.ptr, nsl, n, n + 5, acc, e.stream)
                torch.cuda.synchronize()
                _finish({"out": out}, {"in": X}, what)
                t = torch.cat([x, prev], 0).double() if acc else x.double()
                P.check_all({"out": _val(out)}, {"out": (t.sum(0), (nsl + P.C_RED) * P.PER_TERM * t.abs().sum(0))}, what,
                            exact=("out",) if kind == "exact" else ())


# ---------------------------------------------------------------------------------------------- loss tail
LOSS_B = [1, 15, 16, 17, 257, 4096, 4097]           # 4097: k_per_sample + k_mean whatever tuning key 16 says
LOSS_L = [1, 64, 65, 130]
ULP2 = 2 * 2.0 ** -23                                # 2 ulp, relative


def loss_inputs(B, L, kind):
    """ids [B, L] with ragged padding (every sentence keeps at least one token), ce [B, L] of small integers (777 under
    the padding).  kind "flat": ce = k_b +- 1 in pairs, so the sentence's sum is k_b len and per_sample = k_b exactly;
    kind "ragged": any integers, so most divisions are inexact."""
    g = _gen(31 + B + L)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    t = torch.arange(L)[None]
    live = t < lens[:, None]
    ids = torch.where(live, torch.randint(1, 1000, (B, L), generator=g), torch.zeros(B, L, dtype=torch.long)).int()
    if kind == "flat":
        k = torch.randint(1, 8, (B, 1), generator=g).float()
        alt = torch.where(t % 2 == 0, 1.0, -1.0) * (t < (lens[:, None] // 2 * 2)).float()
        ce = k + alt
    else:
        ce = _ints(g, B, L)
    return ids, torch.where(live, ce, torch.full((B, L), 777.0)), live


def _near(got, ref64, what):
    """Bit for bit where the float64 value is an fp32 number, within 2 ulp elsewhere."""
    ref64 = ref64.reshape(got.shape)
    exact = ref64.float().double() == ref64
    P.assert_elementwise(got, ref64, torch.where(exact, torch.zeros_like(ref64), ULP2 * ref64.abs()), what)


@pytest.mark.parametrize("B", LOSS_B)
def test_loss_tail(B):
    e = eng()
    tune = e.lib.raw("zk_tune")
    old = tune(16, 0)
    try:
        for L in LOSS_L:
            for kind in ("flat", "ragged"):
                ids_c, ce_c, live = loss_inputs(B, L, kind)
                ids = ids_c.cuda()
                n = live.double().sum(1)
                # target_stats: the mask exactly, w = loss_scale mask / (len B): a product and a quotient
                what = "target_stats B=%d L=%d" % (B, L)
                M, W = _G(B, L, F32), _G(B, L, F32)
                e.target_stats(ids, M.window(), W.window(), B, L, 2.0)
                torch.cuda.synchronize()
                _finish({"mask": M, "w": W}, {}, what)
                P.assert_exact(M.value(), live.double(), what + " mask")
                wref = 2.0 * live.double() / (n[:, None] * B)
                P.assert_elementwise(W.value(), wref, ULP2 * wref.abs(), what + " w")
                for two in ((0, 1) if B <= 4096 else (0,)):
                    tune(16, two)
                    what = "loss_reduce B=%d L=%d %s key16=%d" % (B, L, kind, two)
                    CE = _G(1, B * L, F32, ce_c.reshape(1, -1))
                    ps, loss = _G(1, B, F32), _G(1, 1, F32)
                    e.loss_reduce(_vec(CE), ids, _vec(ps), _vec(loss), B, L)
                    torch.cuda.synchronize()
                    _finish({"per_sample": ps, "loss": loss}, {"ce": CE}, what)
                    assert torch.equal(ids.cpu(), ids_c)
                    psum = (ce_c.double() * live.double()).sum(1)
                    _near(_val(ps), psum / n, what + " per_sample")
                    stored = _val(ps).double()
                    if kind == "flat":                       # the per-sentence values are small integers: an exact sum
                        _near(_val(loss), stored.sum(0, keepdim=True) / B, what + " loss")
                    else:
                        P.assert_elementwise(_val(loss), stored.mean(0, keepdim=True),
                                             (B + P.C_RED) * P.PER_TERM * stored.abs().mean(0, keepdim=True), what + " loss")
    finally:
        tune(16, old)
