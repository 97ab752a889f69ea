"""Element-wise parity of the embedding, average-attention and optimiser kernels of zero_amd/csrc/zk_elem.hip against
float64 references with the derived bounds of tests/parity_elem.py, on guarded operands: every output is a NaN-prefilled
window between two guard bands (a gradient table: a finite sentinel, so that a row nobody may write keeps its bits),
every input is compared bit for bit after the call.  The dropout scale is what zk_dropout_mask gives for the engine's seed
and the site: the forward output and both backward forms of the embedding must agree with ONE such tensor of rows x H.

Sums run twice where one lost or doubled term could hide under the worst-case bound: on random values, and on small
integers (|v| <= 8, dropout 0.5 so that the scale 2 keeps them integers, H = 64 so that sqrt(H) = 8 is exact) where the
fp32 result is the float64 one.

Which case reaches which kernel:
  k_embed_fwd          one live lane at H = 8; part-filled, full and repeated 512-column trips of a wave at H = 504, 512,
                       520, 1024; 8200 rows at H = 8 repeat the wave-stride row loop (2048 blocks x 4 waves); pos0 as an
                       argument and through pos0_dev (the argument is then a wrong value); zero_flag unset, 0 and 1
  k_embed_fwd_pair     La != Lb: side b's rows start at B La, each side has its own site
  k_embed_bwd_sorted   runs of 1, 16, 17, 64, 65 and 150 rows of one id: one and two 64-index loads, full and part-filled
                       16-row batches; ids absent from the batch; k_embed_bwd_sorted_pair: blockIdx.y = the side
  k_embed_bwd          the atomic form (dtable and dbias are added to)
  k_aan_fwd, k_aan_bwd, k_cumavg_add_fwd, k_cumavg_bwd
                       L < 4 and L = 5, 9: empty trailing segments; L = 5, 7, 130: the last live segment shorter than the
                       others; L = 4, 8, 64: equal segments; H = 520, 1024: blockIdx.y = 1; H = 8, 504, 520: dead lanes in the last block
                       that must still reach the barrier; zk_aan_bwd flags 0 .. 3 (bit 1: dcat[:, H:] must not be read)
  k_aan_gate_fwd / bwd a part-filled last block (5 x 8, 7 x 520), several blocks (33 x 64, 3 x 1024)
  k_adam<true, U, true> U = 1, 2, 4 (tuning key 9), k_adam<true, 1, false> (key 9 = 0), block counts of key 10, the
                       non-temporal bits of key 18; k_norm_final2; k_adam<false> + k_norm_final through zk_adam_step
                       (norm_free = 0) and zk_adam; k_sumsq_partial + k_norm_final (zk_l2norm); k_norm_flag; k_ema; k_axpy_f32;
                       k_cast_bf16_f32.  The sizes are chosen for the partition edges (ADAM_SIZES).

The case lists and the operand builders are plain CPU code: tests/test_elemkernel_checker.py imports them.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng  # noqa: E402
from tests import parity as P  # noqa: E402
from tests import parity_elem as PE  # noqa: E402
from tests.parity import guarded, pairwise  # noqa: E402
from zero_amd.func import timing_table  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
SEED, SID = 4321, 11


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def _ints(g, *shape, lim=8):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def _G(rows, cols, dtype=BF, prefill=None):
    return guarded(rows, cols, None, 0, dtype, prefill, "cuda")


def _ptr(g):
    return g.window().data_ptr()


def _val(g):
    return g.value().view(-1) if g.rows == 1 else g.value()


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


# ---------------------------------------------------------------------------------------------- embedding forward
EMB_V = 50
EMB_H = [8, 64, 504, 512, 520, 1024]
EMB_FWD_CASES = pairwise(dict(H=EMB_H, shift=[0, 1], pos=[(0, "arg"), (4, "arg"), (0, "dev"), (4, "dev")],
                              zf=[None, 0, 1], drop=[0.0, 0.25]))
for _c in EMB_FWD_CASES:
    _c.update(B=3, L=7)
EMB_FWD_CASES.append(dict(H=8, shift=1, pos=(4, "dev"), zf=0, drop=0.25, B=200, L=41))      # 8200 rows
EMB_MAX_POS = 8


def _emb_id(c):
    return "H%d-s%d-p%d%s-z%s-d%g-r%d" % (c["H"], c["shift"], c["pos"][0], c["pos"][1], c["zf"], c["drop"], c["B"] * c["L"])


def embed_inputs(H, B, L, V=EMB_V, seed=0, kind="random"):
    """ids [B, L], the bf16 table [V, H], the fp32 bias, a gradient dout [B L, H] (bf16; small integers in kind "exact")."""
    g = _gen(41 + H + B * L + seed)
    ids = torch.randint(0, V, (B, L), generator=g)
    dout = _ints(g, B * L, H) if kind == "exact" else torch.randn(B * L, H, generator=g)
    return {"ids": ids, "table": torch.randn(V, H, generator=g).to(BF), "bias": torch.randn(H, generator=g),
            "dout": dout.to(BF)}


def cpu_timing(H):
    """The table Engine.timing hands to the kernel (the tests treat it as data)."""
    return torch.from_numpy(timing_table(256, H))


@pytest.mark.parametrize("case", EMB_FWD_CASES, ids=_emb_id)
def test_embed_fwd(case):
    e = eng()
    H, B, L, drop, (pos0, via) = case["H"], case["B"], case["L"], case["drop"], case["pos"]
    inp = embed_inputs(H, B, L)
    what = "embed_fwd %s" % _emb_id(case)
    ins = {"table": _G(EMB_V, H, BF, inp["table"]), "bias": _G(1, H, F32, inp["bias"])}
    out = _G(B * L, H)
    ids = inp["ids"].int().cuda()
    flag = None if case["zf"] is None else torch.tensor([case["zf"]], dtype=torch.int32, device="cuda")
    pdev = torch.tensor([pos0], dtype=torch.int32, device="cuda") if via == "dev" else None
    tim = e.timing(EMB_MAX_POS + L, H)
    tim0 = tim.cpu().clone()
    e.set_seed(SEED)
    e.embed_fwd(ids, ins["table"].window(), ins["bias"].window(), out.mat, B, L, H, shift=bool(case["shift"]),
                pos0=pos0 if via == "arg" else 2, zero_flag=flag, drop_p=drop, sid=SID, pos0_dev=pdev, max_pos=EMB_MAX_POS)
    torch.cuda.synchronize()
    dm = _mask(e, B * L, H, drop) if drop > 0 else None
    _finish({"out": out}, ins, what)
    assert torch.equal(ids.cpu().long(), inp["ids"]) and torch.equal(e.timing(EMB_MAX_POS + L, H).cpu(), tim0)
    bounds = PE.embed_fwd_bound(inp["ids"], inp["table"], inp["bias"], tim0, PE.embed_scale(H), case["shift"], pos0,
                                bool(case["zf"]), dm)
    print(what, "worst |err| / bound:", P.check_all({"out": _val(out)}, bounds, what))


EMB_PAIR_CASES = [(64, 5, 9, 0.25), (520, 9, 5, 0.25), (8, 7, 3, 0.0), (1024, 3, 7, 0.25)]      # H, La, Lb, dropout


@pytest.mark.parametrize("case", EMB_PAIR_CASES)
def test_embed_fwd_pair(case):
    """Side a is the encoder input, side b the shifted decoder input; each against the mask of its own site."""
    e = eng()
    H, La, Lb, drop = case
    B = 3
    a, b = embed_inputs(H, B, La, seed=1), embed_inputs(H, B, Lb, seed=2)
    what = "embed_fwd_pair %s" % (case,)
    ins = {"table_a": _G(EMB_V, H, BF, a["table"]), "table_b": _G(EMB_V, H, BF, b["table"]), "bias": _G(1, H, F32, a["bias"])}
    outs = {"out_a": _G(B * La, H), "out_b": _G(B * Lb, H)}
    ida, idb = a["ids"].int().cuda(), b["ids"].int().cuda()
    tim0 = e.timing(max(La, Lb), H).cpu().clone()
    e.set_seed(SEED)
    e.embed_fwd_pair(ida, ins["table_a"].window(), outs["out_a"].mat, La, SID, idb, ins["table_b"].window(),
                     outs["out_b"].mat, Lb, SID + 1, ins["bias"].window(), B, H, drop_p=drop)
    torch.cuda.synchronize()
    dma = _mask(e, B * La, H, drop, SID) if drop > 0 else None
    dmb = _mask(e, B * Lb, H, drop, SID + 1) if drop > 0 else None
    _finish(outs, ins, what)
    sc = PE.embed_scale(H)
    for side, x, L, shift, dm in (("a", a, La, 0, dma), ("b", b, Lb, 1, dmb)):
        bounds = PE.embed_fwd_bound(x["ids"], x["table"], a["bias"], tim0, sc, shift, 0, False, dm)
        print(what, side, P.check_all({"out": _val(outs["out_" + side])}, bounds, "%s side %s" % (what, side)))


# ---------------------------------------------------------------------------------------------- embedding backward
EMB_BWD_V = 40
EMB_RUNS = {3: 1, 4: 16, 5: 17, 6: 64, 7: 65, 8: 150}          # id -> rows that carry it; ids 0 .. 2, 9, 30 .. 39 are absent
EMB_BWD_CASES = [dict(c, kind="random") for c in pairwise(dict(H=[8, 64, 520, 1024], shift=[0, 1], acc=[0, 1], drop=[0.0, 0.5]))]
EMB_BWD_CASES += [dict(H=64, shift=s, acc=a, drop=0.5, kind="exact") for s, a in ((0, 0), (1, 1))]
EMB_BWD_PAIR_CASES = [(64, 0.5, 0, 1, "exact"), (520, 0.0, 1, 0, "random"), (8, 0.5, 1, 1, "random")]   # H, drop, acc a, acc b


def embed_run_ids(shift, seed=0):
    """ids [24, 14] (shift: [24, 15], whose last column no row carries) in which the rows that HAVE an embedding carry the
    runs of EMB_RUNS at random places and ids 10 .. 29 elsewhere."""
    g = _gen(53 + seed)
    B, Lc = 24, 14
    carried = torch.cat([torch.full((n,), i) for i, n in EMB_RUNS.items()])
    fill = torch.randint(10, 30, (B * Lc - carried.numel(),), generator=g)
    flat = torch.cat([carried, fill])[torch.randperm(B * Lc, generator=g)].view(B, Lc)
    if shift:
        flat = torch.cat([flat, torch.randint(10, 30, (B, 1), generator=g)], 1)
    return flat


def embed_bwd_inputs(H, shift, kind, seed=0):
    """ids, dout (bf16) and the table before the call: a finite sentinel per element (integers in kind "exact")."""
    ids = embed_run_ids(shift, seed)
    g = _gen(59 + H + seed)
    rows = ids.numel()
    if kind == "exact":
        return {"ids": ids, "dout": _ints(g, rows, H).to(BF), "prev": _ints(g, EMB_BWD_V, H, lim=100) + 0.5}
    return {"ids": ids, "dout": torch.randn(rows, H, generator=g).to(BF), "prev": 0.75 + 0.25 * torch.randn(EMB_BWD_V, H, generator=g)}


def _check_table(got, bounds, what, kind):
    return P.check_all(got, bounds, what, exact=tuple(bounds) if kind == "exact" else ())


@pytest.mark.parametrize("case", EMB_BWD_CASES, ids=lambda c: "H%d-s%d-a%d-d%g-%s" % tuple(c.values()))
def test_embed_bwd_sorted(case):
    from tests.common import device_sort_arrays
    e = eng()
    H, shift, acc, drop, kind = case["H"], case["shift"], case["acc"], case["drop"], case["kind"]
    inp = embed_bwd_inputs(H, shift, kind)
    rows = inp["ids"].numel()
    what = "embed_bwd_sorted %s" % (case,)
    srt = device_sort_arrays(e, "pe%d" % shift, inp["ids"].numpy(), bool(shift))
    dout, dtab = _G(rows, H, BF, inp["dout"]), _G(EMB_BWD_V, H, F32, inp["prev"])
    e.set_seed(SEED)
    e.embed_bwd_sorted(srt, dout.mat, dtab.window(), H, accumulate=bool(acc), drop_p=drop, sid=SID)
    torch.cuda.synchronize()
    dm = _mask(e, rows, H, drop) if drop > 0 else None
    _finish({"dtable": dtab}, {"dout": dout}, what)
    bounds = PE.embed_bwd_bound(inp["ids"], inp["dout"], EMB_BWD_V, PE.embed_scale(H), shift, dm, inp["prev"], acc)
    print(what, _check_table({"dtable": _val(dtab)}, bounds, what, kind))
    rid = PE.embed_row_ids(inp["ids"], shift)
    absent = torch.bincount(rid[rid >= 0], minlength=EMB_BWD_V) == 0
    assert int(absent.sum()) >= 10
    P.assert_exact(_val(dtab)[absent], inp["prev"].double()[absent], what + " [rows of absent ids]")


@pytest.mark.parametrize("case", EMB_BWD_PAIR_CASES)
def test_embed_bwd_sorted_pair(case):
    from tests.common import device_sort_arrays
    e = eng()
    H, drop, acc_a, acc_b, kind = case
    a, b = embed_bwd_inputs(H, 0, kind, 1), embed_bwd_inputs(H, 1, kind, 2)
    what = "embed_bwd_sorted_pair %s" % (case,)
    sa = device_sort_arrays(e, "ppa", a["ids"].numpy(), False)
    sb = device_sort_arrays(e, "ppb", b["ids"].numpy(), True)
    ins = {"dout_a": _G(a["ids"].numel(), H, BF, a["dout"]), "dout_b": _G(b["ids"].numel(), H, BF, b["dout"])}
    outs = {"dtable_a": _G(EMB_BWD_V, H, F32, a["prev"]), "dtable_b": _G(EMB_BWD_V, H, F32, b["prev"])}
    e.set_seed(SEED)
    e.embed_bwd_sorted_pair(sa, ins["dout_a"].mat, outs["dtable_a"].window(), bool(acc_a), SID, sb, ins["dout_b"].mat,
                            outs["dtable_b"].window(), bool(acc_b), SID + 1, H, drop_p=drop)
    torch.cuda.synchronize()
    _finish(outs, ins, what)
    sc = PE.embed_scale(H)
    for side, x, shift, acc, sid in (("a", a, 0, acc_a, SID), ("b", b, 1, acc_b, SID + 1)):
        dm = _mask(e, x["ids"].numel(), H, drop, sid) if drop > 0 else None
        bounds = PE.embed_bwd_bound(x["ids"], x["dout"], EMB_BWD_V, sc, shift, dm, x["prev"], acc)
        print(what, side, _check_table({"dtable": _val(outs["dtable_" + side])}, bounds, "%s side %s" % (what, side), kind))


EMB_ATOMIC_CASES = [(H, s, d) for H in (64, 520) for s in (0, 1) for d in (0.0, 0.25)]
EMB_ATOMIC_V, EMB_ATOMIC_B, EMB_ATOMIC_L = 23, 3, 7


@pytest.mark.parametrize("case", EMB_ATOMIC_CASES)
def test_embed_fwd_and_both_backward_forms_share_one_mask(case):
    """The forward output, the atomic gradient (zk_embed_bwd, with dbias) and the sorted gradient at one seed and site
    against ONE zk_dropout_mask tensor of rows x H elements."""
    from tests.common import device_sort_arrays
    e = eng()
    H, shift, drop = case
    B, L, V = EMB_ATOMIC_B, EMB_ATOMIC_L, EMB_ATOMIC_V
    inp = embed_inputs(H, B, L, V, seed=3)
    g = _gen(61 + H)
    prev, prev_b = 0.75 + 0.25 * torch.randn(V, H, generator=g), torch.randn(H, generator=g)
    what = "embed atomic %s" % (case,)
    ids = inp["ids"].int().cuda()
    ins = {"table": _G(V, H, BF, inp["table"]), "bias": _G(1, H, F32, inp["bias"]), "dout": _G(B * L, H, BF, inp["dout"])}
    outs = {"out": _G(B * L, H), "dtable": _G(V, H, F32, prev), "dbias": _G(1, H, F32, prev_b), "dtable_sorted": _G(V, H, F32, prev)}
    srt = device_sort_arrays(e, "pat%d" % shift, inp["ids"].numpy(), bool(shift))
    tim0 = e.timing(L, H).cpu().clone()
    e.set_seed(SEED)
    e.embed_fwd(ids, ins["table"].window(), ins["bias"].window(), outs["out"].mat, B, L, H, shift=bool(shift), drop_p=drop, sid=SID)
    e.embed_bwd(ids, ins["dout"].mat, outs["dtable"].window(), outs["dbias"].window(), B, L, H, shift=bool(shift), drop_p=drop, sid=SID)
    e.embed_bwd_sorted(srt, ins["dout"].mat, outs["dtable_sorted"].window(), H, accumulate=True, drop_p=drop, sid=SID)
    torch.cuda.synchronize()
    dm = _mask(e, B * L, H, drop) if drop > 0 else None
    _finish(outs, ins, what)
    sc = PE.embed_scale(H)
    got = {k: _val(v) for k, v in outs.items()}
    print(what, P.check_all(got, PE.embed_fwd_bound(inp["ids"], inp["table"], inp["bias"], tim0, sc, shift, 0, False, dm), what))
    bounds = PE.embed_bwd_bound(inp["ids"], inp["dout"], V, sc, shift, dm, prev, 1, prev_b)
    print(what, P.check_all(got, bounds, what + " atomic"),
          P.check_all({"dtable": got["dtable_sorted"]}, {"dtable": bounds["dtable"]}, what + " sorted"))


# ---------------------------------------------------------------------------------------------- average-attention scan
SCAN_L = [1, 2, 3, 4, 5, 7, 8, 9, 64, 130]
SCAN_H = [8, 64, 504, 512, 520, 1024]
SCAN_CASES = [(L, H) for L in SCAN_L for H in SCAN_H]
SCAN_B = 4
SCAN_EXACT = (130, 520)               # the integer runs: two column blocks, dead lanes in the second
DC2_POISON = 30000.0                  # dcat[:, H:] under flag bit 1: finite, and 1e4 times anything the result may hold


def scan_inputs(L, H, kind="random"):
    """bf16 operands of every scan kernel at one shape: x (also vq and dy), att, and dcat [T, 2 H], dxg, dyg, ds."""
    g = _gen(67 + 1000 * L + H)
    T = SCAN_B * L
    mk = (lambda *s: _ints(g, *s).to(BF)) if kind == "exact" else (lambda *s: torch.randn(*s, generator=g).to(BF))
    return {k: mk(T, 2 * H if k == "dcat" else H) for k in ("x", "att", "dcat", "dxg", "dyg", "ds")}


def scan_bwd_case(L, H, kind, use_mask):
    """The operands and the mask of a backward run.  kind "exact" must keep every quotient w / den exact: without
    use_mask the masks count 0, 1 or 2 live steps (PE.scan_masks_dyadic: every step of every segment counts); under
    use_mask the usual masks, and the incoming gradient is 0 wherever the count is not a power of two (the steps that
    remain lie in all four segments, so a segment's carry from the ones behind it shows)."""
    inp = scan_inputs(L, H, kind)
    if kind != "exact":
        return inp, PE.scan_masks(L)
    if not use_mask:
        return inp, PE.scan_masks_dyadic(L)
    mask = PE.scan_masks(L)
    cnt = mask.cumsum(1).clamp_min(1)
    pow2 = (cnt == 2 ** torch.log2(cnt).round()).reshape(-1, 1).to(BF)
    inp["x"], inp["dyg"] = inp["x"] * pow2, inp["dyg"] * pow2
    inp["dcat"][:, H:] = inp["dcat"][:, H:] * pow2
    return inp, mask


def _aan_fwd(e, L, H, kind):
    inp, mask = scan_inputs(L, H, kind), PE.scan_masks(L)
    T = SCAN_B * L
    for use_mask in (0, 1):
        what = "aan_fwd L=%d H=%d use_mask=%d %s" % (L, H, use_mask, kind)
        ins = {"x": _G(T, H, BF, inp["x"]), "mask": _G(SCAN_B, L, F32, mask)}
        cat = _G(T, 2 * H)
        e.aan_fwd(ins["x"].mat, ins["mask"].window(), cat.mat, SCAN_B, L, H, use_mask)
        torch.cuda.synchronize()
        _finish({"cat": cat}, ins, what)
        got = _val(cat)
        P.assert_exact(got[:, :H], inp["x"].double(), what + " [cat_x]")
        ref, bound = PE.scan_fwd_bound(inp["x"], mask, use_mask, exact=kind == "exact")
        print(what, P.check_all({"avg": got[:, H:]}, {"avg": (ref, bound)}, what))


def _cumavg(e, L, H, kind):
    inp = scan_inputs(L, H, kind)
    T = SCAN_B * L
    mask = PE.scan_masks(L)
    for alias in (0, 1):
        what = "cumavg_add_fwd L=%d H=%d alias=%d %s" % (L, H, alias, kind)
        ins = {"vq": _G(T, H, BF, inp["x"]), "mask": _G(SCAN_B, L, F32, mask)}
        att = _G(T, H, BF, inp["att"])
        out = att if alias else _G(T, H)
        e.cumavg_add_fwd(ins["vq"].mat, ins["mask"].window(), att.mat, out.mat, SCAN_B, L, H)
        torch.cuda.synchronize()
        _finish({"out": out}, dict(ins, **({} if alias else {"att": att})), what)
        ref, bound = PE.scan_fwd_bound(inp["x"], mask, 1, att=inp["att"], exact=kind == "exact")
        print(what, P.check_all({"out": _val(out)}, {"out": (ref, bound)}, what))
    inp, mask = scan_bwd_case(L, H, kind, 1)
    what = "cumavg_bwd L=%d H=%d %s" % (L, H, kind)
    ins = {"dy": _G(T, H, BF, inp["x"]), "mask": _G(SCAN_B, L, F32, mask)}
    dvq = _G(T, H)
    e.cumavg_bwd(ins["dy"].mat, ins["mask"].window(), dvq.mat, SCAN_B, L, H)
    torch.cuda.synchronize()
    _finish({"dvq": dvq}, ins, what)
    ref, bound = PE.scan_bwd_bound(inp["x"], inp["x"].double().abs(), mask, 1, exact=kind == "exact")
    print(what, P.check_all({"dvq": _val(dvq)}, {"dvq": (ref, bound)}, what))


def aan_bwd_operands(inp, H, flags):
    """dcat as the kernel gets it: under flag bit 1 its second half holds DC2_POISON."""
    dcat = inp["dcat"].clone()
    if flags & 2:
        dcat[:, H:] = DC2_POISON
    return dcat


def _aan_bwd(e, L, H, kind):
    T = SCAN_B * L
    for flags in (0, 1, 2, 3):
        inp, mask = scan_bwd_case(L, H, kind, flags & 1)
        what = "aan_bwd L=%d H=%d flags=%d %s" % (L, H, flags, kind)
        dcat = aan_bwd_operands(inp, H, flags)
        ins = {"dcat": _G(T, 2 * H, BF, dcat), "dxg": _G(T, H, BF, inp["dxg"]), "dyg": _G(T, H, BF, inp["dyg"]),
               "ds": _G(T, H, BF, inp["ds"]), "mask": _G(SCAN_B, L, F32, mask)}
        dx = _G(T, H)
        e.lib.call("zk_aan_bwd", ins["dcat"].mat.ptr, ins["dxg"].mat.ptr, ins["dyg"].mat.ptr, ins["ds"].mat.ptr,
                   _ptr(ins["mask"]), dx.mat.ptr, SCAN_B, L, H, flags, e.stream)
        torch.cuda.synchronize()
        _finish({"dx": dx}, ins, what)
        g, gmag = PE.aan_bwd_g(inp["dyg"], dcat, H, flags)
        ref, bound = PE.scan_bwd_bound(g, gmag, mask, flags & 1, extra=(inp["ds"], inp["dxg"], dcat[:, :H]), exact=kind == "exact")
        print(what, P.check_all({"dx": _val(dx)}, {"dx": (ref, bound)}, what))


@pytest.mark.parametrize("L,H", SCAN_CASES)
def test_aan_fwd(L, H):
    _aan_fwd(eng(), L, H, "random")


@pytest.mark.parametrize("L,H", SCAN_CASES)
def test_aan_bwd(L, H):
    _aan_bwd(eng(), L, H, "random")


@pytest.mark.parametrize("L,H", SCAN_CASES)
def test_cumavg_add_fwd_and_bwd(L, H):
    _cumavg(eng(), L, H, "random")


def test_scans_on_small_integers():
    """Every running sum is exact (the backward runs keep every quotient exact too: scan_bwd_case): one lost or doubled step at a segment boundary shows."""
    e = eng()
    L, H = SCAN_EXACT
    _aan_fwd(e, L, H, "exact")
    _aan_bwd(e, L, H, "exact")
    _cumavg(e, L, H, "exact")


# ---------------------------------------------------------------------------------------------- average-attention gate
GATE_CASES = [(5, 8), (33, 64), (7, 520), (3, 1024)]
GATE_ROW = 1                                      # the row of special z
GATE_Z = [0.0, 20.0, -20.0, 90.0, -90.0]


def gate_inputs(rows, H):
    """z = [z_i | z_f] from randn * 3, cat = [x | y], dg (bf16).  Row GATE_ROW holds every pair of GATE_Z values."""
    g = _gen(71 + rows + H)
    z = torch.randn(rows, 2 * H, generator=g) * 3
    c = torch.arange(H)
    vals = torch.tensor(GATE_Z)
    z[GATE_ROW, :H], z[GATE_ROW, H:] = vals[c % 5], vals[(c // 5 + c) % 5]
    return {"z": z.to(BF), "cat": torch.randn(rows, 2 * H, generator=g).to(BF), "dg": torch.randn(rows, H, generator=g).to(BF)}


@pytest.mark.parametrize("rows,H", GATE_CASES)
def test_aan_gate(rows, H):
    e, inp = eng(), gate_inputs(rows, H)
    what = "aan_gate rows=%d H=%d" % (rows, H)
    ins = {"z": _G(rows, 2 * H, BF, inp["z"]), "cat": _G(rows, 2 * H, BF, inp["cat"]), "dg": _G(rows, H, BF, inp["dg"])}
    outs = {"out": _G(rows, H), "dz": _G(rows, 2 * H), "dxg": _G(rows, H), "dyg": _G(rows, H)}
    e.aan_gate_fwd(ins["z"].mat, ins["cat"].mat, outs["out"].mat, rows, H)
    e.aan_gate_bwd(ins["dg"].mat, ins["z"].mat, ins["cat"].mat, outs["dz"].mat, outs["dxg"].mat, outs["dyg"].mat, rows, H)
    torch.cuda.synchronize()
    _finish(outs, ins, what)
    got = {k: _val(v) for k, v in outs.items()}
    t = PE.gate_terms(inp["z"], inp["cat"], inp["dg"])
    print(what, "c needed:", PE.gate_c_needed(t, got))
    print(what, "worst |err| / bound:", P.check_all(got, PE.gate_bound(t), what))


# ---------------------------------------------------------------------------------------------- optimiser
# (n, tuning key 10): each size is chosen for a partition edge, with the block count g = min(flat_grid, key 10)
ADAM_SIZES = [(1, 512), (3, 512),                        # the tail alone, n4 = 0
              (4, 512), (1027, 512),
              (4 * 1537 + 2, 3),                         # the last block's range holds one float4
              (4 * (512 * 256 + 1) + 3, 512),            # per_block rounds up to 512: half of the blocks have an empty range
              (4 * (2048 * 256 + 5) + 1, 0)]             # the grid-stride loop repeats past the 2048-block cap
ADAM_LARGEST = ADAM_SIZES[-1][0]
ADAM_KEYS = {9: [0, 1, 2, 4], 10: [0, 3, 512], 18: [0, 1, 2, 3, 4, 7]}
ADAM_DEFAULT = {9: 2, 10: 512, 18: 3}
HYPER = [0.05, 0.9, 0.98, 1e-8, 0.5, 1e-3, 777.0, 5.0, 0.999, 0.0, 3.0, 0.0]
# lr, b1, b2, eps, grad_scale, clip (below every gradient norm here; the norm-free path must not look at it), gnorm (in: garbage
# on the norm-free path), the flag (garbage), EMA decay, the
# safe_nan bound, the sticky count, unused.  lr is large so that the parameter norm before and after the update differ
# by far more than the bound of the norm.


def adam_variants(n, key10):
    """(key 9, key 10, key 18): the pairing ADAM_SIZES names first (key 9 = 0 at the largest n: the grid-stride form), then
    the full cross product -- at the largest n each key's values with the others at their defaults."""
    first = (0 if n == ADAM_LARGEST else ADAM_DEFAULT[9], key10, ADAM_DEFAULT[18])
    if n == ADAM_LARGEST:
        rest = [tuple(v if k == key else ADAM_DEFAULT[k] for k in (9, 10, 18)) for key in (9, 10, 18) for v in ADAM_KEYS[key]]
    else:
        rest = [(a, b, c) for a in ADAM_KEYS[9] for b in ADAM_KEYS[10] for c in ADAM_KEYS[18]]
    return [first] + [v for v in dict.fromkeys(rest) if v != first]


def adam_inputs(n, seed=0):
    """p, g, m, v (fp32).  With n >= 3 two of the last elements are special: one has g = m = v = 0, the one before it g = 0
    and m != 0 (the last two, inside the n % 4 tail where it has more than one element; a one-element tail stays an
    ordinary element and the two lie in front of it).  So have the elements i % 11 == 5 and i % 11 == 7; i % 101 == 9:
    g = v = 0, m != 0 (an update of lr b1 m / eps)."""
    g_ = _gen(73 + n % 100003 + seed)
    p = torch.randn(n, generator=g_)
    g = torch.randn(n, generator=g_) * 0.1
    m = (torch.rand(n, generator=g_) - 0.3) * 0.01
    v = torch.rand(n, generator=g_) * 0.001 + 1e-6
    i = torch.arange(n)
    zero, g0, v0 = i % 11 == 5, i % 11 == 7, i % 101 == 9
    if n >= 3:
        z = n - 2 if n % 4 == 1 else n - 1
        zero[z - 1:z + 1], g0[z - 1:z + 1], v0[z - 1:z + 1] = False, False, False
        zero[z], g0[z - 1] = True, True
    g[zero | g0 | v0] = 0
    m[zero] = 0
    v[zero | v0] = 0
    return {"p": p, "g": g, "m": m, "v": v, "zero": zero}


class AdamBuffers(object):
    """The five 1 x n guarded windows and the small words; reset() puts the first content back."""

    def __init__(self, e, n, inp, hyper=HYPER):
        self.e, self.n = e, n
        self.G = {k: _G(1, n, F32, inp[k].reshape(1, n)) for k in ("p", "g", "m", "v")}
        self.G["shadow"] = _G(1, n, BF)
        self.hyper0 = torch.tensor(hyper, dtype=F32)
        self.hyper = self.hyper0.cuda()
        self.pn = torch.full((1,), float("nan"), device="cuda")
        self.seed = torch.tensor([1234567], dtype=torch.int64, device="cuda")
        self.ws = torch.empty(max(e.lib.query("zk_adam_step_workspace"), e.lib.query("zk_norm_workspace")), dtype=torch.uint8, device="cuda")

    def reset(self, hyper=None):
        for g in self.G.values():
            g.t.copy_(g.before.view(g.dtype))
        self.hyper.copy_(self.hyper0 if hyper is None else torch.tensor(hyper, dtype=F32))
        self.pn.fill_(float("nan"))
        self.seed.fill_(1234567)

    def step(self, norm_free, with_seed=True):
        p = {k: _ptr(g) for k, g in self.G.items()}
        self.e.lib.call("zk_adam_step", p["p"], p["g"], p["m"], p["v"], p["shadow"], self.n, self.hyper.data_ptr(),
                        self.pn.data_ptr(), self.seed.data_ptr() if with_seed else None, norm_free, None, self.ws.data_ptr(),
                        self.ws.numel(), self.e.stream)
        torch.cuda.synchronize()

    def adam(self):
        p = {k: _ptr(g) for k, g in self.G.items()}
        self.e.lib.call("zk_adam", p["p"], p["g"], p["m"], p["v"], p["shadow"], self.n, self.hyper.data_ptr(), self.pn.data_ptr(),
                        self.ws.data_ptr(), self.ws.numel(), self.e.stream)
        torch.cuda.synchronize()

    def l2norm(self, scale):
        self.e.lib.call("zk_l2norm", _ptr(self.G["g"]), self.n, scale, self.hyper.data_ptr() + 24, self.ws.data_ptr(),
                        self.ws.numel(), self.e.stream)
        torch.cuda.synchronize()

    def bits(self):
        return {k: g.t.detach().cpu().view(g._int).clone() for k, g in self.G.items() if k != "g"}

    def values(self):
        return {k: _val(g) for k, g in self.G.items()}


def check_adam_update(got, inp, hyper, norm_free, gnorm, what, skip=None):
    """p, m, v against adam_bound (p staged on the stored m, v), the shadow bit for bit, the exact-zero elements bit for
    bit.  skip: a boolean mask of elements left out (a non-finite gradient)."""
    keep = torch.ones_like(inp["zero"]) if skip is None else ~skip
    sel = lambda t: t[keep]
    bounds = PE.adam_bound(sel(inp["p"]), sel(inp["g"]), sel(inp["m"]), sel(inp["v"]), hyper, norm_free, gnorm,
                           sel(got["m"]), sel(got["v"]))
    worst = P.check_all({k: sel(got[k]) for k in ("m", "v", "p")}, {k: bounds[k] for k in ("m", "v", "p")}, what)
    P.assert_exact(sel(got["shadow"]).float(), sel(got["p"]).to(BF).double(), what + " [shadow]")
    z = inp["zero"] & keep
    assert torch.equal(got["p"][z].view(torch.int32), inp["p"][z].view(torch.int32)), what + ": an element with g = m = v = 0 moved"
    assert float(got["m"][z].abs().max() if z.any() else 0.0) == 0.0 and float(got["v"][z].abs().max() if z.any() else 0.0) == 0.0
    return worst


def _tuned(tune, values):
    return {k: tune(k, v) for k, v in values.items()}


@pytest.mark.parametrize("n,key10", ADAM_SIZES)
def test_adam_step_norm_free(n, key10):
    e = eng()
    inp = adam_inputs(n)
    buf = AdamBuffers(e, n, inp)
    tune = e.lib.raw("zk_tune")
    old = _tuned(tune, ADAM_DEFAULT)
    first = None
    try:
        for k9, k10, k18 in adam_variants(n, key10):
            what = "adam_step n=%d key9=%d key10=%d key18=%d" % (n, k9, k10, k18)
            _tuned(tune, {9: k9, 10: k10, 18: k18})
            buf.reset()
            buf.step(1)
            grid = PE.adam_grid(n, k10)
            T = PE.adam_terms_per_thread(n, grid, k9 != 0)
            hy = buf.hyper.cpu()
            norms = {"gnorm": PE.norm_bound(inp["g"], HYPER[4], T, grid), "pnorm": PE.norm_bound(inp["p"], 1.0, T, grid)}
            worst = P.check_all({"gnorm": hy[6:7], "pnorm": buf.pn.cpu()}, norms, what)
            assert int(buf.seed) == 1234568, what + ": the seed word advances by exactly 1"
            assert float(hy[7]) == 0.0 and float(hy[10]) == HYPER[10], (what, hy)
            assert torch.equal(hy[:6], buf.hyper0[:6]) and torch.equal(hy[8:10], buf.hyper0[8:10])
            if first is None:
                _finish({k: g for k, g in buf.G.items() if k != "g"}, {"g": buf.G["g"]}, what)
                worst.update(check_adam_update(buf.values(), inp, buf.hyper0, 1, None, what))
                first = buf.bits()
                print(what, "worst |err| / bound:", worst)
            else:
                buf.G["g"].check_intact(what + " g")
                for k, b in buf.bits().items():
                    assert torch.equal(b, first[k]), "%s: %s differs from the first variant's bits" % (what, k)
    finally:
        _tuned(tune, old)


ADAM_CLIP_CASES = [(n, api, clip) for n in (1027, 4 * 1537 + 2) for api in ("step", "adam") for clip in ("off", "on", "slack")]


@pytest.mark.parametrize("n,api,clip", ADAM_CLIP_CASES)
def test_adam_with_the_norm_given(n, api, clip):
    """norm_free = 0: zk_l2norm writes hyper[6], the update reads it (clip "on": half the norm; "slack": twice it, which
    leaves the gradient as it is; "off": 0)."""
    e = eng()
    inp = adam_inputs(n, seed=1)
    gs = HYPER[4]
    gn64 = gs * float(inp["g"].double().norm())
    hyper = list(HYPER)
    hyper[5] = {"off": 0.0, "on": 0.5 * gn64, "slack": 2.0 * gn64}[clip]
    buf = AdamBuffers(e, n, inp, hyper)
    what = "adam n=%d %s clip %s" % (n, api, clip)
    buf.l2norm(gs)
    gnorm = buf.hyper.cpu()[6:7].clone()
    T1 = 4 * ((n // 4 + 1024 * 256 - 1) // (1024 * 256)) + 1
    worst = P.check_all({"gnorm": gnorm}, {"gnorm": PE.norm_bound(inp["g"], gs, T1, 1024)}, what)
    buf.G["g"].check_intact(what + " g after l2norm")
    buf.step(0) if api == "step" else buf.adam()
    _finish({k: g for k, g in buf.G.items() if k != "g"}, {"g": buf.G["g"]}, what)
    hy = buf.hyper.cpu()
    grid = PE.adam_grid(n, 0)
    worst.update(P.check_all({"pnorm": buf.pn.cpu()}, {"pnorm": PE.norm_bound(inp["p"], 1.0, PE.adam_terms_per_thread(n, grid, False), grid)}, what))
    assert float(hy[7]) == 0.0 and float(hy[10]) == HYPER[10] and float(hy[6]) == float(gnorm)
    assert int(buf.seed) == (1234568 if api == "step" else 1234567)
    worst.update(check_adam_update(buf.values(), inp, buf.hyper0, 0, float(gnorm), what))
    print(what, "worst |err| / bound:", worst)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_adam_step_norm_free_applies_the_update_beside_a_non_finite_gradient(bad):
    e = eng()
    n = 1027
    inp = adam_inputs(n, seed=2)
    inp["g"][6] = bad
    buf = AdamBuffers(e, n, inp)
    what = "adam_step norm_free g[6]=%r" % bad
    buf.step(1)
    _finish({k: g for k, g in buf.G.items() if k != "g"}, {"g": buf.G["g"]}, what)
    hy = buf.hyper.cpu()
    assert not bool(torch.isfinite(hy[6])) and float(hy[7]) == 1.0 and float(hy[10]) == HYPER[10] + 1, (what, hy)
    skip = torch.zeros(n, dtype=torch.bool)
    skip[6] = True
    got = buf.values()
    assert not bool(torch.isfinite(got["p"][6]))
    print(what, check_adam_update(got, inp, buf.hyper0, 1, None, what, skip=skip))


def test_norm_flag():
    e = eng()
    for gn, flag in ((3.5, 0.0), (float("nan"), 1.0), (float("inf"), 1.0), (float("-inf"), 1.0)):
        hyper = torch.tensor(HYPER, dtype=F32)
        hyper[6] = gn
        H = _G(1, 12, F32, hyper.reshape(1, 12))
        e.lib.call("zk_norm_flag", _ptr(H), e.stream)
        torch.cuda.synchronize()
        H.check_guard("norm_flag")
        got = _val(H)
        want = hyper.clone()
        want[7], want[10] = flag, HYPER[10] + flag
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (gn, got)


FLAT_SIZES = [3, 4, 4003, 4 * (2048 * 256) + 6]


def flat_inputs(n, seed=0):
    g = _gen(79 + n % 100003 + seed)
    return torch.randn(n, generator=g), torch.randn(n, generator=g)


@pytest.mark.parametrize("n", FLAT_SIZES)
def test_ema(n):
    e = eng()
    ema, p = flat_inputs(n)
    d = PE.f32(0.999)
    for gn, bound9, skipped in ((1.0, 0.0, False), (float("nan"), 0.0, True), (float("inf"), 0.0, True), (5.0, 4.0, True),
                                (5.0, 6.0, False)):
        what = "ema n=%d gnorm=%r hyper9=%g" % (n, gn, bound9)
        hyper = torch.tensor(HYPER, dtype=F32)
        hyper[6], hyper[8], hyper[9] = gn, d, bound9
        E, Pm, Hy = _G(1, n, F32, ema.reshape(1, n)), _G(1, n, F32, p.reshape(1, n)), _G(1, 12, F32, hyper.reshape(1, 12))
        e.lib.call("zk_ema", _ptr(E), _ptr(Pm), _ptr(Hy), n, e.stream)
        torch.cuda.synchronize()
        _finish({"ema": E}, {"p": Pm, "hyper": Hy}, what)
        if skipped:
            E.check_intact(what + " (skipped)")
        else:
            print(what, P.check_all({"ema": _val(E)}, {"ema": PE.ema_bound(ema, p, d)}, what))


@pytest.mark.parametrize("n", FLAT_SIZES)
def test_axpby_and_cast(n):
    e = eng()
    y, x = flat_inputs(n, 1)
    a, b = PE.f32(0.75), PE.f32(-1.3)
    what = "axpby n=%d" % n
    Y, X = _G(1, n, F32, y.reshape(1, n)), _G(1, n, F32, x.reshape(1, n))
    e.lib.call("zk_axpby_f32", _ptr(Y), _ptr(X), a, b, n, e.stream)
    torch.cuda.synchronize()
    _finish({"y": Y}, {"x": X}, what)
    print(what, P.check_all({"y": _val(Y)}, {"y": PE.axpby_bound(y, x, a, b)}, what))
    what = "cast_bf16_f32 n=%d" % n
    S, D = _G(1, n, BF, x.reshape(1, n)), _G(1, n, F32)
    e.lib.call("zk_cast_bf16_f32", _ptr(S), _ptr(D), n, e.stream)
    torch.cuda.synchronize()
    _finish({"y": D}, {"x": S}, what)
    P.assert_exact(_val(D), x.to(BF).double(), what + " [y]")
