"""The backward's tail as one launch (zk_step_tail): the grouped reductions, both embedding-gradient scatters, both
sides of the shared input bias' column sum and the zero rows of the source table -- against the four launches it
replaces (zk_zero, zk_reduce_grouped, zk_embed_bwd_sorted_pair, zk_colsum_pair): every output bit for bit, guard bands
around each; then the captured training step with and without it (transformer.py:16-33, 88-119 and their gradients).
Then the other folds, each against the launches it replaces: the loss tail inside the cross entropy's last
block (zk_ce_fused_tail; util.py:88-103), the norm finish inside the Adam pass's last block (zk_adam_step_fold)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng, rand_bf, mat  # noqa: E402

F32 = torch.float32
GUARD = 64            # floats on either side of an output (a multiple of the 16-byte stores' alignment)
SENTINEL = 12345.0


def _guarded(shape, fill):
    """-> (whole buffer, view of `shape` in its middle): sentinel floats before and behind the view"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=F32, device="cuda")
    view = whole[GUARD:GUARD + n].view(*shape)
    view.copy_(fill) if torch.is_tensor(fill) else view.fill_(fill)
    return whole, view


def _guards_intact(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def _sorted(ids):
    """rows grouped by id (stable), ids ascending, as zk_batch_prep leaves them"""
    flat = ids.reshape(-1).cpu().numpy()
    order = np.argsort(flat, kind="stable").astype(np.int32)
    uid, start = np.unique(flat[order], return_index=True)
    seg = np.concatenate([start, [len(flat)]]).astype(np.int32)
    dev = lambda a: torch.tensor(a, dtype=torch.int32, device="cuda")
    pad = np.zeros(len(flat) + 1, np.int32)
    pad[:len(seg)] = seg
    u = np.zeros(len(flat), np.int32)
    u[:len(uid)] = uid
    return {"rows": dev(order), "seg": dev(pad), "uid": dev(u), "n": dev([len(uid)]), "max_uniq": len(flat)}


def _ids(pattern, B, L, V, gen):
    """[B, L] int32 ids < V.  eos: the last column is id 2 (one id owns a run of B rows); run70: one id owns 70 rows (more
    than the scatter's batch of 64 row indices); all: every row of the table is touched; eos_only: none but id 2."""
    if pattern == "all":
        assert B * L >= V
        ids = (torch.arange(B * L) % V).view(B, L)
    elif pattern == "eos_only":
        ids = torch.full((B, L), 2)
    else:
        ids = torch.randint(3, V, (B, L), generator=gen)
        if pattern == "eos":
            ids[:, -1] = 2
        else:
            assert pattern == "run70" and B * L > 70
            flat = ids.view(-1)
            flat[torch.randperm(B * L, generator=gen)[:70]] = 5
    return ids.to(torch.int32).cuda()


def _pad8(v):
    return (v + 7) // 8 * 8


# (pattern, B, L target, L source, H, source vocabulary, target table = softmax table, dropout)
CASES = [
    ("eos", 9, 7, 8, 64, 50, False, 0.0),
    ("eos", 9, 7, 8, 72, 150, True, 0.1),         # 152 table rows: three blocks of the zero-row role, the last one partial
    ("run70", 10, 8, 8, 64, 150, True, 0.0),
    ("run70", 10, 8, 8, 72, 50, False, 0.1),
    ("all", 9, 7, 8, 64, 50, False, 0.1),
    ("all", 9, 7, 8, 72, 50, True, 0.0),
    ("eos_only", 9, 7, 8, 64, 50, True, 0.1),
    ("eos_only", 9, 7, 8, 72, 50, False, 0.0),
]


def _problem(pattern, B, Lt, Ls, H, Vs, seed):
    gen = torch.Generator().manual_seed(seed)
    Vt = 33
    it, is_ = _ids(pattern, B, Lt, Vt, gen), _ids(pattern, B, Ls, Vs, gen)
    return {"it": it, "is": is_, "st": _sorted(it), "ss": _sorted(is_), "dt": rand_bf(B * Lt, H, seed=seed + 1),
            "ds": rand_bf(B * Ls, H, seed=seed + 2), "rows_t": _pad8(Vt), "rows_s": _pad8(Vs),
            "base_t": torch.randn(_pad8(Vt), H, generator=gen).cuda(),      # what the weight-gradient launch left there
            # a LayerNorm-gradient problem and a bias-gradient problem for the reduction role (partials as their producers
            # leave them: [blocks][3][H] and [row chunks][N])
            "ln_rows": 70, "ln_part": torch.randn(eng().lib.raw("zk_ln_bwd_blocks")(70) * 3 * H, generator=gen).cuda(),
            "cs_dy": rand_bf(300, H, seed=seed + 3)}


def _outputs(p, H, shared, nan_source):
    o = {"tab_t": _guarded((p["rows_t"], H), p["base_t"] if shared else 0.0),
         "tab_s": _guarded((p["rows_s"], H), float("nan") if nan_source else 7.0),
         "bias": _guarded((H,), 3.0)}
    for k in ("dgamma", "dbeta", "dbprev", "dcs"):
        o[k] = _guarded((H,), 3.0)
    o["cs_part"] = torch.zeros(eng().lib.raw("zk_colsum_rowchunks")(300) * H, device="cuda")
    return o


def _reductions(e, p, o, H, defer):
    e.__dict__.pop("_red_cache", None)        # (descriptor tables are cached by address: a freed buffer's may come back)
    return e.reductions_grouped([(mat(p["cs_dy"]), o["dcs"][1], o["cs_part"])],
                                [(p["ln_part"], p["ln_rows"], H, o["dgamma"][1], o["dbeta"][1], o["dbprev"][1])],
                                defer_reduce=defer)


@pytest.mark.parametrize("pattern,B,Lt,Ls,H,Vs,shared,drop", CASES)
def test_tail_launch_equals_the_four_launches(pattern, B, Lt, Ls, H, Vs, shared, drop):
    e = eng()
    e.set_seed(11)
    p = _problem(pattern, B, Lt, Ls, H, Vs, seed=len(pattern) + H + Vs)
    # the four launches: zero fill, grouped reductions, scatter pair, column-sum pair
    want = _outputs(p, H, shared, nan_source=False)
    e.zero(want["tab_s"][1])
    _reductions(e, p, want, H, defer=False)
    e.embed_bwd_sorted_pair(p["st"], mat(p["dt"]), want["tab_t"][1], shared, 9002, p["ss"], mat(p["ds"]), want["tab_s"][1],
                            False, 9001, H, drop_p=drop)
    e.colsum_pair(mat(p["dt"]), Lt, 9002, mat(p["ds"]), 0, 9001, want["bias"][1], drop_p=drop)
    # the tail launch, on a source table full of NaN: no zero fill in front of it
    got = _outputs(p, H, shared, nan_source=True)
    red = _reductions(e, p, got, H, defer=True)
    e.step_tail(red, p["st"], mat(p["dt"]), got["tab_t"][1], shared, Lt, 9002, p["ss"], mat(p["ds"]), got["tab_s"][1], False,
                0, 9001, H, got["bias"][1], zero_rows_b=p["rows_s"], drop_p=drop)
    torch.cuda.synchronize()
    for k in ("tab_s", "bias", "dgamma", "dbeta", "dbprev", "dcs"):
        assert torch.equal(got[k][1], want[k][1]), k
        assert _guards_intact(got[k][0]), k
    # (a target table of its own is zero-filled by the caller on both routes: here it keeps its 0.0 outside the batch's ids)
    assert torch.equal(got["tab_t"][1], want["tab_t"][1]) and _guards_intact(got["tab_t"][0])
    assert not bool(got["tab_s"][1][Vs:].any()), "padding rows of the source table must read as zero"
    if pattern == "eos_only":
        assert not bool(got["tab_s"][1][:2].any()) and not bool(got["tab_s"][1][3:].any()) and bool(got["tab_s"][1][2].any())
    if pattern == "all":
        assert bool(got["tab_s"][1][:Vs].any(dim=1).all())


@pytest.mark.parametrize("H,Vs", [(64, 50), (72, 150)])
def test_zero_row_role_alone(H, Vs):
    """NaN everywhere before the launch: afterwards every row is the scatter's value or exactly zero."""
    e = eng()
    B, Lt, Ls = 9, 7, 8
    p = _problem("eos", B, Lt, Ls, H, Vs, seed=5)
    want = _outputs(p, H, False, nan_source=False)
    e.embed_bwd_sorted(p["ss"], mat(p["ds"]), want["tab_s"][1], H, accumulate=False, sid=9001)
    got = _outputs(p, H, False, nan_source=True)
    e.step_tail(None, p["st"], mat(p["dt"]), got["tab_t"][1], False, Lt, 9002, p["ss"], mat(p["ds"]), got["tab_s"][1], False,
                0, 9001, H, got["bias"][1], zero_rows_b=p["rows_s"])
    torch.cuda.synchronize()
    tab = got["tab_s"][1]
    assert not bool(torch.isnan(tab).any()) and _guards_intact(got["tab_s"][0])
    touched = torch.zeros(p["rows_s"], dtype=torch.bool, device="cuda")
    touched[torch.unique(p["is"].long().view(-1))] = True
    assert torch.equal(tab[touched], want["tab_s"][1][touched])
    assert not bool(tab[~touched].any())
    assert int((~touched).sum()) > 0 and int(touched.sum()) > 0


@pytest.mark.parametrize("model", ["transformer", "transformer_aan"])
def test_captured_step_with_the_tail_launch(model, monkeypatch):
    """Four captured steps on the tail launch against ZERO_HIP_MERGE_SMALL=0, under the bounds of
    test_gpu_merged_launches.test_training_steps_with_merged_launches (losses: the same bits up to the per-sentence loss'
    summation order; weights: fp32 round-off of the bias gradient's summation order); then the tail launch against
    itself, replayed: bit-equal.  Launches: the round-6 merges took six nodes out of the graph (pinned there); the tail
    launch takes the source table's zero fill, the reduction launch and one of scatter / column-sum launch: three more."""
    from tests.test_gpu_model import _setup
    from zero_amd.main import Trainer
    from zero_amd.models._factory import reset_cores
    hp, Pn, src, tgt = _setup(model)
    runs = []
    for flag in ("0", "1", "1"):
        monkeypatch.setenv("ZERO_HIP_MERGE_SMALL", flag)
        reset_cores()
        tr = Trainer(hp, initializer=Pn)
        tr.prepare_static({"source": src, "target": tgt})
        losses = [float(tr.step_static(use_graph=True).cpu()[0]) for _ in range(4)]
        torch.cuda.synchronize()
        runs.append((losses, tr.store.export("master"), tr.core.eng.last_graph_nodes))
    off, on, again = runs
    print("graph nodes: %d without the merges, %d with the tail launch" % (off[2], on[2]))
    assert np.allclose(off[0], on[0], rtol=2e-6, atol=0), (off[0], on[0])
    for k, a in off[1].items():
        assert np.abs(a - on[1][k]).max() <= 1e-5 * max(1.0, np.abs(a).max()), k
    assert on[0] == again[0]
    for k, a in on[1].items():
        assert np.array_equal(a, again[1][k]), k
    assert on[2] <= off[2] - 9, (off[2], on[2])


# (64 * 2000 + 8 floats: 126 blocks, so that the last arriver is one of many and not one of five)
@pytest.mark.parametrize("n", [5, 4099, 64 * 2000 + 8])
@pytest.mark.parametrize("skip", [0, 1])
def test_adam_with_the_folded_norm_finish(n, skip):
    """zk_adam_step_fold (the Adam pass's last block finishes the norms) against zk_adam_step (k_norm_final2 as a launch
    of its own), two consecutive calls each on one arrival counter: gradient norm hyper[6], flag hyper[7], sticky count
    hyper[10] and the parameter norm bit for bit, the update itself too.  skip = 1: the skip word set (cycle.py:94-101;
    the update is not applied, the norm is NaN, the sticky count goes up on every call)."""
    lib = eng().lib
    g = torch.Generator().manual_seed(n)
    mk = lambda s: (torch.randn(n, generator=g) * s).cuda()
    p0, gr, m0, v0 = mk(0.1), mk(0.02), mk(0.01), mk(0.001).abs()
    ws = torch.empty(lib.query("zk_adam_step_workspace"), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    word = torch.tensor([skip], dtype=torch.int32, device="cuda")
    arrive = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = {}
    for fold in (False, True):
        hyper = torch.tensor([3e-3, 0.9, 0.98, 1e-8, 0.25, 0.0, 0.5, 0, 0, 0, 0, 0], dtype=F32, device="cuda")
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        sh = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
        pn = torch.zeros(1, device="cuda")
        seed = torch.zeros(1, dtype=torch.int64, device="cuda")
        seen = []
        for _ in range(2):
            lib.call("zk_adam_step_fold" if fold else "zk_adam_step", p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(),
                     sh.data_ptr(), n, hyper.data_ptr(), pn.data_ptr(), seed.data_ptr(), 1, word.data_ptr(), ws.data_ptr(),
                     ws.numel(), *((arrive.data_ptr(), stream) if fold else (stream,)))
            torch.cuda.synchronize()
            seen.append((hyper.clone(), pn.clone()))
        out[fold] = (p, m, v, sh, seen, int(seed.item()))
    assert int(arrive[0].item()) == 0, "the last block leaves the arrival counter at zero"
    for a, b in zip(out[False][:4], out[True][:4]):
        assert torch.equal(a, b)
    for (ha, pa), (hb, pb) in zip(out[False][4], out[True][4]):
        assert torch.equal(ha.view(torch.int32), hb.view(torch.int32)) and torch.equal(pa, pb)   # (NaN compares by its bits)
    assert out[False][5] == out[True][5] == 2
    h = out[True][4][1][0].cpu().numpy()
    if skip:
        assert np.isnan(h[6]) and h[7] == 1 and h[10] == 2 and torch.equal(out[True][0], p0)
    else:
        assert np.isfinite(h[6]) and h[6] > 0 and h[7] == 0 and h[10] == 0 and not torch.equal(out[True][0], p0)


@pytest.mark.parametrize("L", [5, 70])
def test_cross_entropy_with_the_folded_loss_tail(L):
    """B = 3, V = 50: zk_ce_fused_tail (the last block forms the per-sentence loss and its mean) against ce_fused +
    loss_reduce in its one-launch and its two-launch form, captured and replayed three times on one arrival counter."""
    e = eng()
    B, V, ld = 3, 50, 56
    g = torch.Generator().manual_seed(L)
    logits = (torch.randn(B * L, ld, generator=g) * 2).cuda()
    ids = torch.randint(1, V, (B, L), generator=g, dtype=torch.int32)
    ids[1, L - 2:] = 0                                  # padding
    ids = ids.cuda()
    w = torch.rand(B * L, generator=g).cuda()

    def alloc():
        return {"ce": _guarded((B * L,), 9.0), "ps": _guarded((B,), 9.0), "loss": _guarded((1,), 9.0),
                "dl": torch.zeros(B * L, ld, dtype=torch.bfloat16, device="cuda")}
    ref = {}
    for two in (0, 1):
        o = alloc()
        old = e.lib.raw("zk_tune")(16, two)
        try:
            e.ce_fused(mat(logits), ids, w, o["ce"][1], mat(o["dl"]), B * L, V, 0.1)
            e.loss_reduce(o["ce"][1], ids, o["ps"][1], o["loss"][1], B, L)
            torch.cuda.synchronize()
        finally:
            e.lib.raw("zk_tune")(16, old)
        ref[two] = o
    o = alloc()

    def body():
        e.ce_tail_next(o["ps"][1], o["loss"][1], B, L)
        e.ce_fused(mat(logits), ids, w, o["ce"][1], mat(o["dl"]), B * L, V, 0.1)
    with torch.cuda.stream(e.work_stream):
        body()                                          # eager once
        torch.cuda.synchronize()
        first = (o["ps"][1].clone(), o["loss"][1].clone())
        gr = e.graph_capture(body)
        assert e.last_graph_nodes == 1
        for _ in range(3):
            o["ps"][1].fill_(9.0)
            o["loss"][1].fill_(9.0)
            torch.cuda.synchronize()
            e.graph_launch(gr)
            torch.cuda.synchronize()
            assert torch.equal(o["ps"][1], first[0]) and torch.equal(o["loss"][1], first[1])
            assert int(e._ce_arrive[0].item()) == 0
    for k in ("ce", "ps", "loss"):
        assert _guards_intact(o[k][0]), k
    assert torch.equal(o["ce"][1], ref[0]["ce"][1]) and torch.equal(o["dl"], ref[0]["dl"])
    assert torch.equal(o["ps"][1], ref[0]["ps"][1]) and torch.equal(o["loss"][1], ref[0]["loss"][1])
    if L <= 64:
        assert torch.equal(o["ps"][1], ref[1]["ps"][1]) and torch.equal(o["loss"][1], ref[1]["loss"][1])
    else:
        assert torch.allclose(o["ps"][1], ref[1]["ps"][1], rtol=1e-6, atol=0)
        assert torch.allclose(o["loss"][1], ref[1]["loss"][1], rtol=1e-6, atol=0)
    mk = (ids != 0).float()
    want = (ref[0]["ce"][1].view(B, L) * mk).sum(1) / mk.sum(1)
    assert torch.allclose(o["ps"][1], want, rtol=1e-5)
