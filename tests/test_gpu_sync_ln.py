"""The tail of a post-LN sub-layer in one launch (round 4: zk_gemm_add_ln; func.py:321-324 residual_fn, func.py:289-303
layer_norm, transformer.py:57-58): the workgroups of a block of rows exchange the statistics of their 64 columns and
normalise them in the epilogue.  Checked against the two launches it replaces (zk_gemm, zk_add_ln_fwd) on the kernels,
under repetition (the exchange slots are reused by every call), and on the whole training step."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng, rand_bf, mat, rel_err  # noqa: E402

F32 = torch.float32


def _two_launches(e, A, W, b, R, gam, bet, drop, sid, save=True):
    M, N = A.shape[0], W.shape[1]
    y = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    out, s = torch.empty_like(y), torch.empty_like(y)
    mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    e.gemm(mat(A), mat(W), mat(y), M, N, A.shape[1], 0, 0, bias=b)
    e.add_ln_fwd(mat(R), mat(y), gam, bet, mat(out), mat(s) if save else None, mean, rstd, drop, sid)
    return out, s, mean, rstd


def _one_launch(e, A, W, b, R, gam, bet, drop, sid, save=True):
    M, N = A.shape[0], W.shape[1]
    out = torch.full((M, N), 7.0, dtype=torch.bfloat16, device="cuda")
    s = torch.full((M, N), 7.0, dtype=torch.bfloat16, device="cuda") if save else None
    mean = torch.empty(M, device="cuda") if save else None
    rstd = torch.empty(M, device="cuda") if save else None
    e.gemm_add_ln(mat(A), mat(W), M, N, A.shape[1], b, mat(R), gam, bet, mat(out), mat(s) if save else None, mean, rstd,
                  drop, sid)
    return out, s, mean, rstd


def _ulp_close(a, b):
    """bf16 tensors equal up to one unit in the last place of the larger magnitude (the statistics differ in their last
    fp32 bits: Chan's combination of eight partials against two passes over the row)."""
    a, b = a.float(), b.float()
    tol = torch.maximum(a.abs(), b.abs()) * 2.0 ** -7 + 1e-6
    return bool(((a - b).abs() <= tol).all())


@pytest.mark.parametrize("M,N,K", [(4096, 512, 512), (4096, 512, 2048), (66, 512, 512), (700, 512, 512), (130, 512, 2048),
                                   (1000, 1024, 1024), (257, 128, 512), (64, 64, 64), (5, 512, 512)])
@pytest.mark.parametrize("drop", [0.0, 0.1])
def test_one_launch_against_gemm_then_layernorm(M, N, K, drop):
    """Interior and ragged row counts, both tile shapes (64x64 for K = 512, 128x64 for the long K), one to sixteen
    workgroups per row block: the stored sum is the two-launch sum bit for bit (same rounding of the product, same
    dropout mask), y agrees to the last bf16 bit of the statistics, mean / rstd to fp32 rounding."""
    e = eng()
    e.set_seed(5)
    A, W = rand_bf(M, K, seed=1, scale=0.5), rand_bf(K, N, seed=2, scale=0.05)
    R = rand_bf(M, N, seed=3)
    g = torch.Generator().manual_seed(4)
    b = (torch.randn(N, generator=g) * 0.1).cuda()
    gam = (1.0 + 0.2 * torch.randn(N, generator=g)).cuda()
    bet = (0.1 * torch.randn(N, generator=g)).cuda()
    ref = _two_launches(e, A, W, b, R, gam, bet, drop, 11)
    e.ln_epoch_bump()
    got = _one_launch(e, A, W, b, R, gam, bet, drop, 11)
    torch.cuda.synchronize()
    assert e.sync_ln_errors() == 0
    assert torch.equal(got[1], ref[1])
    assert _ulp_close(got[0], ref[0]) and rel_err(got[0], ref[0]) < 2e-3
    assert torch.allclose(got[2], ref[2], rtol=1e-5, atol=1e-6) and torch.allclose(got[3], ref[3], rtol=1e-5, atol=0)
    # without the outputs the backward reads (inference): nothing is saved, so the residual sum is NOT rounded to bf16 before
    # the statistics (round 6: the checker's bf16 storage model has no rounding between residual_fn and layer_norm) -- in
    # the one launch as in zk_add_ln_fwd without sum_out; against the saving form the rows move by the sum's rounding
    e.ln_epoch_bump()
    lean = _one_launch(e, A, W, b, R, gam, bet, drop, 11, save=False)
    ref_lean = _two_launches(e, A, W, b, R, gam, bet, drop, 11, save=False)
    torch.cuda.synchronize()
    assert _ulp_close(lean[0], ref_lean[0]) and rel_err(lean[0], ref_lean[0]) < 2e-3
    assert rel_err(lean[0], got[0]) < 6e-3 and not torch.equal(ref_lean[0], ref[0])
    # the fp32 sum is the better LayerNorm input: closer to the fp32 statement of the same rows
    y32 = (A.float() @ W.float() + b).to(torch.bfloat16).float()
    if drop == 0.0:
        want = torch.nn.functional.layer_norm(R.float() + y32, (N,), gam, bet, 1e-8)
        assert rel_err(lean[0], want) <= rel_err(got[0], want) * 1.02 + 1e-6


@pytest.mark.parametrize("M,N,K", [(4096, 512, 2048), (4096, 512, 512), (4096, 512, 1536), (66, 512, 512), (700, 512, 1536),
                                   (1000, 1024, 1024), (257, 128, 512), (5, 512, 512)])
@pytest.mark.parametrize("drop", [0.0, 0.1])
def test_backward_inside_the_dgrad_launch(M, N, K, drop):
    """zk_gemm_ln_bwd against the two launches it replaces (zk_gemm with tb = 1 and a residual, zk_add_ln_bwd): ds and dy
    to the last bf16 bit of the two row means (eight partial sums combined instead of one wave-wide sum), the three column
    sums after their reduction to fp32 summation-order differences."""
    e = eng()
    e.set_seed(9)
    dY, W = rand_bf(M, K, seed=1, scale=0.5), rand_bf(N, K, seed=2, scale=0.05)
    R, S = rand_bf(M, N, seed=3, scale=0.3), rand_bf(M, N, seed=4)
    g = torch.Generator().manual_seed(4)
    gam = (1.0 + 0.2 * torch.randn(N, generator=g)).cuda()
    mean = S.float().mean(1).contiguous()
    rstd = (1.0 / torch.sqrt(S.float().var(1, unbiased=False) + 1e-8)).contiguous()
    # reference: two launches + the reduction
    dx = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    e.gemm(mat(dY), mat(W), mat(dx), M, N, K, 0, 1, residual=mat(R))
    ds0, dy0 = torch.empty_like(dx), torch.empty_like(dx)
    out0 = [torch.zeros(N, device="cuda") for _ in range(3)]
    e.add_ln_bwd(mat(dx), mat(S), mean, rstd, gam, mat(ds0), mat(dy0) if drop else None, out0[0], out0[1], out0[2], drop, 17)
    # one launch + the grouped reduction over its 64-row partials
    ds1 = torch.full_like(dx, 7.0)
    dy1 = torch.full_like(dx, 7.0)
    nfl = e.lib.query("zk_gemm_ln_bwd_partials", M, N) // 4
    part = torch.full((nfl,), 1e9, device="cuda")
    out1 = [torch.zeros(N, device="cuda") for _ in range(3)]
    e.ln_epoch_bump()
    e.gemm_ln_bwd(mat(dY), mat(W), M, N, K, mat(R), mat(S), mean, rstd, gam, mat(ds1), mat(dy1) if drop else None, part, drop, 17)
    e.reductions_grouped([], [(part, M, N, out1[0], out1[1], out1[2], True)])
    torch.cuda.synchronize()
    assert e.sync_ln_errors() == 0
    assert rel_err(ds1, ds0) < 3e-3 and _ulp_close_abs(ds1, ds0)
    if drop:
        assert rel_err(dy1, dy0) < 3e-3
        assert torch.equal(dy1 == 0, dy0 == 0) or float(((dy1 == 0) != (dy0 == 0)).float().mean()) < 1e-3   # the same mask
    for a, b in zip(out1, out0):
        assert rel_err(a, b) < 2e-3, rel_err(a, b)


def _ulp_close_abs(a, b):
    """ds is a difference of nearly equal terms: compare against the row scale instead of the element"""
    a, b = a.float(), b.float()
    scale = b.abs().amax(dim=1, keepdim=True) + 1e-12
    return bool(((a - b).abs() <= scale * 2.0 ** -6).all())


@pytest.mark.parametrize("B,Lq,Lk,causal,masked,drop", [(64, 64, 64, True, False, 0.1), (64, 64, 64, False, True, 0.0),
                                                        (16, 37, 37, True, False, 0.1), (8, 13, 150, False, True, 0.1),
                                                        (5, 64, 64, False, True, 0.0), (24, 50, 256, False, True, 0.1)])
def test_attention_inside_the_output_projection_launch(B, Lq, Lk, causal, masked, drop):
    """zk_attn_out_ln against zk_attn_fwd followed by zk_gemm_add_ln: the attention output and its log-sum-exp are the
    attention kernel's bit for bit (same tile function), and so are the sum, the normalised rows and the statistics
    (same tile function over the same rows; sentence-aligned instead of 64-aligned row tiles do not change a row).
    Self- and cross-shaped problems, one to four key tiles, ragged sentences, a grid whose row blocks straddle XCDs."""
    e = eng()
    e.set_seed(21)
    nh, d = 8, 64
    H = nh * d
    Tq, Tk = B * Lq, B * Lk
    q, k, v = rand_bf(Tq, H, seed=1), rand_bf(Tk, H, seed=2), rand_bf(Tk, H, seed=3)
    Wo, R = rand_bf(H, H, seed=4, scale=0.05), rand_bf(Tq, H, seed=5)
    g = torch.Generator().manual_seed(6)
    b = (torch.randn(H, generator=g) * 0.1).cuda()
    gam, bet = (1.0 + 0.2 * torch.randn(H, generator=g)).cuda(), (0.1 * torch.randn(H, generator=g)).cuda()
    kmask = None
    if masked:
        kmask = torch.ones(B, Lk, device="cuda")
        for i in range(B):
            kmask[i, Lk - (i % max(1, Lk // 2)):] = 0.0
    def outs():
        return (torch.full((Tq, H), 3.0, dtype=torch.bfloat16, device="cuda"), torch.zeros(B * nh * Lq, device="cuda"),
                torch.full((Tq, H), 3.0, dtype=torch.bfloat16, device="cuda"), torch.full((Tq, H), 3.0, dtype=torch.bfloat16, device="cuda"),
                torch.zeros(Tq, device="cuda"), torch.zeros(Tq, device="cuda"))
    att0, lse0, y0, s0, mean0, rstd0 = outs()
    e.attn_fwd(mat(q), mat(k), mat(v), mat(att0), lse0, B, nh, Lq, Lk, d, kmask=kmask, causal=causal, drop_p=drop, sid=7)
    e.ln_epoch_bump()
    e.gemm_add_ln(mat(att0), mat(Wo), Tq, H, H, b, mat(R), gam, bet, mat(y0), mat(s0), mean0, rstd0, drop, 8)
    att1, lse1, y1, s1, mean1, rstd1 = outs()
    e.ln_epoch_bump()
    ok = e.attn_out_ln(mat(q), mat(k), mat(v), mat(att1), lse1, B, nh, Lq, Lk, d, kmask, causal, drop, 7, mat(Wo), b, mat(R),
                       gam, bet, mat(y1), mat(s1), mean1, rstd1, drop, 8)
    torch.cuda.synchronize()
    assert ok and e.sync_ln_errors() == 0
    assert torch.equal(att1, att0) and torch.equal(lse1, lse0)
    assert torch.equal(s1, s0) and torch.equal(y1, y0) and torch.equal(mean1, mean0) and torch.equal(rstd1, rstd0)


@pytest.mark.parametrize("B,Lq,Lk,pro,causal,masked,drop", [(64, 64, 64, 3, True, False, 0.1), (64, 64, 64, 3, False, True, 0.1),
                                                            (64, 64, 64, 1, False, True, 0.1), (16, 37, 37, 3, True, False, 0.1),
                                                            (8, 13, 150, 1, False, True, 0.1), (5, 64, 64, 3, False, True, 0.0),
                                                            (24, 50, 256, 1, False, True, 0.0), (3, 1, 1, 3, True, False, 0.0)])
def test_projection_inside_the_attention_launch(B, Lq, Lk, pro, causal, masked, drop):
    """zk_proj_attn_out_ln (round 6) against zk_gemm (the merged qkv_map / the q_map, func.py:206-216) followed by
    zk_attn_out_ln: the projected q (k, v) tiles, the attention output, its log-sum-exp, the sum, the normalised rows and the
    statistics are bit for bit the two launches' (same 64x64 tile function and K order whatever tile the projection launch
    picks; each workgroup reads back only what it wrote).  Self-shaped (pro = 3: q, k, v column slices of one matrix) and
    cross-shaped (pro = 1: keys / values given) problems, ragged sentences, a one-row sentence, grids that straddle XCDs."""
    e = eng()
    e.set_seed(23)
    nh, d = 8, 64
    H = nh * d
    Tq, Tk = B * Lq, B * Lk
    x = rand_bf(Tq, H, seed=11)
    Wp, Wo, R = rand_bf(H, pro * H, seed=12, scale=0.05), rand_bf(H, H, seed=4, scale=0.05), rand_bf(Tq, H, seed=5)
    g = torch.Generator().manual_seed(6)
    b = (torch.randn(H, generator=g) * 0.1).cuda()
    bp = (torch.randn(pro * H, generator=g) * 0.1).cuda()
    gam, bet = (1.0 + 0.2 * torch.randn(H, generator=g)).cuda(), (0.1 * torch.randn(H, generator=g)).cuda()
    kvt = rand_bf(Tk, 2 * H, seed=2)
    kmask = None
    if masked:
        kmask = torch.ones(B, Lk, device="cuda")
        for i in range(B):
            kmask[i, Lk - (i % max(1, Lk // 2)):] = 0.0

    def run(fused):
        proj = torch.full((Tq, pro * H), 3.0, dtype=torch.bfloat16, device="cuda")
        att, y, s = (torch.full((Tq, H), 3.0, dtype=torch.bfloat16, device="cuda") for _ in range(3))
        lse, mean, rstd = torch.zeros(B * nh * Lq, device="cuda"), torch.zeros(Tq, device="cuda"), torch.zeros(Tq, device="cuda")
        q = mat(proj, Tq, H, pro * H, 0)
        if pro == 3:
            k, v = mat(proj, Tq, H, 3 * H, H), mat(proj, Tq, H, 3 * H, 2 * H)
        else:
            k, v = mat(kvt, Tk, H, 2 * H, 0), mat(kvt, Tk, H, 2 * H, H)
        if not fused:
            e.gemm(mat(x), mat(Wp), mat(proj), Tq, pro * H, H, 0, 0, bias=bp)
        e.ln_epoch_bump()
        ok = e.attn_out_ln(q, k, v, mat(att), lse, B, nh, Lq, Lk, d, kmask, causal, drop, 7, mat(Wo), b, mat(R), gam, bet,
                           mat(y), mat(s), mean, rstd, drop, 8, proj=(mat(x), mat(Wp), bp, pro) if fused else None)
        torch.cuda.synchronize()
        assert ok and e.sync_ln_errors() == 0
        return proj, att, lse, y, s, mean, rstd

    ref, got = run(False), run(True)
    for name, r, t in zip(("projection", "att", "lse", "y", "s", "mean", "rstd"), ref, got):
        assert torch.equal(r, t), name


def test_repeated_launches_reuse_the_slots():
    """Several hundred launches back to back on the same slots, different inputs and sites, the epoch advancing every 30
    launches as it does in a training step (30 sub-layers): every one of them must see this launch's partials, never an
    earlier launch's.  Two alternating inputs: a stale slot would show up as the other input's statistics."""
    e = eng()
    M, N, K = 4096, 512, 512
    W = rand_bf(K, N, seed=2, scale=0.05)
    gam, bet = torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")
    ins = [(rand_bf(M, K, seed=10 + i, scale=0.5 * (1 + 3 * i)), rand_bf(M, N, seed=20 + i, scale=1.0 + 2 * i)) for i in range(2)]
    want = []
    for A, R in ins:
        e.ln_epoch_bump()
        want.append(_one_launch(e, A, W, None, R, gam, bet, 0.0, 0, save=False)[0].clone())     # (as the loop below: nothing saved)
    torch.cuda.synchronize()
    assert not torch.equal(want[0], want[1])
    out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    bad = 0
    for it in range(360):
        if it % 30 == 0:
            e.ln_epoch_bump()
        A, R = ins[it % 2]
        e.gemm_add_ln(mat(A), mat(W), M, N, K, None, mat(R), gam, bet, mat(out))
        if it % 7 == 0 or it > 340:
            torch.cuda.synchronize()
            bad += int(not torch.equal(out, want[it % 2]))
    torch.cuda.synchronize()
    assert bad == 0 and e.sync_ln_errors() == 0


@pytest.mark.parametrize("model", ["transformer", "transformer_rpr"])
def test_training_steps_with_the_layernorm_inside_the_launch(model, monkeypatch):
    """Trainer with ZERO_HIP_SYNC_LN = 1 (everything) / noattn / fwd / 0: the same losses and weights after five steps up to the last-bit difference
    of the statistics; captured replay == eager bit for bit with it on (the epoch word lives on the device)."""
    from tests.common import make_hp, make_batch, perturb
    from oracle import ref_torch as rt
    from zero_amd.main import Trainer
    from zero_amd.models._factory import reset_cores
    from zero_amd.variables import reset_stores
    hp = make_hp(model, H=128, F=256, lrate=0.02, warmup_steps=10, dropout=0.1, residual_dropout=0.1)
    rng = np.random.default_rng(3)
    src, tgt = make_batch(rng, 6, 11, 13, hp.src_vocab.size(), hp.tgt_vocab.size())
    Pn = perturb(rt.init_params(hp, model, seed=8), rng)
    out = {}
    for sync in ("1", "noattn", "fwd", "0"):
        monkeypatch.setenv("ZERO_HIP_SYNC_LN", sync)
        for use_graph in (False, True):
            reset_cores(); reset_stores()
            tr = Trainer(hp, initializer=Pn)
            assert tr.core.sync_ln_mode == (sync != "0") and tr.core.sync_ln_bwd == (sync != "fwd") and \
                tr.core.sync_attn == (sync == "1")
            tr.prepare_static({"source": src, "target": tgt})
            tr.core.eng.set_seed(11)
            losses = [float(tr.step_static(use_graph).cpu()[0]) for _ in range(5)]
            torch.cuda.synchronize()
            assert tr.core.eng.sync_ln_errors() == 0
            out[(sync, use_graph)] = (losses, tr.store.master.cpu().numpy().copy())
    a, b = out[("1", False)], out[("1", True)]
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    off = out[("0", True)]
    a, b = out[("1", True)], out[("noattn", True)]           # the attention inside the projection / dgrad launches changes
    if model == "transformer":                               # nothing but the blocking of the LayerNorm-parameter column sums
        assert np.allclose(a[0], b[0], rtol=1e-5, atol=0) and np.linalg.norm(a[1] - b[1]) <= 1e-5 * np.linalg.norm(b[1])
    for mode in ("1", "fwd"):
        on = out[(mode, True)]
        assert np.allclose(on[0], off[0], rtol=2e-3, atol=0), (mode, on[0], off[0])
        assert np.linalg.norm(on[1] - off[1]) <= 2e-3 * np.linalg.norm(off[1])


def test_training_steps_with_the_projection_inside_the_attention_launch(monkeypatch):
    """Trainer with ZERO_HIP_PROJ_ATTN = 1 (round 6 default: qkv_map / q_map as the prologue of the attention launch) against 0
    (a launch of its own): losses and every master weight equal bit for bit after five steps, eager and captured -- the
    projection runs the same tile function over the same K order -- with 18 fewer launches per step at six layers a side."""
    from tests.common import make_hp, make_batch, perturb
    from oracle import ref_torch as rt
    from zero_amd.main import Trainer
    from zero_amd.models._factory import reset_cores
    from zero_amd.variables import reset_stores
    hp = make_hp("transformer", H=128, F=256, lrate=0.02, warmup_steps=10, dropout=0.1, residual_dropout=0.1)
    rng = np.random.default_rng(3)
    src, tgt = make_batch(rng, 6, 11, 13, hp.src_vocab.size(), hp.tgt_vocab.size())
    Pn = perturb(rt.init_params(hp, "transformer", seed=8), rng)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("ZERO_HIP_PROJ_ATTN", mode)
        for use_graph in (False, True):
            reset_cores(); reset_stores()
            tr = Trainer(hp, initializer=Pn)
            assert tr.core.proj_attn == (mode == "1")
            tr.prepare_static({"source": src, "target": tgt})
            tr.core.eng.set_seed(11)
            n0 = tr.core.eng.lib.ncalls
            losses = [float(tr.step_static(use_graph).cpu()[0]) for _ in range(5)]
            torch.cuda.synchronize()
            assert tr.core.eng.sync_ln_errors() == 0
            out[(mode, use_graph)] = (losses, tr.store.master.cpu().numpy().copy(), tr.core.eng.lib.ncalls - n0)
    ref = out[("0", False)]
    for key in (("1", False), ("1", True), ("0", True)):
        assert out[key][0] == ref[0] and np.array_equal(out[key][1], ref[1]), key
    nl = hp.num_encoder_layer + 2 * hp.num_decoder_layer
    assert out[("0", False)][2] - out[("1", False)][2] == 5 * nl      # one launch per attention sub-layer and step


def test_the_exchange_passes_its_self_test_on_this_device():
    """Engine.sync_ln_usable(): the one-time probe that decides whether the in-launch forms are used at all (a device on
    which it fails runs the two-launch structure with a warning)."""
    e = eng()
    assert e.sync_ln_usable() is True
    assert e.sync_ln_errors() == 0


def _clear_exchange_error(e):
    torch.cuda.synchronize()
    e._sync_ln[1][1:2].zero_()
    torch.cuda.synchronize()


def test_a_peer_that_never_publishes_is_bounded_loud_and_poisons_its_rows():
    """Round 5: fault injection (tuning key 15 bit 1: the tn = 1 tiles never publish
    their statistics).  The launch must END (bounded spins -- and ONE budget per workgroup, not one per row and peer),
    raise the device error word, and leave NaN rows -- so that the step's own non-finite guard trips on the very step --
    instead of rows normalised with garbage statistics.  Forward and backward forms; afterwards the exchange works again."""
    import time
    e = eng()
    M, N, K = 4096, 512, 512
    A, W, R = rand_bf(M, K, seed=1, scale=0.5), rand_bf(K, N, seed=2, scale=0.05), rand_bf(M, N, seed=3)
    gam, bet = torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")
    e.ln_epoch_bump()
    good = _one_launch(e, A, W, None, R, gam, bet, 0.0, 0)
    torch.cuda.synchronize()
    assert e.sync_ln_errors() == 0
    tune = e.lib.raw("zk_tune")
    tune(15, 2)
    try:
        e.ln_epoch_bump()
        t0 = time.time()
        bad = _one_launch(e, A, W, None, R, gam, bet, 0.0, 0)
        torch.cuda.synchronize()
        dt_fwd = time.time() - t0
        assert e.sync_ln_errors() == 1
        # (the muted tile column itself -- columns 64 .. 127 -- saw all of ITS peers: only the others must be poisoned)
        nan = torch.isnan(bad[0].float())
        assert bool(nan[:, :64].all()) and bool(nan[:, 128:].all()) and not bool(nan[:, 64:128].any()), \
            "rows normalised without a peer's partial must be NaN"
        assert torch.equal(bad[1], good[1])            # the stored sum does not depend on the peers
        _clear_exchange_error(e)
        dY, W2 = rand_bf(M, K, seed=4, scale=0.5), rand_bf(N, K, seed=5, scale=0.05)
        ds = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
        part = torch.empty(e.lib.query("zk_gemm_ln_bwd_partials", M, N) // 4, device="cuda")
        e.ln_epoch_bump()
        t0 = time.time()
        e.gemm_ln_bwd(mat(dY), mat(W2), M, N, K, None, mat(good[1]), good[2], good[3], gam, mat(ds), None, part)
        torch.cuda.synchronize()
        dt_bwd = time.time() - t0
        assert e.sync_ln_errors() == 1
        nan = torch.isnan(ds.float())
        assert bool(nan[:, :64].all()) and bool(nan[:, 128:].all()) and not bool(nan[:, 64:128].any())
        # one spin budget per workgroup (2^15 polls of a few hundred ns .. 2 us), three resident rounds at most
        assert dt_fwd < 5.0 and dt_bwd < 5.0, (dt_fwd, dt_bwd)
    finally:
        tune(15, 0)
        _clear_exchange_error(e)
    e.ln_epoch_bump()
    again = _one_launch(e, A, W, None, R, gam, bet, 0.0, 0)
    torch.cuda.synchronize()
    assert e.sync_ln_errors() == 0 and torch.equal(again[0], good[0])


def test_a_failed_self_test_switches_forward_and_backward_to_the_two_launch_structure():
    """with the self-test failing (fault injection) Engine.sync_ln_usable() is False and NEITHER
    direction of the training step uses the exchange: the step runs, finite, with the error word clear."""
    from tests.common import make_hp, make_batch, perturb
    from oracle import ref_torch as rt
    from zero_amd.main import Trainer
    from zero_amd.models._factory import reset_cores
    from zero_amd.variables import reset_stores
    e = eng()
    tune = e.lib.raw("zk_tune")
    hp = make_hp("transformer", H=128, F=256, lrate=0.02, warmup_steps=10)
    rng = np.random.default_rng(3)
    src, tgt = make_batch(rng, 6, 11, 13, hp.src_vocab.size(), hp.tgt_vocab.size())
    Pn = perturb(rt.init_params(hp, "transformer", seed=8), rng)
    reset_cores(); reset_stores()
    tr = Trainer(hp, initializer=Pn)
    eng2 = tr.core.eng
    tune(15, 2)
    try:
        eng2.__dict__.pop("_sync_ln_ok", None)
        assert eng2.sync_ln_usable() is False
    finally:
        tune(15, 0)
    try:
        tr.prepare_static({"source": src, "target": tgt})
        losses = [float(tr.step_static(False).cpu()[0]) for _ in range(2)]
        torch.cuda.synchronize()
        assert np.isfinite(losses).all() and eng2.sync_ln_errors() == 0
        # the reference run with the exchange switched off by hand gives the same numbers bit for bit
        reset_cores(); reset_stores()
        os.environ["ZERO_HIP_SYNC_LN"] = "0"
        try:
            tr0 = Trainer(hp, initializer=Pn)
            tr0.prepare_static({"source": src, "target": tgt})
            losses0 = [float(tr0.step_static(False).cpu()[0]) for _ in range(2)]
        finally:
            del os.environ["ZERO_HIP_SYNC_LN"]
        assert losses == losses0
    finally:
        eng2.__dict__.pop("_sync_ln_ok", None)
        reset_cores(); reset_stores()


def test_a_step_whose_exchange_gave_up_is_skipped_on_the_device():
    """zk_adam_step(skip_word): non-zero -> parameters, moments and shadow untouched, hyper[6] = NaN, hyper[7] = 1, the
    sticky hyper[10] incremented, in both update forms; zero / NULL -> the ordinary update (bit-identical)."""
    lib = eng().lib
    n = 64 * 1000 + 8
    g = torch.Generator().manual_seed(3)
    mk = lambda s: (torch.randn(n, generator=g) * s).cuda()
    p0, gr, m0, v0 = mk(0.1), mk(0.02), mk(0.01), mk(0.001).abs()
    ws = torch.empty(lib.query("zk_adam_step_workspace"), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def run(word, norm_free):
        hyper = torch.tensor([3e-3, 0.9, 0.98, 1e-8, 0.25, 0.0, 0.5, 0, 0, 0, 0, 0], dtype=torch.float32, device="cuda")
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        sh = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
        pn = torch.zeros(1, device="cuda")
        seed = torch.zeros(1, dtype=torch.int64, device="cuda")
        wd = None if word is None else torch.tensor([word], dtype=torch.int32, device="cuda")
        lib.call("zk_adam_step", p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), sh.data_ptr(), n, hyper.data_ptr(),
                 pn.data_ptr(), seed.data_ptr(), norm_free, None if wd is None else wd.data_ptr(), ws.data_ptr(), ws.numel(),
                 stream)
        torch.cuda.synchronize()
        return p, m, v, sh, hyper.cpu().numpy(), int(seed.item())
    for nf in (1, 0):
        ref = run(None, nf)
        ok = run(0, nf)
        for a, b in zip(ref[:4], ok[:4]):
            assert torch.equal(a, b)
        assert not torch.equal(ref[0], p0) and ref[4][7] == 0 and ref[4][10] == 0
        sk = run(1, nf)
        assert torch.equal(sk[0], p0) and torch.equal(sk[1], m0) and torch.equal(sk[2], v0)
        assert not sk[3].float().abs().sum().item()           # shadow untouched
        assert sk[4][7] == 1 and sk[4][10] == 1 and sk[5] == 1
        if nf:
            assert np.isnan(sk[4][6])


def test_the_exchange_survives_a_busy_second_stream():
    """co-residency of a row block's workgroups is assumed from the grid size; a concurrent stream
    (side-stream batch prep, decode lanes during a dev evaluation) takes CU slots away.  200 exchange launches of the
    training shape (forward and backward forms) run while a second stream keeps every CU busy with large GEMM launches:
    no give-up, no deadlock, results bit-identical to the quiescent ones."""
    e = eng()
    M, N, K = 4096, 512, 512
    A, W, R = rand_bf(M, K, seed=1, scale=0.5), rand_bf(K, N, seed=2, scale=0.05), rand_bf(M, N, seed=3)
    gam, bet = torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")
    dY, W2 = rand_bf(M, K, seed=4, scale=0.5), rand_bf(N, K, seed=5, scale=0.05)
    e.ln_epoch_bump()
    good = _one_launch(e, A, W, None, R, gam, bet, 0.0, 0)
    ds0 = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
    part = torch.empty(e.lib.query("zk_gemm_ln_bwd_partials", M, N) // 4, device="cuda")
    e.gemm_ln_bwd(mat(dY), mat(W2), M, N, K, None, mat(good[1]), good[2], good[3], gam, mat(ds0), None, part)
    torch.cuda.synchronize()
    assert e.sync_ln_errors() == 0
    # the competitor: 4096 x 2048 x 2048 products (512 workgroups of 128 x 128, two rounds of the chip each) and the
    # 1024-thread cross-entropy-sized streaming kernel (zk_zero over 256 MB), alternating
    side = torch.cuda.Stream()
    Xa, Xb = rand_bf(4096, 2048, seed=7, scale=0.1), rand_bf(2048, 2048, seed=8, scale=0.1)
    Xc = torch.empty(4096, 2048, dtype=torch.bfloat16, device="cuda")
    big = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    ds = torch.empty_like(ds0)
    # (the loop's forward saves nothing: the inference form of the launch, whose residual sum is not rounded to bf16)
    e.ln_epoch_bump()
    good_out = _one_launch(e, A, W, None, R, gam, bet, 0.0, 0, save=False)[0].clone()
    torch.cuda.synchronize()
    bad = 0
    for rep in range(4):
        with torch.cuda.stream(side):
            for i in range(60):
                e.gemm(mat(Xa), mat(Xb), mat(Xc), 4096, 2048, 2048, 0, 0)
                if i % 6 == 0:
                    e.zero(big)
        for it in range(50):
            if it % 25 == 0:
                e.ln_epoch_bump()
            e.gemm_add_ln(mat(A), mat(W), M, N, K, None, mat(R), gam, bet, mat(out))
            e.gemm_ln_bwd(mat(dY), mat(W2), M, N, K, None, mat(good[1]), good[2], good[3], gam, mat(ds), None, part)
            if it % 10 == 9:
                torch.cuda.current_stream().synchronize()
                bad += int(not torch.equal(out, good_out)) + int(not torch.equal(ds, ds0))
        torch.cuda.synchronize()
    assert e.sync_ln_errors() == 0 and bad == 0
