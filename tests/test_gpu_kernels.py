"""GPU parity of every HIP kernel (through the C-ABI) against plain torch fp32 math on the
same bf16 inputs.  The reference (TF1) cannot run; the op semantics checked here are the ones
the oracle (oracle/ref_torch.py) restates from func.py / util.py / search.py."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng, bf, rand_bf, mat, rel_err, max_err  # noqa: E402
from zero_amd import hip  # noqa: E402
from zero_amd.func import Mat  # noqa: E402


# ------------------------------------------------------------------ the bf16 rounding every kernel stores with
def test_bf16_conversion_is_round_to_nearest_even_on_every_class_of_value():
    """f2bf / pack2bf (zk_common.h) compile to v_cvt_pk_bf16_f32 since round 6 (the integer sequence of rounds 1-5 before).
    zk_cast_f32_bf16 exposes exactly that conversion: against round-to-nearest-even computed on the bit patterns (numpy) -- and
    against torch's own cast -- for random values, EXACT ties with even and odd kept mantissas, the neighbours of ties, values
    that round up into the next binade / into infinity, fp32 denormals, signed zeros and infinities; NaN stays NaN."""
    e = eng()
    rng = np.random.default_rng(7)
    hi = rng.integers(0, 1 << 16, size=200000, dtype=np.uint32)          # every exponent, both signs
    hi = hi[(hi & 0x7f80) != 0x7f80]                                       # finite (and zero / denormal) upper halves
    ties = (hi << 16) | 0x8000
    cases = [rng.standard_normal(300000).astype(np.float32).view(np.uint32),
             (rng.standard_normal(100000) * 1e-3).astype(np.float32).view(np.uint32),
             ties, ties + 1, ties - 1, (hi << 16) | 0xffff, (hi << 16) | 0x7fff, hi << 16,
             rng.integers(0, 1 << 23, size=50000, dtype=np.uint32),                     # denormals
             rng.integers(0, 1 << 23, size=50000, dtype=np.uint32) | 0x80000000,
             np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff, 0x7f7f8000, 0x7f7f7fff,
                       0x00008000, 0x00018000, 0x00007fff], dtype=np.uint32)]
    u = np.concatenate([c.astype(np.uint32) for c in cases])
    u = u[: (u.size // 8) * 8]
    want = ((u.astype(np.uint64) + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)     # RNE on the bit pattern
    x = torch.from_numpy(u.view(np.float32).copy()).cuda()
    y = torch.empty(x.numel(), dtype=torch.bfloat16, device="cuda")
    e.lib.call("zk_cast_f32_bf16", x.data_ptr(), y.data_ptr(), x.numel(), e.stream)
    torch.cuda.synchronize()
    got = y.view(torch.int16).cpu().numpy().view(np.uint16)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(hex(int(u[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]]
    assert torch.equal(y, x.to(torch.bfloat16))
    nan = torch.tensor([float("nan"), -float("nan"), 1.0, 2.0, 3.0, 4.0, 5.0, 6.0], device="cuda")
    yn = torch.empty(8, dtype=torch.bfloat16, device="cuda")
    e.lib.call("zk_cast_f32_bf16", nan.data_ptr(), yn.data_ptr(), 8, e.stream)
    torch.cuda.synchronize()
    assert bool(torch.isnan(yn[:2].float()).all()) and torch.equal(yn[2:].float(), nan[2:])


# ------------------------------------------------------------------ hardware layout probes
def test_probe_mfma_layouts():
    e = eng()
    A = rand_bf(32, 16, seed=1); Bt = rand_bf(32, 16, seed=2)
    D = torch.zeros(32, 32, device="cuda")
    e.lib.call("zk_probe_mfma32", A.data_ptr(), Bt.data_ptr(), D.data_ptr(), e.stream)
    torch.cuda.synchronize()
    assert max_err(D, A.float() @ Bt.float().t()) < 1e-4
    A = rand_bf(16, 32, seed=3); Bt = rand_bf(16, 32, seed=4)
    D = torch.zeros(16, 16, device="cuda")
    e.lib.call("zk_probe_mfma16", A.data_ptr(), Bt.data_ptr(), D.data_ptr(), e.stream)
    torch.cuda.synchronize()
    assert max_err(D, A.float() @ Bt.float().t()) < 1e-4


def test_probe_tr16_dump():
    e = eng()
    out = torch.zeros(256, dtype=torch.int16, device="cuda")
    e.lib.call("zk_probe_tr16", out.data_ptr(), e.stream)
    torch.cuda.synchronize()
    print("ds_read_b64_tr_b16 (lds[i]=i, lane l addr=8*l):")
    print(out.cpu().numpy().reshape(64, 4)[:32].tolist())


# ------------------------------------------------------------------ GEMM
def _gemm_case(impl, M, N, K, ta, tb, out_f32=False, bias=False, residual=False, act=0, drop=0.0, alpha=1.0,
               seed=0):
    e = eng()
    A = rand_bf(*((K, M) if ta else (M, K)), seed=seed + 1)
    Bm = rand_bf(*((N, K) if tb else (K, N)), seed=seed + 2)
    C = torch.zeros(M, N, dtype=torch.float32 if out_f32 else torch.bfloat16, device="cuda")
    bias_t = torch.randn(N, device="cuda") if bias else None
    res_t = rand_bf(M, N, seed=seed + 3) if residual else None
    aux_t = rand_bf(M, N, seed=seed + 4) if act == 2 else None
    e.set_seed(1234)
    e.gemm(mat(A), mat(Bm), mat(C), M, N, K, ta, tb, alpha=alpha, bias=bias_t,
           residual=mat(res_t) if residual else None, act=act, aux=mat(aux_t) if act == 2 else None,
           aux_scale=1.25, drop_p=drop, sid=77, impl=impl)
    torch.cuda.synchronize()
    a = A.float().t() if ta else A.float()
    b = Bm.float().t() if tb else Bm.float()
    ref = alpha * (a @ b)
    if bias:
        ref = ref + bias_t
    if residual:
        ref = ref + res_t.float()
    if act == 1:
        ref = torch.relu(ref)
    if act == 2:
        ref = torch.where(aux_t.float() > 0, ref * 1.25, torch.zeros_like(ref))
    if drop > 0:
        msk = torch.zeros(M * N, device="cuda")
        e.lib.call("zk_dropout_mask", msk.data_ptr(), M * N, drop, e.seed.data_ptr(), 77, e.stream)
        torch.cuda.synchronize()
        keep = float((msk > 0).float().mean())
        assert abs(keep - (1 - drop)) < 0.02, keep
        ref = ref * msk.view(M, N)
    return rel_err(C, ref), C, ref


# impl: 1 = reference HIP kernel, 2 = MFMA LDS-DMA ring kernel (default), 3 = MFMA register-staged kernel
@pytest.mark.parametrize("impl", [1, 2, 3])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("shape", [(128, 128, 64), (256, 192, 160), (72, 40, 24), (200, 264, 136), (64, 512, 1024)])
def test_gemm_plain(impl, ta, tb, shape):
    M, N, K = shape
    err, _, _ = _gemm_case(impl, M, N, K, ta, tb)
    assert err < 8e-3, err


@pytest.mark.parametrize("impl", [1, 2, 3])
def test_gemm_ragged_rows(impl):
    # token dimension not a multiple of 8 (M for forward, K for wgrad)
    assert _gemm_case(impl, 100, 64, 72, 0, 0)[0] < 8e-3
    assert _gemm_case(impl, 100, 64, 72, 0, 1)[0] < 8e-3
    assert _gemm_case(impl, 64, 72, 100, 1, 0)[0] < 8e-3


@pytest.mark.parametrize("impl", [1, 2, 3])
def test_gemm_epilogues(impl):
    assert _gemm_case(impl, 192, 256, 128, 0, 0, bias=True)[0] < 8e-3
    assert _gemm_case(impl, 192, 256, 128, 0, 0, bias=True, act=1)[0] < 8e-3
    assert _gemm_case(impl, 192, 256, 128, 0, 1, residual=True)[0] < 8e-3
    assert _gemm_case(impl, 192, 256, 128, 0, 1, act=2)[0] < 8e-3
    assert _gemm_case(impl, 192, 256, 128, 0, 0, bias=True, act=1, drop=0.3)[0] < 8e-3
    assert _gemm_case(impl, 192, 256, 128, 1, 0, out_f32=True)[0] < 2e-3
    assert _gemm_case(impl, 192, 256, 128, 0, 1, out_f32=True, alpha=0.5)[0] < 2e-3


@pytest.mark.parametrize("impl", [2, 3])
def test_gemm_splitk_wgrad(impl):
    # 512x512 output, K=4096: the auto configuration splits K
    err, _, _ = _gemm_case(impl, 512, 512, 4096, 1, 0, out_f32=True)
    assert err < 2e-3, err
    err, _, _ = _gemm_case(impl, 512, 1536, 4096, 1, 0, out_f32=True)
    assert err < 2e-3, err
    err, _, _ = _gemm_case(impl, 4096, 512, 8192, 0, 0)      # split with bf16 output
    assert err < 8e-3, err


@pytest.mark.parametrize("impl", [2, 3])
def test_gemm_base_shapes(impl):
    for (M, N, K, ta, tb, f32) in [(4096, 1536, 512, 0, 0, False), (4096, 512, 2048, 0, 0, False),
                                   (4096, 2048, 512, 0, 1, False), (2048, 512, 4096, 1, 0, True),
                                   (1024, 4000, 512, 0, 1, True), (4000, 520, 1000, 1, 1, False)]:
        err, _, _ = _gemm_case(impl, M, N, K, ta, tb, out_f32=f32)
        assert err < 8e-3, (M, N, K, ta, tb, err)


@pytest.mark.parametrize("impl", [2, 3])
@pytest.mark.parametrize("tile", [1, 2, 3, 4])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_every_tile_shape(impl, tile, ta, tb):
    # force each block-tile variant (impl bits [11:8]) on a ragged shape with a K tail
    err, _, _ = _gemm_case(impl | (tile << 8), 328, 200, 456, ta, tb, bias=True, residual=True)
    assert err < 8e-3, (impl, tile, ta, tb, err)


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_256x128_macro_tile(ta, tb):
    # eight-wave 256x128 tile of the LDS-DMA kernel (impl bits [11:8] = 5): ragged shape with a K tail,
    # epilogues, and a shape smaller than one tile
    assert _gemm_case(2 | (5 << 8), 328, 200, 456, ta, tb, bias=True, residual=True)[0] < 8e-3
    assert _gemm_case(2 | (5 << 8), 600, 384, 128, ta, tb)[0] < 8e-3
    assert _gemm_case(2 | (5 << 8), 72, 40, 24, ta, tb)[0] < 8e-3
    assert _gemm_case(2 | (5 << 8), 512, 256, 512, ta, tb, out_f32=True)[0] < 2e-3


@pytest.mark.parametrize("ta,tb", [(1, 0), (0, 0), (0, 1)])
def test_gemm_grouped(ta, tb):
    e = eng()
    shapes = [(512, 384, 1000), (136, 520, 264), (128, 128, 64), (264, 72, 4096)]
    probs, refs = [], []
    for i, (M, N, K) in enumerate(shapes):
        A = rand_bf(*((K, M) if ta else (M, K)), seed=10 + i)
        Bm = rand_bf(*((N, K) if tb else (K, N)), seed=20 + i)
        f32 = (i % 2 == 0)
        C = torch.zeros(M, N, dtype=torch.float32 if f32 else torch.bfloat16, device="cuda")
        bias = torch.randn(N, device="cuda") if i == 1 else None
        probs.append((mat(A), mat(Bm), mat(C), M, N, K, bias))
        a = A.float().t() if ta else A.float()
        b = Bm.float().t() if tb else Bm.float()
        refs.append(a @ b + (bias if bias is not None else 0))
    for tile in (128, 64):
        for p in probs:
            p[2].t.zero_()
        e.gemm_grouped(probs, ta, tb, tile=tile)
        torch.cuda.synchronize()
        for p, r in zip(probs, refs):
            assert rel_err(p[2].t, r) < 8e-3, (tile, p[3:6], rel_err(p[2].t, r))


@pytest.mark.parametrize("tile", [(256, 256), (256, 256, 0)])
def test_gemm_grouped_256_tiles_with_bias_column_sums(tile):
    """Weight-gradient form (ta = 1, tb = 0: dW = X^T dY, fp32 out) on 256x256 tiles with the bias gradient
    db = column sums of dY (func.py:16, 58-60) by MFMA beside the tm = 0 tiles: ragged M / N / K (K tails of the 64-deep
    two-stage ring), several row tiles, a problem without column sums in the launch."""
    e = eng()
    shapes = [(512, 1536, 1000, True), (136, 520, 264, True), (600, 72, 4096, False), (256, 256, 64, True),
              (264, 300, 40, True), (256, 512, 24, False)]
    probs, refs = [], []
    for i, (M, N, K, cs) in enumerate(shapes):
        X = rand_bf(K, M, seed=30 + i)
        dY = rand_bf(K, N, seed=40 + i)
        C = torch.full((M, N), 3.0, dtype=torch.float32, device="cuda")
        db = torch.full((N,), 9.0, device="cuda") if cs else None
        probs.append((mat(X), mat(dY), mat(C), M, N, K, None, None, db))
        refs.append((X.float().t() @ dY.float(), dY.float().sum(0)))
    e.gemm_grouped(probs, 1, 0, tile=tile)
    torch.cuda.synchronize()
    for p, (r, rcs) in zip(probs, refs):
        assert rel_err(p[2].t, r) < 2e-3, (p[3:6], rel_err(p[2].t, r))
        if p[8] is not None:
            assert rel_err(p[8], rcs) < 1e-4, (p[3:6], rel_err(p[8], rcs))


# ------------------------------------------------------------------ attention
def _attn_ref(q, k, v, B, nh, Lq, Lk, d, kmask, causal, rk=None, rv=None, max_rel=0, drop_mask=None):
    """func.py:218-256 in torch fp32 on [B*L, nh*d] matrices."""
    H = nh * d
    qh = q.float().view(B, Lq, nh, d).permute(0, 2, 1, 3) * d ** -0.5
    kh = k.float().view(B, Lk, nh, d).permute(0, 2, 1, 3)
    vh = v.float().view(B, Lk, nh, d).permute(0, 2, 1, 3)
    lg = qh @ kh.transpose(-1, -2)
    if rk is not None:
        idx = (torch.arange(Lq)[:, None] - torch.arange(Lk)[None, :]).clamp(-max_rel, max_rel) + max_rel
        lg = lg + torch.einsum("bhqd,qkd->bhqk", qh, rk.float()[idx.cuda()])
    if kmask is not None:
        lg = lg + ((1 - kmask) * -1e8)[:, None, None, :]
    if causal:
        lg = lg + (-1e8 * (1 - torch.tril(torch.ones(Lq, Lk, device="cuda"))))[None, None]
    w = torch.softmax(lg, -1)
    lse = torch.logsumexp(lg, -1)
    wd = w if drop_mask is None else w * drop_mask
    o = wd @ vh
    if rv is not None:
        o = o + torch.einsum("bhqk,qkd->bhqd", wd, rv.float()[idx.cuda()])
    return o.permute(0, 2, 1, 3).reshape(B * Lq, H), lse, w


def _attn_case(impl, B, nh, Lq, Lk, d, use_mask, causal, rpr=False, drop=0.0, seed=0):
    e = eng()
    H = nh * d
    max_rel = 4
    qkv_q = rand_bf(B * Lq, H, seed=seed + 1).requires_grad_(False)
    k = rand_bf(B * Lk, H, seed=seed + 2)
    v = rand_bf(B * Lk, H, seed=seed + 3)
    kmask = None
    if use_mask:
        kmask = torch.ones(B, Lk, device="cuda")
        for b in range(B):
            kmask[b, Lk - (b * 3) % max(Lk - 1, 1):] = 0 if b > 0 else 1
        kmask[:, 0] = 1
    rk = rand_bf(2 * max_rel + 1, d, scale=0.3, seed=seed + 4) if rpr else None
    rv = rand_bf(2 * max_rel + 1, d, scale=0.3, seed=seed + 5) if rpr else None
    out = torch.zeros(B * Lq, H, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(B * nh * Lq, device="cuda")
    e.set_seed(99)
    e.attn_fwd(mat(qkv_q), mat(k), mat(v), mat(out), lse, B, nh, Lq, Lk, d, kmask=kmask, causal=causal,
               rpr_k=rk, rpr_v=rv, max_rel=max_rel, drop_p=drop, sid=5, impl=impl)
    torch.cuda.synchronize()
    drop_mask = None
    if drop > 0:
        n = B * nh * Lq * Lk
        msk = torch.zeros(n, device="cuda")
        e.lib.call("zk_dropout_mask", msk.data_ptr(), n, drop, e.seed.data_ptr(), 5, e.stream)
        drop_mask = msk.view(B, nh, Lq, Lk)
    # autograd reference
    qf = qkv_q.float().clone().requires_grad_(True)
    kf = k.float().clone().requires_grad_(True)
    vf = v.float().clone().requires_grad_(True)
    rkf = rk.float().clone().requires_grad_(True) if rpr else None
    rvf = rv.float().clone().requires_grad_(True) if rpr else None
    o_ref, lse_ref, _ = _attn_ref(qf, kf, vf, B, nh, Lq, Lk, d, kmask, causal, rkf, rvf, max_rel, drop_mask)
    errs = {"out": rel_err(out, o_ref), "lse": max_err(lse.view(B, nh, Lq), lse_ref)}
    # backward
    dout = rand_bf(B * Lq, H, seed=seed + 9)
    dq = torch.zeros_like(qkv_q); dk = torch.zeros_like(k); dv = torch.zeros_like(v)
    drk = torch.zeros(2 * max_rel + 1, d, device="cuda") if rpr else None
    drv = torch.zeros(2 * max_rel + 1, d, device="cuda") if rpr else None
    e.attn_bwd(mat(qkv_q), mat(k), mat(v), mat(out), mat(dout), lse, mat(dq), mat(dk), mat(dv), B, nh, Lq, Lk, d,
               kmask=kmask, causal=causal, rpr_k=rk, rpr_v=rv, drpr_k=drk, drpr_v=drv, max_rel=max_rel,
               drop_p=drop, sid=5, impl=impl)
    torch.cuda.synchronize()
    o_ref.backward(dout.float())
    errs["dq"] = rel_err(dq, qf.grad); errs["dk"] = rel_err(dk, kf.grad); errs["dv"] = rel_err(dv, vf.grad)
    if rpr:
        errs["drk"] = rel_err(drk, rkf.grad); errs["drv"] = rel_err(drv, rvf.grad)
    return errs


ATT_CASES = [(2, 2, 64, 64, False, False), (3, 2, 37, 53, True, False), (2, 3, 50, 50, False, True),
             (2, 2, 70, 130, True, False), (1, 2, 130, 130, False, True), (2, 8, 64, 64, True, False)]


# impl 1 = reference kernels, 2 = MFMA (single-tile cases take the fused backward), 3 = MFMA backward
# forced to the two-kernel dQ / dK,dV form (forward falls to the reference kernel)
@pytest.mark.parametrize("impl", [1, 2, 3])
@pytest.mark.parametrize("case", ATT_CASES)
def test_attention_d64(impl, case):
    B, nh, Lq, Lk, um, causal = case
    errs = _attn_case(impl, B, nh, Lq, Lk, 64, um, causal)
    print(impl, case, errs)
    assert errs["out"] < 1.5e-2 and errs["lse"] < 2e-2
    assert errs["dq"] < 2.5e-2 and errs["dk"] < 2.5e-2 and errs["dv"] < 2.5e-2, errs


@pytest.mark.parametrize("impl", [1, 2, 3])
def test_attention_dropout(impl):
    errs = _attn_case(impl, 2, 2, 64, 64, 64, True, False, drop=0.2)
    print(errs)
    assert errs["out"] < 1.5e-2 and errs["dq"] < 2.5e-2 and errs["dk"] < 2.5e-2 and errs["dv"] < 2.5e-2, errs


def _attn_bwd_oproj_pair(B, nh, Lq, Lk, H_out, use_mask, causal, rpr=False, drop=0.0, impl=2, seed=0):
    """attention backward with the gradient of its output given (a) as the matrix dY . W_o^T formed by zk_gemm and
    (b) as the (dY, W_o) pair -> (dq, dk, dv[, drk, drv]) of both."""
    e = eng()
    d = 64
    H = nh * d
    max_rel = 4
    q = rand_bf(B * Lq, H, seed=seed + 1)
    k = rand_bf(B * Lk, H, seed=seed + 2)
    v = rand_bf(B * Lk, H, seed=seed + 3)
    kmask = None
    if use_mask:
        kmask = torch.ones(B, Lk, device="cuda")
        for b in range(1, B):
            kmask[b, Lk - (b * 3) % max(Lk - 1, 1):] = 0
        kmask[:, 0] = 1
    rk = rand_bf(2 * max_rel + 1, d, scale=0.3, seed=seed + 4) if rpr else None
    rv = rand_bf(2 * max_rel + 1, d, scale=0.3, seed=seed + 5) if rpr else None
    out = torch.zeros(B * Lq, H, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(B * nh * Lq, device="cuda")
    e.set_seed(99)
    e.attn_fwd(mat(q), mat(k), mat(v), mat(out), lse, B, nh, Lq, Lk, d, kmask=kmask, causal=causal, rpr_k=rk, rpr_v=rv,
               max_rel=max_rel, drop_p=drop, sid=5, impl=impl)
    dy = rand_bf(B * Lq, H_out, seed=seed + 9)
    Wo = rand_bf(H, H_out, scale=0.05, seed=seed + 10)
    res = []
    for fused in (False, True):
        dout = torch.full((B * Lq, H), float("nan"), dtype=torch.bfloat16, device="cuda")
        if not fused:
            e.gemm(mat(dy), mat(Wo), mat(dout), B * Lq, H, H_out, 0, 1)
        dq = torch.zeros_like(q); dk = torch.zeros_like(k); dv = torch.zeros_like(v)
        drk = torch.zeros(2 * max_rel + 1, d, device="cuda") if rpr else None
        drv = torch.zeros(2 * max_rel + 1, d, device="cuda") if rpr else None
        n0 = e.lib.ncalls
        e.attn_bwd(mat(q), mat(k), mat(v), mat(out), mat(dout), lse, mat(dq), mat(dk), mat(dv), B, nh, Lq, Lk, d,
                   kmask=kmask, causal=causal, rpr_k=rk, rpr_v=rv, drpr_k=drk, drpr_v=drv, max_rel=max_rel, drop_p=drop,
                   sid=5, impl=impl, oproj=(mat(dy), mat(Wo)) if fused else None)
        torch.cuda.synchronize()
        res.append(dict(dq=dq, dk=dk, dv=dv, drk=drk, drv=drv, dout=dout, calls=e.lib.ncalls - n0))
    return res


OPROJ_CASES = [(2, 2, 64, 64, 128, False, False), (3, 8, 37, 53, 512, True, False), (2, 3, 50, 50, 384, False, True),
               (2, 16, 64, 64, 1024, True, False), (1, 2, 1, 7, 128, True, False)]


@pytest.mark.parametrize("case", OPROJ_CASES)
@pytest.mark.parametrize("variant", ["plain", "dropout", "rpr"])
def test_attention_backward_with_the_output_projection_folded_in(case, variant):
    """zk_attn_bwd (oproj_dy, oproj_w): dO = dY . W_o^T computed per (sentence, head) inside the single-tile kernel must
    give what the dgrad GEMM + the plain call give (same bf16 rounding of dO; fp32 summation order inside the
    64 x 64 x n product differs between the two MFMA shapes, hence a tolerance instead of equality)."""
    B, nh, Lq, Lk, n, um, causal = case
    plain, fused = _attn_bwd_oproj_pair(B, nh, Lq, Lk, n, um, causal, rpr=variant == "rpr",
                                        drop=0.2 if variant == "dropout" else 0.0)
    assert torch.isnan(fused["dout"].float()).all(), "the fused call must not have formed dout"
    assert fused["calls"] == 1, fused["calls"]
    for key in ("dq", "dk", "dv") + (("drk", "drv") if variant == "rpr" else ()):
        err = rel_err(fused[key], plain[key].float())
        assert err < 4e-3, (key, err)
        assert torch.isfinite(fused[key].float()).all()


@pytest.mark.parametrize("why", ["long", "impl", "columns"])
def test_attention_backward_forms_the_output_gradient_itself_when_the_fold_does_not_apply(why):
    """return code 2 of zk_attn_bwd: nothing launched, func.attn_bwd runs the GEMM and calls again -> identical results"""
    if why == "long":
        plain, fused = _attn_bwd_oproj_pair(2, 2, 70, 130, 128, True, False)
    elif why == "impl":
        plain, fused = _attn_bwd_oproj_pair(2, 2, 64, 64, 128, True, False, impl=3)
    else:
        plain, fused = _attn_bwd_oproj_pair(2, 2, 64, 64, 192, True, False)      # n not a multiple of 128
    assert fused["calls"] >= 3                      # declined call + GEMM + the plain call
    assert torch.equal(fused["dout"], plain["dout"])
    for key in ("dq", "dk", "dv"):
        assert torch.equal(fused[key], plain[key]), key


def test_attention_small_head_and_rpr():
    errs = _attn_case(1, 2, 2, 9, 11, 8, True, False)
    assert max(errs.values()) < 2.5e-2, errs
    errs = _attn_case(1, 2, 2, 20, 20, 64, False, True, rpr=True)
    print(errs)
    assert max(errs.values()) < 2.5e-2, errs
    errs = _attn_case(1, 2, 2, 13, 17, 16, True, False, rpr=True)
    assert max(errs.values()) < 2.5e-2, errs


def test_attention_fully_masked_row_is_uniform():
    # func.py:386: the mask is a finite -1e8, so an all-pad key row softmaxes to uniform
    e = eng()
    B, nh, L, d = 1, 1, 8, 64
    q = rand_bf(L, d, seed=1); k = rand_bf(L, d, seed=2); v = rand_bf(L, d, seed=3)
    kmask = torch.zeros(B, L, device="cuda")
    for impl in (1, 2):
        out = torch.zeros(L, d, dtype=torch.bfloat16, device="cuda")
        e.attn_fwd(mat(q), mat(k), mat(v), mat(out), None, B, nh, L, L, d, kmask=kmask, impl=impl)
        torch.cuda.synchronize()
        assert max_err(out, v.float().mean(0, keepdim=True).expand(L, d)) < 2e-2


# ------------------------------------------------------------------ embedding / LN / colsum
def test_embed_fwd_bwd():
    e = eng()
    B, L, H, V = 3, 7, 64, 50
    ids = torch.randint(0, V, (B, L), dtype=torch.int32, device="cuda")
    table = rand_bf(V, H, seed=1); bias = torch.randn(H, device="cuda")
    tim = e.timing(L + 5, H)
    for shift in (False, True):
        out = torch.zeros(B * L, H, dtype=torch.bfloat16, device="cuda")
        e.embed_fwd(ids, table, bias, mat(out), B, L, H, shift=shift)
        torch.cuda.synchronize()
        emb = table.float()[ids.long()] * H ** 0.5 + bias
        if shift:
            emb = torch.cat([torch.zeros(B, 1, H, device="cuda"), emb[:, :-1]], 1)
        ref = emb + tim[:L][None]
        assert rel_err(out.view(B, L, H), ref) < 5e-3
        dout = rand_bf(B * L, H, seed=5)
        dtab = torch.zeros(V, H, device="cuda"); dbias = torch.zeros(H, device="cuda")
        e.embed_bwd(ids, mat(dout), dtab, dbias, B, L, H, shift=shift)
        torch.cuda.synchronize()
        g = dout.float().view(B, L, H)
        idl = ids.long()
        if shift:
            g = g[:, 1:]; idl = idl[:, :-1]
        ref_t = torch.zeros(V, H, device="cuda").index_add_(0, idl.reshape(-1), g.reshape(-1, H) * H ** 0.5)
        assert rel_err(dtab, ref_t) < 1e-4 and rel_err(dbias, g.reshape(-1, H).sum(0)) < 1e-4
    # decode position + zero flag
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    out = torch.zeros(B, H, dtype=torch.bfloat16, device="cuda")
    e.embed_fwd(ids[:, 0].contiguous(), table, bias, mat(out), B, 1, H, pos0=4, zero_flag=flag)
    torch.cuda.synchronize()
    assert rel_err(out, tim[4][None].expand(B, H)) < 5e-3


@pytest.mark.parametrize("H", [64, 512, 1024])
def test_embed_bwd_sorted_long_runs_of_one_id(H):
    """A frequent id (the eos of every sentence) owns a long run of rows: runs of 1 .. 150 rows (more than the 64
    indices one coalesced load brings in, not a multiple of the 8-row batches), with dropout regenerated per element;
    the sums must equal the serial walk's (fp32, same order) -- checked against an index_add in float64."""
    from tests.common import device_sort_arrays
    e = eng()
    B, L, V = 30, 17, 40
    rng = np.random.default_rng(11)
    ids_np = rng.integers(3, V, (B, L))
    ids_np[:, -1] = 2                      # eos in every sentence: a run of 30
    ids_np[:10, 3:] = 7                    # a run of 140
    ids_np[rng.random((B, L)) < 0.2] = 5   # and a scattered one
    dout = rand_bf(B * L, H, seed=7)
    srt = device_sort_arrays(e, "runs%d" % H, ids_np, False)
    dtab = torch.zeros(V, H, device="cuda")
    e.set_seed(97)
    e.embed_bwd_sorted(srt, mat(dout), dtab, H, accumulate=False, drop_p=0.5, sid=13)
    msk = torch.zeros(B * L * H, device="cuda")
    e.lib.call("zk_dropout_mask", msk.data_ptr(), B * L * H, 0.5, e.seed.data_ptr(), 13, e.stream)
    torch.cuda.synchronize()
    assert 0.4 < float((msk == 0).float().mean()) < 0.6 and set(msk.unique().tolist()) == {0.0, 2.0}
    ref = torch.zeros(V, H, dtype=torch.float64, device="cuda")
    ref.index_add_(0, torch.tensor(ids_np.reshape(-1), device="cuda"), dout.double() * msk.view(B * L, H).double() * H ** 0.5)
    assert rel_err(dtab, ref.float()) < 2e-6
    assert float(dtab[0].abs().max()) == 0.0


def test_embed_bwd_sorted_and_bias_colsum():
    # atomics-free table gradient (rows grouped by id on the device) + shared-bias gradient with skipped rows
    from tests.common import device_sort_arrays
    e = eng()
    B, L, H, V = 4, 9, 64, 23
    rng = np.random.default_rng(3)
    ids_np = rng.integers(0, V, (B, L))
    ids = torch.tensor(ids_np, dtype=torch.int32, device="cuda")
    dout = rand_bf(B * L, H, seed=5)
    for shift in (False, True):
        srt = device_sort_arrays(e, "t%d" % shift, ids_np, shift)
        for acc in (False, True):
            dtab = torch.full((V, H), 0.5 if acc else 0.0, device="cuda")
            e.embed_bwd_sorted(srt, mat(dout), dtab, H, accumulate=acc)
            dbias = torch.full((H,), 3.0, device="cuda")
            e.colsum(mat(dout), dbias, skip_L=L if shift else 0, accumulate=acc)
            torch.cuda.synchronize()
            g = dout.float().view(B, L, H)
            idl = ids.long()
            if shift:
                g = g[:, 1:]; idl = idl[:, :-1]
            ref_t = torch.full((V, H), 0.5 if acc else 0.0, device="cuda")
            ref_t.index_add_(0, idl.reshape(-1), g.reshape(-1, H) * H ** 0.5)
            assert rel_err(dtab, ref_t) < 1e-5
            ref_b = g.reshape(-1, H).sum(0) + (3.0 if acc else 0.0)
            assert rel_err(dbias, ref_b) < 1e-5


@pytest.mark.parametrize("B,L,V", [(64, 64, 32000), (1, 1, 5), (3, 2, 7), (50, 100, 32000), (79, 63, 200),
                                   (160, 128, 70000), (5, 1, 9)])
def test_batch_prep_groups_rows_like_the_stable_host_sort(B, L, V):
    """zk_batch_prep against numpy's stable argsort + unique (what rounds 1-3 computed on the host): rows, group
    boundaries, ids and the group count must be IDENTICAL -- so that zk_embed_bwd_sorted adds the rows of an id in the
    same order and the table gradient is bit-identical.  Sizes: the bench batch (4096 rows: keys in 32 KB of LDS),
    5000 rows (the 128-KB instantiation), 20480 rows (keys in the global scratch), degenerate shapes; eos runs;
    ids beyond 16 bits.  Also the masks / loss weights against zk_make_mask / zk_target_stats' definitions."""
    from tests.common import host_sort_arrays, device_sort_arrays
    e = eng()
    rng = np.random.default_rng(B * 1000 + L)
    ids = rng.integers(0, V, (B, L))
    ids[:, -1] = 2
    if L > 4:
        ids[::3, L // 2:] = 0              # ragged rows: padding
    for shift, max_id in ((False, 0), (True, 0), (False, V), (True, V)):      # max_id = V: 32-bit keys where they fit
        srt = device_sort_arrays(e, "p%d" % shift, ids, shift, max_id)
        torch.cuda.synchronize()
        rows, seg, uid = host_sort_arrays(ids, shift)
        n = int(srt["n"].cpu()[0])
        assert n == len(uid)
        assert np.array_equal(srt["uid"].cpu().numpy()[:n], uid)
        assert np.array_equal(srt["seg"].cpu().numpy()[:n + 1], seg)
        assert np.array_equal(srt["rows"].cpu().numpy()[:len(rows)], rows)
    # masks and loss weights in the same launch
    dev_s = e.buf("t.m.src", (B, L), torch.int32); dev_s.copy_(torch.from_numpy(ids.astype(np.int32)))
    batch = {"B": B, "Ls": L, "Lt": L, "src": dev_s, "tgt": dev_s, "smask": e.buf("t.m.sm", (B, L), torch.float32),
             "tmask": e.buf("t.m.tm", (B, L), torch.float32), "tw": e.buf("t.m.tw", (B, L), torch.float32), "tw_scale": 2.0}
    e.batch_prep(batch)
    torch.cuda.synchronize()
    m = (ids != 0).astype(np.float32)
    assert np.array_equal(batch["smask"].cpu().numpy(), m) and np.array_equal(batch["tmask"].cpu().numpy(), m)
    w = 2.0 * m / (m.sum(1, keepdims=True) * B)
    assert np.allclose(batch["tw"].cpu().numpy(), w, rtol=1e-6, atol=0)


def test_timing_signal_closed_form():
    from zero_amd.func import timing_table
    t = timing_table(5, 8)
    inv = np.exp(-np.arange(4) * math.log(1e4) / 3.0)
    assert np.allclose(t[3, :4], np.sin(3 * inv), atol=1e-6) and np.allclose(t[3, 4:], np.cos(3 * inv), atol=1e-6)


@pytest.mark.parametrize("H", [64, 512, 1024])
@pytest.mark.parametrize("drop", [0.0, 0.25])
def test_add_ln_fwd_bwd(H, drop):
    e = eng()
    T = 37
    x = rand_bf(T, H, seed=1); y = rand_bf(T, H, seed=2)
    gamma = (1 + 0.1 * torch.randn(H)).cuda(); beta = (0.1 * torch.randn(H)).cuda()
    out = torch.zeros(T, H, dtype=torch.bfloat16, device="cuda"); s = torch.zeros_like(out)
    mean = torch.zeros(T, device="cuda"); rstd = torch.zeros(T, device="cuda")
    e.set_seed(5)
    e.add_ln_fwd(mat(x), mat(y), gamma, beta, mat(out), mat(s), mean, rstd, drop, 3)
    msk = torch.ones(T * H, device="cuda")
    if drop > 0:
        e.lib.call("zk_dropout_mask", msk.data_ptr(), T * H, drop, e.seed.data_ptr(), 3, e.stream)
    torch.cuda.synchronize()
    msk = msk.view(T, H)
    xf = x.float().clone().requires_grad_(True); yf = y.float().clone().requires_grad_(True)
    gf = gamma.clone().requires_grad_(True); bfp = beta.clone().requires_grad_(True)
    sf = xf + yf * msk
    mu = sf.mean(-1, keepdim=True); var = ((sf - mu) ** 2).mean(-1, keepdim=True)
    ref = gf * (sf - mu) * torch.rsqrt(var + 1e-8) + bfp
    assert rel_err(out, ref) < 6e-3 and rel_err(s, sf) < 5e-3
    # the fp32 statistics the backward (and tests/test_gpu_sync_ln.py) build on: against float64 of the STORED sum, with the
    # derived bounds of tests/parity.py (the unbiased variance moves rstd by 1 / (2 H), a bf16 `out` does not show that)
    from tests import parity
    bounds = parity.ln_fwd_bound(x, y, msk if drop > 0 else None, gamma, beta, float(torch.tensor(1e-8)), s_stored=s)
    parity.assert_elementwise(mean, *bounds["mean"], "add_ln_fwd mean")
    parity.assert_elementwise(rstd, *bounds["rstd"], "add_ln_fwd rstd")
    dout = rand_bf(T, H, seed=3)
    ref.backward(dout.float())
    dsum = torch.zeros_like(out); dy = torch.zeros_like(out)
    dg = torch.zeros(H, device="cuda"); db = torch.zeros(H, device="cuda"); dbp = torch.zeros(H, device="cuda")
    e.add_ln_bwd(mat(dout), mat(s), mean, rstd, gamma, mat(dsum), mat(dy) if drop > 0 else None, dg, db, dbp,
                 drop, 3)
    torch.cuda.synchronize()
    assert rel_err(dsum, xf.grad) < 1.5e-2, rel_err(dsum, xf.grad)
    if drop > 0:
        assert rel_err(dy, yf.grad) < 1.5e-2
    assert rel_err(dg, gf.grad) < 1.5e-2 and rel_err(db, bfp.grad) < 1e-3
    assert rel_err(dbp, yf.grad.sum(0)) < 1.5e-2


def test_layer_norm_constant_row_gives_offset():
    # known answer: LN of a constant row is exactly `offset` (eps=1e-8 keeps rstd finite)
    e = eng()
    H = 64
    x = bf(torch.full((2, H), 3.0)).cuda()
    gamma = torch.ones(H, device="cuda") * 2; beta = torch.randn(H, device="cuda")
    out = torch.zeros(2, H, dtype=torch.bfloat16, device="cuda")
    e.add_ln_fwd(mat(x), None, gamma, beta, mat(out))
    torch.cuda.synchronize()
    assert max_err(out, bf(beta)[None].expand(2, H)) < 1e-6


def test_colsum():
    e = eng()
    for rows, N, ld, off in [(100, 64, 64, 0), (4096, 1536, 1536, 0), (300, 128, 256, 128)]:
        a = rand_bf(rows, ld, seed=1)
        out = torch.zeros(N, device="cuda")
        e.colsum(Mat(a, rows, N, ld, off), out)
        torch.cuda.synchronize()
        assert rel_err(out, a.float()[:, off:off + N].sum(0)) < 1e-4


# ------------------------------------------------------------------ loss
@pytest.mark.parametrize("V,ld", [(11, 16), (1000, 1000), (32000, 32000), (517, 520)])
@pytest.mark.parametrize("ls", [0.0, 0.1])
def test_ce_fused(V, ld, ls):
    e = eng()
    T = 19
    logits = torch.zeros(T, ld, device="cuda")
    logits[:, :V] = torch.randn(T, V, device="cuda") * 3
    logits[:, V:] = 777.0   # pad columns must be ignored
    ids = torch.randint(0, V, (T,), dtype=torch.int32, device="cuda")
    w = torch.rand(T, device="cuda"); w[3] = 0
    ce = torch.zeros(T, device="cuda")
    dl = torch.full((T, ld), 5.0, dtype=torch.bfloat16, device="cuda")
    e.ce_fused(Mat(logits, T, ld), ids, w, ce, Mat(dl, T, ld), T, V, ls)
    torch.cuda.synchronize()
    z = logits[:, :V].clone().requires_grad_(True)
    if ls > 0:
        n = V - 1.0; p = 1 - ls; q = ls / n
        soft = torch.full((T, V), q, device="cuda"); soft[torch.arange(T), ids.long()] = p
        norm = -(p * math.log(p) + n * q * math.log(q + 1e-20))
    else:
        soft = torch.zeros(T, V, device="cuda"); soft[torch.arange(T), ids.long()] = 1.0
        norm = 0.0
    ref = -(soft * torch.log_softmax(z, -1)).sum(-1) - norm
    assert max_err(ce, ref) < 2e-4 * max(1.0, float(ref.abs().max()))
    (ref * w).sum().backward()
    assert rel_err(dl[:, :V], z.grad) < 6e-3
    assert float(dl[:, V:].float().abs().max()) == 0.0 if ld > V else True


def test_uniform_logits_known_answer():
    # all-equal logits: ce = log V - normaliser exactly (label smoothing on)
    e = eng()
    V, T, ls = 64, 4, 0.1
    logits = torch.zeros(T, V, device="cuda")
    ids = torch.tensor([0, 1, 2, 63], dtype=torch.int32, device="cuda")
    ce = torch.zeros(T, device="cuda")
    e.ce_fused(Mat(logits, T, V), ids, None, ce, None, T, V, ls)
    torch.cuda.synchronize()
    n = V - 1.0; p = 1 - ls; q = ls / n
    norm = -(p * math.log(p) + n * q * math.log(q + 1e-20))
    assert max_err(ce, torch.full((T,), math.log(V) - norm)) < 1e-5


def test_target_stats_and_loss_reduce():
    e = eng()
    B, L = 4, 6
    ids = torch.tensor([[5, 6, 2, 0, 0, 0], [7, 8, 9, 10, 11, 2], [3, 2, 0, 0, 0, 0], [4, 4, 4, 2, 0, 0]],
                       dtype=torch.int32, device="cuda")
    mask = torch.zeros(B, L, device="cuda"); w = torch.zeros(B, L, device="cuda")
    e.target_stats(ids, mask, w, B, L, 2.0)
    ce = torch.rand(B, L, device="cuda")
    ps = torch.zeros(B, device="cuda"); loss = torch.zeros(1, device="cuda")
    e.loss_reduce(ce, ids, ps, loss, B, L)
    torch.cuda.synchronize()
    m = (ids != 0).float()
    assert max_err(mask, m) == 0
    assert max_err(w, 2.0 * m / (m.sum(1, keepdim=True) * B)) < 1e-7
    ref = (ce * m).sum(1) / m.sum(1)
    assert max_err(ps, ref) < 1e-6 and abs(float(loss) - float(ref.mean())) < 1e-6


# ------------------------------------------------------------------ AAN
@pytest.mark.parametrize("use_mask", [True, False])
def test_aan_scan_and_gate(use_mask):
    e = eng()
    B, L, H = 3, 9, 64
    x = rand_bf(B * L, H, seed=1)
    mask = torch.ones(B, L, device="cuda"); mask[1, 6:] = 0; mask[2, 3:] = 0
    cat = torch.zeros(B * L, 2 * H, dtype=torch.bfloat16, device="cuda")
    e.aan_fwd(mat(x), mask, mat(cat), B, L, H, use_mask)
    torch.cuda.synchronize()
    xf = x.float().view(B, L, H).clone().requires_grad_(True)
    if use_mask:   # func.py:390-398
        cum = torch.cumsum(torch.eye(L, device="cuda"), 0)[None]
        mm = mask[:, None, :] * mask[:, :, None] * cum
        wgt = torch.softmax(mm + (1 - mm) * -1e8, -1) * mm
        y = wgt @ xf
    else:          # transformer_aan.py:103-108
        c = torch.cumsum(mask, 1); c = torch.where(c <= 0, torch.ones_like(c), c)
        y = torch.cumsum(xf, 1) / c[..., None]
    assert rel_err(cat[:, :H], x) == 0 and rel_err(cat[:, H:], y.reshape(B * L, H)) < 6e-3
    # gate + backward chain against autograd
    z = rand_bf(B * L, 2 * H, seed=2)
    g = torch.zeros(B * L, H, dtype=torch.bfloat16, device="cuda")
    e.aan_gate_fwd(mat(z), mat(cat), mat(g), B * L, H)
    zf = z.float().clone().requires_grad_(True)
    catf = cat.float().clone().requires_grad_(True)
    gref = torch.sigmoid(zf[:, :H]) * catf[:, :H] + torch.sigmoid(zf[:, H:]) * catf[:, H:]
    torch.cuda.synchronize()
    assert rel_err(g, gref) < 6e-3
    dg = rand_bf(B * L, H, seed=3)
    gref.backward(dg.float())
    dz = torch.zeros_like(z); dxg = torch.zeros_like(g); dyg = torch.zeros_like(g)
    e.aan_gate_bwd(mat(dg), mat(z), mat(cat), mat(dz), mat(dxg), mat(dyg), B * L, H)
    torch.cuda.synchronize()
    assert rel_err(dz, zf.grad) < 1e-2 and rel_err(dxg, catf.grad[:, :H]) < 1e-2
    assert rel_err(dyg, catf.grad[:, H:]) < 1e-2
    # scan backward: dx = ds + dxg + dcat_x + revscan(dyg + dcat_y)
    dcat = rand_bf(B * L, 2 * H, seed=4); ds = rand_bf(B * L, H, seed=5)
    dx = torch.zeros_like(g)
    e.aan_bwd(mat(dcat), mat(dxg), mat(dyg), mat(ds), mask, mat(dx), B, L, H, use_mask)
    torch.cuda.synchronize()
    y.backward((dyg.float() + dcat.float()[:, H:]).view(B, L, H))
    ref = ds.float() + dxg.float() + dcat.float()[:, :H] + xf.grad.reshape(B * L, H)
    assert rel_err(dx, ref) < 1e-2


# ------------------------------------------------------------------ optimiser
def test_l2norm_and_adam_tf1_semantics():
    e = eng()
    torch.manual_seed(20260927)          # the data decides how large m / sqrt(v) gets: keep it fixed
    n = 100003
    n_pad = (n + 3) // 4 * 4
    p = torch.randn(n_pad, device="cuda"); g = torch.randn(n_pad, device="cuda") * 0.1
    m = torch.rand(n_pad, device="cuda") * 0.01; v = torch.rand(n_pad, device="cuda") * 0.001
    sh = torch.zeros(n_pad, dtype=torch.bfloat16, device="cuda")
    hyper = torch.zeros(12, device="cuda")
    ws = torch.empty(e.lib.query("zk_norm_workspace"), dtype=torch.uint8, device="cuda")
    e.lib.call("zk_l2norm", g.data_ptr(), n, 0.5, hyper.data_ptr() + 24, ws.data_ptr(), ws.numel(), e.stream)
    torch.cuda.synchronize()
    gn = 0.5 * float(g[:n].double().norm())
    assert abs(float(hyper[6]) - gn) / gn < 1e-5
    lr, b1, b2, eps, clip = 0.01, 0.9, 0.98, 1e-8, gn * 0.5
    hyper[:6] = torch.tensor([lr, b1, b2, eps, 0.5, clip])
    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    pn = torch.zeros(1, device="cuda")
    e.lib.call("zk_adam", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), sh.data_ptr(), n,
               hyper.data_ptr(), pn.data_ptr(), ws.data_ptr(), ws.numel(), e.stream)
    torch.cuda.synchronize()
    assert abs(float(pn) - float(p0[:n].double().norm())) / float(p0[:n].double().norm()) < 1e-5
    gg = g * 0.5 * (clip / max(gn, clip))
    m1 = b1 * m0 + (1 - b1) * gg; v1 = b2 * v0 + (1 - b2) * gg * gg
    p1 = p0 - lr * m1 / (v1.sqrt() + eps)
    assert max_err(m[:n], m1[:n]) < 1e-7 and max_err(v[:n], v1[:n]) < 1e-8
    # the update lr * m / (sqrt(v) + eps) can be O(1) where v is tiny: tolerance relative to its size
    upd = (p1 - p0)[:n].abs()
    assert bool(((p[:n] - p1[:n]).abs() <= 1e-6 + 2e-6 * upd).all())
    assert max_err(sh[:n], p[:n].to(torch.bfloat16)) == 0     # the shadow is the rounded NEW parameter
    # non-finite norm -> update skipped, flag raised
    hyper[6] = float("nan")
    pb = p.clone()
    e.lib.call("zk_adam", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), sh.data_ptr(), n,
               hyper.data_ptr(), None, None, 0, e.stream)
    torch.cuda.synchronize()
    assert float(hyper[7]) == 1.0 and max_err(p, pb) == 0
    # safe_nan (main.py:325-329): a finite norm above hyper[9] skips the update as well
    hyper[6], hyper[7], hyper[9] = 5.0, 0.0, 4.0
    e.lib.call("zk_adam", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), sh.data_ptr(), n,
               hyper.data_ptr(), None, None, 0, e.stream)
    torch.cuda.synchronize()
    assert float(hyper[7]) == 1.0 and max_err(p, pb) == 0
    hyper[7], hyper[9] = 0.0, 6.0
    e.lib.call("zk_adam", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), sh.data_ptr(), n,
               hyper.data_ptr(), None, None, 0, e.stream)
    torch.cuda.synchronize()
    assert float(hyper[7]) == 0.0 and max_err(p, pb) > 0


# ------------------------------------------------------------------ decode tail
@pytest.mark.parametrize("B,K,V,ld", [(3, 4, 1000, 1000), (2, 1, 37, 40), (5, 4, 32000, 32000), (2, 8, 517, 520),
                                     (1, 2, 70001, 70008), (2, 3, 9, 16)])   # 70001: one-block-per-row fallback
def test_beam_topk(B, K, V, ld):
    e = eng()
    logits = torch.zeros(B * K, ld, device="cuda")
    logits[:, :V] = torch.randn(B * K, V, device="cuda") * 2
    logits[0, 5] = logits[0, 9] = 6.5   # an exact tie: lower flat index must win
    prev = torch.randn(B * K, device="cuda")
    ts = torch.zeros(B, 2 * K, device="cuda"); ti = torch.zeros(B, 2 * K, dtype=torch.int32, device="cuda")
    pen = 1.2345
    for forbid in (2, -1):
        e.beam_topk(Mat(logits, B * K, ld), prev, ts, ti, B, K, V, 2 * K, 1.0, pen, forbid, 1e8)
        torch.cuda.synchronize()
        lp = logits[:, :V] - torch.logsumexp(logits[:, :V], -1, keepdim=True)
        if forbid >= 0:
            lp[:, forbid] += -1e8
        sc = ((prev[:, None] + lp) / pen).view(B, K * V).cpu().numpy()
        idx = np.argsort(-sc, axis=-1, kind="stable")[:, :2 * K]
        ref_s = np.take_along_axis(sc, idx, -1)
        assert np.array_equal(ti.cpu().numpy(), idx), (ti.cpu().numpy(), idx)
        assert np.abs(ts.cpu().numpy() - ref_s).max() < 1e-4


def test_beam_topk_device_scalars():
    # the per-step scalars (length penalty, EOS ban) can come from device memory (captured graphs)
    e = eng()
    B, K, V = 2, 4, 300
    logits = torch.randn(B * K, V, device="cuda")
    prev = torch.randn(B * K, device="cuda")
    outs = []
    for mode in ("args", "dev"):
        ts = torch.zeros(B, 2 * K, device="cuda"); ti = torch.zeros(B, 2 * K, dtype=torch.int32, device="cuda")
        scal = torch.tensor([np.float32(1.7).view(np.int32), 2], dtype=torch.int32, device="cuda")
        if mode == "args":
            e.beam_topk(Mat(logits, B * K, V), prev, ts, ti, B, K, V, 2 * K, 1.0, 1.7, 2, 1e8)
        else:
            e.beam_topk(Mat(logits, B * K, V), prev, ts, ti, B, K, V, 2 * K, 1.0, 99.0, -1, 1e8, scal_dev=scal)
        torch.cuda.synchronize()
        outs.append((ts.cpu().numpy(), ti.cpu().numpy()))
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][0], outs[1][0])


def test_gather_rows():
    e = eng()
    src = torch.randn(6, 40, device="cuda")
    idx = torch.tensor([3, 3, 0, 5], dtype=torch.int32, device="cuda")
    dst = torch.zeros(4, 64, device="cuda")
    e.lib.call("zk_gather_rows", src.data_ptr(), 160, idx.data_ptr(), dst.data_ptr(), 256, 4, 32 * 4, e.stream)
    torch.cuda.synchronize()
    assert max_err(dst[:, :32], src[idx.long(), :32]) == 0 and float(dst[:, 32:].abs().max()) == 0


# ------------------------------------------------------------------ merged attention / EMA helpers
@pytest.mark.parametrize("B,L,H", [(3, 7, 64), (2, 64, 512), (5, 1, 16)])
def test_cumavg_add_fwd_bwd(B, L, H):
    """func.py:258-275 + 390-398: out = att + W vq with W = row-normalised causal∧valid matrix."""
    e = eng()
    vq = rand_bf(B * L, H, seed=1); att = rand_bf(B * L, H, seed=2); dy = rand_bf(B * L, H, seed=3)
    mask = torch.ones(B, L, device="cuda")
    for b in range(1, B):
        mask[b, max(1, L - b):] = 0
    if L > 3:
        mask[0, 2] = 0                       # a hole in the middle of a row
    out = torch.empty_like(att); dvq = torch.empty_like(vq)
    e.cumavg_add_fwd(mat(vq), mask, mat(att), mat(out), B, L, H)
    e.cumavg_bwd(mat(dy), mask, mat(dvq), B, L, H)
    torch.cuda.synchronize()
    m = mask
    pair = m[:, None, :] * m[:, :, None] * torch.tril(torch.ones(L, L, device="cuda"))[None]
    W = torch.softmax(pair + (1 - pair) * -1e8, -1) * pair
    v = vq.float().view(B, L, H).clone().requires_grad_(True)
    ref = att.float().view(B, L, H) + W @ v
    ref.backward(dy.float().view(B, L, H))
    assert rel_err(out.view(B, L, H), ref) < 6e-3
    assert rel_err(dvq.view(B, L, H), v.grad) < 6e-3
    # in place (out aliases att) gives the same result
    att2 = att.clone()
    e.cumavg_add_fwd(mat(vq), mask, mat(att2), mat(att2), B, L, H)
    torch.cuda.synchronize()
    assert torch.equal(att2, out)


def test_fuse_decode_and_add_bf16():
    e = eng()
    rows, H = 12, 64
    vq = rand_bf(rows, H, seed=4); att = rand_bf(rows, H, seed=5)
    cache = torch.randn(rows, H, device="cuda")
    ref_cache = cache + vq.float()
    ref_att = att.float() + ref_cache / 4.0
    tdev = torch.tensor([3], dtype=torch.int32, device="cuda")
    c1, a1 = cache.clone(), att.clone()
    e.lib.call("zk_fuse_decode", vq.data_ptr(), c1.data_ptr(), a1.data_ptr(), rows, H, 0.25, None, e.stream)
    c2, a2 = cache.clone(), att.clone()
    e.lib.call("zk_fuse_decode", vq.data_ptr(), c2.data_ptr(), a2.data_ptr(), rows, H, 1.0, tdev.data_ptr(), e.stream)
    torch.cuda.synchronize()
    assert max_err(c1, ref_cache) < 1e-6 and rel_err(a1, ref_att) < 5e-3
    assert torch.equal(c1, c2) and torch.equal(a1, a2)          # host scalar == device time step
    a = rand_bf(rows, 3 * H, seed=6); b = rand_bf(rows, 2 * H, seed=7)
    out = torch.zeros(rows, H, dtype=torch.bfloat16, device="cuda")
    e.lib.call("zk_add_bf16", out.data_ptr(), H, a.data_ptr() + H * 2, 3 * H, b.data_ptr() + H * 2, 2 * H, rows, H,
               e.stream)
    torch.cuda.synchronize()
    assert rel_err(out, a[:, H:2 * H].float() + b[:, H:].float()) < 5e-3


def test_ema_kernel_and_skip():
    e = eng()
    n = 1000 * 4 + 3
    p = torch.randn(n, device="cuda"); ema = torch.randn(n, device="cuda")
    hyper = torch.zeros(12, device="cuda")
    hyper[6], hyper[8] = 1.5, 0.9
    want = ema - (1 - 0.9) * (ema - p)
    got = ema.clone()
    e.lib.call("zk_ema", got.data_ptr(), p.data_ptr(), hyper.data_ptr(), n, e.stream)
    torch.cuda.synchronize()
    assert max_err(got, want) < 1e-6
    hyper[6] = float("nan")                  # non-finite gradient norm: the update (and the EMA) is skipped
    got2 = ema.clone()
    e.lib.call("zk_ema", got2.data_ptr(), p.data_ptr(), hyper.data_ptr(), n, e.stream)
    torch.cuda.synchronize()
    assert torch.equal(got2, ema)


def test_gumbel_noise_distribution():
    """util.py:189-195: -log(-log(u)) has mean = Euler's gamma and variance pi^2/6."""
    e = eng()
    rows, V, ld = 64, 5000, 5008
    logits = torch.zeros(rows, ld, device="cuda")
    e.set_seed(5)
    e.lib.call("zk_add_gumbel", logits.data_ptr(), rows, V, ld, 1e-8, e.seed.data_ptr(), 1, e.stream)
    torch.cuda.synchronize()
    x = logits[:, :V].double()
    assert float(logits[:, V:].abs().max()) == 0.0                    # padding columns untouched
    assert abs(float(x.mean()) - 0.5772) < 0.01 and abs(float(x.var()) - np.pi ** 2 / 6) < 0.03
    again = torch.zeros(rows, ld, device="cuda")
    e.lib.call("zk_add_gumbel", again.data_ptr(), rows, V, ld, 1e-8, e.seed.data_ptr(), 1, e.stream)
    torch.cuda.synchronize()
    assert torch.equal(again, logits)                                 # counter-based: same seed, same noise


@pytest.mark.parametrize("variant", [2, 4])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_two_wave_workgroups(variant, ta, tb):
    """The 64x64 tile with two-wave workgroups (A/B variant selected by zk_tune key 4)."""
    e = eng()
    old = e.lib.raw("zk_tune")(4, variant)
    try:
        for M, N, K in [(128, 128, 64), (200, 264, 136), (72, 40, 24), (64, 512, 1024)]:
            err, _, _ = _gemm_case(2 | (4 << 8), M, N, K, ta, tb)
            assert err < 8e-3, (M, N, K, err)
        assert _gemm_case(2 | (4 << 8), 192, 256, 128, 0, 0, bias=True, act=1, drop=0.3)[0] < 8e-3
        assert _gemm_case(2 | (4 << 8), 192, 256, 128, 0, 1, residual=True)[0] < 8e-3
    finally:
        e.lib.raw("zk_tune")(4, old)


@pytest.mark.parametrize("tile,tune", [(4, 0), (4, 2), (4, 4), (4, 8), (1, 0), (1, 2 << 4), (1, 4 << 4), (1, 8 << 4),
                                       (1, (4 << 4) | 256), (2, 4 << 12), (3, 8 << 12)])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_producer_wave_workgroups(tile, tune, ta, tb):
    """Producer-wave workgroups of the gen-2 GEMM (zk_tune key 6; 0x44 is the default): every variant against
    the fp32 reference over ragged / K-tail / split-free shapes and the fused epilogues, and the epilogue-free
    result bit-identical to the variant without producer waves (same MFMA order)."""
    e = eng()
    old = e.lib.raw("zk_tune")(6, tune)
    try:
        impl = 2 | (tile << 8) | (1 << 16)
        for M, N, K in [(128, 128, 64), (200, 264, 136), (72, 40, 24), (256, 512, 1024), (136, 136, 72)]:
            err, _, _ = _gemm_case(impl, M, N, K, ta, tb)
            assert err < 8e-3, (M, N, K, err)
        assert _gemm_case(impl, 192, 256, 128, ta, tb, bias=True, act=1, drop=0.3)[0] < 8e-3
        assert _gemm_case(impl, 192, 256, 128, ta, tb, residual=True)[0] < 8e-3
        M, N, K = 384, 256, 200
        A = torch.randn((K, M) if ta else (M, K), device="cuda").bfloat16()
        B = torch.randn((N, K) if tb else (K, N), device="cuda").bfloat16()
        outs = []
        for t in (tune, 0):
            e.lib.raw("zk_tune")(6, t)
            C = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
            e.gemm(Mat(A, *A.shape), Mat(B, *B.shape), Mat(C, M, N), M, N, K, ta, tb, impl=impl)
            torch.cuda.synchronize()
            outs.append(C)
        assert torch.equal(outs[0], outs[1])
    finally:
        e.lib.raw("zk_tune")(6, old)


@pytest.mark.parametrize("tb", [0, 1])
@pytest.mark.parametrize("shape", [(4096, 512, 512, 12), (200, 264, 128, 3), (72, 40, 64, 1), (130, 512, 192, 16)])
def test_gemm_k_segmented(tb, shape):
    """zk_gemm_kseg: C = sum_s A_s B_s with every segment its own matrix, against the fp32 sum of products;
    with and without the residual (which may alias C)."""
    e = eng()
    M, N, kseg, nseg = shape
    A = [rand_bf(M, kseg, seed=10 + i) for i in range(nseg)]
    Bm = [rand_bf(*((N, kseg) if tb else (kseg, N)), seed=40 + i) for i in range(nseg)]
    C = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
    e.gemm_kseg([(mat(a), mat(b)) for a, b in zip(A, Bm)], mat(C), M, N, kseg, tb)
    torch.cuda.synchronize()
    ref = sum(a.float() @ (b.float().t() if tb else b.float()) for a, b in zip(A, Bm))
    assert rel_err(C, ref) < 8e-3
    R = rand_bf(M, N, seed=99)
    C2 = R.clone()
    e.gemm_kseg([(mat(a), mat(b)) for a, b in zip(A, Bm)], mat(C2), M, N, kseg, tb, residual=mat(C2))
    torch.cuda.synchronize()
    assert rel_err(C2, ref + R.float()) < 8e-3
    with pytest.raises(hip.ZeroHipError):
        e.gemm_kseg([(mat(A[0]), mat(Bm[0]))] * 17, mat(C), M, N, kseg, tb)


@pytest.mark.parametrize("tile", [6, 7])
@pytest.mark.parametrize("tt", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("ns", [0, 2])
def test_gemm_wide_register_tiles(tile, tt, ns):
    """256x128 / 128x256 workgroup tiles with a 128x64 register tile per compute wave + four producer waves (ring depth
    3 or 2): every transposition, ragged M / N / K, epilogues, fp32 and bf16 outputs, split-K -- against fp32 torch."""
    e = eng()
    ta, tb = tt
    for (M, N, K, f32, split) in [(512, 512, 256, 0, 0), (304, 520, 200, 1, 0), (776, 264, 4096, 1, 3), (256, 768, 72, 0, 0)]:
        A = rand_bf(K, M, seed=1) if ta else rand_bf(M, K, seed=1)
        Bm = rand_bf(N, K, seed=2) if tb else rand_bf(K, N, seed=2)
        bias = torch.randn(N, device="cuda") if not split else None
        res = rand_bf(M, N, seed=3) if not split else None
        C = torch.zeros(M, N, device="cuda", dtype=torch.float32 if f32 else torch.bfloat16)
        e.gemm(mat(A), mat(Bm), mat(C), M, N, K, ta, tb, bias=bias, residual=mat(res) if res is not None else None,
               act=1 if not split else 0, impl=2 | (tile << 8) | (split << 16) | (ns << 24))
        torch.cuda.synchronize()
        ref = (A.float().t() if ta else A.float()) @ (Bm.float().t() if tb else Bm.float())
        if bias is not None:
            ref = torch.relu(ref + bias + res.float())
        assert rel_err(C, ref) < (1e-5 if f32 else 8e-3), (tile, tt, ns, M, N, K, rel_err(C, ref))


def test_gemm_plan_reports_producer_waves():
    """zk_gemm_plan labels the instance that runs: bits [30:28] carry the producer waves of the tile class."""
    e = eng()
    plan = e.lib.raw("zk_gemm_plan")
    old = e.lib.raw("zk_tune")(6, 0x44)
    try:
        code = plan(4096, 512, 512, 0, 1)
        assert (code & 255, ((code >> 8) & 255) * 8, ((code >> 16) & 255) * 8, (code >> 28) & 7) == (2, 64, 64, 4)
        wide = plan(4096, 512, 32000, 0, 1)          # dlogits x E: 128x256 tiles of 128x64 register tiles, split 4
        assert (((wide >> 8) & 255) * 8, ((wide >> 16) & 255) * 8, (wide >> 24) & 15, (wide >> 28) & 7) == (128, 256, 4, 4)
        e.lib.raw("zk_tune")(6, 0)
        assert (plan(4096, 512, 512, 0, 1) >> 28) & 7 == 0
    finally:
        e.lib.raw("zk_tune")(6, old)


@pytest.mark.parametrize("case", [(2, 2, 64, 64, False, True), (3, 2, 37, 53, True, False), (2, 8, 64, 64, True, False),
                                  (2, 2, 20, 20, False, True), (2, 2, 70, 130, True, False), (1, 2, 130, 130, False, True),
                                  (2, 2, 100, 40, False, False)])
def test_attention_rpr_on_mfma_kernels(case):
    """modules/rpr.py on the MFMA path (decomposed: gather of Q.Rk^T, bucket sums of P / dS, table GEMMs)
    against the autograd reference, forward and backward, incl. both table gradients."""
    B, nh, Lq, Lk, um, causal = case
    errs = _attn_case(2, B, nh, Lq, Lk, 64, um, causal, rpr=True)
    print(case, errs)
    assert errs["out"] < 1.5e-2 and errs["lse"] < 3e-2
    assert max(errs[k] for k in ("dq", "dk", "dv", "drk", "drv")) < 3e-2, errs


@pytest.mark.parametrize("case", [(2, 2, 64, 64, False, True, 0.0), (3, 8, 37, 53, True, False, 0.0), (2, 2, 20, 20, False, True, 0.2),
                                  (4, 8, 64, 64, True, False, 0.1), (1, 1, 1, 1, False, False, 0.0)])
def test_attention_rpr_backward_in_72kb_equals_the_resident_form(case):
    """k_attn_bwd_rpr64 (tiles taking turns in 72 KB of LDS, two workgroups per CU, bucket sums from the registers of
    phase 1) against k_attn_bwd_fused64<true> (impl | 1024: every tile resident, bucket sums by a second walk over the LDS
    tiles): the same MFMA sequences per output on the same bf16 P / dS; only the fp32 order of the two clipped-tail sums
    differs, i.e. a rare last-bit flip of a bf16 bucket -> gradients equal to ~1e-3, the untouched dK / dV bit for bit."""
    B, nh, Lq, Lk, um, causal, drop = case
    e = eng()
    res = []
    for resident in (True, False):
        old = e.rpr_bwd_resident
        e.rpr_bwd_resident = resident
        try:
            plain, _ = _attn_bwd_oproj_pair(B, nh, Lq, Lk, 128, um, causal, rpr=True, drop=drop)
        finally:
            e.rpr_bwd_resident = old
        res.append(plain)
    for key in ("dk", "dv"):
        assert torch.equal(res[0][key], res[1][key]), (key, rel_err(res[1][key], res[0][key].float()))
    for key in ("dq", "drk", "drv"):
        assert rel_err(res[1][key], res[0][key].float()) < 2e-3, (key, rel_err(res[1][key], res[0][key].float()))


def test_attention_rpr_mfma_forward_long_keys_and_dropout():
    # auto dispatch with several key / query tiles (two-kernel backward), then dropout on the fused one
    errs = _attn_case(0, 2, 2, 70, 130, 64, True, False, rpr=True)
    assert errs["out"] < 1.5e-2 and max(errs[k] for k in ("dq", "dk", "dv", "drk", "drv")) < 3e-2, errs
    errs = _attn_case(2, 2, 2, 64, 64, 64, True, False, rpr=True, drop=0.2)
    assert errs["out"] < 1.5e-2 and max(errs[k] for k in ("dq", "dk", "dv", "drk", "drv")) < 3e-2, errs


@pytest.mark.parametrize("tile", [(128, 256), (256, 128)])
def test_grouped_wgrad_with_folded_bias_column_sums(tile):
    """zk_gemm_grouped on the wide tiles: the producer waves of the tm = 0 tiles also write sum_k dY[k][n] (the bias
    gradient of func.py:14-65 linear) -- several problems in one grid, ragged K / N, against fp32 torch."""
    e = eng()
    probs, refs = [], []
    for i, (K, Min, Nout) in enumerate([(4096, 512, 1536), (1000, 512, 520), (72, 128, 64), (4096, 2048, 512)]):
        X, dY = rand_bf(K, Min, seed=10 + i), rand_bf(K, Nout, seed=20 + i)
        G = torch.zeros(Min, Nout, device="cuda")
        cs = torch.full((Nout,), 7.0, device="cuda")
        probs.append((mat(X), mat(dY), mat(G), Min, Nout, K, None, None, cs if i != 2 else None))
        refs.append((G, X.float().t() @ dY.float(), cs, dY.float().sum(0)))
    e.gemm_grouped(probs, 1, 0, tile=tile)
    torch.cuda.synchronize()
    for i, (G, gref, cs, cref) in enumerate(refs):
        assert rel_err(G, gref) < 1e-5, i
        if i != 2:
            assert rel_err(cs, cref) < 1e-5, (i, rel_err(cs, cref))
        else:
            assert float(cs.min()) == 7.0                 # no output requested: untouched


def test_dropout_decisions_are_fair_and_independent():
    """The dropout hash (zk_common.h: two decisions per mixer round, 16 bits each): keep rate = 1 - p to sampling noise
    for several p, the two halves of a pair and neighbouring pairs are independent (joint drop rate p^2), different sites
    and seeds give different masks, and the 8-element form used by the row kernels is the per-element function."""
    e = eng()
    n = 1 << 22
    msk = torch.empty(n, device="cuda")
    for p in (0.1, 0.3, 0.5):
        e.set_seed(123)
        e.lib.call("zk_dropout_mask", msk.data_ptr(), n, p, e.seed.data_ptr(), 9, e.stream)
        torch.cuda.synchronize()
        keep = (msk > 0).double()
        assert abs(float(msk.max()) - 1.0 / (1.0 - p)) < 1e-5
        sd = (p * (1 - p) / n) ** 0.5
        assert abs(float(keep.mean()) - (1 - p)) < 5 * sd + 2.0 ** -16, (p, float(keep.mean()))
        d = 1.0 - keep
        for lag in (1, 2, 3, 8, 512):           # within a pair, across pairs, the next row of a 512-wide matrix
            joint = float((d[:-lag] * d[lag:]).mean())
            assert abs(joint - p * p) < 6 * (p * p * (1 - p * p) / n) ** 0.5 + 1e-4, (p, lag, joint)
    e.lib.call("zk_dropout_mask", msk.data_ptr(), n, 0.1, e.seed.data_ptr(), 9, e.stream)
    m2 = torch.empty(n, device="cuda")
    e.lib.call("zk_dropout_mask", m2.data_ptr(), n, 0.1, e.seed.data_ptr(), 10, e.stream)
    torch.cuda.synchronize()
    agree = float(((msk > 0) == (m2 > 0)).double().mean())
    assert abs(agree - (0.81 + 0.01)) < 2e-3          # independent masks agree with probability (1-p)^2 + p^2
    # the row kernels' 8-wide form == the per-element mask: residual + LayerNorm forward stores x + dropout(y)
    T, H = 257, 512
    x, y = rand_bf(T, H, seed=1), rand_bf(T, H, seed=2)
    out, ssum = torch.empty_like(x), torch.empty_like(x)
    e.add_ln_fwd(mat(x), mat(y), torch.ones(H, device="cuda"), torch.zeros(H, device="cuda"), mat(out), mat(ssum), None, None, 0.3, 21)
    mk = torch.empty(T * H, device="cuda")
    e.lib.call("zk_dropout_mask", mk.data_ptr(), T * H, 0.3, e.seed.data_ptr(), 21, e.stream)
    torch.cuda.synchronize()
    want = (x.float() + y.float() * mk.view(T, H)).to(torch.bfloat16)
    assert torch.equal(ssum, want)


def test_the_copy_node_of_a_captured_graph_takes_new_arguments():
    """zk_graph_set_copy_many: the one zk_copy_many launch inside an instantiated graph is re-pointed before a replay (the
    training step's graph starts with the copy out of a staging set that changes from step to step); a destination in PINNED
    HOST memory works too (the commit's sequence word); graphs without, or with two, such launches are refused."""
    import ctypes
    from zero_amd.hip import ZeroHipError
    e = eng()
    a = [torch.arange(1000, dtype=torch.int32, device="cuda") + 1000 * k for k in range(3)]
    b = [torch.full((7,), float(k), device="cuda") for k in range(3)]
    da, db = torch.zeros(1000, dtype=torch.int32, device="cuda"), torch.zeros(7, device="cuda")
    pin = torch.full((1,), -1, dtype=torch.int32).pin_memory()
    seq = [torch.tensor([40 + k], dtype=torch.int32, device="cuda") for k in range(3)]
    y = torch.zeros(1000, device="cuda")
    with torch.cuda.stream(e.work_stream):
        def body():
            e.copy_many([(da, a[0]), (db, b[0]), (pin, seq[0])])
            y.copy_(da.float() * 2)                     # a consumer behind the copy, inside the same graph
        body()
        torch.cuda.synchronize()
        g = e.graph_capture(body)
        for k in (1, 2, 0, 2):
            assert e.graph_set_copy_many(g, [(da, a[k]), (db, b[k]), (pin, seq[k])])
            e.graph_launch(g)
            torch.cuda.synchronize()
            assert torch.equal(da, a[k]) and torch.equal(db, b[k]) and torch.equal(y, a[k].float() * 2)
            assert int(pin[0]) == 40 + k
        assert not e.graph_set_copy_many(g, [])         # nothing to copy: not one launch
        g0 = e.graph_capture(lambda: y.mul_(1.0))
        with pytest.raises(ZeroHipError):
            e.graph_set_copy_many(g0, [(da, a[0])])
        g2 = e.graph_capture(lambda: (e.copy_many([(da, a[0])]), e.copy_many([(db, b[0])])))
        with pytest.raises(ZeroHipError):
            e.graph_set_copy_many(g2, [(da, a[1])])
        for h in (g, g0, g2):
            e.lib.call("zk_graph_destroy", h)
