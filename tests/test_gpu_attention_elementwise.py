"""zk_attn_fwd / zk_attn_bwd checked per (sentence, head, position) d-vector, on the operand layout of the model:
q / k / v column slices of one guarded [T, 3H] buffer (cross attention: q its own matrix, k / v slices of [T, 2H]), the
output with ld > H, dq / dk / dv written into the slices of a guarded, NaN-prefilled dqkv buffer.  Inputs must be
bit-identical after the calls, nothing outside an output window may change, every output element must be written.

Row check (tests/parity.py): ||got_row - ref_row|| <= c_x max(||ref_row||, rms row norm of the tensor) against the
float64 reference; no row is excused.  c_x is not chosen: it is twice the worst row ratio of the CPU emulation (the same
math in fp32 with bf16 rounding of the probabilities, the attention output and the gradients of scores / q / k / v, the
sites Cfg.store_bf16 of oracle/ref_torch.py names) over all of parity.ATTN_CASES; the factor 2 allows for another
summation order and another exp.  tests/test_parity_checker.py re-measures the emulation on every CPU run (it must stay
within c_x) and shows that a zeroed vector, the neighbouring row's vector and a stale 8-element chunk all fail, planted
at the vector that differs most from its neighbour and at one that differs by the median amount.

    tensor   emulation, worst row ratio over the 20 cases   c_x
    out      3.93e-03                                        7.9e-03
    dq       4.48e-03                                        9.0e-03
    dk       4.08e-03                                        8.2e-03
    dv       4.08e-03                                        8.2e-03
    drk      2.57e-03                                        5.2e-03
    drv      1.88e-03                                        3.8e-03

Found with this check and fixed: k_attn_bwd_dq_mfma (the two-kernel backward: more than one 64-key or 64-query tile,
impl 3) took D_i = rowsum(dO o O) from the stored bf16 O, so every dS_ij of a row carried a common offset
~2^-9 |dO.O| P_ij.  Case (1, 2, 130, 130, causal), impl 2: dq row 2, head 1 (three visible keys) at 9.59e-03, dk at
5.04e-03.  D_i is now sum_j P_ij dP_ij from a first walk over the key tiles, as the single-tile kernel computes it: dq
3.19e-03, dk 3.69e-03 on that case; the worst ratios of all kernels over all cases on an MI355X are then out 3.93e-03,
dq 4.48e-03, dk 3.99e-03, dv 4.08e-03, drk 2.99e-03, drv 2.02e-03.

lse stays a per-element check (2e-2, 3e-2 with relative positions), as in tests/test_gpu_kernels.py.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng  # noqa: E402
from tests import parity as P  # noqa: E402

C_X = {"out": 7.9e-3, "dq": 9.0e-3, "dk": 8.2e-3, "dv": 8.2e-3, "drk": 5.2e-3, "drv": 3.8e-3}
BF, F32 = torch.bfloat16, torch.float32


def run_attention(impl, case):
    e = eng()
    B, nh, Lq, Lk, mask, causal, rpr, drop = case
    d, H, max_rel = P.ATTN_D, nh * P.ATTN_D, P.ATTN_MAX_REL
    x = P.attn_inputs(case)
    Tq, Tk = B * Lq, B * Lk
    G = lambda rows, cols, pad, off, dtype=BF, prefill=None: P.guarded(rows, cols, cols + pad, off, dtype, prefill, "cuda")
    if Lq == Lk:
        qkv = G(Tq, 3 * H, 16, 8, prefill=torch.cat([x["q"], x["k"], x["v"]], 1))
        q, k, v = (qkv.mat.cols_slice(i * H, (i + 1) * H) for i in range(3))
        dqkv = G(Tq, 3 * H, 24, 16)
        dq, dk, dv = (dqkv.mat.cols_slice(i * H, (i + 1) * H) for i in range(3))
        inputs, grads = [qkv], [dqkv]
    else:
        qg = G(Tq, H, 8, 8, prefill=x["q"])
        kv = G(Tk, 2 * H, 24, 16, prefill=torch.cat([x["k"], x["v"]], 1))
        q, k, v = qg.mat, kv.mat.cols_slice(0, H), kv.mat.cols_slice(H, 2 * H)
        dqg, dkv = G(Tq, H, 16, 8), G(Tk, 2 * H, 8, 8)
        dq, dk, dv = dqg.mat, dkv.mat.cols_slice(0, H), dkv.mat.cols_slice(H, 2 * H)
        inputs, grads = [qg, kv], [dqg, dkv]
    out = G(Tq, H, 32, 8)
    dout = G(Tq, H, 8, 0, prefill=x["dout"])
    lse = G(1, B * nh * Lq, 0, 0, F32)
    kmask = x["kmask"].cuda() if x["kmask"] is not None else None
    rk = x["rk"].cuda() if rpr else None
    rv = x["rv"].cuda() if rpr else None
    drk = G(2 * max_rel + 1, d, 0, 0, F32, prefill=torch.zeros(2 * max_rel + 1, d)) if rpr else None
    drv = G(2 * max_rel + 1, d, 0, 0, F32, prefill=torch.zeros(2 * max_rel + 1, d)) if rpr else None
    lse_t = lse.window().view(-1)
    e.set_seed(99)
    e.attn_fwd(q, k, v, out.mat, lse_t, B, nh, Lq, Lk, d, kmask=kmask, causal=causal, rpr_k=rk, rpr_v=rv,
               max_rel=max_rel, drop_p=drop, sid=5, impl=impl)
    torch.cuda.synchronize()
    out.check_guard("out")
    lse.check_guard("lse")
    out.rebase()                 # the backward reads them: bit-identical afterwards
    lse.rebase()
    e.attn_bwd(q, k, v, out.mat, dout.mat, lse_t, dq, dk, dv, B, nh, Lq, Lk, d, kmask=kmask, causal=causal, rpr_k=rk,
               rpr_v=rv, drpr_k=drk.window() if rpr else None, drpr_v=drv.window() if rpr else None, max_rel=max_rel,
               drop_p=drop, sid=5, impl=impl)
    torch.cuda.synchronize()
    drop_mask = None
    if drop > 0:
        n = B * nh * Lq * Lk
        msk = torch.zeros(n, device="cuda")
        e.lib.call("zk_dropout_mask", msk.data_ptr(), n, drop, e.seed.data_ptr(), 5, e.stream)
        torch.cuda.synchronize()
        drop_mask = msk.view(B, nh, Lq, Lk).cpu()
    ref = P.attn_math(x["q"], x["k"], x["v"], x["dout"], B, nh, Lq, Lk, d, kmask=x["kmask"], causal=causal, rk=x["rk"],
                      rv=x["rv"], max_rel=max_rel, drop_mask=drop_mask)
    for g in grads + ([drk, drv] if rpr else []):
        g.check_guard("gradient buffer")
    for g in inputs + [dout, out, lse]:
        g.check_intact("attention operand")
    got = {"out": out.value(), "dq": dq.torch().cpu(), "dk": dk.torch().cpu(), "dv": dv.torch().cpu()}
    if rpr:
        got["drk"], got["drv"] = drk.value(), drv.value()
    what = "impl %d case %s" % (impl, (case,))
    ratios = {key: float(P.attn_row_ratio(got[key], ref[key], d).max()) for key in got}
    lse_err = float((lse.value().view(B, nh, Lq).double() - ref["lse"]).abs().max())
    print(what, {k_: "%.2e" % r for k_, r in ratios.items()}, "lse %.2e" % lse_err)
    for key in got:
        P.assert_attn_rows(got[key], ref[key], d, C_X[key], what + " " + key, heads=nh if key in ("out", "dq", "dk", "dv") else 1)
    assert lse_err < (3e-2 if rpr else 2e-2), (what, lse_err)


# impl 1 = reference kernels, 2 = MFMA, 3 = MFMA backward in the two-kernel form (forward: the reference kernel)
@pytest.mark.parametrize("impl", [1, 2, 3])
@pytest.mark.parametrize("case", [c for c in P.ATTN_CASES if not c[6]])
def test_attention_rows(impl, case):
    run_attention(impl, case)


# relative positions: the reference kernels and the MFMA path (tables folded into the tile, or decomposed)
@pytest.mark.parametrize("impl", [1, 2])
@pytest.mark.parametrize("case", [c for c in P.ATTN_CASES if c[6]])
def test_attention_rows_relative_positions(impl, case):
    run_attention(impl, case)
