"""The single-tile attention backward (k_attn_bwd_fused64) with one LDS image per operand and transposed reads: its dq, dk
and dv must be the BYTES the kernel with transposed copies produced (tests/golden/attn_bwd_parent.json, written by
tests/golden/make_attn_bwd_golden.py on the commit before the change: every MFMA keeps its operand values and k order),
must leave everything beyond the live rows alone, and must agree with the fp32 autograd reference."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attn_bwd_cases as AC  # noqa: E402
from tests.test_gpu_kernels import _attn_ref  # noqa: E402
from tests.util_gpu import eng, rel_err  # noqa: E402
from zero_amd.func import Mat  # noqa: E402


@functools.lru_cache(maxsize=None)
def _case(name):
    c = AC.inputs(name)
    return c, AC.run(c)


@functools.lru_cache(maxsize=None)
def _golden():
    return AC.load()


@pytest.mark.parametrize("name", AC.CASES)
def test_attention_backward_bytes_are_those_of_the_kernel_with_transposed_copies(name):
    _, (dq, dk, dv) = _case(name)
    want = _golden()[name]
    for key, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        got = AC.digest(t)
        assert got["sha256"] == want[key]["sha256"], (name, key, got["head"], want[key]["head"])


@pytest.mark.parametrize("n", [0, 512])
def test_attention_backward_writes_live_rows_only(n):
    """Lq = 37, Lk = 53: tile rows 37 .. 63 / 53 .. 63 are zeros in LDS and take part in every transposed read.  The outputs
    live in NaN-filled buffers with 4 guard rows in front, 4 behind and 8 guard columns per row: every live element must
    come out finite (a NaN or stale word in a dead tile row would reach them through the products) and every other
    element must keep its bit pattern."""
    c = AC.inputs("ragged_mask-%s" % ("plain" if n == 0 else "oproj%d" % n))
    H, G, ld = c["H"], 4, c["H"] + 8
    bufs, mats = [], []
    for rows in (c["B"] * c["Lq"], c["B"] * c["Lk"], c["B"] * c["Lk"]):
        t = torch.full((rows + 2 * G, ld), float("nan"), dtype=torch.bfloat16, device="cuda")
        bufs.append(t)
        mats.append(Mat(t, rows, H, ld, G * ld))
    fill = bufs[0].view(torch.int16)[0, 0].item()
    got = AC.run(c, *mats)
    for t, g, key in zip(bufs, got, ("dq", "dk", "dv")):
        assert torch.isfinite(g.float()).all(), key
        bits = t.view(torch.int16)
        rows = g.shape[0]
        assert bool((bits[:G] == fill).all()) and bool((bits[G + rows:] == fill).all()), key + ": guard rows"
        assert bool((bits[G:G + rows, H:] == fill).all()), key + ": guard columns"
    # and the values are those of the contiguous call
    want = AC.run(c)
    for g, w in zip(got, want):
        assert torch.equal(g, w)


@pytest.mark.parametrize("name", AC.CASES)
def test_attention_backward_against_the_fp32_autograd_reference(name):
    """the bounds of test_attention_d64 / test_attention_dropout (2.5e-2 on the relative Frobenius error)"""
    c, (dq, dk, dv) = _case(name)
    e = eng()
    B, nh, Lq, Lk = c["B"], c["nh"], c["Lq"], c["Lk"]
    drop_mask = None
    if c["drop"] > 0:
        cnt = B * nh * Lq * Lk
        msk = torch.zeros(cnt, device="cuda")
        e.set_seed(AC.SEED)
        e.lib.call("zk_dropout_mask", msk.data_ptr(), cnt, c["drop"], e.seed.data_ptr(), AC.SID, e.stream)
        drop_mask = msk.view(B, nh, Lq, Lk)
    qf, kf, vf = (c[x].float().clone().requires_grad_(True) for x in ("q", "k", "v"))
    o_ref, _, _ = _attn_ref(qf, kf, vf, B, nh, Lq, Lk, AC.D, c["kmask"], c["causal"], drop_mask=drop_mask)
    if c["n"]:
        dout = (c["dy"].float() @ c["Wo"].float().t()).to(torch.bfloat16).float()     # rounded like the GEMM's output
    else:
        dout = c["dout"].float()
    o_ref.backward(dout)
    errs = {"dq": rel_err(dq, qf.grad), "dk": rel_err(dk, kf.grad), "dv": rel_err(dv, vf.grad)}
    print(name, errs)
    assert errs["dq"] < 2.5e-2 and errs["dk"] < 2.5e-2 and errs["dv"] < 2.5e-2, errs
