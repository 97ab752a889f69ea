"""zk_rnn_ff_residual and zk_f32_rnn_ff_residual called directly (zero_amd/csrc/zk_rnn.hip, through Engine.rnn_ff_residual)
and compared element by element with the float64 reference of tests/deepnmt_ref.py under its derived bound.  Every operand
and output is a parity.guarded buffer: outputs are prefilled with NaN, nothing outside their windows may change, inputs must
be bit-identical after the call; every row stride is larger than the row, and out_copy is a column slice of a wider buffer.

Shapes: a pairwise covering (parity.pairwise: every PAIR of levels of two factors occurs in some case; the full product of the
three factors, i.e. every triple, is not run -- the three dimensions meet only in the tile loops, two at a time) of
    R  1, 17, 64, 65, 130            one row, an edge wave, exactly one row block, one row past it, three blocks (two in fp32: 5)
    K  8, 40, 1000, 2048 (+ 4096 in bf16: the largest LDS image, 131 KB)      below one MFMA step, a K tail, past 64 KB of LDS
    N  8, 24, 64, 616 (+ 620 in fp32)      half a bf16 tile, one and a half, exactly one fp32 tile, the recipe's embedding size
Each shape runs three calls: out apart from x with a copy, out == x in place with a copy, and out apart without a copy; odd R
takes the scalar loads of a (a row stride that is no multiple of 16 bytes).  W = 0 with an x that is not bf16-representable:
out is x bit for bit.  Every refusal by its message.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng  # noqa: E402
from tests import parity as P  # noqa: E402
from tests import deepnmt_ref as D  # noqa: E402
from tests import variant_ref as V  # noqa: E402
from tests.rnn_cell_cases import ff_run as _run  # noqa: E402
from zero_amd.func import Mat  # noqa: E402
from zero_amd.hip import ZeroHipError  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
ST = {"bf16": BF, "fp32": F32}


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def _shapes(form):
    Ks = [8, 40, 1000, 2048] + ([4096] if form == "bf16" else [])
    Ns = [8, 24, 64, 616] + ([620] if form == "fp32" else [])
    return [(form, r["R"], r["K"], r["N"]) for r in P.pairwise({"R": [1, 17, 64, 65, 130], "K": Ks, "N": Ns})]


@pytest.mark.parametrize("form,R,K,N", _shapes("bf16") + _shapes("fp32"))
def test_ff_residual(form, R, K, N):
    x = D.ff_inputs(R, K, N, form, R + K + N)
    ref = D.ff_residual(**x)
    label = "%s R=%d K=%d N=%d" % (form, R, K, N)
    worst = {}
    for name, kw in (("apart", {}), ("in place", dict(in_place=True)), ("no copy", dict(with_copy=False))):
        out, cp = _run(x, form, **kw)
        worst[name] = V.assert_within(out, ref["out"], D.ff_residual_bound(ref, form), "%s %s out" % (label, name))
        if cp is not None:
            worst[name + " copy"] = V.assert_within(cp, ref["out"], D.ff_residual_bound(ref, form, True),
                                                    "%s %s copy" % (label, name))
            want = _t(out).float().to(ST[form]).double().numpy()
            assert np.array_equal(cp, want), "the copy is the stream rounded once to the storage type"
    print("%s: largest |err| / bound %s" % (label, "  ".join("%s %.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("form", ["bf16", "fp32"])
def test_ff_residual_keeps_the_stream_in_fp32(form):
    """W = 0, b = 0: out is x.  With an x that is not bf16-representable the bound has no bf16 term, so a kernel that keeps or
    reads the stream in bf16 fails it (tests/test_deepnmt_host.py shows that); a correct one returns x bit for bit."""
    x = D.ff_inputs(17, 40, 24, form, 7, zero_w=True)
    ref = D.ff_residual(**x)
    assert D.ff_residual_bound(ref, form).max() < 2.0 ** -16
    for kw in ({}, dict(in_place=True)):
        out, _ = _run(x, form, **kw)
        assert np.array_equal(out, x["x"])


def _plain(form, R=4, K=16, N=24):
    st = ST[form]
    z = lambda *s, dt=st: torch.zeros(*s, dtype=dt, device="cuda")
    return dict(a=Mat(z(R, K), R, K), W=Mat(z(K, N), K, N), b=z(N, dt=F32), stream=z(2 * R * 2 * N, dt=F32), R=R, K=K, N=N)


@pytest.mark.parametrize("form", ["bf16", "fp32"])
def test_ff_residual_refuses_a_partial_overlap_of_out_and_x(form):
    e = eng()
    p = _plain(form)
    R, N, buf = p["R"], p["N"], p["stream"]
    x = Mat(buf, R, N, 2 * N, 0)
    what = "zk_(f32_)?rnn_ff_residual: out overlaps x without being x"
    with pytest.raises(ZeroHipError, match=what):
        e.rnn_ff_residual(p["a"], p["W"], p["b"], x, Mat(buf, R, N, 2 * N, N - 1))           # one column shared per row
    with pytest.raises(ZeroHipError, match=what):
        e.rnn_ff_residual(p["a"], p["W"], p["b"], x, Mat(buf, R, N, 2 * N + 1, 0))           # the same address, another stride
    with pytest.raises(ZeroHipError, match=what):
        e.rnn_ff_residual(p["a"], p["W"], p["b"], x, Mat(buf, R, N, 2 * N, 2 * N))           # one row down
    # in place, and the two halves of one [R, 2 N] buffer side by side (rows interleave without sharing an element)
    e.rnn_ff_residual(p["a"], p["W"], p["b"], x, x)
    e.rnn_ff_residual(p["a"], p["W"], p["b"], x, Mat(buf, R, N, 2 * N, N))
    torch.cuda.synchronize()
    if form == "fp32":        # a and the outputs share a type there
        with pytest.raises(ZeroHipError, match="zk_f32_rnn_ff_residual: the span of out or out_copy meets the span of a"):
            e.rnn_ff_residual(Mat(buf, R, p["K"], 2 * N, 0), p["W"], p["b"], Mat(torch.zeros(R, N, device="cuda"), R, N), x)


def test_bf16_form_refuses_sizes_it_does_not_take():
    e = eng()
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device="cuda")

    def call(K, N, R=2, ldw=None, woff=0):
        ldw = N if ldw is None else ldw
        W = Mat(z(K * ldw + 16), K, N, ldw, woff)
        st = Mat(z(R, N, dt=F32), R, N)
        e.rnn_ff_residual(Mat(z(R, K), R, K), W, z(N, dt=F32), st, st)
    with pytest.raises(ZeroHipError, match="K and N multiples of 8.*K=20 N=24.*zk_f32_rnn_ff_residual takes any K and N"):
        call(20, 24)
    with pytest.raises(ZeroHipError, match="K and N multiples of 8.*K=16 N=20.*zk_f32_rnn_ff_residual"):
        call(16, 20)
    with pytest.raises(ZeroHipError, match="K at most 4096.*K=4104.*zk_f32_rnn_ff_residual"):
        call(4104, 24)                                # past the LDS image: refused by name, nothing launched
    with pytest.raises(ZeroHipError, match="rows must be 16-byte aligned .ldw=28"):
        call(16, 24, ldw=28)
    with pytest.raises(ZeroHipError, match="rows must be 16-byte aligned .ldw=32, W % 16 = 8"):
        call(16, 24, ldw=32, woff=4)
    call(16, 24, ldw=32, woff=8)
    torch.cuda.synchronize()
