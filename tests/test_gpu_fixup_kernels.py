"""zk_fixup_residual / zk_fixup_relu_shift and their zk_f32_ forms called directly (zero_amd/csrc/zk_fixup.hip) and compared
element by element with the float64 statements of tests/fixup_ref.py under its derived bounds.  Every operand and output
is a parity.guarded buffer: outputs are prefilled with NaN, nothing outside their windows may change, inputs must be
bit-identical after the call.  tests/test_fixup_host.py shows on the CPU that a correct stand-in passes this check on every
case and that each planted defect fails it on at least one.

Cases (fixup_ref.CASES / FFN_CASES): (rows 1, H 128), (rows 5, H 136, ld 200: column slices of a wider matrix), (rows 130,
H 2048); x NULL, y NULL, xs_out NULL, x_out NULL, each scalar NULL; x_out aliasing x and the ReLU pass in place; a branch
below half a bf16 ulp of x, which must still move the fp32 stream; a captured graph replayed after the device scalars were
overwritten; a hidden size that is no multiple of 8, refused without a launch.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng  # noqa: E402
from tests import parity as P  # noqa: E402
from tests import fixup_ref as R  # noqa: E402
from tests import variant_ref as V  # noqa: E402

F32 = torch.float32
ENTRY = {"bf16": "zk_fixup_residual", "fp32": "zk_f32_fixup_residual"}
FFN_ENTRY = {"bf16": "zk_fixup_relu_shift", "fp32": "zk_f32_fixup_relu_shift"}
INT = {"bf16": torch.int16, "fp32": torch.int32}


def G(rows, cols, ld, dtype, prefill=None, off=0):
    return P.guarded(rows, cols, ld, off, dtype, prefill, "cuda")


def _scalar(v):
    return None if v is None else torch.tensor([v], dtype=F32, device="cuda")


class Operands(object):
    """The guarded operands of one residual case and the argument tuple of the entry points."""

    def __init__(self, name, form, x):
        cs = R.CASES[name]
        st = V.STORAGE[form]
        rows, H, ld = cs["rows"], cs["H"], cs["ld"]
        null = cs.get("null", ())
        off = 8 if ld > H else 0                                  # a column slice that does not start the row
        self.cs, self.rows, self.H = cs, rows, H
        self.x = G(rows, H, ld, F32, x["x"], off) if x["x"] is not None else None
        self.y = G(rows, H, ld, st, x["y"], off) if x["y"] is not None else None
        self.alias = bool(cs.get("alias"))
        self.x_out = None if "x_out" in null else (self.x if self.alias else G(rows, H, ld, F32, None, off))
        self.xs = None if "xs_out" in null else G(rows, H, ld, st, None, off)
        self.a, self.o, self.b = _scalar(x["a"]), _scalar(x["o"]), _scalar(x["b"])

    def args(self, stream):
        mp = lambda g: (g.mat.ptr, g.ld) if g is not None else (None, 0)
        sp = lambda t: t.data_ptr() if t is not None else None
        return mp(self.x) + mp(self.y) + (sp(self.a), sp(self.o), sp(self.b)) + mp(self.x_out) + mp(self.xs) + \
            (self.rows, self.H, stream)

    def check(self, what):
        if self.y is not None:
            self.y.check_intact(what + " y")
        if self.x is not None:
            (self.x.check_guard if self.alias else self.x.check_intact)(what + " x")
        for g in (self.x_out, self.xs):
            if g is not None:
                g.check_guard(what + " output")


def _assert_case(ops, ref, form, what):
    bx, bxs = R.residual_bound(ref, V.STORAGE[form])
    r = 0.0
    if ops.x_out is not None:
        r = max(r, V.assert_within(ops.x_out.value().double().numpy(), ref["x_out"], bx, what + " x_out"))
    if ops.xs is not None:
        r = max(r, V.assert_within(ops.xs.value().double().numpy(), ref["xs"], bxs, what + " xs_out"))
    return r


RUNS = [(name, form) for name in R.CASES for form in ("bf16", "fp32")]


@pytest.mark.parametrize("name,form", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_residual_case(name, form):
    e = eng()
    x = R.case_inputs(name, form)
    ref = R.case_reference(name, x, form)
    ops = Operands(name, form, x)
    e.lib.call(ENTRY[form], *ops.args(e.stream))
    torch.cuda.synchronize()
    ops.check(ENTRY[form] + " " + name)
    ratio = _assert_case(ops, ref, form, "%s %s" % (name, form))
    print("%s %s: largest |err| / bound %.3f" % (name, form, ratio))
    if name == "small_update":
        # every update is below half a bf16 ulp of x (tests/test_fixup_host.py): the fp32 stream still moves, everywhere
        got = ops.x_out.value()
        assert (got != x["x"]).all()
        assert (got.bfloat16() == x["x"].bfloat16()).float().mean() > 0.5


FFN_RUNS = [(name, form, inplace) for name in R.FFN_CASES for form in ("bf16", "fp32") for inplace in (False, True)
            if not inplace or name in ("strided", "wide")]


@pytest.mark.parametrize("name,form,inplace", FFN_RUNS, ids=["%s-%s%s" % (n, f, "-inplace" if i else "") for n, f, i in FFN_RUNS])
def test_relu_shift_case(name, form, inplace):
    e = eng()
    cs = R.FFN_CASES[name]
    st = V.STORAGE[form]
    x = R.case_inputs(name, form, ffn=True)
    ref = R.case_reference(name, x, form, ffn=True)
    off = 8 if cs["ld"] > cs["H"] else 0
    h = G(cs["rows"], cs["H"], cs["ld"], st, x["h"], off)
    out = h if inplace else G(cs["rows"], cs["H"], cs["ld"], st, None, off)
    o = _scalar(x["o"])
    e.lib.call(FFN_ENTRY[form], h.mat.ptr, h.ld, o.data_ptr() if o is not None else None, out.mat.ptr, out.ld, cs["rows"], cs["H"],
               e.stream)
    torch.cuda.synchronize()
    if not inplace:
        h.check_intact(FFN_ENTRY[form] + " h")
    out.check_guard(FFN_ENTRY[form] + " output")
    ratio = V.assert_within(out.value().double().numpy(), ref["out"], R.relu_shift_bound(ref, st), "%s %s" % (name, form))
    print("%s %s: largest |err| / bound %.3f" % (name, form, ratio))


@pytest.mark.parametrize("form", ["bf16", "fp32"])
def test_a_replayed_graph_reads_the_new_scalars(form):
    """Both kernels captured once with the scalars (1.25, 0.375, 0.8125); the device scalars are overwritten with (0.5, -1.5,
    2.0) and the graph replayed: the outputs are those of the NEW values (the reference with the old ones is the planted
    defect host_baked, which tests/test_fixup_host.py shows to leave the bound)."""
    e = eng()
    st = V.STORAGE[form]
    x = R.case_inputs("strided", form)
    fx = R.case_inputs("strided", form, ffn=True)
    cs = R.CASES["strided"]
    with torch.cuda.stream(e.work_stream):
        ops = Operands("strided", form, x)
        h = G(cs["rows"], cs["H"], cs["ld"], st, fx["h"], 8)
        hout = G(cs["rows"], cs["H"], cs["ld"], st, None, 8)
        torch.cuda.synchronize()

        def body():
            e.lib.call(ENTRY[form], *ops.args(e.stream))
            e.lib.call(FFN_ENTRY[form], h.mat.ptr, h.ld, ops.o.data_ptr(), hout.mat.ptr, hout.ld, cs["rows"], cs["H"], e.stream)
        g = e.graph_capture(body)
        try:
            assert torch.isnan(ops.xs.value()).all() and torch.isnan(hout.value()).all(), "capturing must not run the kernels"
            e.graph_launch(g)
            torch.cuda.synchronize()
            _assert_case(ops, R.case_reference("strided", x, form), form, "first replay")
            V.assert_within(hout.value().double().numpy(), R.case_reference("strided", fx, form, ffn=True)["out"],
                     R.relu_shift_bound(R.case_reference("strided", fx, form, ffn=True), st), "first replay, relu_shift")
            for t, v in zip((ops.a, ops.o, ops.b), R.STALE):      # "a weight reload": new values at the same addresses
                t.fill_(v)
            e.graph_launch(g)
            torch.cuda.synchronize()
        finally:
            e.lib.call("zk_graph_destroy", g)
    n = lambda t: t.double().numpy()
    ref = R.residual(n(x["x"]), n(x["y"]), *R.STALE, st=st)
    _assert_case(ops, ref, form, "replay with new scalars")
    fref = R.relu_shift(n(fx["h"]), R.STALE[1])
    V.assert_within(hout.value().double().numpy(), fref["out"], R.relu_shift_bound(fref, st), "replay with new scalars, relu_shift")
    ops.check("replayed " + ENTRY[form])
    h.check_intact("replayed relu_shift h")
    hout.check_guard("replayed relu_shift output")


@pytest.mark.parametrize("form", ["bf16", "fp32"])
def test_a_misaligned_width_is_refused_without_a_launch(form):
    e = eng()
    st = V.STORAGE[form]
    rows, H = 3, 132                      # a multiple of 4, not of 8
    g = torch.Generator().manual_seed(2)
    x, y = G(rows, H, 136, F32, torch.randn(rows, H, generator=g)), G(rows, H, 136, st, torch.randn(rows, H, generator=g))
    xo, xs = G(rows, H, 136, F32), G(rows, H, 136, st)
    rc = e.lib.raw(ENTRY[form])(x.mat.ptr, 136, y.mat.ptr, 136, None, None, None, xo.mat.ptr, 136, xs.mat.ptr, 136, rows, H, e.stream)
    msg = e.lib.raw("zk_last_error_string")()
    assert rc == -1 and b"multiple of 8" in msg, (rc, msg)
    rc = e.lib.raw(FFN_ENTRY[form])(y.mat.ptr, 136, None, xs.mat.ptr, 136, rows, H, e.stream)
    msg = e.lib.raw("zk_last_error_string")()
    assert rc == -1 and b"multiple of 8" in msg, (rc, msg)
    # a row stride that would misalign the rows
    rc = e.lib.raw(ENTRY[form])(x.mat.ptr, 132, y.mat.ptr, 132, None, None, None, xo.mat.ptr, 132, xs.mat.ptr, 132, rows, 128, e.stream)
    assert rc == -1
    torch.cuda.synchronize()
    for b in (x, y, xo, xs):
        b.check_intact("the refused call's operand")
    assert torch.isnan(xo.value()).all() and torch.isnan(xs.value()).all()
