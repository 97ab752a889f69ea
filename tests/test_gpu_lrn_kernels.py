"""zk_rnn_lrn_scan and zk_f32_rnn_lrn_scan called directly (zero_amd/csrc/zk_rnn.hip, through Engine.rnn_lrn_scan) and compared
element by element with the float64 reference of tests/lrn_ref.py under its propagated bound.  Every operand and output is a
parity.guarded buffer: outputs are prefilled with NaN, nothing outside their windows may change, inputs must be bit-identical
after the call.  Every operand has its own layout: lo position-major, hi sentence-major, seq position-major with another row
stride, the mask [R, T] with padded rows -- so a kernel that mixes up a position stride with a row stride, or one operand's with
another's, reads or writes the wrong element.

Shapes (R, H, T), the smallest that reach every edge
    bf16: (5, 72, 3) a partial wave, (33, 128, 17) nine waves and more positions than the operand ring has stages several times
          over, (3, 1000, 5) the recipe's width (125 groups per row: rows straddle waves), (2, 2048, 2) fewer positions than stages;
    fp32: (5, 20, 3), (33, 128, 17), (3, 12, 1) one position.
Each with lrn and olrn, single and paired, forward and reverse; a null state, and a gather index that repeats rows; masks that
are all ones, and mixed: an all-zero row, a hole in the middle, trailing padding (which a reversed scan meets first).  Carried
rows are bit-equal.  A T-step launch is bit-equal to T chained one-step launches.  Every refusal leaves its buffers untouched.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng  # noqa: E402
from tests import parity as P  # noqa: E402
from tests import lrn_ref as L  # noqa: E402
from tests import variant_ref as V  # noqa: E402
from zero_amd.func import Mat  # noqa: E402
from zero_amd.hip import ZeroHipError  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
ST = {"bf16": BF, "fp32": F32}
SHAPES = [("bf16", 5, 72, 3), ("bf16", 33, 128, 17), ("bf16", 3, 1000, 5), ("bf16", 2, 2048, 2),
          ("fp32", 5, 20, 3), ("fp32", 33, 128, 17), ("fp32", 3, 12, 1)]


def G(rows, cols, ld=None, off=0, dtype=BF, prefill=None):
    return P.guarded(rows, cols, ld, off, dtype, prefill, "cuda")


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64))


class Bufs(object):
    """The guarded operands of one launch.  Strides in elements; every stride and offset a multiple of 8."""

    def __init__(self, x, form, gated, with_seq=True):
        st = ST[form]
        T, R, W = x["lo"].shape
        H = W // (4 if gated else 3)
        self.T, self.R, self.H = T, R, H
        n_prev = x["h_prev"].shape[0]
        self.hp = G(n_prev, H, H + 12, 4, F32, _t(x["h_prev"]))
        self.lo = G(T * R, W, W + 16, 8, st, _t(x["lo"]).reshape(T * R, W))                           # row t R + r
        self.lo_op = (self.lo.mat, R * self.lo.ld, self.lo.ld)
        self.hi = self.hi_op = None
        if x["hi"] is not None:
            self.hi = G(R * T, W, W + 8, 0, st, _t(x["hi"]).transpose(0, 1).reshape(R * T, W))        # row r T + t
            self.hi_op = (self.hi.mat, self.hi.ld, T * self.hi.ld)
        self.m = self.m_op = None
        if x["mask"] is not None:
            self.m = G(R, T, T + 3, 1, F32, _t(x["mask"]).t())
            self.m_op = (self.m.mat, 1, self.m.ld)
        self.idx = torch.as_tensor(x["idx"].astype(np.int32)).cuda()
        self.out = G(R, H, 2 * H + 4, 4, F32)
        self.seq = self.seq_op = None
        if with_seq:
            self.seq = G(T * R, H, 3 * H + 8, 8, st)                                                  # row t R + r, a column slice
            self.seq_op = (self.seq.mat, R * self.seq.ld, self.seq.ld)

    def inputs(self):
        return [(b, n) for b, n in ((self.hp, "h_prev"), (self.lo, "lo"), (self.hi, "hi"), (self.m, "mask")) if b is not None]

    def run(self, reverse, gated, with_state=True, with_idx=True):
        e = eng()
        e.rnn_lrn_scan(self.hp.mat if with_state else None, self.lo_op, self.hi_op, self.out.mat, self.seq_op,
                       self.idx if (with_state and with_idx) else None, self.m_op, self.T, reverse, gated)
        torch.cuda.synchronize()
        for b, n in self.inputs():
            b.check_intact("lrn_scan " + n)
        self.out.check_guard("lrn_scan out")
        got = {"out": self.out.value().double().numpy()}
        if self.seq is not None:
            self.seq.check_guard("lrn_scan seq")
            got["seq"] = self.seq.value().double().numpy().reshape(self.T, self.R, self.H)
        return got


def _check(got, ref, form, label):
    worst = {w: V.assert_within(got[w], ref[w], L.lrn_bound(ref, form, w), "%s %s" % (label, w)) for w in got}
    print("%s: largest |err| / bound %s" % (label, "  ".join("%s %.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("form,R,H,T", SHAPES)
@pytest.mark.parametrize("gated", [False, True], ids=["lrn", "olrn"])
@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_scan(form, R, H, T, gated, paired):
    for reverse in (False, True):
        for variant in ("gather+mixed", "null+ones", "plain"):
            x = L.scan_inputs(T, R, H, form, R + H + T, gated, paired, mask={"gather+mixed": "mixed", "null+ones": "ones",
                                                                             "plain": None}[variant])
            label = "%s R=%d H=%d T=%d %s %s %s %s" % (form, R, H, T, "olrn" if gated else "lrn", "paired" if paired else "single",
                                                       "reverse" if reverse else "forward", variant)
            b = Bufs(x, form, gated)
            if variant == "gather+mixed":
                ref = L.lrn_scan(x["lo"], x["hi"], x["h_prev"], x["idx"], x["mask"], reverse, gated)
                got = b.run(reverse, gated)
                carried = (x["mask"] == 0).all(0)                      # rows masked at every position
                assert carried[0] and np.array_equal(got["out"][carried], ref["h0"][carried]), label + ": a carried row"
                for t in range(T):                                     # and every carried position repeats the state before it
                    prev = t + 1 if reverse else t - 1
                    if 0 <= prev < T:
                        rows = x["mask"][t] == 0
                        assert np.array_equal(got["seq"][t][rows], got["seq"][prev][rows]), (label, t)
            elif variant == "null+ones":
                ref = L.lrn_scan(x["lo"], x["hi"], None, None, x["mask"], reverse, gated)
                got = b.run(reverse, gated, with_state=False)
            else:
                ref = L.lrn_scan(x["lo"], x["hi"], x["h_prev"], None, None, reverse, gated)
                got = b.run(reverse, gated, with_idx=False)
            _check(got, ref, form, label)
            last = 0 if reverse else T - 1                            # out is the state of the last scanned position
            if form == "fp32":
                assert np.array_equal(got["out"], got["seq"][last]), label
            else:
                assert np.array_equal(L._bf(got["out"]), got["seq"][last]), label + ": seq is the rounded state"


@pytest.mark.parametrize("form", ["bf16", "fp32"])
def test_out_alone_and_one_step_into_a_column_slice(form):
    """seq NULL: out is still written.  T = 1 through the Mat form of the binding: the operands are plain [R, W] Mats, seq a
    column slice of a wider buffer (the out_copy of the other cell launches)."""
    R, H = 6, 24
    x = L.scan_inputs(4, R, H, form, 11, True, True)
    ref = L.lrn_scan(x["lo"], x["hi"], x["h_prev"], x["idx"], x["mask"], True, True)
    b = Bufs(x, form, True, with_seq=False)
    _check(b.run(True, True), ref, form, form + " no seq")
    x1 = L.scan_inputs(1, R, H, form, 12, False, True, mask="ones")
    ref1 = L.lrn_scan(x1["lo"], x1["hi"], x1["h_prev"], x1["idx"], None, False, False)
    st = ST[form]
    lo, hi = G(R, 3 * H, 3 * H + 8, 0, st, _t(x1["lo"][0])), G(R, 3 * H, 4 * H, 8, st, _t(x1["hi"][0]))
    hp = G(R + 2, H, H + 4, 0, F32, _t(x1["h_prev"]))
    out, cat = G(R, H, H, 0, F32), G(R, H, 3 * H + 16, 2 * H, st)
    eng().rnn_lrn_scan(hp.mat, lo.mat, hi.mat, out.mat, cat.mat, torch.as_tensor(x1["idx"].astype(np.int32)).cuda())
    torch.cuda.synchronize()
    for buf in (lo, hi, hp):
        buf.check_intact("one step")
    out.check_guard("one step out")
    cat.check_guard("one step seq")
    _check({"out": out.value().double().numpy(), "seq": cat.value().double().numpy()[None]}, ref1, form, form + " T = 1")


@pytest.mark.parametrize("form,R,H,T", [("bf16", 5, 72, 7), ("fp32", 5, 20, 7)])
@pytest.mark.parametrize("gated", [False, True], ids=["lrn", "olrn"])
@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_a_scan_is_bit_equal_to_its_chained_steps(form, R, H, T, gated, paired):
    e = eng()
    st = ST[form]
    x = L.scan_inputs(T, R, H, form, 31, gated, paired)
    for reverse in (False, True):
        b = Bufs(x, form, gated)
        whole = b.run(reverse, gated)
        hs = [torch.zeros(R, H, dtype=F32, device="cuda") for _ in (0, 1)]
        seq = torch.full((T, R, H), float("nan"), dtype=st, device="cuda")
        prev, idx = b.hp.mat, b.idx
        for n in range(T):
            t = T - 1 - n if reverse else n
            at = lambda g, t=t: None if g is None else Mat(g.mat.t, R, g.mat.cols, g.mat.ld * (T if g is b.hi else 1),
                                                           g.mat.off + t * g.mat.ld * (1 if g is b.hi else R))
            e.rnn_lrn_scan(prev, at(b.lo), at(b.hi), Mat(hs[n & 1], R, H), Mat(seq, R, H, H, t * R * H), idx,
                           (Mat(b.m.mat.t, R, 1, b.m.ld, b.m.mat.off + t), 1, b.m.ld), 1, False, gated)
            prev, idx = Mat(hs[n & 1], R, H), None
        torch.cuda.synchronize()
        assert np.array_equal(hs[(T - 1) & 1].cpu().double().numpy(), whole["out"]), "out, reverse=%s" % reverse
        assert np.array_equal(seq.cpu().double().numpy(), whole["seq"]), "seq, reverse=%s" % reverse


@pytest.mark.parametrize("form", ["bf16", "fp32"])
def test_refusals_leave_every_buffer_untouched(form):
    e = eng()
    st = ST[form]
    nv = 8 if form == "bf16" else 4
    T, R, H = 3, 4, 24
    x = L.scan_inputs(T, R, H, form, 5, True, True)
    b = Bufs(x, form, True)
    every = [buf for buf, _ in b.inputs()] + [b.out, b.seq]
    other = "zk_f32_rnn_lrn_scan" if form == "bf16" else ""

    def refused(match, **kw):
        a = dict(h_prev=b.hp.mat, lo=b.lo_op, hi=b.hi_op, out=b.out.mat, seq=b.seq_op, idx=b.idx, mask=b.m_op, T=T, reverse=False,
                 gated=True)
        a.update(kw)
        with pytest.raises(ZeroHipError, match=match):
            e.rnn_lrn_scan(**a)
        torch.cuda.synchronize()
        for buf in every:
            buf.check_intact("refusal: " + match)

    refused("out overlaps h_prev", out=b.hp.mat, idx=None)
    refused("out overlaps h_prev", out=Mat(b.hp.mat.t, R, H, b.hp.ld, b.hp.mat.off + b.hp.ld))      # shifted by one row
    refused("seq overlaps lo / hi", seq=(Mat(b.lo.mat.t, T * R, H, b.lo.ld, b.lo.mat.off), R * b.lo.ld, b.lo.ld))
    refused("seq overlaps lo / hi", seq=(Mat(b.hi.mat.t, T * R, H, b.hi.ld, b.hi.mat.off + H), b.hi.ld, T * b.hi.ld))
    refused("at least one position", T=0)
    refused("at least one position", T=-2)
    # H that is no multiple of the 16-byte group: the same buffers read as H - 2 channels wide
    odd = Mat(b.out.mat.t, R, H - 2, b.out.ld, b.out.mat.off)
    refused("multiple of %d.*%s" % (nv, other), out=odd)
    # rows that are not 16-byte aligned: a base shifted by one element, a row stride that is no multiple of the group
    refused("16 bytes at a time.*%s" % other, lo=(Mat(b.lo.mat.t, T * R, 4 * H, b.lo.ld, b.lo.mat.off + 1), R * b.lo.ld, b.lo.ld))
    refused("16 bytes at a time.*%s" % other, hi=(b.hi.mat, b.hi.ld, T * b.hi.ld + nv // 2))
    refused("16 bytes at a time.*%s" % other, seq=(b.seq.mat, R * b.seq.ld + 1, b.seq.ld))
    refused("n_prev", idx=None, h_prev=Mat(b.hp.mat.t, R - 1, H, b.hp.ld, b.hp.mat.off))
    got = b.run(False, True)                                          # and the same buffers still serve a launch
    _check(got, L.lrn_scan(x["lo"], x["hi"], x["h_prev"], x["idx"], x["mask"], False, True), form, form + " after the refusals")
