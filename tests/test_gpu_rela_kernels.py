"""zk_rela_attn / zk_f32_rela_attn called directly (zero_amd/csrc/zk_rela.hip) and compared element by element with the
float64 reference of tests/rela_ref.py under rela_ref.bound.  Every operand and output is a parity.guarded buffer: outputs
are prefilled with NaN, nothing outside their windows may change, inputs must be bit-identical after the call.

Cases (rela_ref.CASES; tests/test_rela_host.py shows on the CPU that a correct stand-in passes this check on every one of
them and that each planted defect fails it on at least one):
    cross       decode form, 2 sentences x 3 beam rows (kv_group 3), nh 2, d 64, 17 keys as column slices of one
                [B*Lk, 2H] matrix; sentence 1 has 6 valid keys and 11 masked ones with large positive scores
    self        cached step, 5 rows, H = 192 (3 heads), 24 slots; the position is read from device memory at 0, 1, 8, 23;
                the slots behind it hold NaN; one captured graph replayed with the position advanced on the device
    encoder     3 sentences of 19 positions (lengths 19, 1, 7), q / k / v slices of one [T, 3H] matrix
    special     rows without a positive score (exact zeros), rows with ONE positive score of 0.05, 1, 20 and 3e-3
    bf16_d32, bf16_H2048, fp32_d8      the edges of the forms' limits; the bf16 form refuses d = 12
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng  # noqa: E402
from tests import parity as P  # noqa: E402
from tests import rela_ref as R  # noqa: E402
from tests import variant_ref as V  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
ENTRY = {"bf16": "zk_rela_attn", "fp32": "zk_f32_rela_attn"}


def G(rows, cols, ld=None, off=0, dtype=BF, prefill=None):
    return P.guarded(rows, cols, ld, off, dtype, prefill, "cuda")


class Operands(object):
    """The guarded operands of one case in its layout and the argument tuple of the entry points."""

    def __init__(self, name, form, x, time=None):
        cs = R.CASES[name]
        st = V.STORAGE[form]
        B, Gp, nh, d, Lq, Lk = (cs[k] for k in ("B", "G", "nh", "d", "Lq", "Lk"))
        H, nB = nh * d, B // Gp
        self.cs, self.st, self.H = cs, st, H
        q, k, v = x["q"].reshape(B * Lq, H), x["k"].reshape(nB * Lk, H).clone(), x["v"].reshape(nB * Lk, H).clone()
        if time is not None:          # the slots behind the position hold NaN: reading one of them shows
            dead = (torch.arange(nB * Lk) % Lk) > time
            k[dead], v[dead] = float("nan"), float("nan")
        lay = cs["layout"]
        if lay == "qkv":              # slices of one [T, 3H] matrix
            ld = 3 * H + 8
            self.bufs = [G(B * Lq, 3 * H, ld, 0, st, torch.cat([q, k, v], 1))]
            m = self.bufs[0].mat
            self.q, self.k, self.v = m.cols_slice(0, H), m.cols_slice(H, 2 * H), m.cols_slice(2 * H, 3 * H)
        elif lay == "kv":             # k / v as column slices of one [B*Lk, 2H] matrix
            ld = 2 * H + 16
            self.bufs = [G(B * Lq, H, H + 8, 0, st, q), G(nB * Lk, 2 * H, ld, 8, st, torch.cat([k, v], 1))]
            self.q = self.bufs[0].mat
            self.k, self.v = self.bufs[1].mat.cols_slice(0, H), self.bufs[1].mat.cols_slice(H, 2 * H)
        else:                         # "cache": q a slice of the step's [rows, 3H] projection, per-row caches [B, Tmax, H]
            self.bufs = [G(B, 3 * H, 3 * H, 0, st, torch.cat([q, q * 0 + 7, q * 0 - 7], 1)), G(nB * Lk, H, H, 0, st, k),
                         G(nB * Lk, H, H, 0, st, v)]
            self.q, self.k, self.v = self.bufs[0].mat.cols_slice(0, H), self.bufs[1].mat, self.bufs[2].mat
        self.mask = G(nB, Lk, Lk + 3, 0, F32, x["kmask"]) if x["kmask"] is not None else None
        self.scale, self.gate = G(1, H, dtype=F32, prefill=x["scale"]), G(1, H, dtype=F32, prefill=x["gate"])
        self.bufs += [b for b in (self.mask, self.scale, self.gate) if b is not None]

    def out(self):
        cs = self.cs
        return G(cs["B"] * cs["Lq"], self.H, self.H + 8, 0, self.st)

    def args(self, out, tdev, stream):
        cs, q, k, v, o = self.cs, self.q, self.k, self.v, out.mat
        Lq, Lk = cs["Lq"], cs["Lk"]
        return (q.ptr, k.ptr, v.ptr, o.ptr, cs["B"], cs["nh"], Lq, Lk, cs["d"], q.ld, k.ld, v.ld, o.ld, Lq * q.ld, Lk * k.ld,
                Lk * v.ld, Lq * o.ld, self.mask.mat.ptr if self.mask is not None else None,
                self.mask.ld if self.mask is not None else 0, cs["G"], float(cs["d"]) ** -0.5,
                tdev.data_ptr() if tdev is not None else None, self.scale.mat.ptr, self.gate.mat.ptr, R.EPS, stream)

    def check_intact(self, what):
        for b in self.bufs:
            b.check_intact(what + " operand")


@pytest.fixture(scope="module")
def refs():
    """Inputs and float64 references, computed once per (case, form, time) and left unchanged."""
    cache = {}

    def get(name, form, time=None):
        key = (name, form, time)
        if key not in cache:
            if (name, form) not in cache:
                cache[(name, form)] = R.case_inputs(name, form)
            x = cache[(name, form)]
            cache[key] = (x, R.case_reference(name, x, time))
        return cache[key]
    return get


def _run(name, form, x, time=None):
    e = eng()
    ops = Operands(name, form, x, time)
    out = ops.out()
    tdev = torch.tensor([time], dtype=torch.int32, device="cuda") if time is not None else None
    e.lib.call(ENTRY[form], *ops.args(out, tdev, e.stream))
    torch.cuda.synchronize()
    ops.check_intact(ENTRY[form])
    out.check_guard(ENTRY[form] + " output")
    return out.value().double().numpy()


RUNS = [(name, form, t) for name, cs in R.CASES.items() for form in cs["forms"] for (t,) in R.case_runs(name)]


@pytest.mark.parametrize("name,form,time", RUNS, ids=["%s-%s%s" % (n, f, "" if t is None else "-t%d" % t) for n, f, t in RUNS])
def test_case(refs, name, form, time):
    x, ref = refs(name, form, time)
    got = _run(name, form, x, time)
    ratio = V.assert_within(got, ref["out"], R.bound(ref, V.STORAGE[form]), "%s %s time %s" % (name, form, time))
    print("%s %s time %s: largest |err| / bound %.3f" % (name, form, time, ratio))
    if name == "special":
        assert (got[:2] == 0).all(), "a row without a positive score must be exact zeros"
        # the rows with one positive score of 0.05, 1 and 20: the same normalised value vector whatever the score, up to
        # eps / ms (<= 1e-8 / 2.5e-3 mean v^2) and the roundings the bound allows
        v, sc = x["v"].double().numpy(), x["scale"].double().numpy()
        for b in (2, 3, 4):
            picked = np.concatenate([v[b, (b + h) % 9, h * 64:(h + 1) * 64] for h in range(2)])
            want = 0.5 * sc * picked / np.sqrt((picked ** 2).mean())
            tol = R.bound(ref, V.STORAGE[form])[b, 0] + 1e-5 * np.abs(want)
            assert (np.abs(got[b] - want) <= tol).all(), b


@pytest.mark.parametrize("form", ["bf16", "fp32"])
def test_self_graph_replay_reads_the_position_from_the_device(refs, form):
    """One capture at position 1; the position is advanced ON THE DEVICE to 8 between two replays: each replay equals the
    eager call at its position (and so the reference).  The cache holds the keys 0 .. 8; the slots behind hold NaN."""
    e = eng()
    x, _ = refs("self", form, 8)
    ops = Operands("self", form, x, 8)
    with torch.cuda.stream(e.work_stream):
        tdev = torch.tensor([1], dtype=torch.int32, device="cuda")
        eager = {}
        for t in (1, 8):
            tdev.fill_(t)
            o = ops.out()
            e.lib.call(ENTRY[form], *ops.args(o, tdev, e.stream))
            torch.cuda.synchronize()
            eager[t] = o.value()
            ref = refs("self", form, t)[1]
            V.assert_within(eager[t].double().numpy(), ref["out"], R.bound(ref, V.STORAGE[form]), "eager t %d" % t)
        tdev.fill_(1)
        rep = ops.out()
        torch.cuda.synchronize()
        g = e.graph_capture(lambda: e.lib.call(ENTRY[form], *ops.args(rep, tdev, e.stream)))
        try:
            assert torch.isnan(rep.value()).all(), "capturing must not run the kernel"
            e.graph_launch(g)
            torch.cuda.synchronize()
            assert torch.equal(rep.value().view(torch.int16 if form == "bf16" else torch.int32),
                               eager[1].view(torch.int16 if form == "bf16" else torch.int32))
            tdev.add_(7)                      # on the device, between the replays
            e.graph_launch(g)
            torch.cuda.synchronize()
            assert torch.equal(rep.value().view(torch.int16 if form == "bf16" else torch.int32),
                               eager[8].view(torch.int16 if form == "bf16" else torch.int32))
        finally:
            e.lib.call("zk_graph_destroy", g)
    rep.check_guard("replayed output")
    ops.check_intact("replayed " + ENTRY[form])


def test_bf16_form_refuses_a_head_size_of_12():
    e = eng()
    nh, d, B, Lk = 2, 12, 2, 5
    H = nh * d
    g = torch.Generator().manual_seed(1)
    q, k, v = (G(n, H, H, 0, BF, torch.randn(n, H, generator=g)) for n in (B, B * Lk, B * Lk))
    scale, gate = G(1, H, dtype=F32, prefill=torch.ones(H)), G(1, H, dtype=F32, prefill=torch.zeros(H))
    out = G(B, H, H, 0, BF)
    rc = e.lib.raw("zk_rela_attn")(q.mat.ptr, k.mat.ptr, v.mat.ptr, out.mat.ptr, B, nh, 1, Lk, d, H, H, H, H, H, Lk * H, Lk * H, H,
                                   None, 0, 1, d ** -0.5, None, scale.mat.ptr, gate.mat.ptr, R.EPS, e.stream)
    torch.cuda.synchronize()
    assert rc < 0
    msg = e.lib.raw("zk_last_error_string")()
    assert b"multiple of 8" in msg and b"zk_f32_rela_attn" in msg, msg
    out.check_intact("the refused call's output")
    assert torch.isnan(out.value()).all()
    # the fp32 form takes the same shape
    x = {"q": torch.randn(B, 1, H, generator=g), "k": torch.randn(B, Lk, H, generator=g), "v": torch.randn(B, Lk, H, generator=g)}
    qf, kf, vf = G(B, H, H, 0, F32, x["q"]), G(B * Lk, H, H, 0, F32, x["k"]), G(B * Lk, H, H, 0, F32, x["v"])
    of = G(B, H, H, 0, F32)
    e.lib.call("zk_f32_rela_attn", qf.mat.ptr, kf.mat.ptr, vf.mat.ptr, of.mat.ptr, B, nh, 1, Lk, d, H, H, H, H, H, Lk * H, Lk * H,
               H, None, 0, 1, d ** -0.5, None, scale.mat.ptr, gate.mat.ptr, R.EPS, e.stream)
    torch.cuda.synchronize()
    ref = R.rela_attention(x["q"].numpy(), x["k"].numpy(), x["v"].numpy(), nh, np.ones(H), np.zeros(H))
    of.check_guard("zk_f32_rela_attn d = 12")
    V.assert_within(of.value().double().numpy(), ref["out"], R.bound(ref, F32), "fp32 form, d = 12")
