"""zk_attn_fwd in its decode forms, checked per (row, position, head) d-vector against the float64 reference of
tests/attn_decode_ref.py: kv_group > 1, given sentence strides, the position read from device memory (pos_flags 1 and 3),
a single query row, and the fall-back to the reference kernel (d != 64, more than 256 keys).  The whole-model beam
searches that reach these forms compare token ids only.

Every operand and output is a parity.guarded buffer: outputs (ld = H + 8) are prefilled with NaN and every element must
be written, nothing outside an output window may change, q, the k / v buffers, the mask (fp32 [sentences, Lk], row stride
Lk) and the tables must be bit-identical after every call.  The slots of a cache behind the position hold NaN.  Calls go
through Engine.attn_fwd, so whether the tables are folded into the tile is the model's decision: impl 1 = the reference
kernel, tables applied directly; impl 2 = MFMA, tables folded; impl None = the engine's default.  lse is null, as the
decode callers pass it; one run of `cross` passes it and holds it to 2e-2 per element.

Cases (attn_decode_ref.CASES; tests/test_attn_decode_checker.py shows on the CPU that a correct stand-in passes this check
on every run and that each of ten planted defects fails it on named runs):
    cross                 2 sentences x 3 beam rows (kv_group 3), 17 keys, lengths (17, 6): sentence 1's 11 masked keys
                          carry the largest raw scores; k / v column slices of one [34, 2H + 16] matrix
    cross_tiles_*         the same with 64, 65, 130, 256 keys: one to four key tiles, the MFMA limit
    cross_long            300 keys: the default falls back to the reference kernel, impl 2 refuses
    cross_one_sentence    kv_group 6, 5 keys          cross_flat   kv_group 1, the same strides
    cross_rpr             cross with relative positions, the position on the device at 0, 3, 16, 40 (every key in the
                          clipped tail) with position + 7 passed by value; once by value alone
    self_cached_24 / 130  5 rows, H = 192, q the first H columns of [5, 3H] (the others hold +-7), caches [5, Tmax, H];
                          positions 0, 1, 8, 23 / 0, 63, 64, 129 on the device (the call names Tmax keys) and by value (the
                          call names position + 1 keys under the cache's stride), with and without relative positions
    small_head            nh 4, d 16: reference kernel only, impl 2 refuses
    block_offset          2 sentences of 3 query rows at q_pos0 = 5 over 9 keys, relative positions, with and without the
                          causal mask: the only form with more than one live query row
Not run, by name: NOT_RUN below (what impl 2 refuses; test_mfma_refuses_what_only_the_reference_kernel_takes holds the
refusal).  No run leaves out rows; the share of excused d-vectors is 0.

The constant (measured with the stand-in against the float64 reference on the CPU, never with a kernel):

    tensor   stand-in, worst row ratio over the 48 runs   twice that   c_out
    out      3.53e-03 (block_offset, causal)              7.1e-03      7.9e-03 = C_X["out"] of the training layout: the
                                                                       doubled figure is not larger, the existing
                                                                       constant is used

Worst row ratio per kernel observed on an MI355X, over all runs of all cases:

    k_attn_fwd_naive (impl 1; the default on cross_long, small_head)     2.12e-03   small_head
    k_attn_fwd_mfma<NKT> (impl 2 and the default, no tables)             3.30e-03   cross (NKT 1); 2.13e-03 over NKT 2 .. 4
    k_attn_fwd_mfma<NKT, RPR> (impl 2 and the default, tables folded)    3.53e-03   block_offset, causal; one query row:
                                                                                    3.06e-03 (self_cached_24)
    lse of `cross`: 3.0e-07 at most.  A row with one visible key equals the key's value vector to one bf16 rounding.

No defect was found: every run of every kernel is inside the constant with guards and operands intact, the refusals
touch nothing, and the replayed graphs are bit-equal to the eager calls at both positions.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from zero_amd.hip import ZeroHipError  # noqa: E402
from tests.util_gpu import eng  # noqa: E402
from tests import parity as P  # noqa: E402
from tests import attn_decode_ref as A  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
IMPLS = (1, 2, None)
NOT_RUN = [(name, 2) for name in A.REFERENCE_KERNEL_ONLY]
COMBOS = [(name, impl) for name in A.CASES for impl in IMPLS if (name, impl) not in NOT_RUN]


def G(rows, cols, ld=None, off=0, dtype=BF, prefill=None):
    return P.guarded(rows, cols, ld, off, dtype, prefill, "cuda")


class Operands(object):
    """The guarded operands of one run in the case's layout, and the call.  filled_to: the last cache slot that holds
    data (default: the run's position); the slots behind hold NaN."""

    def __init__(self, name, x, r, filled_to=None):
        cs = A.CASES[name]
        B, Gp, nh, d, Lq, Lk = (cs[n] for n in ("B", "G", "nh", "d", "Lq", "Lk"))
        H, nB = nh * d, B // Gp
        self.name, self.cs, self.r, self.H = name, cs, r, H
        self.pos, self.nkeys = A.positions(name, r)
        q, k, v = x["q"].reshape(B * Lq, H), x["k"].reshape(nB * Lk, H).clone(), x["v"].reshape(nB * Lk, H).clone()
        if cs["layout"] == "cache":
            dead = (torch.arange(nB * Lk) % Lk) > (self.pos if filled_to is None else filled_to)
            k[dead], v[dead] = float("nan"), float("nan")
            self.bufs = [G(B, 3 * H, 3 * H, 0, BF, torch.cat([q, q * 0 + 7, q * 0 - 7], 1)), G(nB * Lk, H, H, 0, BF, k),
                         G(nB * Lk, H, H, 0, BF, v)]
            self.q, self.k, self.v = self.bufs[0].mat.cols_slice(0, H), self.bufs[1].mat, self.bufs[2].mat
            self.strides = (3 * H, Lk * H, Lk * H)
        else:
            ld = 2 * H + 16
            self.bufs = [G(B * Lq, H, H + 8, 0, BF, q), G(nB * Lk, 2 * H, ld, 8, BF, torch.cat([k, v], 1))]
            self.q = self.bufs[0].mat
            self.k, self.v = self.bufs[1].mat.cols_slice(0, H), self.bufs[1].mat.cols_slice(H, 2 * H)
            self.strides = (0, 0, 0) if cs.get("default_strides") else (Lq * self.q.ld, Lk * ld, Lk * ld)
        self.mask = G(nB, Lk, Lk, 0, F32, x["kmask"]) if x["kmask"] is not None else None
        self.rk = G(2 * A.MAX_REL + 1, d, d, 0, BF, x["rk"]) if r["rpr"] else None
        self.rv = G(2 * A.MAX_REL + 1, d, d, 0, BF, x["rv"]) if r["rpr"] else None
        self.bufs += [b for b in (self.mask, self.rk, self.rv) if b is not None]

    def out(self):
        return G(self.cs["B"] * self.cs["Lq"], self.H, self.H + 8, 0, BF)

    def call(self, out, impl, tdev=None, lse=None):
        """As the decode callers call it: with the position on the device the call names every allocated key and passes a
        WRONG position by value; by value a cache is named up to the position."""
        cs, r = self.cs, self.r
        dev = r["pos"] == "dev"
        assert dev == (tdev is not None)
        Lk = self.nkeys if (cs["layout"] == "cache" and not dev) else cs["Lk"]
        eng().attn_fwd(self.q, self.k, self.v, out.mat, lse, cs["B"], cs["nh"], cs["Lq"], Lk, cs["d"],
                       kmask=self.mask.window() if self.mask is not None else None, causal=r["causal"],
                       q_pos0=self.pos + A.WRONG_BY if dev else self.pos,
                       rpr_k=self.rk.window() if r["rpr"] else None, rpr_v=self.rv.window() if r["rpr"] else None,
                       max_rel=A.MAX_REL if r["rpr"] else 0, bsq=self.strides[0], bsk=self.strides[1], bsv=self.strides[2],
                       kv_group=cs["G"], impl=impl, pos_dev=tdev, pos_flags=cs["pos_flags"])

    def check_intact(self, what):
        for b in self.bufs:
            b.check_intact(what + " operand")


@pytest.fixture(scope="module")
def refs():
    """Inputs and float64 references, computed once per (case, run) and left unchanged."""
    cache = {}

    def get(name, r):
        if name not in cache:
            cache[name] = A.case_inputs(name)
        key = (name, A.run_id(r))
        if key not in cache:
            cache[key] = A.case_reference(name, cache[name], r)
        return cache[name], cache[key]
    return get


def _device_word(r):
    return torch.tensor([r["time"]], dtype=torch.int32, device="cuda") if r["pos"] == "dev" else None


def _run(name, x, r, impl, ref, lse=None):
    """One eager call, guards and operands checked, the output inside the constant.  -> (output, worst row ratio)"""
    what = "%s %s impl %s" % (name, A.run_id(r), impl)
    ops = Operands(name, x, r)
    out = ops.out()
    ops.call(out, impl, _device_word(r), lse)
    torch.cuda.synchronize()
    out.check_guard(what + " output")
    ops.check_intact(what)
    got = out.value().double().numpy().reshape(ref["out"].shape)
    assert np.isfinite(got).all(), what + ": an element of the output was not written"
    ratio = A.row_ratio(name, got, ref["out"])
    print("%s: worst row ratio %.2e" % (what, ratio))
    A.check(name, got, ref["out"], what)
    want = A.single_key_rows(name, x, r)
    if want is not None:
        A.check_single_key(got, want, what)
    return out, ratio


@pytest.mark.parametrize("name,impl", COMBOS, ids=["%s-impl%s" % c for c in COMBOS])
def test_case(refs, name, impl):
    worst = 0.0
    for r in A.CASES[name]["runs"]:
        x, ref = refs(name, r)
        worst = max(worst, _run(name, x, r, impl, ref)[1])
    print("%s impl %s: worst row ratio over %d run(s) %.2e (c_out %.1e)" % (name, impl, len(A.CASES[name]["runs"]), worst, A.C_OUT))


@pytest.mark.parametrize("name", A.REFERENCE_KERNEL_ONLY)
def test_mfma_refuses_what_only_the_reference_kernel_takes(refs, name):
    """impl 2 returns an error and touches nothing; the default takes the reference kernel: bit-equal to impl 1."""
    r = A.CASES[name]["runs"][0]
    x, ref = refs(name, r)
    ops = Operands(name, x, r)
    out = ops.out()
    with pytest.raises(ZeroHipError, match="MFMA kernel needs"):
        ops.call(out, 2)
    torch.cuda.synchronize()
    out.check_intact("the refused call's output")
    assert torch.isnan(out.value()).all()
    ops.check_intact("refused " + name)
    auto, ref1 = _run(name, x, r, None, ref)[0], _run(name, x, r, 1, ref)[0]
    assert torch.equal(auto.value().view(torch.int16), ref1.value().view(torch.int16))


@pytest.mark.parametrize("impl", IMPLS)
def test_cross_with_a_log_sum_exp_buffer(refs, impl):
    cs = A.CASES["cross"]
    r = cs["runs"][0]
    x, ref = refs("cross", r)
    lse = G(1, cs["B"] * cs["nh"] * cs["Lq"], dtype=F32)
    _run("cross", x, r, impl, ref, lse.window().view(-1))
    lse.check_guard("lse")
    err = float(np.abs(lse.value().double().numpy().reshape(ref["lse"].shape) - ref["lse"]).max())
    print("cross impl %s: lse %.2e" % (impl, err))
    assert err < 2e-2, err


# (case, relative positions, position at the capture, position of the second replay)
REPLAYS = [("self_cached_24", False, 1, 8), ("self_cached_24", True, 1, 8), ("cross_rpr", True, 3, 16)]


@pytest.mark.parametrize("impl", [None, 1])
@pytest.mark.parametrize("name,rpr,t0,t1", REPLAYS)
def test_graph_replay_reads_the_position_from_the_device(refs, name, rpr, t0, t1, impl):
    """One capture at position t0 (one node: a linear graph); the device word is advanced to t1 ON THE DEVICE between two
    replays.  Each replay is bit-equal to the eager call at its position, which is inside the constant.  The cache holds
    the keys 0 .. t1; the slots behind hold NaN."""
    e = eng()
    runs = {t: A.run(t, rpr, "dev") for t in (t0, t1)}
    x = refs(name, runs[t0])[0]
    ops = Operands(name, x, runs[t1], filled_to=t1)
    with torch.cuda.stream(e.work_stream):
        tdev = torch.tensor([t0], dtype=torch.int32, device="cuda")
        eager = {}
        for t in (t0, t1):
            tdev.fill_(t)
            ops.pos = t                       # (the by-value position of the call: t + WRONG_BY)
            o = ops.out()
            ops.call(o, impl, tdev)
            torch.cuda.synchronize()
            o.check_guard("eager output")
            eager[t] = o.value()
            A.check(name, eager[t].double().numpy(), refs(name, runs[t])[1]["out"], "%s eager at %d impl %s" % (name, t, impl))
        tdev.fill_(t0)
        ops.pos = t0
        rep = ops.out()
        torch.cuda.synchronize()
        g = e.graph_capture(lambda: ops.call(rep, impl, tdev))
        try:
            assert e.last_graph_nodes == 1
            torch.cuda.synchronize()
            assert torch.isnan(rep.value()).all(), "capturing must not run the kernel"
            e.graph_launch(g)
            torch.cuda.synchronize()
            assert torch.equal(rep.value().view(torch.int16), eager[t0].view(torch.int16))
            tdev.add_(t1 - t0)                # on the device, between the replays
            e.graph_launch(g)
            torch.cuda.synchronize()
            assert torch.equal(rep.value().view(torch.int16), eager[t1].view(torch.int16))
        finally:
            e.lib.call("zk_graph_destroy", g)
    rep.check_guard("replayed output")
    ops.check_intact("replayed " + name)
