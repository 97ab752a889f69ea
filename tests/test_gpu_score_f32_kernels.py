"""zk_f32_attn_seq, zk_f32_cumavg and zk_f32_embed_shift called directly (zero_amd/csrc/zk_f32_seq.hip) and compared
element by element with the float64 references of tests/score_f32_ref.py under its derived bounds.  Every operand and output
is a parity.guarded buffer: outputs are prefilled with NaN and have ld > H, nothing outside their windows may change, inputs
must be bit-identical after the call.  tests/test_score_f32_checker.py shows on the CPU that a correct float32 stand-in
passes these checks on every case and that each planted defect fails them on at least one.

The attention kernel works on blocks of TILE_ROWS = 32 query rows and key tiles of TILE_KEYS = 64 (score_f32_ref names them
after SEQ_BR / SEQ_TK of the kernel): the cases hold one length on each side of both borders (31, 33; 63, 65), several blocks
and tiles (130), a single row, ragged and fully masked sentences, relative positions with clipping and a query offset, and
d = 8.  In the causal cases the last key of a sentence scores highest for every query and carries a large value row.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng  # noqa: E402
from tests import parity as P  # noqa: E402
from tests import score_f32_ref as R  # noqa: E402
from zero_amd.hip import ZeroHipError  # noqa: E402

F32 = torch.float32
assert (R.TILE_ROWS, R.TILE_KEYS) == (32, 64)


def G(rows, cols, ld=None, off=0, prefill=None):
    return P.guarded(rows, cols, ld, off, F32, prefill, "cuda")


class Operands(object):
    def __init__(self, name, x):
        cs = R.ATTN_CASES[name]
        B, nh, d, Lq, Lk = (cs[k] for k in ("B", "nh", "d", "Lq", "Lk"))
        H = nh * d
        self.cs, self.H = cs, H
        if cs.get("slices"):          # q / k / v as column slices of one [T, 3H] matrix
            self.bufs = [G(B * Lq, 3 * H, 3 * H + 8, 0, torch.cat([x["q"], x["k"], x["v"]], 1))]
            m = self.bufs[0].mat
            self.q, self.k, self.v = m.cols_slice(0, H), m.cols_slice(H, 2 * H), m.cols_slice(2 * H, 3 * H)
        else:                         # k / v as column slices of one [B*Lk, 2H] matrix behind 8 guard columns
            self.bufs = [G(B * Lq, H, H + 4, 0, x["q"]), G(B * Lk, 2 * H, 2 * H + 16, 8, torch.cat([x["k"], x["v"]], 1))]
            self.q = self.bufs[0].mat
            self.k, self.v = self.bufs[1].mat.cols_slice(0, H), self.bufs[1].mat.cols_slice(H, 2 * H)
        self.mask = G(B, Lk, Lk + 3, 0, x["kmask"]) if x["kmask"] is not None else None
        self.rk = G(2 * cs["rpr"] + 1, d, prefill=x["rk"]) if cs.get("rpr") else None
        self.rv = G(2 * cs["rpr"] + 1, d, prefill=x["rv"]) if cs.get("rpr") else None
        self.bufs += [b for b in (self.mask, self.rk, self.rv) if b is not None]

    def out(self):
        return G(self.cs["B"] * self.cs["Lq"], self.H, self.H + 8, 4)

    def head(self, out):
        cs, q, k, v, o = self.cs, self.q, self.k, self.v, out.mat
        Lq, Lk = cs["Lq"], cs["Lk"]
        return (q.ptr, k.ptr, v.ptr, o.ptr, cs["B"], cs["nh"], Lq, Lk, cs["d"], q.ld, k.ld, v.ld, o.ld, Lq * q.ld, Lk * k.ld,
                Lk * v.ld, Lq * o.ld, self.mask.mat.ptr if self.mask is not None else None,
                self.mask.ld if self.mask is not None else 0)

    def tables(self):
        return (self.rk.mat.ptr if self.rk is not None else None, self.rv.mat.ptr if self.rv is not None else None,
                self.cs.get("rpr", 0), self.cs.get("q_pos0", 0))

    def seq_args(self, out, stream):
        return self.head(out) + (float(self.cs["d"]) ** -0.5, R.MASK_INF) + self.tables() + \
            (1 if self.cs.get("causal") else 0, stream)

    def row_args(self, out, stream):          # the per-row kernel of the decode step, same operands (non-causal only)
        return self.head(out) + (1, float(self.cs["d"]) ** -0.5, R.MASK_INF, None) + self.tables() + (None, stream)

    def check_intact(self, what):
        for b in self.bufs:
            b.check_intact(what + " operand")


@pytest.fixture(scope="module")
def refs():
    """Inputs, float64 references and bounds, computed once per case and left unchanged."""
    cache = {}

    def get(name):
        if name not in cache:
            x = R.attn_inputs(name)
            cache[name] = (x, R.attn_reference(name, x).numpy(), R.attn_bound(name, x))
        return cache[name]
    return get


def _check(entry, args_of, name, refs):
    e = eng()
    x, ref, bound = refs(name)
    ops = Operands(name, x)
    out = ops.out()
    e.lib.call(entry, *args_of(ops, out, e.stream))
    torch.cuda.synchronize()
    ops.check_intact(entry)
    out.check_guard(entry + " output")
    got = out.value()
    P.assert_elementwise(got, torch.as_tensor(ref), torch.as_tensor(bound), "%s %s" % (entry, name))
    ratio = R.worst_ratio(got.double().numpy(), ref, bound)
    print("%s %s: largest |err| / bound %.3f" % (entry, name, ratio))
    return got


@pytest.mark.parametrize("name", sorted(R.ATTN_CASES))
def test_attn_seq(refs, name):
    got = _check("zk_f32_attn_seq", lambda ops, out, s: ops.seq_args(out, s), name, refs)
    if name == "fully_masked":          # uniform weights: every query row of the masked sentence is the mean value row
        x = refs(name)[0]
        cs = R.ATTN_CASES[name]
        v = x["v"].double().view(cs["B"], cs["Lk"], -1)[1].mean(0)
        rows = got.double().view(cs["B"], cs["Lq"], -1)[1]
        assert float((rows - v[None]).abs().max()) < 1e-5


@pytest.mark.parametrize("name", sorted(n for n, cs in R.ATTN_CASES.items() if not cs.get("causal")))
def test_per_row_kernel_on_the_same_operands(refs, name):
    """The existing zk_f32_attn (one wave per query row) lies within the bound of the same reference."""
    _check("zk_f32_attn", lambda ops, out, s: ops.row_args(out, s), name, refs)


@pytest.mark.parametrize("use_mask", [1, 0])
@pytest.mark.parametrize("form", ["plain", "addend", "columns"])
def test_cumavg(use_mask, form):
    """Both mask forms; out = add + average (transformer_fuse); the output as the right half of a [x | avg] matrix whose
    left half must stay as it is.  B = 3, L = 9, H = 64, one sentence of length 1."""
    e = eng()
    cs = R.CUMAVG_SHAPE
    B, L, H = cs["B"], cs["L"], cs["H"]
    x = R.cumavg_inputs()
    add = x["add"] if form == "addend" else None
    ref, bound = R.cumavg_reference(x["x"], x["mask"], use_mask, add)
    gx, gm = G(B * L, H, H + 4, 0, x["x"]), G(B, L, L, 0, x["mask"])
    ga = G(B * L, H, H + 12, 4, add) if add is not None else None
    if form == "columns":
        left = torch.full((B * L, H), 3.0)
        wide = G(B * L, 2 * H, 2 * H + 8, 0, torch.cat([left, torch.full((B * L, H), float("nan"))], 1))
        om = wide.mat.cols_slice(H, 2 * H)
    else:
        wide = G(B * L, H, H + 8, 4)
        om = wide.mat
    e.lib.call("zk_f32_cumavg", gx.mat.ptr, gx.ld, gm.mat.ptr, ga.mat.ptr if ga is not None else None,
               ga.ld if ga is not None else 0, om.ptr, om.ld, B, L, H, use_mask, e.stream)
    torch.cuda.synchronize()
    for b in (gx, gm, ga):
        if b is not None:
            b.check_intact("zk_f32_cumavg operand")
    wide.check_guard("zk_f32_cumavg output")
    got = wide.value()
    if form == "columns":
        assert bool((got[:, :H] == 3.0).all()), "the left half of the wide matrix was written"
        got = got[:, H:]
    P.assert_elementwise(got, torch.as_tensor(ref), torch.as_tensor(bound), "zk_f32_cumavg %s use_mask %d" % (form, use_mask))
    print("zk_f32_cumavg %s use_mask %d: largest |err| / bound %.3f" % (form, use_mask,
                                                                      R.worst_ratio(got.double().numpy(), ref, bound)))
    if use_mask and add is None:
        pad = (x["mask"].reshape(-1) == 0).numpy()
        assert bool((got.numpy()[pad] == 0).all()), "a padded row averages to exact zeros under aan_mask"


def test_embed_shift():
    """B = 2, L = 5: row 0 of a sentence is the timing signal alone (exactly), row i embeds token i - 1."""
    e = eng()
    cs = R.EMBED_SHAPE
    B, L, H = cs["B"], cs["L"], cs["H"]
    x = R.embed_inputs()
    tim = e.timing(L + 1, H)
    ref, bound = R.embed_reference(x["ids"], x["table"], x["bias"], tim.cpu())
    gt, gb = G(cs["V"], H, prefill=x["table"]), G(1, H, prefill=x["bias"])
    ids = x["ids"].cuda()
    out = G(B * L, H)
    e.lib.call("zk_f32_embed_shift", ids.data_ptr(), B * L, L, gt.mat.ptr, gb.mat.ptr, tim.data_ptr(), int(tim.shape[0]),
               out.mat.ptr, H, float(H) ** 0.5, e.stream)
    torch.cuda.synchronize()
    gt.check_intact("table")
    gb.check_intact("bias")
    out.check_guard("zk_f32_embed_shift output")
    got = out.value()
    P.assert_elementwise(got, torch.as_tensor(ref), torch.as_tensor(bound), "zk_f32_embed_shift")
    assert torch.equal(got.view(B, L, H)[:, 0], tim[:1].cpu().expand(B, H))


def test_argument_errors_are_codes_with_text(refs):
    e = eng()
    x, _, _ = refs("ragged")
    ops = Operands("ragged", x)
    out = ops.out()
    good = list(ops.seq_args(out, e.stream))
    with pytest.raises(ZeroHipError, match="causal together with kmask"):
        a = list(good)
        a[-2] = 1
        e.lib.call("zk_f32_attn_seq", *a)
    with pytest.raises(ZeroHipError, match="multiple of 4"):
        a = list(good)
        a[8] = 6
        e.lib.call("zk_f32_attn_seq", *a)
    with pytest.raises(ZeroHipError, match="16-byte aligned"):
        a = list(good)
        a[1] = a[1] + 4
        e.lib.call("zk_f32_attn_seq", *a)
    with pytest.raises(ZeroHipError, match="both tables"):
        a = list(good)
        a[21] = ops.q.ptr
        e.lib.call("zk_f32_attn_seq", *a)
    a = list(good)
    a[4] = 0                                       # B = 0: nothing to do, no launch
    e.lib.call("zk_f32_attn_seq", *a)
    with pytest.raises(ZeroHipError, match="zk_f32_cumavg"):
        e.lib.call("zk_f32_cumavg", ops.q.ptr, 4, ops.q.ptr, None, 0, out.mat.ptr, 8, 1, 1, 8, 1, e.stream)
    with pytest.raises(ZeroHipError, match="zk_f32_embed_shift"):
        e.lib.call("zk_f32_embed_shift", ops.q.ptr, 4, 0, ops.q.ptr, ops.q.ptr, ops.q.ptr, 1, out.mat.ptr, 8, 1.0, e.stream)
    torch.cuda.synchronize()
    out.check_guard("refused calls")
    assert bool(torch.isnan(out.value()).all()), "a refused call wrote its output"
