"""zk_shortlist_build called directly (zero_amd/csrc/zk_shortlist.hip) and held to EXACT equality with the numpy reference of
tests/shortlist_ref.py.  Every operand and output is a parity.guarded buffer (int32 bits in an fp32 window): the outputs are
prefilled with a sentinel, nothing outside their windows may change, the inputs must be bit-identical after the call.

The cases are shortlist_ref.product(): V in {40, 64, 70, 4100, 33000} (a partial mask word, exact words, more words than a
wave, more words than the finishing workgroup has threads), the three sources (1 x 1; 3 x 5 with padding and an all-pad
row; 8 x 16 with repeated tokens, empty table rows and ids without a row -- each in a wider leading dimension), best in
{0, 1, 3, 1000}, first in {3, 17, V}, round in {8, 64, 1024}, plus n an exact multiple of round and roundups beyond V.
tests/test_shortlist_host.py shows that this check rejects planted defects.

Every argument error leaves ids, count and the workspace untouched and names the argument.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import parity as P  # noqa: E402
from tests import shortlist_ref as SR  # noqa: E402
from tests.util_gpu import eng  # noqa: E402
from zero_amd.hip import ZeroHipError  # noqa: E402

F32 = torch.float32


def _in(a, ld=None, off=0):
    """int32 [rows, cols] as a guarded input (the bits travel in an fp32 window)."""
    a = np.ascontiguousarray(np.atleast_2d(a), dtype=np.int32)
    return P.guarded(a.shape[0], a.shape[1], ld, off, F32, torch.from_numpy(a).view(F32), "cuda")


def _out(n):
    return P.guarded(1, n, dtype=F32, device="cuda")          # prefilled with NaN bits: no id, no count


def _ints(g):
    return g.value().contiguous().view(torch.int32).numpy().reshape(-1)


class _Args(object):
    def __init__(self, src, off, lex, V, cap):
        self.src = _in(src, src.shape[1] + 3, 1)              # a leading dimension wider than Ls
        self.off, self.lex = _in(off), _in(lex if len(lex) else np.zeros(1, np.int32))
        self.ids, self.cnt = _out(cap), _out(2)
        self.ws = _out((V + 31) // 32)                         # the mask, 4 bytes per 32 ids: exactly what the query asks for
        self.rows, self.Ls, self.Vsrc, self.V, self.cap = src.shape[0], src.shape[1], len(off) - 1, V, cap

    def call(self, e, best, first, rnd, V=None, cap=None, ws_bytes=None):
        e.lib.call("zk_shortlist_build", self.src.mat.ptr, self.rows, self.src.ld, self.Ls, self.off.mat.ptr, self.lex.mat.ptr,
                   self.Vsrc, best, first, self.V if V is None else V, rnd, self.ids.mat.ptr, self.cap if cap is None else cap,
                   self.cnt.mat.ptr, self.ws.mat.ptr, self.ws.cols * 4 if ws_bytes is None else ws_bytes, e.stream)
        torch.cuda.synchronize()


@pytest.mark.parametrize("case", SR.product(), ids=lambda c: "V%d-%s-best%d-first%d-round%d" % c)
def test_equals_the_numpy_reference(case):
    e = eng()
    V, name, best, first, rnd = case
    src, off, lex = SR.case_inputs(case)
    cap = V + 5
    a = _Args(src, off, lex, V, cap)
    assert e.lib.query("zk_shortlist_workspace", V) == a.ws.cols * 4
    a.call(e, best, first, rnd)
    for g in (a.src, a.off, a.lex):
        g.check_intact("zk_shortlist_build operand")
    for g in (a.ids, a.cnt, a.ws):
        g.check_guard("zk_shortlist_build output")
    ref_ids, (n, Vs) = SR.build(src, off, lex, first, best, V, rnd, cap)
    got_ids, got_cnt = _ints(a.ids), _ints(a.cnt)
    assert tuple(got_cnt) == (n, Vs), (tuple(got_cnt), (n, Vs))
    assert np.array_equal(got_ids, ref_ids), np.flatnonzero(got_ids != ref_ids)[:8]
    # deterministic: a second call on the same buffers gives the same bits
    a.call(e, best, first, rnd)
    assert np.array_equal(_ints(a.ids), ref_ids) and tuple(_ints(a.cnt)) == (n, Vs)


ERRORS = [
    ("first", dict(first=2)),
    ("round", dict(rnd=12)),
    ("round", dict(rnd=0)),
    ("cap", dict(cap=69)),
    ("V =", dict(V=(1 << 22) + 1, cap=(1 << 22) + 1, ws_bytes=1 << 20)),
    ("workspace", dict(ws_bytes=8)),
]


@pytest.mark.parametrize("word, kw", ERRORS, ids=[w.strip(" =") + str(i) for i, (w, _) in enumerate(ERRORS)])
def test_argument_errors_launch_nothing(word, kw):
    e = eng()
    case = (70, "3x5", 3, 17, 64)
    src, off, lex = SR.case_inputs(case)
    a = _Args(src, off, lex, 70, 75)
    args = dict(best=3, first=17, rnd=64)
    args.update(kw)
    with pytest.raises(ZeroHipError, match=word):
        a.call(e, **args)
    torch.cuda.synchronize()
    for g in (a.src, a.off, a.lex, a.ids, a.cnt, a.ws):
        g.check_intact("buffer of a refused zk_shortlist_build")
    assert e.lib.raw("zk_shortlist_max_vocab")() == 1 << 22


def test_engine_wrapper():
    e = eng()
    case = (4100, "8x16", 3, 17, 64)
    src, off, lex = SR.case_inputs(case)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()
    out = torch.full((4100 + 2,), -7, dtype=torch.int32, device="cuda")
    e.shortlist_build(dev(src), src.shape[0], src.shape[1], src.shape[1], dev(off), dev(lex), 3, 17, 4100, 64, out[:4100], out[4100:])
    torch.cuda.synchronize()
    ref_ids, (n, Vs) = SR.build(src, off, lex, 17, 3, 4100, 64, 4100)
    assert np.array_equal(out[:4100].cpu().numpy(), ref_ids) and tuple(out[4100:].cpu().numpy()) == (n, Vs)
