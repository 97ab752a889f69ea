"""zk_ngram_ban called directly (zero_amd/csrc/zk_ngram.hip) and held to EXACT equality with the rule of tests/ngram_ref.py.

The logits are a parity.guarded fp32 buffer prefilled with random finite values, the history a guarded int32 buffer (its bits
travel in an fp32 window).  After every call the WHOLE logits buffer -- window, the columns between V and ld, the guard bands --
is compared on the device, bit for bit, with the prefill in which the banned entries are replaced by `value`; the whole history
buffer must be bit-identical to what it was.  tests/test_ngram_host.py shows that the rule rejects planted defects.

Cases: rows in {1, 5, 128} (one wave; a part-filled workgroup; 32 workgroups), V / ld in {37 / 40, 32000 / 32000}, histories
over two and three symbols (many matches, several lanes storing to one entry; one of the three symbols is >= V and must be
skipped) and all-distinct ones (no match for n >= 2; tokens >= V), n in {1, 2, 3, 4, 8, 16}, t in {0, n - 2, n - 1, n, 63, 64,
65, 130, ldh - 1} (nothing to ban yet; the first possible ban; the second and third trip of the lane loop; the last position of
the row), ldh = 136 with every position behind t holding tokens too.  Each (n, t) runs with the time by value and with the time
read from a device word.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ngram_ref as N  # noqa: E402
from tests import parity as P  # noqa: E402
from tests.util_gpu import eng  # noqa: E402
from zero_amd.hip import ZeroHipError  # noqa: E402

F32 = torch.float32
LDH = 136
VALUE = -1e8
NS = (1, 2, 3, 4, 8, 16)


def _times(n, ldh=LDH):
    return sorted(set(t for t in (0, n - 2, n - 1, n, 63, 64, 65, 130, ldh - 1) if 0 <= t < ldh))


def _history(rows, V, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "two":
        h = rng.choice(np.array([3, 4]), size=(rows, LDH))
    elif kind == "three":
        h = rng.choice(np.array([3, 4, V + 5]), size=(rows, LDH))
    else:                           # all distinct within a row; most of them >= V at V = 37
        h = np.stack([rng.permutation(LDH) + 3 + 17 * r for r in range(rows)])
    h[:, 0] = 0                     # the start symbol
    return h.astype(np.int32)


class _Case(object):
    def __init__(self, rows, V, ld, hist, seed=1):
        g = torch.Generator().manual_seed(seed)
        self.rows, self.V, self.ld, self.hist = rows, V, ld, hist
        self.lg = P.guarded(rows, V, ld, 0, F32, torch.randn(rows, V, generator=g) * 5.0, "cuda")
        self.h = P.guarded(rows, hist.shape[1], None, 0, F32, torch.from_numpy(hist).view(F32), "cuda")
        self.pristine = self.lg.t.clone()
        self.h0 = self.h.t.clone()
        self.word = torch.zeros(1, dtype=torch.int32, device="cuda")

    def reset(self):
        self.lg.t.copy_(self.pristine)

    def expected(self, n, t):
        """The whole flat logits buffer after the call."""
        exp = self.pristine.clone()
        pos = [P.LEAD + r * self.ld + int(v) for r, b in enumerate(N.banned_rows(self.hist, t, n)) for v in b if 0 <= v < self.V]
        if pos:
            exp[torch.as_tensor(pos, dtype=torch.long, device="cuda")] = VALUE
        return exp, len(pos)

    def call(self, e, n, t, by_value, rows=None, V=None, ld=None, ldh=None):
        if not by_value:
            self.word.fill_(t)
        e.lib.call("zk_ngram_ban", self.lg.mat.ptr, self.ld if ld is None else ld, self.rows if rows is None else rows,
                   self.V if V is None else V, self.h.mat.ptr, self.h.ld if ldh is None else ldh, t if by_value else -7,
                   None if by_value else self.word.data_ptr(), n, VALUE, e.stream)

    def check(self, exp, what):
        torch.cuda.synchronize()
        if not torch.equal(self.lg.t.view(torch.int32), exp.view(torch.int32)):
            self.lg.check_guard(what)               # names a write outside the window, if that is what happened
            bad = torch.nonzero(self.lg.t.view(torch.int32) != exp.view(torch.int32)).reshape(-1)
            r, c = self.lg._where(bad[0])
            raise AssertionError("%s: %d logits differ from the rule; the first at row %d, column %d: %r, expected %r"
                                 % (what, bad.numel(), r, c, float(self.lg.t[bad[0]]), float(exp[bad[0]])))
        assert torch.equal(self.h.t.view(torch.int32), self.h0.view(torch.int32)), what + ": the history changed"


@pytest.mark.parametrize("kind", ["two", "three", "distinct"])
@pytest.mark.parametrize("V,ld", [(37, 40), (32000, 32000)])
@pytest.mark.parametrize("rows", [1, 5, 128])
def test_equals_the_rule(rows, V, ld, kind):
    e = eng()
    c = _Case(rows, V, ld, _history(rows, V, kind, rows + V))
    total = 0
    for n in NS:
        for t in _times(n):
            exp, nb = c.expected(n, t)
            total += nb
            for by_value in (True, False):
                c.reset()
                c.call(e, n, t, by_value)
                c.check(exp, "rows %d V %d %s n %d t %d %s" % (rows, V, kind, n, t, "by value" if by_value else "device word"))
            if t < n - 1:
                assert nb == 0
    assert total > 0            # (the distinct histories ban at n = 1 only)
    if kind != "distinct":
        assert c.expected(3, 130)[1] > 0


def test_a_history_token_outside_the_vocabulary_is_skipped():
    """Negative ids and ids >= V in a matching position: no write, no fault; the in-range ones of the same row are banned."""
    e = eng()
    V = 37
    hist = np.zeros((2, LDH), dtype=np.int32)
    hist[0, 1:9] = [5, V, 5, -3, 5, 2 ** 30, 5, 6]        # n = 2 at t = 9 .. : the suffix (5) was followed by V, -3, 2^30, 6
    hist[0, 9] = 5
    hist[1, 1:10] = [7, 8, 7, 9, 7, V - 1, 7, 0, 7]       # followed by 8, 9, V - 1 and 0: all banned
    c = _Case(2, V, 40, hist)
    assert [list(b) for b in N.banned_rows(hist, 9, 2)] == [[-3, 6, V, 2 ** 30], [0, 8, 9, V - 1]]
    exp, nb = c.expected(2, 9)
    assert nb == 5
    for by_value in (True, False):
        c.reset()
        c.call(e, 2, 9, by_value)
        c.check(exp, "out-of-range tokens")


def test_graph_replay_reads_the_time_from_the_device():
    """ONE captured launch (at a time word below n - 1: it must be a node all the same), replayed with the word advanced on the
    device between the replays: every replay equals the rule at its step."""
    e = eng()
    rows, V, n = 5, 37, 3
    c = _Case(rows, V, 40, _history(rows, V, "two", 9))
    with torch.cuda.stream(e.work_stream):
        c.word.fill_(0)
        torch.cuda.synchronize()
        g = e.graph_capture(lambda: e.lib.call("zk_ngram_ban", c.lg.mat.ptr, c.ld, rows, V, c.h.mat.ptr, c.h.ld, 0,
                                               c.word.data_ptr(), n, VALUE, e.stream))
        try:
            assert e.last_graph_nodes == 1
            c.check(c.pristine, "capturing must not run the kernel")
            t = 0
            for step in (0, 1, 1, 1, 60, 1, 1, 66):
                c.word.add_(step)                 # on the device, between the replays
                t += step
                c.reset()
                e.graph_launch(g)
                c.check(c.expected(n, t)[0], "replay at t %d" % t)
            assert c.expected(n, t)[1] > 0
        finally:
            e.lib.call("zk_graph_destroy", g)


def test_a_time_word_outside_the_history_is_a_no_op():
    e = eng()
    c = _Case(5, 37, 40, _history(5, 37, "two", 3))
    for t in (LDH, LDH + 1000, -1):
        c.reset()
        c.call(e, 1, t, False)
        c.check(c.pristine, "time word %d" % t)


ERRORS = [
    ("n=0", dict(n=0)), ("n=17", dict(n=17)), ("n=-1", dict(n=-1)),
    ("ld=36", dict(ld=36)),
    ("ldh=8", dict(ldh=8, t=8)), ("ldh=8", dict(ldh=8, t=100)),
    ("rows=-1", dict(rows=-1)),
]


@pytest.mark.parametrize("word, kw", ERRORS, ids=["%s-%d" % (w, i) for i, (w, _) in enumerate(ERRORS)])
def test_refusals_name_the_argument_and_touch_nothing(word, kw):
    e = eng()
    c = _Case(5, 37, 40, _history(5, 37, "two", 4))
    kw = dict(kw)
    n, t = kw.pop("n", 2), kw.pop("t", 20)
    with pytest.raises(ZeroHipError, match=word):
        c.call(e, n, t, True, **kw)
    c.check(c.pristine, "refused call")


def test_nothing_to_do_returns_without_an_error():
    e = eng()
    c = _Case(5, 37, 40, _history(5, 37, "two", 5))
    c.call(e, 2, 20, True, rows=0)
    c.call(e, 2, 20, False, rows=0)
    c.call(e, 4, 2, True)                # t < n - 1
    c.check(c.pristine, "rows = 0 / t < n - 1")
