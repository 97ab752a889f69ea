"""zk_prefix_force called directly (zero_amd/csrc/zk_prefix.hip) and held to EXACT equality with the rule of
tests/prefix_ref.py.

The logits are a parity.guarded fp32 buffer whose window is prefilled with NaN (the kernel never reads a row, and the forced
entry and every row that is not forced must keep their bits), the table an int32 tensor.  After every call the WHOLE logits
buffer -- window, the columns between V and ld, the guard bands -- is compared on the device, bit for bit, with the prefill in
which prefix_ref.force has rewritten the window; the table must be what it was.  tests/test_prefix_checker.py shows that the
rule rejects planted defects.

Cases: (rows, rows_per_sentence) in {(1, 1), (4, 4), (4, 1), (24, 6), (24, 4)}; V in {5, 37, 4099, 32000} (below one vector's
worth of columns; no multiple of 4; more than one workgroup per row with a part-filled last one; eight workgroups per row);
ld = V, ld = V + 3 (rows of every alignment) and the window one float into the buffer (a base that is not 16-byte aligned);
forced tokens 1, 3, 4, 5 and V - 1 (5 = V at V = 5: an id the row lacks, which forces nothing); sentences of the lengths 5, 0,
3, 6, 1, 2 in a table of ldp = 6, so every time has rows whose prefix has ended (a 0 at t) beside forced ones; t in {0, 1, 2,
ldp - 1, ldp}.  Each runs with the time by value and with the time read from a device word.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import parity as P  # noqa: E402
from tests import prefix_ref as PR  # noqa: E402
from tests.util_gpu import eng  # noqa: E402
from zero_amd.hip import ZeroHipError  # noqa: E402

F32 = torch.float32
LDP = 6
VALUE = -1e8
EOS = 2
SHAPES = [(1, 1), (4, 4), (4, 1), (24, 6), (24, 4)]
LENGTHS = (5, 0, 3, 6, 1, 2)
TIMES = (0, 1, 2, LDP - 1, LDP)


def _table(B, V, shift=0):
    toks = [1, 3, 4, 5, V - 1]
    out = np.zeros((B, LDP), dtype=np.int32)
    for b in range(B):
        n = LENGTHS[(b + shift) % len(LENGTHS)]
        out[b, :n] = [toks[(b + t) % 5] for t in range(n)]
    return out


class _Case(object):
    def __init__(self, rows, rps, V, ld, off, table):
        self.rows, self.rps, self.V, self.ld, self.table = rows, rps, V, ld, table
        self.lg = P.guarded(rows, V, ld, off, F32, None, "cuda")
        self.pristine = self.lg.t.clone()
        self.host = self.pristine.cpu()
        self.tab = torch.from_numpy(table).to("cuda")
        self.tab0 = self.tab.clone()
        self.word = torch.zeros(1, dtype=torch.int32, device="cuda")

    def reset(self):
        self.lg.t.copy_(self.pristine)

    def expected(self, t, eos=EOS):
        """The whole flat logits buffer after the call, and the number of forced rows."""
        exp = self.host.clone()
        win = self.lg.window(exp)
        new = PR.force(win.numpy(), self.V, self.table, t, self.rps, VALUE, eos)
        forced = int((~np.isnan(new)).any(axis=1).sum())
        win.copy_(torch.from_numpy(new))
        return exp.to("cuda"), forced

    def call(self, e, t, by_value, eos=EOS, rows=None, V=None, ld=None, ldp=None, rps=None):
        if not by_value:
            self.word.fill_(t)
        e.lib.call("zk_prefix_force", self.lg.mat.ptr, self.ld if ld is None else ld, self.rows if rows is None else rows,
                   self.V if V is None else V, self.tab.data_ptr(), LDP if ldp is None else ldp,
                   self.rps if rps is None else rps, t if by_value else -7, None if by_value else self.word.data_ptr(), eos,
                   VALUE, e.stream)

    def check(self, exp, what):
        torch.cuda.synchronize()
        if not torch.equal(self.lg.t.view(torch.int32), exp.view(torch.int32)):
            self.lg.check_guard(what)               # names a write outside the window, if that is what happened
            bad = torch.nonzero(self.lg.t.view(torch.int32) != exp.view(torch.int32)).reshape(-1)
            r, c = self.lg._where(bad[0])
            raise AssertionError("%s: %d logits differ from the rule; the first at row %d, column %d: %r, expected %r"
                                 % (what, bad.numel(), r, c, float(self.lg.t[bad[0]]), float(exp[bad[0]])))
        assert torch.equal(self.tab, self.tab0), what + ": the table changed"


def _layouts(V):
    return [(V, 0), (V + 3, 0), (V + 3, 1), (V + 1, 1)]


@pytest.mark.parametrize("V", [5, 37, 4099, 32000])
@pytest.mark.parametrize("rows,rps", SHAPES)
def test_equals_the_rule(rows, rps, V):
    e = eng()
    forced_rows = free_rows = 0
    for ld, off in _layouts(V):
        c = _Case(rows, rps, V, ld, off, _table(rows // rps, V, shift=ld + off))
        assert (c.lg.mat.ptr % 16 != 0) == (off == 1)
        for t in TIMES:
            exp, nf = c.expected(t)
            forced_rows += nf
            free_rows += rows - nf
            if t == LDP:
                assert nf == 0
            for by_value in (True, False):
                c.reset()
                c.call(e, t, by_value)
                c.check(exp, "rows %d/%d V %d ld %d off %d t %d %s" % (rows, rps, V, ld, off, t,
                                                                     "by value" if by_value else "device word"))
    assert forced_rows > 0 and free_rows > 0


def test_every_forced_token_and_an_untouched_row():
    """By hand at V = 37, one sentence per row: the tokens 1, 3, 4, 5 and V - 1 (in the first vector, across its end, in the
    tail columns), a 0 (NaNs intact) and the ids 37 = V and 2^30, which force nothing."""
    e = eng()
    V = 37
    table = np.zeros((8, LDP), dtype=np.int32)
    table[:, 0] = [1, 3, 4, 5, V - 1, 0, V, 2 ** 30]
    for ld, off in _layouts(V):
        c = _Case(8, 1, V, ld, off, table)
        exp, nf = c.expected(0)
        assert nf == 5
        win = c.lg.window(exp.cpu())
        for r, tok in enumerate([1, 3, 4, 5, V - 1]):
            row = win[r]
            assert torch.isnan(row[tok]) and row[EOS] == 2 * VALUE
            assert int((row == VALUE).sum()) == V - 2 and int(torch.isnan(row).sum()) == 1
        assert torch.isnan(win[5:]).all()
        for by_value in (True, False):
            c.reset()
            c.call(e, 0, by_value)
            c.check(exp, "tokens by hand, ld %d off %d" % (ld, off))


def test_no_eos_entry_is_lowered_with_eos_id_minus_1():
    e = eng()
    c = _Case(24, 6, 4099, 4102, 1, _table(4, 4099))
    exp, nf = c.expected(0, eos=-1)
    assert nf > 0 and not bool((exp == 2 * VALUE).any())
    for by_value in (True, False):
        c.reset()
        c.call(e, 0, by_value, eos=-1)
        c.check(exp, "eos_id = -1")


def test_a_time_word_outside_the_table_is_a_no_op():
    e = eng()
    c = _Case(4, 4, 37, 40, 0, _table(1, 37))
    for t in (LDP, LDP + 1000, -1, -2 ** 31):
        c.reset()
        c.call(e, t, False)
        c.check(c.pristine, "time word %d" % t)


def test_graph_replay_reads_the_time_from_the_device():
    """ONE captured launch, replayed three times with the word advanced on the device between the replays: every replay equals
    the rule at its step."""
    e = eng()
    rows, rps, V = 24, 4, 4099
    c = _Case(rows, rps, V, V + 3, 1, _table(rows // rps, V))
    with torch.cuda.stream(e.work_stream):
        c.word.fill_(0)
        torch.cuda.synchronize()
        g = e.graph_capture(lambda: e.lib.call("zk_prefix_force", c.lg.mat.ptr, c.ld, rows, V, c.tab.data_ptr(), LDP, rps, 0,
                                               c.word.data_ptr(), EOS, VALUE, e.stream))
        try:
            assert e.last_graph_nodes == 1
            c.check(c.pristine, "capturing must not run the kernel")
            seen = set()
            for t in (0, 1, 2):
                c.reset()
                e.graph_launch(g)
                exp, nf = c.expected(t)
                c.check(exp, "replay at t %d" % t)
                seen.add(nf)
                c.word.add_(1)                    # on the device, between the replays
            assert len(seen) > 1                  # (the replays did not all force the same rows)
        finally:
            e.lib.call("zk_graph_destroy", g)


ERRORS = [
    ("ld=36", dict(ld=36)),
    ("rows=5 is no multiple of rows_per_sentence=4", dict(rows=5)),
    ("rows_per_sentence=0", dict(rps=0)),
    ("ldp=0", dict(ldp=0)), ("ldp=-3", dict(ldp=-3)),
    ("time=-1", dict(t=-1)),
    ("rows=-4", dict(rows=-4)),
]


@pytest.mark.parametrize("word, kw", ERRORS, ids=["%s-%d" % (w.split(" ")[0], i) for i, (w, _) in enumerate(ERRORS)])
def test_refusals_name_the_argument_and_touch_nothing(word, kw):
    e = eng()
    c = _Case(4, 4, 37, 40, 0, _table(1, 37))
    kw = dict(kw)
    t = kw.pop("t", 0)
    with pytest.raises(ZeroHipError, match=word):
        c.call(e, t, True, **kw)
    c.check(c.pristine, "refused call")


def test_nothing_to_do_returns_without_an_error():
    e = eng()
    c = _Case(4, 4, 37, 40, 0, _table(1, 37))
    c.call(e, 0, True, rows=0)
    c.call(e, 0, False, rows=0)
    c.call(e, LDP, True)                 # by value past the table: no launch
    c.check(c.pristine, "rows = 0 / t = ldp")
