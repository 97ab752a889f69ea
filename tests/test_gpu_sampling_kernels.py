"""zk_sample_truncate called directly (zero_amd/csrc/zk_sample.hip) and held to the rule of tests/sampling_ref.py.

The logits are a parity.guarded fp32 buffer.  After every call the WHOLE buffer is compared with what it held: the guard
bands and the columns V .. ld-1 bit for bit, the window by sampling_ref.check -- kept entries bit-identical, dropped entries
equal to the value, the kept set a threshold set, and every token the rule decides on the right side.  The by-construction cases
have no undecided token (asserted) and are compared bit for bit with sampling_ref.apply; the random cases go under the band
checker, whose undecided share tests/test_sampling_host.py bounds on the CPU for the same inputs.

Shapes (sampling_ref.SHAPES, ROWS): rows in {1, 5, 128}; V / ld = 1 / 4, 37 / 40, 255 / 256, 257 / 264 (less than, and just
over, one trip of the 256-thread loops), 1000 / 1000, 32000 / 32000 (the flagship row), 32768 / 32768 (the longest row the
kernel stages in LDS) and 32769 / 32776 (the shortest one it re-reads per pass); and 37 / 39, 32001 / 32003, 32769 / 32771,
strides that are no multiple of four words, where the kernel reads word by word instead of 16 bytes at a time.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import parity as P  # noqa: E402
from tests import sampling_ref as S  # noqa: E402
from tests.util_gpu import eng  # noqa: E402
from zero_amd.hip import ZeroHipError  # noqa: E402
from zero_amd.models import _decode  # noqa: E402

F32 = torch.float32
VALUE = -1e8


class _Case(object):
    def __init__(self, x, ld):
        x = torch.as_tensor(x, dtype=F32)
        self.rows, self.V, self.ld = x.shape[0], x.shape[1], ld
        self.lg = P.guarded(self.rows, self.V, ld, 0, F32, x, "cuda")
        self.pristine = self.lg.t.clone()
        self.flat0 = self.pristine.cpu().numpy()
        self.before = self.block(self.flat0)
        self._band = None

    def block(self, flat):
        return flat[P.LEAD:P.LEAD + self.rows * self.ld].reshape(self.rows, self.ld)

    @property
    def band(self):
        if self._band is None:
            self._band = S.Band(self.before[:, :self.V])
        return self._band

    def reset(self):
        self.lg.t.copy_(self.pristine)

    def call(self, e, topk, topp, min_keep, value=VALUE, **kw):
        e.lib.call("zk_sample_truncate", kw.get("ptr", self.lg.mat.ptr), kw.get("ld", self.ld), kw.get("rows", self.rows),
                   kw.get("V", self.V), topk, topp, min_keep, value, e.stream)
        torch.cuda.synchronize()

    def after(self, what):
        """The buffer after a call: everything outside the rows bit-identical -> the [rows, ld] block."""
        flat = self.lg.t.cpu().numpy()
        a, b = flat.view(np.int32), self.flat0.view(np.int32)
        assert np.array_equal(a[:P.LEAD], b[:P.LEAD]) and np.array_equal(a[-P.LEAD:], b[-P.LEAD:]), what + ": a guard band changed"
        return self.block(flat)

    def check_band(self, topk, topp, min_keep, what):
        S.check(self.before, self.after(what), self.V, topk, S.f32(topp), min_keep, VALUE, what, band=self.band)

    def check_exact(self, topk, topp, min_keep, what):
        """No token is undecided: the result is sampling_ref.apply's, bit for bit."""
        assert int(self.band.undecided(topk, S.f32(topp), min_keep).max()) == 0, what
        exp = S.apply(self.before, self.V, topk, S.f32(topp), min_keep, np.float32(VALUE))
        got = self.after(what)
        if not np.array_equal(got.view(np.int32), exp.view(np.int32)):
            r, v = np.argwhere(got.view(np.int32) != exp.view(np.int32))[0]
            raise AssertionError("%s: %d entries differ from the rule; the first at row %d, column %d: %r, expected %r (input %r)"
                                 % (what, int((got.view(np.int32) != exp.view(np.int32)).sum()), r, v, got[r, v], exp[r, v],
                                    self.before[r, v]))

    def unchanged(self, what):
        assert torch.equal(self.lg.t.view(torch.int32), self.pristine.view(torch.int32)), what + ": the buffer changed"


# ---------------------------------------------------------------------------------------------- random rows, the band checker
@pytest.mark.parametrize("rows,V,ld,variant", S.random_cases(), ids=lambda v: str(v))
def test_random_rows_under_the_band_checker(rows, V, ld, variant):
    e = eng()
    c = _Case(S.random_logits(rows, V, variant), ld)
    dropped = 0
    for topk, topp, mk in S.random_settings(rows, V):
        what = "rows %d V %d %s topk %d topp %g min_keep %d" % (rows, V, variant, topk, topp, mk)
        c.reset()
        c.call(e, topk, topp, mk)
        c.check_band(topk, topp, mk, what)
        dropped += int((c.after(what).view(np.int32) != c.before.view(np.int32)).sum())
    assert dropped > 0 or V <= 1


@pytest.mark.parametrize("V,ld", S.SHAPES)
def test_topp_one_alone_changes_nothing(V, ld):
    """topp = 1.0 with topk = 0 is an active setting (the launch happens) that keeps every token: bit-identical."""
    e = eng()
    for variant in ("plain", "peaked"):
        c = _Case(S.random_logits(5, V, variant), ld)
        c.call(e, 0, 1.0, 1)
        c.unchanged("topp = 1 V %d %s" % (V, variant))


def test_both_off_launches_nothing():
    """topk = topp = 0: the library returns without a launch (the buffer is untouched, even with arguments that a launch
    would refuse nothing of), and the host helper does not even call (the call counter stands still)."""
    e = eng()
    c = _Case(S.random_logits(5, 37, "plain"), 40)
    c.call(e, 0, 0.0, 1)
    c.unchanged("both off")
    n0 = e.lib.ncalls
    _decode.sample_truncate(e, c.lg.mat, 5, 37, 0, 0.0, 9, 1e8)
    assert e.lib.ncalls == n0
    _decode.sample_truncate(e, c.lg.mat, 5, 37, 2, 0.0, 1, 1e8)          # (and with a setting on it writes -forbid_value)
    torch.cuda.synchronize()
    assert e.lib.ncalls == n0 + 1
    c.check_exact(2, 0.0, 1, "through the helper")


def test_two_runs_are_bit_identical():
    """The largest case, every kind of setting: the second run on the same input gives the same bits."""
    e = eng()
    V, ld = S.LDS_MAX_V + 1, S.LDS_MAX_V + 8
    c = _Case(S.random_logits(128, V, "plain"), ld)
    for topk, topp, mk in ((0, 0.9, 1), (10, 0.5, 9), (V - 1, 0.999, 3)):
        runs = []
        for _ in range(2):
            c.reset()
            c.call(e, topk, topp, mk)
            runs.append(c.lg.t.clone())
        assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), (topk, topp, mk)
        assert not torch.equal(runs[0].view(torch.int32), c.pristine.view(torch.int32))


# ---------------------------------------------------------------------------------------------- by construction
@pytest.mark.parametrize("V,ld", S.CONSTRUCTED_SHAPES)
@pytest.mark.parametrize("kind", S.CONSTRUCTED)
def test_rows_built_for_one_answer(kind, V, ld):
    """sampling_ref.constructed: planted ties straddling rank k, all-equal rows, two-level rows either side of the mass
    boundary, geometric rows, rows that already hold -1e8 entries.  Where no token is undecided (everywhere but the nucleus
    settings of the pre-banned random rows; tests/test_sampling_host.py asserts it on the CPU) the result is the rule's bit
    for bit; the number of kept tokens is the one the construction names."""
    e = eng()
    x, settings = S.constructed(kind, V)
    c = _Case(x, ld)
    for topk, topp, mk, count in settings:
        what = "%s V %d topk %d topp %g min_keep %d" % (kind, V, topk, topp, mk)
        c.reset()
        c.call(e, topk, topp, mk)
        if kind == "prebanned" and topp > 0:
            c.check_band(topk, topp, mk, what)
        else:
            c.check_exact(topk, topp, mk, what)
        got = c.after(what)[:, :V]
        if kind == "equal":
            c.unchanged(what)
        if kind == "prebanned":
            assert (got[c.before[:, :V] == np.float32(VALUE)] == np.float32(VALUE)).all(), what
        n = ((got != np.float32(VALUE)).sum(1))
        if isinstance(count, dict):
            for r, want in count.items():
                assert n[r] == want, (what, r, n[r], want)
        elif count is not None:
            assert (n == count).all(), (what, n, count)


@pytest.mark.parametrize("V,ld", [(1, 4)])
def test_a_single_candidate_is_kept(V, ld):
    e = eng()
    c = _Case(np.full((5, V), 0.375, np.float32), ld)
    for topk, topp in ((1, 0.0), (0, 1e-6), (1, 0.5)):
        c.call(e, topk, topp, 1)
        c.unchanged("V = 1 topk %d topp %g" % (topk, topp))


# ---------------------------------------------------------------------------------------------- refusals
ERRORS = [
    ("ld=36", dict(ld=36)), ("V=0", dict(V=0)), ("V=-3", dict(V=-3)), ("rows=-1", dict(rows=-1)),
    ("topk=-1", dict(topk=-1)), ("topp=-0.1", dict(topp=-0.1)), ("topp=1.5", dict(topp=1.5)), ("topp=nan", dict(topp=float("nan"))),
    ("min_keep=0", dict(min_keep=0)), ("min_keep=-2", dict(min_keep=-2)), ("logits", dict(ptr=None)),
]


@pytest.mark.parametrize("word, kw", ERRORS, ids=[w for w, _ in ERRORS])
def test_refusals_name_the_argument_and_touch_nothing(word, kw):
    e = eng()
    c = _Case(S.random_logits(5, 37, "plain"), 40)
    kw = dict(kw)
    topk, topp, mk = kw.pop("topk", 3), kw.pop("topp", 0.5), kw.pop("min_keep", 1)
    with pytest.raises(ZeroHipError, match=word):
        c.call(e, topk, topp, mk, **kw)
    c.unchanged("refused call")


def test_no_rows_returns_without_an_error():
    e = eng()
    c = _Case(S.random_logits(5, 37, "plain"), 40)
    c.call(e, 3, 0.5, 1, rows=0)
    c.call(e, 3, 0.5, 1, rows=0, ptr=None)
    c.unchanged("rows = 0")
