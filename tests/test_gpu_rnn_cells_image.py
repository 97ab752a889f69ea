"""The dense recurrent cell launches of zk_rnn.hip (ATR step, GRU gates, GRU out, ff + residual; bf16 and fp32 forms) as
cell epilogues over one tile driver per storage form: every output window must be the BYTES the eight hand-written kernels
produced (tests/golden/rnn_cells_parent.json, written by tests/golden/make_rnn_cell_golden.py on the commit before the
change: every sum keeps its order and every product its rounding).  The cases are those of tests/rnn_cell_cases.py; a case
the file does not hold fails."""
import functools

import pytest

pytestmark = pytest.mark.gpu

from tests import rnn_cell_cases as RC  # noqa: E402


@functools.lru_cache(maxsize=None)
def _golden():
    return RC.load()


@pytest.mark.parametrize("name", RC.CASES)
def test_cell_output_bytes_are_those_of_the_hand_written_kernels(name):
    golden = _golden()
    assert name in golden, "%s is not in %s: record it on the parent commit" % (name, RC.GOLDEN)
    got, want = RC.record(name), golden[name]
    assert sorted(got) == sorted(want), (name, sorted(got), sorted(want))
    for key in sorted(want):
        assert got[key]["sha256"] == want[key]["sha256"], (name, key, got[key]["head"], want[key]["head"])
