"""The host side of decoding issues the launches pinned in tests/golden/decode_launch_trace.json: the same entry points
in the same order with the same scalar arguments and the same pointer pattern, for every model in both decode dtypes, for
both forms of every decode switch, on the launch-per-op path, for an ensemble, for rnnsearch with both encoder forms, for
rnnsearch_deepatt with each of its four cells, for deepnmt in five configurations (tests/deepnmt_ref.CONFIGS (A), (B), (C),
(A) with olrn, (B) with lrn) and for the score_fn of the fp32 scorer and of transformer_fixup (tests/decode_trace.py; the file is written by
tests/golden/make_decode_launch_trace.py).  The library itself runs: nothing is faked."""
import pytest

from tests import decode_trace as DT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return DT.load()


def test_every_case_is_pinned(golden):
    assert sorted(golden) == sorted(DT.CASES)


@pytest.mark.parametrize("name", sorted(DT.CASES))
def test_launch_trace(name, golden, monkeypatch):
    got = DT.run_case(name, monkeypatch)
    print("%s: %s" % (name, DT.summary(got)))
    assert tuple(ph for ph in got if ph != "graph_nodes") == DT.phases(name)
    assert DT.CASES[name].get("score") or got["graph_nodes"] > 0
    msgs = DT.diff(golden[name], got)
    assert not msgs, "\n".join(msgs[:20])
