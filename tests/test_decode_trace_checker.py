"""tests/decode_trace.diff, the comparison of tests/test_gpu_decode_launch_trace.py, on hand-made traces: it accepts a
trace that went through the file format, and names a swapped pair of launches, a dropped launch, an added launch, a
changed integer, a changed float, a pointer that became NULL and a changed graph node count."""
import copy

from tests import decode_trace as DT


def _trace():
    step = [["zk_dec_embed", ["nonnull", 0, "nonnull", None, 20, 128, 11.313708498984761, 0]],
            ["zk_gemm", ["nonnull", "nonnull", 20, 104, 128, 1.0, None]],
            ["zk_ln_decode", ["nonnull", None, 20, 128, 1e-06]]]
    return {"encode": [["zk_zero", ["nonnull", 4096, "nonnull"]]], "step0": copy.deepcopy(step), "reorder": [],
            "step1": copy.deepcopy(step), "graph_nodes": 17}


def test_round_trip_through_the_file(tmp_path):
    path = str(tmp_path / "trace.json")
    DT.dump({"a": _trace(), "b": _trace()}, path)
    back = DT.load(path)
    assert sorted(back) == ["a", "b"]
    assert DT.diff(_trace(), back["a"]) == [] and DT.diff(back["b"], _trace()) == []


def test_swapped_launches_and_a_changed_integer_are_named():
    got = _trace()
    got["step0"][1], got["step0"][2] = got["step0"][2], got["step0"][1]
    got["step1"][1][1][3] = 105
    msgs = DT.diff(_trace(), got)
    assert len(msgs) == 2
    assert "step0: launch 1 is zk_ln_decode, recorded zk_gemm" in msgs[0]
    assert "step1: launch 1 (zk_gemm) argument 3 is 105, recorded 104" in msgs[1]


def test_every_other_kind_of_change_is_named():
    for change, word in ((lambda t: t["step0"].pop(), "2 launches, recorded 3"),
                         (lambda t: t["encode"].append(["zk_zero", ["nonnull", 8, "nonnull"]]), "2 launches, recorded 1"),
                         (lambda t: t["step1"][0][1].__setitem__(6, 11.0), "argument 6 is 11.0"),
                         (lambda t: t["step1"][0][1].__setitem__(0, None), "argument 0 is None, recorded 'nonnull'"),
                         (lambda t: t["step1"][1][1].__setitem__(5, 1), "argument 5 is 1, recorded 1.0"),
                         (lambda t: t["step1"][2][1].pop(), "has 4 arguments, recorded 5"),
                         (lambda t: t.__setitem__("graph_nodes", 18), "graph_nodes: 18, recorded 17"),
                         (lambda t: t.pop("reorder"), "phases differ")):
        got = _trace()
        change(got)
        msgs = DT.diff(_trace(), got)
        assert len(msgs) == 1 and word in msgs[0], (word, msgs)
