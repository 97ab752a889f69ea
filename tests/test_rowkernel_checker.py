"""The row-kernel references and bounds of tests/parity.py have teeth (CPU only).  Over the case lists of
tests/test_gpu_rowkernels_elementwise.py:

  * a correct stand-in (parity.*_standin: the kernel's arithmetic in fp32, bf16 at the storage sites, torch's summation
    order) passes every case with nothing excused; the worst |err| / bound is printed and is below 1;
  * each planted defect fails at every case listed beside it (``*_DEFECTS``: defect -> the cases it applies to), and the
    checker's message names an output and a (row, col) inside the defect.
"""
import math
import re

import pytest
import torch

from tests import parity as P
from tests.test_gpu_rowkernels_elementwise import (
    EPS, KINDS, LN_FWD_CASES, ROW_TINY, ln_fwd_inputs, cpu_mask, LN_BWD_CASES, LN_BWD_EXACT, ln_bwd_inputs, CE_CASES,
    CE_T, CE_ROW_W0, CE_ROW_EQUAL, ce_inputs, COLSUM_CASES, colsum_inputs, COLSUM_PAIR_CASES, colsum_pair_terms)


def _fails(check, names=None, rows=None, cols=None, index_is_col=("mean", "rstd")):
    """``check`` raises the checker's error; the output it names is one of ``names`` and its (row, col) lies in rows x cols
    (None: anywhere).  The per-row fp32 outputs (1 x rows windows) carry the row in their column."""
    with pytest.raises(AssertionError, match="outside their bound") as info:
        check()
    m = re.search(r"\[(\w+)\]: .*?\(row (\d+), col (\d+)\)", str(info.value))
    assert m, str(info.value)
    name, r, c = m.group(1), int(m.group(2)), int(m.group(3))
    assert names is None or name in names, str(info.value)
    if name in index_is_col:
        r, c = c, None
    assert rows is None or r in rows, str(info.value)
    assert cols is None or c is None or c in cols, str(info.value)
    return name


def _report(what, worst):
    print("%s: worst |err| / bound %s" % (what, {k: "%.3g" % v for k, v in worst.items()}))
    assert all(v < 1 for v in worst.values()), (what, worst)


# ---------------------------------------------------------------------------------------------- LayerNorm forward
def _ln_fwd(case, defect=None, at=(0, 0)):
    inp = ln_fwd_inputs(case)
    scale = cpu_mask(case["rows"], case["H"], case["drop"])
    a = (inp["x"], inp["y"], scale, inp["gamma"], inp["beta"], EPS)
    got = P.ln_fwd_standin(*a, case["save"], defect, at)
    return got, P.ln_fwd_bound(*a, s_stored=got["s"])


def test_ln_fwd_standin_passes_everywhere():
    assert {c["H"] for c in LN_FWD_CASES} == {8, 64, 72, 504, 512, 520, 1024, 1032, 2048}
    worst = {}
    for case in LN_FWD_CASES:
        got, bounds = _ln_fwd(case)
        for k, v in P.check_all(got, bounds, "stand-in %s" % case).items():
            worst[k] = max(worst.get(k, 0.0), v)
    _report("LayerNorm forward stand-in", worst)


_ANY = lambda c: True
_SPECIAL = lambda c: c["rows"] >= 5
LN_FWD_DEFECTS = {            # defect -> (the cases, at(case), the rows and the columns the message may name)
    "short_stats": (lambda c: c["H"] >= 16, lambda c: (0, 0), lambda c: None, lambda c: None),
    "eps_outside": (_SPECIAL, lambda c: (ROW_TINY, 0), lambda c: {ROW_TINY}, lambda c: None),
    "neighbour": (_SPECIAL, lambda c: (0, 0), lambda c: {0}, lambda c: None),
    "stale": (_ANY, lambda c: (c["rows"] - 1, c["H"] - 8), lambda c: {c["rows"] - 1}, lambda c: range(c["H"] - 8, c["H"])),
    "drop_ignored": (lambda c: c["drop"] > 0, lambda c: (0, 0), lambda c: {0}, lambda c: range(8) if c["save"] else None),
}


@pytest.mark.parametrize("defect", list(LN_FWD_DEFECTS))
def test_each_planted_ln_fwd_defect_fails(defect):
    applies, at, rows, cols = LN_FWD_DEFECTS[defect]
    cases = [c for c in LN_FWD_CASES if applies(c)]
    assert len(cases) >= 5
    for case in cases:
        got, bounds = _ln_fwd(case, defect, at(case))
        names = ("out",) if defect in ("neighbour", "stale") else None
        _fails(lambda: P.check_all(got, bounds, "%s %s" % (defect, case)), names, rows(case), cols(case))
    print("LayerNorm forward defect %s: fails at each of its %d cases" % (defect, len(cases)))


def test_unbiased_variance_fails_through_rstd_at_every_h_and_through_out_up_to_512():
    """At H = 1024 and above the unbiased variance moves no element of a bf16 ``out`` beyond its rounding: the fp32
    ``rstd`` is where it shows."""
    seen = set()
    for case in LN_FWD_CASES:
        got, bounds = _ln_fwd(case, "unbiased")
        what = "unbiased %s" % case
        if case["save"]:
            _fails(lambda: P.assert_elementwise(got["rstd"], *bounds["rstd"], what + " [rstd]"), ("rstd",))
            seen.add(case["H"])
        if case["H"] <= 512:
            _fails(lambda: P.assert_elementwise(got["out"], *bounds["out"], what + " [out]"), ("out",))
    assert seen == {c["H"] for c in LN_FWD_CASES}
    print("LayerNorm forward defect unbiased: fails through rstd at every H, through out at every case with H <= 512")


# ---------------------------------------------------------------------------------------------- LayerNorm backward
def _ln_bwd(case, defect=None, at=0):
    inp = ln_bwd_inputs(case)
    scale = cpu_mask(case["rows"], case["H"], case["drop"])
    a = (inp["dout"], inp["s"], inp["mean"], inp["rstd"], inp["gamma"], scale)
    got = P.ln_bwd_standin(*a, defect, at)
    return got, P.ln_bwd_bound(*a, got["ds"], got["dy"]), (LN_BWD_EXACT if case["kind"] == "exact" else ())


def test_ln_bwd_standin_passes_everywhere():
    worst = {}
    for case in LN_BWD_CASES:
        got, bounds, exact = _ln_bwd(case)
        for k, v in P.check_all(got, bounds, "stand-in %s" % case, exact=exact).items():
            worst[k] = max(worst.get(k, 0.0), v)
    _report("LayerNorm backward stand-in", worst)


_SUMS = ("dgamma", "dbeta", "dbias_prev")
LN_BWD_DEFECTS = {            # defect -> (the cases, the outputs the message may name)
    "drop_term": (lambda c: c["kind"] == "random", ("ds",)),            # (the term is 0 by construction in the exact kind)
    "rows16_31": (lambda c: c["rows"] >= 32, _SUMS),
    "last_row": (lambda c: c["kind"] == "exact", _SUMS),               # 37 and 4100 rows of small integers
    "dbp_noscale": (lambda c: c["drop"] > 0, ("dbias_prev",)),
}


@pytest.mark.parametrize("defect", list(LN_BWD_DEFECTS))
def test_each_planted_ln_bwd_defect_fails(defect):
    applies, names = LN_BWD_DEFECTS[defect]
    cases = [c for c in LN_BWD_CASES if applies(c)]
    assert len(cases) >= 4 and (defect != "last_row" or any(c["rows"] == 4100 for c in cases))
    for case in cases:
        at = case["rows"] // 2
        got, bounds, exact = _ln_bwd(case, defect, at)
        _fails(lambda: P.check_all(got, bounds, "%s %s" % (defect, case), exact=exact), names,
               {at} if defect == "drop_term" else None)
    print("LayerNorm backward defect %s: fails at each of its %d cases" % (defect, len(cases)))


# ---------------------------------------------------------------------------------------------- cross entropy
def _ce(case, defect=None, at=0):
    V, ld, ls = case
    inp = ce_inputs(case)
    got = P.ce_standin(inp["z"], inp["ids"], inp["w"], V, ld, ls, defect, at)
    return got, P.ce_bound(P.ce_terms(inp["z"], inp["ids"], inp["w"], V, ld, ls)), inp


def test_ce_reference_gives_the_known_answer_on_the_all_equal_row():
    for V, ld, ls in CE_CASES:
        inp = ce_inputs((V, ld, ls))
        t = P.ce_terms(inp["z"], inp["ids"], inp["w"], V, ld, ls)
        # (p + (V - 1) q is 1 only to fp32 rounding, and the row's logits are 0.5: 2^-24 of that is the slack)
        assert abs(float(t["ce"][CE_ROW_EQUAL]) - (math.log(V) - P.ce_constants(V, ls)[2])) < 2.0 ** -24
        assert float(t["dl"][:, V:].abs().max() if ld > V else 0.0) == 0.0 and float(t["dl"][CE_ROW_W0].abs().max()) == 0.0


def test_ce_standin_passes_everywhere():
    worst, need = {}, 0.0
    for case in CE_CASES:
        got, bounds, inp = _ce(case)
        for k, v in P.check_all(got, bounds, "stand-in V=%d ld=%d ls=%g" % case).items():
            worst[k] = max(worst.get(k, 0.0), v)
        fwd = P.ce_standin(inp["z"], inp["ids"], None, *case)
        P.check_all(fwd, {"ce": bounds["ce"]}, "stand-in forward only V=%d ld=%d ls=%g" % case)
        need = max([need] + list(P.ce_c_exp_needed(P.ce_terms(inp["z"], inp["ids"], inp["w"], *case), got["ce"], got["dl"]).values()))
    print("cross entropy stand-in (torch's exp and log, not the GPU's): c_exp needed %.3g, C_EXP %g" % (need, P.C_EXP))
    _report("cross entropy stand-in", worst)


_LIVE = set(range(CE_T)) - {CE_ROW_W0}
CE_DEFECTS = {                # defect -> (the cases, the outputs, the rows, the columns(case) the message may name)
    "no_q": (lambda c: c[2] > 0, ("dl",), _LIVE, lambda c: range(c[0])),
    "gold_shift": (_ANY, ("ce", "dl"), None, lambda c: None),
    "no_norm": (lambda c: c[2] > 0, ("ce",), None, lambda c: None),
    "lse_tail": (lambda c: c[0] % 4 != 0, ("ce", "dl"), None, lambda c: None),
    "pad": (lambda c: c[1] > c[0], ("dl",), {0}, lambda c: {c[0]}),
    "w0": (_ANY, ("dl",), {CE_ROW_W0}, lambda c: range(c[0])),
}


@pytest.mark.parametrize("defect", list(CE_DEFECTS))
def test_each_planted_ce_defect_fails(defect):
    applies, names, rows, cols = CE_DEFECTS[defect]
    cases = [c for c in CE_CASES if applies(c)]
    assert len(cases) >= 10
    for case in cases:
        got, bounds, _ = _ce(case, defect)
        _fails(lambda: P.check_all(got, bounds, "%s V=%d ld=%d ls=%g" % ((defect,) + case)), names, rows, cols(case),
               index_is_col=("ce",))
    print("cross entropy defect %s: fails at each of its %d cases with C_EXP = %g" % (defect, len(cases), P.C_EXP))


# ---------------------------------------------------------------------------------------------- column sums
def _colsum(case, kind, p, defect=None):
    rows, N = case["rows"], case["N"]
    a, prev = colsum_inputs(rows, N, kind, acc=case["acc"])
    scale = cpu_mask(rows, N, p if case["drop"] else 0.0)
    got = P.colsum_standin(a, case["skip"], scale, prev, defect)
    return {"out": got}, {"out": P.colsum_ref(a, case["skip"], scale, prev)}, (("out",) if kind == "exact" else ())


def test_colsum_standin_passes_everywhere():
    assert {c["rows"] for c in COLSUM_CASES} == {1, 31, 32, 33, 255, 256, 257, 16500}
    worst = 0.0
    for case in COLSUM_CASES:
        for kind, p in KINDS:
            got, bounds, exact = _colsum(case, kind, p)
            worst = max(worst, P.check_all(got, bounds, "stand-in %s %s" % (case, kind), exact=exact)["out"])
    _report("column sum stand-in", {"out": worst})


# defect -> (the cases, the kinds(case)): the worst-case bound of 16500 random rows hides a chunk of 32 and a
# previous value of order 1; the integers show both
_UP_TO_257 = lambda c: ("random", "exact") if c["rows"] <= 257 else ("exact",)
COLSUM_DEFECTS = {
    "skip_included": (lambda c: c["skip"] > 0, _UP_TO_257),
    "last_chunk": (lambda c: not (c["rows"] == 1 and c["skip"] > 0), _UP_TO_257),      # (row 0 is skipped anyway)
    "acc_ignored": (lambda c: c["acc"], _UP_TO_257),
}


@pytest.mark.parametrize("defect", list(COLSUM_DEFECTS))
def test_each_planted_colsum_defect_fails(defect):
    applies, kinds = COLSUM_DEFECTS[defect]
    cases = [c for c in COLSUM_CASES if applies(c)]
    assert len(cases) >= 6 and any(c["rows"] == 16500 for c in cases)
    for case in cases:
        for kind, p in KINDS:
            if kind in kinds(case):
                got, bounds, exact = _colsum(case, kind, p, defect)
                _fails(lambda: P.check_all(got, bounds, "%s %s %s" % (defect, case, kind), exact=exact), ("out",))
    print("column sum defect %s: fails at each of its %d cases" % (defect, len(cases)))


@pytest.mark.parametrize("case", COLSUM_PAIR_CASES)
def test_colsum_pair_standin_passes_and_side_b_added_twice_fails(case):
    ra, rb, ska, skb, N = case
    for kind, p in KINDS:
        for drop in (0.0, p):
            a, _ = colsum_inputs(ra, N, kind, 1, acc=0)
            b, _ = colsum_inputs(rb, N, kind, 2, acc=0)
            sa, sb = cpu_mask(ra, N, drop, 5), cpu_mask(rb, N, drop, 6)
            bounds = {"out": P.colsum_ref(colsum_pair_terms(a, ska, sa, b, skb, sb))}
            exact = ("out",) if kind == "exact" else ()
            good = P.colsum_standin(a, ska, sa) + P.colsum_standin(b, skb, sb)
            worst = P.check_all({"out": good}, bounds, "stand-in pair %s %s" % (case, kind), exact=exact)
            assert worst["out"] < 1
            twice = good + P.colsum_standin(b, skb, sb)
            _fails(lambda: P.check_all({"out": twice}, bounds, "b_twice %s %s" % (case, kind), exact=exact), ("out",))


def test_exact_check_names_the_first_element_that_differs():
    ref = torch.arange(12.0).double()
    got = ref.float().clone()
    P.assert_exact(got, ref, "sum [out]")
    got[7] += 2.0 ** -17
    with pytest.raises(AssertionError, match=r"row 0, col 7"):
        P.assert_exact(got, ref, "sum [out]")
    got[3] = float("nan")
    with pytest.raises(AssertionError, match=r"row 0, col 3"):
        P.assert_exact(got, ref, "sum [out]")
