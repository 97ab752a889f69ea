"""The check of tests/test_gpu_chain_elementwise.py has teeth (CPU only): the stand-in of tests/chain_ref.py (fp32, bf16 at
the storage sites, Chan's combination of per-64-column partials, per-64-column partial row means in the backward) stays
inside every staged bound on every case, and each planted defect fails the check on the cases named here.

The stand-in's worst |err| / bound per tensor over all cases (re-measured on every run; every one must be <= 1):

    forward   (60 cases)   s 0.990   mean 0.0061   rstd 0.032   y 0.991
    backward  (60 cases)   ds 0.845   dy 0.663   partials 0.964
    attention (31 cases)   q 0.989   k 0.989   v 0.988   att 4.36e-3 (row ratio, bar 7.9e-3)   lse 3.3e-5 of its bar
                           s 0.983   mean 0.0023   rstd 0.015   y 0.987

s, y, ds and the partials sit near 1 because their bounds are dominated by ONE half-ulp bf16 rounding (of the value itself,
or of the product / dout that is never stored), which a correct kernel does reach; mean and rstd have no bf16 term.

Every planted defect is caught on EVERY case it can change anything on (chain_ref.fwd_applies / bwd_applies); NOT_CAUGHT is
empty.  (A missing peer partial of the backward's row means is planted at the row's largest partial: with a signed gamma a
partial can be ~0, and leaving out nothing changes nothing.)
"""
import pytest
import torch

from tests import chain_ref as C
from tests import parity as P
from tests.test_gpu_attention_elementwise import C_X

# defect -> the applicable cases that do NOT catch it, with the reason (none)
NOT_CAUGHT = {}


def _masks(c):
    B, nh, Lq, Lk = c["B"], c["nh"], c["Lq"], c["Lk"]
    am = C.cpu_mask(B * nh * Lq, Lk, c["drop"], 3)
    return {"attn": None if am is None else am.view(B, nh, Lq, Lk), "tail": C.cpu_mask(B * Lq, nh * C.ATT_D, c["drop"], 4)}


@pytest.fixture(scope="module")
def fwd_runs():
    """Inputs, mask and stand-in of every forward case, computed once and left unchanged."""
    out = []
    for c in C.FWD_CASES:
        x, m = C.fwd_inputs(c), C.cpu_mask(c["M"], c["N"], c["drop"], 1)
        out.append((c, x, m, C.fwd_standin(x, m, c["save"])))
    return out


@pytest.fixture(scope="module")
def bwd_runs():
    out = []
    for c in C.BWD_CASES:
        x, m = C.bwd_inputs(c), C.cpu_mask(c["M"], c["N"], c["drop"], 2)
        out.append((c, x, m, C.bwd_standin(x, m)))
    return out


@pytest.fixture(scope="module")
def attn_runs():
    out = []
    for c in C.ATTN_CASES:
        x, m = C.attn_inputs(c), _masks(c)
        out.append((c, x, m, C.attn_standin(c, x, m)))
    return out


def _upd(worst, new):
    for k, v in new.items():
        worst[k] = max(worst.get(k, 0.0), v)


def test_the_cases_are_the_edges_the_kernels_have():
    for cases, extra in ((C.FWD_CASES, ("bias", "save")), (C.BWD_CASES, ("res",))):
        lv = lambda n: {c[n] for c in cases}
        assert lv("N") == {64, 128, 512, 1024} and lv("M") == {1, 5, 63, 64, 65, 130, 448, 500, 512, 513}
        assert lv("K") == {8, 64, 72, 200, 264, 2048} and lv("layout") == {"contig", "win"} and lv("drop") == {0.0, 0.25}
        assert lv("gamma") == {"plain", "signed"} and all(lv(n) == {True, False} for n in extra)
        # every pair of levels appears: in particular every M with every N and every K
        assert {(c["M"], c["N"]) for c in cases} >= {(M, N) for M in lv("M") for N in lv("N")}
        assert {(c["M"], c["K"]) for c in cases} == {(M, K) for M in lv("M") for K in lv("K")}
    assert [C.sy_local(M) for M in (448, 500, 512, 513, 64, 130)] == [0, 1, 1, 0, 0, 0]
    assert C.sy_local(C.MEM_ROUTE_CASE["M"]) == 1
    lv = lambda n: {c[n] for c in C.ATTN_CASES}
    assert lv("nh") == {2, 8, 16} and lv("Lq") == {1, 13, 37, 64} and lv("Lk") >= {1, 37, 64, 65, 150, 256}
    assert lv("B") == {5, 8} and lv("G") == {1, 2} and lv("pro") == {0, 1, 3} and lv("mask") == {None, "ragged", "key0"}
    assert {(c["pro"], c["Kp"]) for c in C.ATTN_CASES} >= {(1, 64), (1, 192), (3, 64), (3, 192)}
    assert lv("causal") == {False, True} and lv("drop") == {0.0, 0.2} and lv("save") == {True, False}
    assert C.C_ATT == C_X["out"]


def test_the_new_keyword_of_ln_fwd_bound_leaves_the_old_bounds_bit_identical():
    c = C.FWD_CASES[0]
    x = C.fwd_inputs(c)
    y = (x["A"].float() @ x["B"].float()).to(C.BF)
    m = C.cpu_mask(c["M"], c["N"], 0.25, 9)
    old = P.ln_fwd_bound(x["R"], y, m, x["gamma"], x["beta"], C.EPS)
    mag = x["R"].double().abs() + (y.double() * m.double()).abs()
    new = P.ln_fwd_bound(x["R"], y, m, x["gamma"], x["beta"], C.EPS, e=2 * P.PER_TERM * mag)
    for k in old:
        assert torch.equal(old[k][0], new[k][0]) and torch.equal(old[k][1], new[k][1]), k
    wider = P.ln_fwd_bound(x["R"], y, m, x["gamma"], x["beta"], C.EPS, e=4 * P.PER_TERM * mag)
    assert bool((wider["out"][1] > old["out"][1]).all())


def test_forward_standin_is_inside_every_bound_on_every_case(fwd_runs):
    worst = {}
    for c, x, m, good in fwd_runs:
        _upd(worst, C.check_fwd(x, m, good, "stand-in " + C.case_id(c)))
    print("forward stand-in, worst |err| / bound:", {k: "%.3g" % v for k, v in worst.items()})
    assert set(worst) == {"s", "mean", "rstd", "y"} and max(worst.values()) <= 1.0


def test_backward_standin_is_inside_every_bound_on_every_case(bwd_runs):
    worst = {}
    for c, x, m, good in bwd_runs:
        _upd(worst, C.check_bwd(x, m, good, "stand-in " + C.case_id(c)))
    print("backward stand-in, worst |err| / bound:", {k: "%.3g" % v for k, v in worst.items()})
    assert set(worst) == {"ds", "dy", "part"} and max(worst.values()) <= 1.0


def test_attention_standin_is_inside_every_bound_on_every_case(attn_runs):
    worst = {}
    for c, x, m, good in attn_runs:
        _upd(worst, C.check_attn(c, x, good, m, "stand-in " + C.case_id(c)))
    print("attention stand-in, worst ratios:", {k: "%.3g" % v for k, v in worst.items()})
    assert set(worst) == {"q", "k", "v", "att", "lse", "s", "mean", "rstd", "y"}
    assert worst.pop("att") <= C.C_ATT and max(worst.values()) <= 1.0       # (the row check's constant is the existing one)


def _sweep(runs, defect, applies, plant, check):
    caught, missed = [], []
    for c, x, m, good in runs:
        if not applies(defect, c):
            continue
        try:
            check(c, x, m, plant(c, x, m))
            missed.append(C.case_id(c))
        except AssertionError:
            caught.append(C.case_id(c))
    print("%s: caught on %d cases, not on %s" % (defect, len(caught), missed))
    assert caught and missed == NOT_CAUGHT.get(defect, []), (defect, missed)


@pytest.mark.parametrize("defect", [d for d in C.FWD_DEFECTS if d != "row_M_processed"])
def test_each_planted_forward_defect_fails_on_every_case_it_applies_to(fwd_runs, defect):
    plant = lambda c, x, m: C.fwd_standin(x, m, c["save"], defect, other=C.fwd_inputs(c, 1),
                                          other_mask=C.cpu_mask(c["M"], c["N"], c["drop"], 5))
    _sweep(fwd_runs, defect, C.fwd_applies, plant, lambda c, x, m, bad: C.check_fwd(x, m, bad, defect))


@pytest.mark.parametrize("defect", [d for d in C.BWD_DEFECTS if d != "bwd_row_M_processed"])
def test_each_planted_backward_defect_fails_on_every_case_it_applies_to(bwd_runs, defect):
    _sweep(bwd_runs, defect, C.bwd_applies, lambda c, x, m: C.bwd_standin(x, m, defect),
           lambda c, x, m, bad: C.check_bwd(x, m, bad, defect))


def test_a_row_tile_that_reaches_into_the_next_sentence_fails(attn_runs):
    """attn_out_ln with Lq < 64: sentence 1's first row normalised with the statistics of sentence 0's last row."""
    _sweep(attn_runs, "next_sentence_row", lambda d, c: c["Lq"] < 64, lambda c, x, m: C.attn_standin(c, x, m, "next_sentence_row"),
           lambda c, x, m, bad: C.check_attn(c, x, bad, m, "next_sentence_row"))


def test_the_exact_check_of_s_is_what_catches_an_unrounded_product(fwd_runs):
    """bf16(R + p) is inside the derived bound of s (which allows the product half a bf16 ulp): only the exact statement
    -- s is bf16(R + mask c) for a bf16 c -- tells it from bf16(R + bf16(p))."""
    c, x, m, good = next(r for r in fwd_runs if r[0]["save"] and r[0]["M"] >= 63)
    bad = C.fwd_standin(x, m, True, "product_unrounded")
    bounds, ok = C.fwd_bounds(x, m, bad)
    P.check_all({"s": bad["s"]}, {"s": bounds["s"]}, "unrounded product, derived bound")       # passes
    assert int((~ok).sum()) > 0
    assert bool(C.fwd_bounds(x, m, good)[1].all())


def test_a_blocks_partial_in_another_blocks_place_fails(bwd_runs):
    n = 0
    for c, x, m, good in bwd_runs:
        if C.nblocks(c["M"]) < 2:
            continue
        n += 1
        bad = dict(good)
        bad["part"] = good["part"].clone()
        bad["part"][[0, 1]] = good["part"][[1, 0]]
        with pytest.raises(AssertionError):
            C.check_bwd(x, m, bad, "swapped blocks " + C.case_id(c))
        last = C.nblocks(c["M"]) - 1
        if last > 1:                                  # (the ragged last block in the first one's place)
            bad["part"] = good["part"].clone()
            bad["part"][[0, last]] = good["part"][[last, 0]]
            with pytest.raises(AssertionError):
                C.check_bwd(x, m, bad, "swapped blocks " + C.case_id(c))
    assert n >= 30


@pytest.mark.parametrize("kind", ["fwd", "bwd"])
def test_a_ragged_block_that_also_processes_row_M_fails(fwd_runs, bwd_runs, kind):
    """The outputs are windows of M + 1 rows whose last row is a sentinel: the values of the rows 0 .. M - 1 are the
    correct ones, only the buffer check can see the defect."""
    runs, applies, names = (fwd_runs, C.fwd_applies, ("y", "s")) if kind == "fwd" else (bwd_runs, C.bwd_applies, ("ds", "dy"))
    defect = "row_M_processed" if kind == "fwd" else "bwd_row_M_processed"
    n = 0
    for c, x, m, good in runs:
        if not applies(defect, c):
            continue
        bad = C.fwd_standin(x, m, c["save"], defect) if kind == "fwd" else C.bwd_standin(x, m, defect)
        for name in names:
            if bad.get(name) is None:
                continue
            n += 1
            M, N = bad[name].shape
            ok_buf, bad_buf = C.out_rows(M, N), C.out_rows(M, N)
            C.deposit(ok_buf, good[name])
            assert torch.equal(C.out_value(ok_buf, M, name), good[name])
            C.deposit(bad_buf, bad[name], bad["row_M"][name])
            with pytest.raises(AssertionError, match="row M"):
                C.out_value(bad_buf, M, name)
    assert n >= 30
