"""The references, bounds and the checker of tests/beam_ref.py have teeth (CPU only).  Over the case tables that
tests/test_gpu_beam_elementwise.py runs on the device:

  * the clean stand-ins (beam_ref.topk_standin in the form the host picks, beam_ref.book_standin) pass every case;
  * each planted defect fails at least one case;
  * the conditions that keep the checks from being vacuous hold FROM THE REFERENCE ALONE: at least 0.9 of the sentences
    of every random case are decisive, at most 0.5 % of the Gumbel elements have a bound above 1e-3.
"""
import functools

import numpy as np
import pytest
import torch

from tests import beam_ref as R
from tests import parity as P

DECISIVE_FLOOR = R.DECISIVE_FLOOR
SIGMAS = 5.0                     # the sampling conditions below: five standard deviations of the sample statistic


@functools.lru_cache(maxsize=None)
def _shape_inputs(i):
    return R.topk_inputs(R.TOPK_SHAPES[i])


def _run_shape(i, defect=None):
    """Every variant of shape i through the stand-in and the checker -> (smallest decisive share, largest c_exp needed)."""
    s = R.TOPK_SHAPES[i]
    z, prev = _shape_inputs(i)
    share, need = 1.0, 0.0
    for temp, pen, forbid, dev in R.topk_variants(s):
        ref, bound, fixed, shape = R.topk_ref(z, prev, s["K"], s["V"], R.inv_temp_of(temp), pen, forbid, R.FORBID_VALUE,
                                              terms=True)
        args = (99.0, -1, R.scal_words(pen, forbid)) if dev else (pen, forbid, None)      # scal_dev: decoys in the arguments
        gs, gi = R.topk_standin(z, prev, s["B"], s["K"], s["V"], s["ld"], s["k2"], temp, args[0], args[1], R.FORBID_VALUE,
                                scal=args[2], defect=defect)
        what = "%s %s T=%g forbid=%d dev=%d" % (defect or "stand-in", s["note"], temp, forbid, dev)
        share = min(share, R.assert_topk(gs, gi, ref, bound, s["K"], s["V"], what))
        need = max(need, R.topk_c_exp_needed(gs, gi, ref, fixed, shape))
        if s["kind"] == "step0":
            assert (gi // s["V"] == 0).all(), what + ": a survivor of step 0 outside beam 0"
    return share, need


@pytest.mark.parametrize("i", range(len(R.TOPK_SHAPES)), ids=lambda i: R.TOPK_SHAPES[i]["note"])
def test_topk_standin_passes_and_the_case_is_decisive(i):
    share, need = _run_shape(i)
    print("%s: decisive share %.2f, c_exp needed %.3g of %g" % (R.TOPK_SHAPES[i]["note"], share, need, P.C_EXP))
    assert share >= DECISIVE_FLOOR and need <= P.C_EXP


def test_topk_shapes_reach_every_path():
    path = lambda s: R.topk_path(s["K"], s["V"], s["k2"])
    assert {path(s) for s in R.TOPK_SHAPES} == {"rows", "nv4", "nv8"}
    by = {(s["K"], s["V"], s["k2"]): s for s in R.TOPK_SHAPES}
    assert R.topk_chunks(16, 8189, 16) == 1 and R.topk_chunk(8189, 1) == R.TOPK_CHUNK_MAX and R.topk_chunks(16, 8190, 16) == 0
    assert R.topk_chunks(8, 16378, 16) == 2 and R.topk_chunk(16378, 2) == R.TOPK_CHUNK_MAX and R.topk_chunks(8, 16379, 16) == 0
    assert all(k in by for k in ((16, 8189, 16), (16, 8190, 16), (8, 16378, 16), (8, 16379, 16)))
    assert any(s["ld"] % 4 for s in R.TOPK_SHAPES) and any(s["off"] % 4 for s in R.TOPK_SHAPES)
    # the chunked layout uses every byte of the workspace at nc = 8
    assert R.topk_chunks(4, 1000, 8) == 8 and 3 * 4 * 8 * (2 + 2 * 8) * 4 == R.topk_workspace(3, 4, 8)
    for K, V, ld, k2 in R.EXACT_SHAPES:
        nc = R.topk_chunks(K, V, k2)
        pairs = R.exact_pairs(V, R.topk_chunk(V, nc) if nc else V)
        assert (8, 9) in pairs and (8, 1032) in pairs and (1023, 1024) in pairs and (0, V - 1) in pairs
        assert nc == 0 or any(c2 == R.topk_chunk(V, nc) for _, c2 in pairs)
    assert {R.topk_path(K, V, k2) for K, V, ld, k2 in R.EXACT_SHAPES} == {"rows", "nv4", "nv8"}
    # the fused entry has no row fallback: its cases are chunked, in both widths, with K = 1, 4, 8 and unaligned rows
    assert {R.topk_path(K, V, 2 * K) for K, V, ld, off, t in R.FUSED_CASES} == {"nv4", "nv8"}
    assert {K for K, V, ld, off, t in R.FUSED_CASES} == {1, 4, 8} and any(ld % 4 or off % 4 for K, V, ld, off, t in R.FUSED_CASES)


def _exact(K, V, ld, k2, family, defect=None):
    c = R.topk_exact_case(K, V, k2, family)
    gs, gi = R.topk_standin(c["logits"], c["prev"], c["B"], K, V, ld, k2, 1.0, c["penalty"], c["forbid"], R.FORBID_VALUE,
                            defect=defect)
    what = "%s exact %s K=%d V=%d" % (defect or "stand-in", family, K, V)
    P.assert_exact(torch.from_numpy(gi), torch.from_numpy(c["expect"]), what)
    ref, bound = R.topk_ref(c["logits"], c["prev"], K, V, R.inv_temp_of(1.0), c["penalty"], c["forbid"], R.FORBID_VALUE)
    R.assert_topk(gs, gi, ref, bound, K, V, what)


@pytest.mark.parametrize("family", R.EXACT_FAMILIES)
@pytest.mark.parametrize("K,V,ld,k2", R.EXACT_SHAPES)
def test_topk_standin_gives_the_exact_order(K, V, ld, k2, family):
    _exact(K, V, ld, k2, family)


def _topk_defect_runs(defect):
    """(label, thunk) per case a defect is tried on: the random shapes (the small ones), then the exact families."""
    runs = [(s["note"], functools.partial(_run_shape, i, defect)) for i, s in enumerate(R.TOPK_SHAPES) if s["V"] <= 1100]
    for K, V, ld, k2 in R.EXACT_SHAPES[:1] + R.EXACT_SHAPES[3:]:
        runs += [("exact %s V=%d ld=%d" % (family, V, ld), functools.partial(_exact, K, V, ld, k2, family, defect))
                 for family in R.EXACT_FAMILIES]
    return runs


def _fails(thunk):
    try:
        thunk()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("defect", R.TOPK_DEFECTS)
def test_each_planted_topk_defect_fails(defect):
    failed = [(label, thunk) for label, thunk in _topk_defect_runs(defect) if _fails(thunk)]
    print("top-k defect %s fails at %d case(s): %s" % (defect, len(failed), [f[0] for f in failed]))
    assert failed, defect
    with pytest.raises(AssertionError):
        failed[0][1]()


# ---------------------------------------------------------------------------------------------- bookkeeping
def _book_run(scenario, B, K, defect=None, extra=2):
    """Steps of prepare + advance through the stand-in, each against book_ref, until the stop and `extra` replays past it
    (which must change nothing).  -> (steps taken, the cause of the stop)."""
    cfg, finish_at = R.book_scenario(scenario, B, K)
    d = R.dev_init(cfg)
    cause, past = None, 0
    for step in range(cfg["Tcap"] + extra + 1):
        want, c = R.dev_prepare_expected(d, cfg)
        got = R.book_standin(d, cfg, "prepare", defect)
        R.assert_book_equal(got, want, "%s %s step %d prepare" % (defect or "stand-in", scenario, step))
        cause = cause or c
        time = int(want["ctrl"][0]) - 1
        want["topk_scores"], want["topk_idx"] = R.book_survivors(cfg, max(time, 0), seed=K, finish_at=finish_at)
        got["topk_scores"], got["topk_idx"] = want["topk_scores"], want["topk_idx"]
        exp = R.dev_advance_expected(want, cfg)
        d = R.book_standin(got, cfg, "advance", defect)
        R.assert_book_equal(d, exp, "%s %s step %d advance" % (defect or "stand-in", scenario, step))
        if not want["ctrl"][1]:
            n = time + 2
            assert (d["seq"][:, :, n:] == R.SENTINEL).all() and (d["fin_seq"][:, :, n:] == R.SENTINEL).all()
        else:
            past += 1
            if past > extra:
                break
    return int(d["ctrl"][0]), cause


@pytest.mark.parametrize("K", R.BOOK_K)
def test_book_standin_matches_book_ref(K):
    causes = set()
    for scenario in R.BOOK_SCENARIOS:
        for B in R.BOOK_B:
            steps, cause = _book_run(scenario, B, K)
            causes.add(cause)
            assert steps >= 1
    assert causes == {"length", "bound"}, causes          # both causes of the stop are in the table


@pytest.mark.parametrize("scenario", list(R.BOOK_SCENARIOS))
def test_book_scenarios_stop_for_their_cause(scenario):
    """From the reference alone, for every K and B of the device test: the scenario runs at least two steps and stops for
    the cause it is named after."""
    for K in R.BOOK_K:
        for B in R.BOOK_B:
            cfg, finish_at = R.book_scenario(scenario, B, K)
            d = R.dev_init(cfg)
            for step in range(cfg["Tcap"] + 1):
                d, cause = R.dev_prepare_expected(d, cfg)
                if cause is not None:
                    break
                d["topk_scores"], d["topk_idx"] = R.book_survivors(cfg, step, seed=K, finish_at=finish_at)
                d = R.dev_advance_expected(d, cfg)
            # (five sentences under the length caps can all be bounded one step before the last cap: either cause is a stop)
            assert step >= 2 and (cause == scenario or (scenario == "length" and B == 5 and cause == "bound")), (K, B, cause)


def test_book_standin_overflow_branch():
    cfg = R.book_cfg(2, 3, R.BOOK_V, 3, [9, 9])
    d = R.dev_init(cfg)
    d["ctrl"][0] = cfg["Tmax"]
    want, cause = R.dev_prepare_expected(d, cfg)
    assert cause == "overflow" and list(want["ctrl"][:3]) == [3, 1, 1]
    R.assert_book_equal(R.book_standin(d, cfg, "prepare"), want, "overflow")


@pytest.mark.parametrize("defect", R.BOOK_DEFECTS)
def test_each_planted_book_defect_fails(defect):
    failed = []
    for scenario in R.BOOK_SCENARIOS:
        for K in (3, 5):
            try:
                _book_run(scenario, 5, K, defect)
            except AssertionError as e:
                failed.append((scenario, K, str(e)[:120]))
    print("bookkeeping defect %s fails at %s" % (defect, failed))
    assert failed, defect
    with pytest.raises(AssertionError):
        _book_run(failed[0][0], 5, failed[0][1], defect)


# ---------------------------------------------------------------------------------------------- Gumbel noise
def test_rand_u32_ref_high_words():
    idx = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 5 * 2 ** 32 + 7], dtype=np.uint64)
    a = R.rand_u32_ref(5, 1, idx)
    assert a.dtype == np.uint32 and len(set(a.tolist())) == len(idx)
    assert a[1] != a[4]                                   # the high index word enters
    assert not np.array_equal(a, R.rand_u32_ref(5 + (1 << 32), 1, idx))      # and so does the high seed word
    assert not np.array_equal(a, R.rand_u32_ref(5, 2, idx))
    # the generator is uniform enough for the cap below to be a statement about the function, not the seed
    # (a uniform variable has variance 1 / 12 and fourth central moment 1 / 80)
    n = 1 << 16
    w = R.rand_u32_ref(11, 7001, np.arange(n, dtype=np.uint64)).astype(np.float64) * 2.0 ** -32
    assert abs(w.mean() - 0.5) < SIGMAS * (1 / 12.0 / n) ** 0.5
    assert abs(w.var() - 1 / 12.0) < SIGMAS * ((1 / 80.0 - 1 / 144.0) / n) ** 0.5


@pytest.mark.parametrize("case", R.GUMBEL_CASES, ids=lambda c: "%dx%d" % c[:2])
def test_gumbel_wide_bound_cap_holds_from_the_reference(case):
    ref, bound = R.gumbel_case_ref(case)
    share = R.gumbel_wide_share(bound)
    print("gumbel %r: %.4f %% of %d elements have a bound above %g; mean %.4f" %
          (case, 100 * share, ref.size, R.GUMBEL_CAP_BOUND, ref.mean()))
    assert np.isfinite(ref).all() and np.isfinite(bound).all() and share <= R.GUMBEL_CAP_SHARE
    if ref.size > 2 ** 21:
        # util.py:189-195: -log(-log(u)) has mean = Euler's gamma, variance pi^2 / 6 and excess kurtosis 12 / 5
        var = np.pi ** 2 / 6
        assert abs(ref.mean() - np.euler_gamma) < SIGMAS * (var / ref.size) ** 0.5
        assert abs(ref.var() - var) < SIGMAS * ((3 + 12 / 5.0 - 1) * var ** 2 / ref.size) ** 0.5
        # uniformly drawn 32-bit words in place of the generator: the same share (the conditioning of the function)
        rng = np.random.default_rng(0)
        _, b2 = R.gumbel_ref(rng.integers(0, 2 ** 32, ref.size, dtype=np.uint64).astype(np.uint32), R.GUMBEL_EPS)
        print("uniform words: %.4f %%" % (100 * R.gumbel_wide_share(b2)))
        assert R.gumbel_wide_share(b2) <= R.GUMBEL_CAP_SHARE


def test_gumbel_fp32_standin_is_inside_the_bound_and_a_wrong_counter_is_not():
    rows, V, ld, seed, sid = R.GUMBEL_CASES[0]
    ref, bound = R.gumbel_case_ref(R.GUMBEL_CASES[0])

    def noise(index):
        u = (R.rand_u32_ref(seed, sid, index).astype(np.float32) * np.float32(2.0 ** -32)).astype(np.float32)
        e = np.float32(R.GUMBEL_EPS)
        return -np.log(-np.log(u + e, dtype=np.float32) + e, dtype=np.float32)
    r, c = np.divmod(np.arange(rows * V, dtype=np.uint64), np.uint64(V))
    P.assert_elementwise(torch.from_numpy(noise(r * np.uint64(V) + c).reshape(rows, V)), torch.from_numpy(ref),
                         torch.from_numpy(bound), "gumbel stand-in")
    with pytest.raises(AssertionError):                   # the counter formed with ld instead of V
        P.assert_elementwise(torch.from_numpy(noise(r * np.uint64(ld) + c).reshape(rows, V)), torch.from_numpy(ref),
                             torch.from_numpy(bound), "gumbel counter r * ld + c")
