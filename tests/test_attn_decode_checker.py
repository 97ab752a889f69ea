"""The check of tests/test_gpu_attn_decode_elementwise.py has teeth (CPU only): the stand-in of tests/attn_decode_ref.py
(float32, another summation order, bf16 rounding of the probabilities and of the output) passes it on every run of every
case, and each planted defect fails it on the runs named here.

The constant.  The stand-in's worst row ratio over all runs is re-measured here; twice that (another summation order,
another exp) is not larger than C_X["out"] = 7.9e-3 of the training layout, so attn_decode_ref.C_OUT is that constant.
"""
import numpy as np
import pytest

from tests import attn_decode_ref as A
from tests.test_gpu_attention_elementwise import C_X

@pytest.fixture(scope="module")
def refs():
    """Inputs, float64 reference and stand-in of every run, computed once and left unchanged."""
    inputs = {name: A.case_inputs(name) for name in A.CASES}
    return [(name, r, inputs[name], A.case_reference(name, inputs[name], r)["out"], A.case_standin(name, inputs[name], r))
            for name, r in A.RUNS]


def test_the_cases_are_the_ones_the_decode_callers_make():
    cs = A.CASES
    assert cs["cross"]["G"] == 3 and cs["cross"]["B"] == 6 and cs["cross"]["Lk"] == 17 and cs["cross"]["lengths"] == (17, 6)
    assert [cs["cross_tiles_%d" % n]["lengths"] for n in (64, 65, 130, 256)] == [(64, 32), (65, 32), (130, 70), (256, 70)]
    assert cs["cross_long"]["Lk"] == 300 and cs["cross_one_sentence"]["G"] == 6 and cs["cross_flat"]["G"] == 1
    assert [(r["time"], r["pos"]) for r in cs["cross_rpr"]["runs"]] == [(0, "dev"), (3, "dev"), (16, "dev"), (40, "dev"), (3, "value")]
    assert 40 > cs["cross_rpr"]["Lk"] + A.MAX_REL
    for Tmax, times in ((24, (0, 1, 8, 23)), (130, (0, 63, 64, 129))):
        c = cs["self_cached_%d" % Tmax]
        assert c["nh"] * c["d"] == 192 and c["B"] == 5 and c["pos_flags"] == 3
        assert {(r["time"], r["rpr"], r["pos"]) for r in c["runs"]} == {(t, rp, p) for t in times for rp in (False, True)
                                                                          for p in ("dev", "value")}
    assert cs["small_head"]["nh"] == 4 and cs["small_head"]["d"] == 16
    bo = cs["block_offset"]
    assert (bo["B"], bo["Lq"], bo["Lk"], bo["q_pos0"]) == (2, 3, 9, 5) and [r["causal"] for r in bo["runs"]] == [False, True]


def test_masked_keys_score_highest_and_sentences_differ():
    """The inputs that make the mask and the sentence index matter."""
    x = A.case_inputs("cross")
    cs = A.CASES["cross"]
    q, k, v = (x[n].double().numpy() for n in ("q", "k", "v"))
    s = np.einsum("bhd,jhd->bhj", q[3:, 0].reshape(3, cs["nh"], cs["d"]), k[1].reshape(-1, cs["nh"], cs["d"])) * cs["d"] ** -0.5
    assert s[..., 6:].min() > s[..., :6].max() and s[..., 6:].min() > 2.0
    assert np.linalg.norm(v[0].mean(0) - v[1].mean(0)) > 0.5 * np.linalg.norm(v[0].mean(0))


def test_standin_is_inside_the_constant_on_every_run(refs):
    worst, at = 0.0, None
    for name, r, x, ref, good in refs:
        ratio = A.check(name, good, ref, "stand-in %s %s" % (name, A.run_id(r)))
        if ratio > worst:
            worst, at = ratio, (name, A.run_id(r))
    print("stand-in: worst row ratio %.3e at %s; C_OUT %.3e" % (worst, at, A.C_OUT))
    # the constant is at least TWICE the stand-in's worst ratio (measured: STANDIN_WORST; another BLAS may move a rounding)
    assert worst <= A.C_OUT / 2, (worst, at)
    assert abs(worst - A.STANDIN_WORST) <= 0.1 * A.STANDIN_WORST, (worst, at)
    assert 2 * A.STANDIN_WORST <= C_X["out"] and A.C_OUT == C_X["out"]


def test_reference_equals_parity_attn_math_where_the_two_overlap():
    """The float64 reference against an independent statement in torch (parity.attn_math) where the two overlap: one
    sentence per query row, no device position -- cross_flat."""
    import torch
    from tests import parity as PR
    x = A.case_inputs("cross_flat")
    cs = A.CASES["cross_flat"]
    B, nh, d, Lk = cs["B"], cs["nh"], cs["d"], cs["Lk"]
    H = nh * d
    ref = A.reference("cross_flat", x)
    other = PR.attn_math(x["q"].reshape(B, H), x["k"].reshape(B * Lk, H), x["v"].reshape(B * Lk, H), torch.zeros(B, H), B, nh,
                         1, Lk, d, kmask=x["kmask"])
    assert np.abs(ref["out"].reshape(B, H) - other["out"].numpy()).max() < 1e-12
    assert np.abs(ref["lse"].reshape(B, nh, 1) - other["lse"].numpy()).max() < 1e-9


def test_a_row_with_one_visible_key_is_that_keys_value_vector(refs):
    n = 0
    for name, r, x, ref, good in refs:
        want = A.single_key_rows(name, x, r)
        if want is None:
            continue
        n += 1
        assert np.abs(ref - want).max() < 1e-12, (name, r)
        A.check_single_key(good, want, "%s %s" % (name, A.run_id(r)))
        if not r["rpr"]:
            assert (good == want).all()                # a probability of exactly 1 times a bf16 value
        bad = good.copy()
        bad[2, 0, 70] *= 1 + 2.0 ** -6                 # two bf16 ulp
        with pytest.raises(AssertionError):
            A.check_single_key(bad, want, "planted")
    assert n == 8                                      # position 0 of both caches, with and without tables, both forms


# defect -> the runs that must catch it (measured; the test asserts them) .  Where a defect applies but is NOT listed the
# reason is in the comment.
CAUGHT_ON = {
    "neighbour_keys": [("cross", ""), ("cross_tiles_130", ""), ("cross_rpr", "t3-rpr-dev"), ("small_head", "")],
    "mask_row_of_b": [("cross", ""), ("cross_tiles_65", ""), ("cross_long", "")],
    "mask_ignored": [("cross", ""), ("cross_one_sentence", ""), ("cross_flat", ""), ("cross_tiles_256", ""),
                     ("block_offset", "-rpr")],
    # position 129 of 130 and 23 of 24 have no slot behind them; 65 keys against 64 still shows
    "one_key_more": [("self_cached_24", "t0-dev"), ("self_cached_24", "t8-rpr-dev"), ("self_cached_130", "t64-dev"),
                     ("self_cached_130", "t0-rpr-value")],
    # not where the last key is masked anyway (cross_one_sentence) or above the causal diagonal (block_offset, causal)
    "one_key_less": [("self_cached_24", "t1-dev"), ("self_cached_24", "t23-value"), ("self_cached_130", "t64-rpr-dev"),
                     ("cross", ""), ("cross_long", "")],
    # position 40 (+ 7) is in the clipped tail for every key either way: only the positions 0, 3, 16 can show it
    "position_by_value": [("cross_rpr", "t0-rpr-dev"), ("cross_rpr", "t3-rpr-dev"), ("cross_rpr", "t16-rpr-dev"),
                          ("self_cached_24", "t1-rpr-dev"), ("self_cached_130", "t64-rpr-dev")],
    "rpr_sign": [("cross_rpr", "t3-rpr-dev"), ("cross_rpr", "t3-rpr-value"), ("self_cached_24", "t8-rpr-dev"),
                 ("block_offset", "-rpr"), ("block_offset", "-rpr-causal")],
    # row 0's sentence starts at 0 under any stride: the rows 1 .. 4 show it
    "batch_stride_default": [("self_cached_24", "t0-value"), ("self_cached_24", "t8-rpr-value"), ("self_cached_130", "t63-value")],
    "dead_row_leak": [("cross", ""), ("self_cached_24", "t8-dev"), ("block_offset", "-rpr-causal")],
    "stale_chunk": [("cross", ""), ("small_head", ""), ("self_cached_130", "t129-rpr-dev"), ("block_offset", "-rpr")],
}


@pytest.mark.parametrize("defect", A.DEFECTS)
def test_each_planted_defect_fails_the_check(refs, defect):
    caught, missed = [], []
    for name, r, x, ref, good in refs:
        if not A.applies(defect, name, r):
            continue
        bad = A.case_standin(name, x, r, defect)
        try:
            A.check(name, bad, ref, defect)
            missed.append((name, A.run_id(r)))
        except AssertionError:
            caught.append((name, A.run_id(r)))
    print("%s: caught on %d runs, not on %s" % (defect, len(caught), missed))
    for at in CAUGHT_ON[defect]:
        assert at in caught, (defect, at, caught)


def test_position_beyond_the_clip_hides_a_wrong_position():
    """Why position 40 alone would not do: every key is in the clipped tail for 40 and for 40 + 7."""
    x = A.case_inputs("cross_rpr")
    r = A.run(40, True, "dev")
    assert (A.case_standin("cross_rpr", x, r, "position_by_value") == A.case_standin("cross_rpr", x, r)).all()
