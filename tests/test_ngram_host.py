"""no_repeat_ngram_size on the CPU: the HParam, what is refused, the rule of tests/ngram_ref.py against an independent
restatement, the planted defects, and what the reference's search shows under the ban on the tiny fixtures of the GPU tests."""
import numpy as np
import pytest

from tests import ngram_ref as N
from tests.common import make_hp
from zero_amd.config import default_params


# ---------------------------------------------------------------------------------------------- the HParam
def test_hparam_default_and_parse():
    hp = default_params()
    assert hp.no_repeat_ngram_size == 0
    hp.parse("no_repeat_ngram_size=3,beam_size=2")
    assert hp.no_repeat_ngram_size == 3 and isinstance(hp.no_repeat_ngram_size, int)


@pytest.mark.parametrize("n", [-1, 17, 100])
@pytest.mark.parametrize("model", ["transformer", "rnnsearch"])
def test_n_outside_the_range_is_refused_before_any_device_work(model, n):
    from zero_amd.models import model as registry, load_all
    load_all()
    hp = make_hp(model, search_mode="cache", no_repeat_ngram_size=n)
    with pytest.raises(ValueError, match=r"no_repeat_ngram_size=%d.*1 \.\. 16" % n):
        registry.get_model(model).infer_fn(hp)


@pytest.mark.parametrize("n", [0, 1, 16])
def test_n_inside_the_range_is_taken(n):
    from zero_amd.models import _decode
    assert _decode.ngram_size(make_hp("transformer", no_repeat_ngram_size=n)) == n
    bare = make_hp("transformer")
    bare.del_hparam("no_repeat_ngram_size")
    assert _decode.ngram_size(bare) == 0


def test_too_few_candidates_are_refused_by_name():
    """V_eff - Tmax < 2 K: the message names the three sizes; one candidate more and the check passes; off: never."""
    from zero_amd.models import _decode
    hp = make_hp("transformer", no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match=r"no_repeat_ngram_size=2: up to 24 tokens .* 2 \* beam_size = 8 of the 31 candidates"):
        _decode.check_ngram(hp, 31, 24, 4)
    _decode.check_ngram(hp, 32, 24, 4)
    hp.no_repeat_ngram_size = 0
    _decode.check_ngram(hp, 5, 24, 4)


# ---------------------------------------------------------------------------------------------- the rule
def _banned_sets(hist, t, n):
    """The rule once more, with Python sets of tuples: every n-gram of y_1 .. y_t, looked up by its first n - 1 tokens."""
    y = [int(v) for v in hist[1:t + 1]]
    if t < n - 1:
        return set()
    grams = {tuple(y[i:i + n]) for i in range(len(y) - n + 1)}
    suffix = tuple(y[len(y) - (n - 1):]) if n > 1 else ()
    return {g[-1] for g in grams if g[:-1] == suffix}


@pytest.mark.parametrize("symbols", [2, 3, 5000])
def test_rule_against_sets_of_tuples(symbols):
    """Random histories over 2 and 3 symbols (matches everywhere) and over 5000 (hardly any), every n, every t."""
    rng = np.random.default_rng(symbols)
    hits = 0
    for trial in range(6):
        hist = rng.integers(3, 3 + symbols, 70)
        for n in range(1, N.NMAX + 1):
            for t in list(range(0, 40)) + [63, 64, 65, 69]:
                got = N.banned(hist, t, n)
                want = _banned_sets(hist, t, n)
                assert set(got.tolist()) == want and len(got) == len(want), (trial, n, t)
                assert list(got) == sorted(got)
                hits += len(want) > 0 and n >= 2
    assert (hits > 500) if symbols <= 3 else (hits < 20)


def test_rule_by_hand():
    hist = np.array([0, 5, 6, 7, 5, 6, 8, 5, 6, 9])
    assert list(N.banned(hist, 8, 3)) == [7, 8]
    assert list(N.banned(hist, 8, 1)) == [5, 6, 7, 8]
    assert list(N.banned(hist, 2, 3)) == [] and list(N.banned(hist, 1, 3)) == [] and list(N.banned(hist, 0, 1)) == []
    assert list(N.banned(hist, 5, 3)) == [7]                 # y = 5 6 7 5 6: the first possible ban of this row
    logits = np.zeros((1, 12))
    out = N.apply(logits, 8, hist[None], 8, 3, -N.INF)       # V = 8: token 8 is outside and skipped
    assert (out[0] == [0] * 7 + [-N.INF] + [0] * 4).all()


@pytest.mark.parametrize("defect", [d for d in N.DEFECTS if d != "after_norm"])
def test_planted_defects_change_the_banned_set(defect):
    hist, t, n = N.CASES[defect]
    good, bad = N.banned_rows(hist, t, n), N.banned_rows(hist, t, n, defect)
    assert any(list(a) != list(b) for a, b in zip(good, bad)), (good, bad)
    # and the right rule on that case is the one the independent restatement gives
    assert [set(g.tolist()) for g in good] == [_banned_sets(h, t, n) for h in hist]


def test_ban_after_the_normalisation_gives_other_scores():
    hist, t, n = N.CASES["after_norm"]
    rng = np.random.default_rng(1)
    logits = rng.normal(size=(hist.shape[0], 12)) * 3.0
    good, bad = N.step_logprobs(logits, hist, t, n), N.step_logprobs(logits, hist, t, n, "after_norm")
    row = 0
    banned = N.banned(hist[row], t, n)
    keep = np.setdiff1d(np.arange(12), banned)
    assert len(banned) == 2
    assert np.allclose(np.exp(good[row, keep]).sum(), 1.0, atol=1e-12)           # renormalised over what is left
    assert np.exp(bad[row, keep]).sum() < 1.0 - 1e-6
    assert np.abs(good[row, keep] - bad[row, keep]).min() > 1e-6                 # every surviving score differs
    assert (good[row, banned] < -0.9 * N.INF).all() and np.isfinite(good).all()  # finite everywhere: zk_beam_topk's precondition
    assert np.array_equal(good[1], bad[1])                                       # (a row without a ban is the plain log-softmax)


# ---------------------------------------------------------------------------------------------- the reference's search
@pytest.mark.parametrize("model", sorted(N.MODELS))
def test_reference_search_with_the_ban(model):
    """make_fixture's own assertions (float64 and fp32 token- and order-identical, gap > 4 err, the bf16 storage model keeps
    the sharpened best hypotheses, no constrained hypothesis repeats, at least one unconstrained best hypothesis does), and the
    fp32 reference within a quarter of the project's fp32 score tolerance, which the GPU tests then use."""
    f = N.make_fixture(model)
    for n in N.NS:
        print("%s n=%d: gap %.2e err %.1e (x %.1f) rel %.3f repeats %d of %d"
              % (model, n, f[n]["gap"], f[n]["err"], f[n]["gap"] / f[n]["err"], f[n]["rel"], f[n]["repeats"], f["src"].shape[0]))
        assert f[n]["gap"] > 4.0 * f[n]["err"] and f[n]["rel"] <= 0.25 and f[n]["repeats"] >= 1
        assert N.score_tol(f[n]["rel"], f[n]["err"]) == (N.RTOL, N.ATOL)
