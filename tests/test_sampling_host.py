"""sampling_topk / sampling_topp on the CPU: the HParams, what is refused, the graph key, the rule of tests/sampling_ref.py by
hand, the checker against planted defects, the undecided share of the GPU kernel test's inputs, and what the reference's search
shows under the truncation on the tiny fixtures of the GPU model test."""
import numpy as np
import pytest

from tests import sampling_ref as S
from tests.common import make_hp
from zero_amd.config import default_params
from zero_amd.models import _decode


# ---------------------------------------------------------------------------------------------- the HParams
def test_hparam_defaults_and_parse():
    hp = default_params()
    assert hp.sampling_topk == 0 and hp.sampling_topp == 0.0
    hp.parse("sampling_topk=10,sampling_topp=0.9,beam_size=1")
    assert hp.sampling_topk == 10 and isinstance(hp.sampling_topk, int)
    assert hp.sampling_topp == 0.9 and isinstance(hp.sampling_topp, float)
    assert _decode.sampling_opts(hp) == (10, 0.9)


@pytest.mark.parametrize("kw, text", [
    (dict(sampling_topk=-1), r"sampling_topk=-1"), (dict(sampling_topk=-100), r"sampling_topk=-100"),
    (dict(sampling_topp=-0.1), r"sampling_topp=-0\.1"), (dict(sampling_topp=1.0001), r"sampling_topp=1\.0001"),
    (dict(sampling_topp=float("nan")), r"sampling_topp=nan")])
@pytest.mark.parametrize("model", ["transformer", "rnnsearch"])
def test_settings_outside_the_range_are_refused_before_any_device_work(model, kw, text):
    from zero_amd.models import model as registry, load_all
    load_all()
    hp = make_hp(model, search_mode="cache", **kw)
    with pytest.raises(ValueError, match=text):
        registry.get_model(model).infer_fn(hp)


@pytest.mark.parametrize("k, p, on", [(0, 0.0, False), (1, 0.0, True), (0, 1.0, True), (0, 1e-6, True), (32000, 0.5, True)])
def test_settings_inside_the_range_are_taken(k, p, on):
    hp = make_hp("transformer", sampling_topk=k, sampling_topp=p)
    assert _decode.sampling_opts(hp) == (k, p) and _decode.sampling_on(_decode.sampling_opts(hp)) == on
    bare = make_hp("transformer")
    bare.del_hparam("sampling_topk")
    bare.del_hparam("sampling_topp")
    assert _decode.sampling_opts(bare) == (0, 0.0) and not _decode.sampling_on(_decode.sampling_opts(bare))
    assert not _decode.sampling_on(None)


def test_too_few_candidates_are_refused_by_name():
    """V_eff < min_keep = 2 K + 1, and with the n-gram ban V_eff - Tmax < min_keep: the messages name the sizes; one candidate
    more and the check passes; off: never."""
    hp = make_hp("transformer", sampling_topk=3)
    with pytest.raises(ValueError, match=r"sampling_topk=3, sampling_topp=0: .* 2 \* beam_size \+ 1 = 9 candidates .* only 8"):
        _decode.check_sampling(hp, 8, 24, 4)
    _decode.check_sampling(hp, 9, 24, 4)
    hp.no_repeat_ngram_size = 2
    with pytest.raises(ValueError, match=r"sampling_topk=3.*no_repeat_ngram_size=2: up to 24 tokens .* 2 \* beam_size \+ 1 = 9 "
                                         r"of the 32 candidates"):
        _decode.check_sampling(hp, 32, 24, 4)
    _decode.check_sampling(hp, 33, 24, 4)
    hp.sampling_topk = 0
    _decode.check_sampling(hp, 2, 24, 4)
    assert _decode.sampling_min_keep(4) == 9 == S.min_keep_of(4)


def test_graph_key():
    """Off: the key of a step is the tuple it was before the option existed.  On: one more entry holding k and the bits of p,
    so that no two settings share a key."""
    state = {"B": 4, "K": 4, "Ls": 16, "Tmax": 24, "f32": True}
    args = (state, None, 1.0, 1e8, False, 0)
    before = (4, 4, 16, 24, False, 1.0, 1e8, False, 0, True)
    assert _decode.graph_key(*args) == before
    assert _decode.graph_key(*args, 0, None) == before and _decode.graph_key(*args, 0, (0, 0.0)) == before
    assert _decode.graph_key(*args, 3, (0, 0.0)) == before + (("ngram", 3),)
    keys = {s: _decode.graph_key(*args, 0, s) for s in [(10, 0.0), (9, 0.0), (0, 0.9), (0, 1.0), (10, 0.9), (0, 0.9000001)]}
    assert len(set(keys.values())) == len(keys) and before not in keys.values()
    assert keys[(0, 1.0)] == before + (("sample", 0, 0x3f800000),)
    assert _decode.graph_key(*args, 3, (10, 0.9)) == before + (("ngram", 3), ("sample", 10, 0x3f666666))


# ---------------------------------------------------------------------------------------------- the rule
def test_rule_by_hand():
    x = np.array([2.0, 5.0, 5.0, 1.0, 0.0, -1e8])
    c, M, s = S.rank_mass(x)
    assert list(c) == [2, 0, 0, 3, 4, 5]
    e = np.exp(x - 5.0)
    assert np.allclose(M, [2 * e[1] / e.sum(), 0, 0, (2 * e[1] + e[0]) / e.sum(), 1 - e[4] / e.sum(), 1.0], atol=1e-15)
    assert list(S.kept(x, 1, 0.0, 1)) == [False, True, True, False, False, False]          # tied tokens share their fate
    assert list(S.kept(x, 3, 0.0, 1)) == [True, True, True, False, False, False]
    assert list(S.kept(x, 0, 0.9, 1)) == [False, True, True, False, False, False]          # the two fives hold 0.964
    assert list(S.kept(x, 0, 0.97, 1)) == [True, True, True, False, False, False]
    assert list(S.kept(x, 1, 0.5, 4)) == [True, True, True, True, False, False]            # min_keep wins
    assert S.kept(x, 0, 1.0, 1).all() and S.kept(x, 6, 0.0, 1).all()
    assert list(S.kept(x, 5, 0.0, 1)) == [True] * 5 + [False]                              # a banned entry has the lowest rank
    out = S.apply(np.concatenate([x, [7.0, 7.0]])[None].astype(np.float32), 6, 1, 0.0, 1)
    assert list(out[0]) == [-1e8, 5, 5, -1e8, -1e8, -1e8, 7, 7]                            # the columns behind V are not touched


def test_rank_mass_against_a_loop():
    rng = np.random.default_rng(0)
    x = rng.integers(-4, 5, (6, 40)).astype(np.float64) * 0.5
    c, M, s = S.rank_mass(x)
    for r in range(x.shape[0]):
        sm = np.exp(x[r]) / np.exp(x[r]).sum()
        for v in range(x.shape[1]):
            above = x[r] > x[r, v]
            assert c[r, v] == above.sum() and abs(M[r, v] - sm[above].sum()) < 1e-14 and abs(s[r, v] - sm[v]) < 1e-15


# ---------------------------------------------------------------------------------------------- the checker
def _window(x, kept_mask, ld=None):
    """before / after fp32 [1, ld] of one row x with the tokens outside kept_mask overwritten."""
    ld = x.size + 2 if ld is None else ld
    before = np.full((1, ld), 3.25, np.float32)
    before[0, :x.size] = x
    after = before.copy()
    after[0, :x.size][~kept_mask] = -S.INF
    return before, after


@pytest.mark.parametrize("defect", S.DEFECTS)
def test_the_checker_rejects_a_defect_of_the_rule(defect):
    """k off by one, a tie split, <= for < on the mass, min_keep ignored: each on the case named for it, exact (delta = 0)."""
    x, topk, topp, mk = S.CASES[defect]
    band = S.Band(x, delta=0.0)
    good, bad = S.kept(x, topk, topp, mk), S.kept(x, topk, topp, mk, defect)
    assert not np.array_equal(good, bad)
    S.check(*_window(x, good), x.size, topk, topp, mk, band=band)
    with pytest.raises(AssertionError):
        S.check(*_window(x, bad), x.size, topk, topp, mk, band=band)


def test_the_checker_rejects_the_mass_after_the_temperature():
    """temperature 2 flattens the geometric row: s = 0.29, 0.21, ..; its nucleus of 0.7 holds four tokens, the rule's two."""
    x = S.CASES["mass_le"][0]
    good = S.step(x, 0, 0.7, 1, temperature=2.0)
    bad = S.step(x, 0, 0.7, 1, temperature=2.0, defect="after_temperature")
    assert (good > -1e7).sum() == 2 and (bad > -1e7).sum() == 4
    S.check_mask(x, good > -1e7, 0, 0.7, 1)
    with pytest.raises(AssertionError, match="dropped by the rule and was kept"):
        S.check_mask(x, bad > -1e7, 0, 0.7, 1)


def test_the_checker_rejects_the_truncation_after_the_noise():
    """A draw that lifts the fourth token over the rest: truncating after the noise keeps it, the rule does not -- the sample
    would come from outside the two most probable tokens."""
    x = np.array([3.0, 2.0, 1.0, 0.0, -1.0, -2.0])
    g = np.array([0.0, 0.0, 0.0, 5.0, 0.0, 0.0])
    good, bad = S.step(x, 2, 0.0, 1, noise=g), S.step(x, 2, 0.0, 1, noise=g, defect="after_noise")
    assert list(good > -1e7) == [True, True, False, False, False, False] and list(good[:2]) == [3.0, 2.0]
    assert list(bad > -1e7) == [True, False, False, True, False, False]
    S.check_mask(x, good > -1e7, 2, 0.0, 1)
    with pytest.raises(AssertionError):
        S.check_mask(x, bad > -1e7, 2, 0.0, 1)


def test_the_checker_rejects_a_written_column_behind_v_and_a_changed_kept_entry():
    x = np.array([3.0, 2.0, 1.0, 0.0, -1.0, -2.0])
    before, after = _window(x, S.kept(x, 2, 0.0, 1))
    S.check(before, after, 6, 2, 0.0, 1)
    for col in (6, 7):
        bad = after.copy()
        bad[0, col] = -S.INF
        with pytest.raises(AssertionError, match="a column >= V = 6 was written"):
            S.check(before, bad, 6, 2, 0.0, 1)
    bad = after.copy()
    bad.view(np.int32)[0, 1] ^= 1                       # the kept 2.0, its last bit
    with pytest.raises(AssertionError, match="neither its input"):
        S.check(before, bad, 6, 2, 0.0, 1)
    bad = after.copy()
    bad[0, 3] = -1e7                                    # a dropped entry that does not hold the value
    with pytest.raises(AssertionError, match="neither its input"):
        S.check(before, bad, 6, 2, 0.0, 1)
    with pytest.raises(AssertionError, match="the option is off"):
        S.check(before, after, 6, 0, 0.0, 1)


# ---------------------------------------------------------------------------------------------- the undecided share
@pytest.mark.parametrize("rows,V,ld,variant", S.random_cases(), ids=lambda v: str(v))
def test_the_band_leaves_little_undecided_on_the_random_kernel_cases(rows, V, ld, variant):
    """A condition on the inputs of tests/test_gpu_sampling_kernels.py, shown with the reference alone: at most 1 % of a row's
    tokens are undecided under any of the case's settings (top-k alone: none)."""
    band = S.Band(S.random_logits(rows, V, variant).numpy())
    worst = 0
    for topk, topp, mk in S.random_settings(rows, V):
        u = int(band.undecided(topk, S.f32(topp), mk).max())
        assert u <= 0.01 * V and (topp > 0 or u == 0), (topk, topp, mk, u)
        worst = max(worst, u)
    print("rows %d V %d %s: delta up to %.2e, at most %d undecided" % (rows, V, variant, float(np.max(band.delta)), worst))


@pytest.mark.parametrize("V,ld", S.CONSTRUCTED_SHAPES)
@pytest.mark.parametrize("kind", S.CONSTRUCTED)
def test_the_constructed_kernel_cases_are_decided(kind, V, ld):
    """At most 2 undecided tokens per row; none where the GPU test compares bit for bit (everything but the nucleus settings of
    the pre-banned random rows).  And the kept counts the constructions name are the rule's."""
    x, settings = S.constructed(kind, V)
    band = S.Band(x)
    for topk, topp, mk, count in settings:
        u = int(band.undecided(topk, S.f32(topp), mk).max())
        assert u <= 2 and (u == 0 or (kind == "prebanned" and topp > 0)), (kind, V, topk, topp, mk, u)
        n = (S.kept(x, topk, S.f32(topp), mk) & (x > -1e7)).sum(1)
        if isinstance(count, dict):
            assert all(n[r] == want for r, want in count.items()), (n, count)
        elif count is not None:
            assert (n == count).all(), (n, count)


# ---------------------------------------------------------------------------------------------- the reference's search
@pytest.mark.parametrize("model", S.MODELS)
def test_reference_search_with_the_truncation(model):
    """make_fixture's own assertions on every setting and beam of the GPU model test (float64 and fp32 token- and
    order-identical, gap > 4 err, every threshold decision decided at 4 x the fp32 error, the bf16 storage model keeps the
    sharpened best hypotheses), the fp32 reference within a quarter of the project's fp32 score tolerance, and at least one
    sentence whose beams differ from the untruncated search."""
    f = S.make_fixture(model)
    for st in S.SETTINGS:
        r = f[st]
        print("%s topk=%d topp=%g: gap %.2e err %.1e (x %.1f) rel %.3f changed %d of %d; decisions beam 1 %s beam 4 %s"
              % (model, st[0], st[1], r["gap"], r["err"], r["gap"] / r["err"], r["rel"], r["changed"], f["src"].shape[0],
                 " ".join("%.1e" % v for v in r["decided_1"]), " ".join("%.1e" % v for v in r["decided_4"])))
        assert r["gap"] > 4.0 * r["err"] and r["rel"] <= 0.25 and r["changed"] >= 1
    r = f["with_ngram"]
    print("%s with the n-gram ban: gap %.2e err %.1e rel %.3f" % (model, r["gap"], r["err"], r["rel"]))
    assert r["gap"] > 4.0 * r["err"] and r["rel"] <= 0.25
