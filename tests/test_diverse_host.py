"""diverse_beam_groups / diverse_beam_strength on the CPU: the HParams, what is refused (without a core), the graph key, the
rule of tests/diverse_ref.py by hand, the exactness of the candidate-list depth K + K/G, lambda = 0, every planted defect on the
case named for it, the final merge, and what the reference search alone shows on the fixtures of the GPU model test."""
import numpy as np
import pytest
import torch

from tests import diverse_ref as D
from tests import variant_ref as V
from tests.common import make_hp
from zero_amd.config import default_params
from zero_amd.models import _decode


# ---------------------------------------------------------------------------------------------- the HParams
def test_hparam_defaults_and_parse():
    hp = default_params()
    assert hp.diverse_beam_groups == 1 and hp.diverse_beam_strength == 0.5
    assert _decode.diverse_opts(hp) == (1, 0.0) and not _decode.diverse_on(_decode.diverse_opts(hp))
    hp.parse("diverse_beam_groups=2,diverse_beam_strength=0.25,beam_size=4")
    assert hp.diverse_beam_groups == 2 and isinstance(hp.diverse_beam_groups, int)
    assert _decode.diverse_opts(hp) == (2, 0.25) and _decode.diverse_on(_decode.diverse_opts(hp))
    assert _decode.diverse_opts(hp, 6) == (2, 0.25)
    assert not _decode.diverse_on(None)
    bare = make_hp("transformer")
    bare.del_hparam("diverse_beam_groups")
    bare.del_hparam("diverse_beam_strength")
    assert _decode.diverse_opts(bare) == (1, 0.0)


REFUSALS = [
    (dict(beam_size=4, diverse_beam_groups=0), r"diverse_beam_groups=0"),
    (dict(beam_size=4, diverse_beam_groups=-2, diverse_beam_strength=-1.0), r"diverse_beam_groups=-2"),      # G first
    (dict(beam_size=4, diverse_beam_groups=3, diverse_beam_strength=-1.0), r"diverse_beam_groups=3: beam_size=4 is no multiple"),
    (dict(beam_size=4, diverse_beam_groups=2, diverse_beam_strength=-0.5), r"diverse_beam_strength=-0\.5"),
    (dict(beam_size=4, diverse_beam_groups=2, diverse_beam_strength=float("nan")), r"diverse_beam_strength=nan"),
    (dict(beam_size=4, diverse_beam_groups=2, diverse_beam_strength=float("inf")), r"diverse_beam_strength=inf"),
    (dict(beam_size=12, diverse_beam_groups=2, diverse_beam_strength=-1.0), r"diverse_beam_strength=-1"),     # before the depth
    (dict(beam_size=12, diverse_beam_groups=2), r"diverse_beam_groups=2 with beam_size=12: .* 12 \+ 6 = 18 .* at most 16"),
    (dict(beam_size=14, diverse_beam_groups=7), r"14 \+ 2 = 16")]


@pytest.mark.parametrize("kw, text", REFUSALS[:-1])
@pytest.mark.parametrize("model", ["transformer", "rnnsearch"])
def test_bad_settings_are_refused_before_a_core_is_built(model, kw, text):
    from zero_amd.models import model as registry, load_all
    load_all()
    hp = make_hp(model, search_mode="cache", **kw)
    with pytest.raises(ValueError, match=text):
        registry.get_model(model).infer_fn(hp)
    with pytest.raises(ValueError, match=text):
        _decode.diverse_opts(hp)


def test_the_search_refuses_too(monkeypatch):
    """zero_amd.search.beam_search with a beam size of its own: refused before encoding_fn is called."""
    from zero_amd import search
    hp = make_hp("transformer", search_mode="cache", beam_size=4, diverse_beam_groups=2)
    hp.beam_size = 5

    def encoding_fn(*a, **k):
        raise AssertionError("encoding_fn was called")
    with pytest.raises(ValueError, match=r"beam_size=5 is no multiple"):
        search._beam_search_body({"source": np.ones((2, 3), dtype=np.int64)}, encoding_fn, None, hp, [])


def test_the_limits_that_are_taken():
    for K, G in D.KG_SETTINGS + ((14, 7), (5, 5), (8, 8), (10, 2), (15, 15)):
        hp = make_hp("transformer", beam_size=K, diverse_beam_groups=G, diverse_beam_strength=0.0)
        assert _decode.diverse_opts(hp) == (G, 0.0) and D.depth(K, G) <= D.DEPTH_MAX == _decode.DIVERSE_DEPTH_MAX
    # G = 1: the strength is ignored, and a beam of 16 stays what it was
    hp = make_hp("transformer", beam_size=16, diverse_beam_groups=1, diverse_beam_strength=-3.0)
    assert _decode.diverse_opts(hp) == (1, 0.0)


def test_graph_key():
    """Off: the key of a step is the tuple it was before the option existed.  On: one more entry holding G and the bits of
    lambda, so that no two settings share a key."""
    state = {"B": 4, "K": 4, "Ls": 16, "Tmax": 24, "f32": True}
    args = (state, None, 1.0, 1e8, False, 0)
    before = (4, 4, 16, 24, False, 1.0, 1e8, False, 0, True)
    assert _decode.graph_key(*args) == before
    assert _decode.graph_key(*args, 0, None, None) == before and _decode.graph_key(*args, 0, None, (1, 0.0)) == before
    assert _decode.graph_key(*args, diverse=_decode.diverse_opts(default_params())) == before
    keys = {d: _decode.graph_key(*args, 0, None, d) for d in [(2, 0.5), (4, 0.5), (2, 0.0), (2, 0.25), (2, 0.5000001)]}
    assert len(set(keys.values())) == len(keys) and before not in keys.values()
    assert keys[(2, 0.5)] == before + (("diverse", 2, 0x3f000000),)
    assert _decode.graph_key(*args, 3, (10, 0.9), (2, 0.5, 2)) == \
        before + (("ngram", 3), ("sample", 10, 0x3f666666), ("diverse", 2, 0x3f000000))


# ---------------------------------------------------------------------------------------------- the rule
def test_rule_by_hand():
    """K = 4, G = 2, V = 5, EOS = 2, lambda = 1, penalty 2 (so a counted token loses 0.5)."""
    S = np.array([[-1.0, -2.0, -9.0, -3.0, -4.0],       # group 0, beam 0
                  [-1.5, -9.0, -1.25, -9.0, -9.0],      # group 0, beam 1
                  [-1.0, -1.25, -9.0, -3.0, -1.5],      # group 1, beam 0
                  [-9.0, -9.0, -1.0, -9.0, -1.75]])     # group 1, beam 1
    ts, ti = D.select_full(S, 2, 1.0, 2.0, D.EOS)
    # group 0: (b0, 0) -1, (b1, 2 = EOS) -1.25, (b1, 0) -1.5, (b0, 1) -2; it counts token 0 only (EOS is not counted)
    assert list(ti[0]) == [0, 5 + 2, 5 + 0, 1] and list(ts[0]) == [-1.0, -1.25, -1.5, -2.0]
    # group 1: token 0 loses 0.5: (b1, EOS) -1, (b0, 1) -1.25, then (b0, 0) -1.5 ties (b0, 4) -1.5: the lower index first
    assert list(ti[1]) == [5 + 2, 1, 0, 4] and list(ts[1]) == [-1.0, -1.25, -1.5, -1.5]
    # the same from lists of depth K + Kg = 6 > V (here: the whole rows), and in fp32
    for S_ in (S, S.astype(np.float32)):
        a = D.select_lists(*D.row_lists(S_, 5), 5, 2, 1.0, 2.0, D.EOS)
        assert np.array_equal(a[0], ts) and np.array_equal(a[1], ti) and a[0].dtype == S_.dtype
    # a token counted twice loses twice: three groups
    S3 = np.array([[-1.0, -2.0, -9.0], [-1.0, -2.0, -9.0], [-1.0, -1.75, -9.0]])
    ts, ti = D.select_full(S3, 3, 0.5, 1.0, D.EOS)
    assert list(ti[:, 0]) == [0, 0, 1] and list(ts[:, 0]) == [-1.0, -1.5, -1.75] and ts[2, 1] == -2.0


def _depth_mismatches(K, G, n=300):
    """n random cases with colliding dyadic scores -> the mismatches against the full matrix at depth K + K/G and at 2 K/G."""
    bad_deep, bad_shallow = 0, 0
    for seed in range(n):
        V_ = (D.depth(K, G) + 1, 24, 40)[seed % 3]
        S = D.dyadic_scores(1000 * K + 10 * G + seed, K, V_, levels=(5, 9, 17)[seed % 3])
        lam = (0.25, 0.5, 1.0, 4.0)[seed % 4]
        full = D.select_full(S, G, lam, 1.0, D.EOS)
        deep = D.step(S, G, lam, 1.0, D.EOS)
        shallow = D.step(S, G, lam, 1.0, D.EOS, defect="shallow")
        bad_deep += not (np.array_equal(full[0], deep[0]) and np.array_equal(full[1], deep[1]))
        bad_shallow += not (np.array_equal(full[0], shallow[0]) and np.array_equal(full[1], shallow[1]))
    return bad_deep, bad_shallow


def test_depth_K_plus_Kg_is_exact_and_2Kg_is_not():
    """300 random cases per (K, G) of KG_SETTINGS -- 2100 in all -- with colliding dyadic scores: lists of depth K + K/G give the
    full matrix's result, bit for bit, in every case; lists of depth 2 K/G do not."""
    shallow = {}
    for K, G in D.KG_SETTINGS:
        bad_deep, shallow[(K, G)] = _depth_mismatches(K, G)
        print("(K, G) = (%d, %d): depth K + Kg %d mismatches, depth 2 Kg %d of 300" % (K, G, bad_deep, shallow[(K, G)]))
        assert bad_deep == 0, (K, G)
    assert sum(shallow.values()) > 0, shallow


def test_lambda_zero_gives_identical_groups_each_a_plain_beam():
    """The rule: with lambda = 0 and equal rows per group every group selects what a plain beam of K/G selects."""
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((2, 50))
    S = np.concatenate([rows, rows, rows])                  # K = 6, G = 3: three equal groups
    ts, ti = D.step(S, 3, 0.0, 1.3, D.EOS)
    assert np.array_equal(ts[0], ts[1]) and np.array_equal(ts[0], ts[2]) and np.array_equal(ti[0], ti[1])
    flat = rows.reshape(-1)
    order = np.argsort(-flat, kind="stable")[:4]
    assert np.array_equal(ti[0], order) and np.array_equal(ts[0], flat[order])


# ---------------------------------------------------------------------------------------------- planted defects
@pytest.mark.parametrize("defect", [d for d in D.DEFECTS if d != "merge_unsorted"])
def test_every_step_defect_fails_on_its_case(defect):
    seed, K, G, V_, lam, pen = D.DEFECT_CASES[defect]
    S = D.dyadic_scores(seed, K, V_)
    good, full = D.step(S, G, lam, pen, D.EOS), D.select_full(S, G, lam, pen, D.EOS)
    assert np.array_equal(good[0], full[0]) and np.array_equal(good[1], full[1])
    bad = D.step(S, G, lam, pen, D.EOS, defect=defect)
    assert not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1]))


def test_merge_and_its_defect():
    """Two sentences, G = 2, Kg = 2: sorted by score, equal scores in group order; the product's merge is the same."""
    from zero_amd.search import merge_groups
    scores = np.array([[-1.0, -3.0], [-0.5, -3.0], [-2.0, D.F32_MIN], [-2.0, -2.5]], dtype=np.float32)
    seqs = np.arange(4 * 2 * 3).reshape(4, 2, 3)
    q, s = D.merge(seqs, scores, 2)
    assert s.tolist() == [[-0.5, -1.0, -3.0, -3.0], [-2.0, -2.0, -2.5, float(D.F32_MIN)]]
    assert q[0, :, 0].tolist() == [6, 0, 3, 9] and q[1, :, 0].tolist() == [12, 18, 21, 15]
    q2, s2 = merge_groups(seqs, scores, 2)
    assert np.array_equal(q, q2) and np.array_equal(s, s2)
    q3, s3 = D.merge(seqs, scores, 2, defect="merge_unsorted")
    assert not np.array_equal(s, s3)
    q1, s1 = merge_groups(seqs, scores, 1)
    assert q1 is seqs and s1 is scores


# ---------------------------------------------------------------------------------------------- the fixtures of the model test
@pytest.fixture(scope="module", params=list(D.MODELS))
def fx(request):
    hp, src, Pn, fns = D.fixture(request.param)
    return dict(model=request.param, hp=hp, src=src, Pn=Pn, fns=fns)


@pytest.mark.parametrize("K, G, lam", D.SETTINGS, ids=str)
def test_the_reference_alone_is_far_from_a_tie(fx, K, G, lam):
    """diverse_ref.margin on the fixture seeds: float64 and fp32 reference token- and order-identical, the smallest decisive
    gap more than 4 x the measured fp32 error (the rule of tests/rnnsearch_ref.py), the fp32 reference within a quarter of the
    score tolerance; the groups differ from each other, and with the large lambda their first tokens do."""
    m = D.margin(fx["fns"], fx["hp"], fx["Pn"], fx["src"], K, G, lam, what=(fx["model"], K, G, lam))
    print("%s K=%d G=%d lambda=%g: gap %.3e err %.3e rel %.3f" % (fx["model"], K, G, lam, m["gap"], m["err"], m["rel"]))
    assert m["rel"] <= 0.25
    groups = m["ref"]["groups"]["seq"]
    per = groups.reshape(-1, G, groups.shape[1], groups.shape[2])
    assert any(not np.array_equal(per[b, 0], per[b, g]) for b in range(per.shape[0]) for g in range(1, G))
    if lam >= 8.0:
        first = D.first_tokens(groups, G)
        assert all(len(set(row.tolist())) == G for row in first), first
    s = m["ref"]["score"]
    assert (np.diff(s.astype(np.float64), axis=1) <= 0).all()


@pytest.mark.parametrize("kind", sorted(D.COMBOS))
def test_the_combinations_are_far_from_a_tie_too(kind):
    """The n-gram ban and the top-k truncation around the model (the combination cases of the GPU model test)."""
    model = D.COMBOS[kind][0]
    hp, src, Pn, fns = D.fixture(model)
    K, G, lam = D.SETTINGS[0]
    m = D.margin(D.combo_fns(kind, fns, K), hp, Pn, src, K, G, lam, what=(kind, model))
    print("%s on %s: gap %.3e err %.3e rel %.3f" % (kind, model, m["gap"], m["err"], m["rel"]))
    assert m["rel"] <= 0.25


@pytest.mark.parametrize("K, G, lam", D.SETTINGS, ids=str)
def test_the_sharpened_model_keeps_its_best_hypotheses_under_bf16_storage(fx, K, G, lam):
    """Output distribution sharpened x 6 (the bf16 case of the GPU model test): ref_torch's bf16 storage model keeps the best
    hypothesis of every sentence of the fp32 run."""
    from oracle import ref_torch as rt
    Ps = V.sharpen(fx["hp"], fx["Pn"])
    a = D.search(fx["fns"], fx["hp"], Ps, fx["src"], K, G, lam, torch.float32)
    b = D.search(fx["fns"], fx["hp"], Ps, fx["src"], K, G, lam, torch.float32, store_bf16=True)
    assert rt.decode_hypothesis(a["seq"], fx["hp"]) == rt.decode_hypothesis(b["seq"], fx["hp"])


def test_lambda_zero_search_equals_the_plain_beam(fx):
    """lambda = 0: the G groups of every sentence are identical, and each is the plain search of beam K/G (tokens; the scores
    to fp32 rounding: the model runs on twice as many rows)."""
    ref = D.search(fx["fns"], fx["hp"], fx["Pn"], fx["src"], 4, 2, 0.0, torch.float32)
    plain, _ = V.search(fx["fns"], fx["hp"], fx["Pn"], fx["src"], 2, torch.float32)
    g = ref["groups"]
    n = min(g["seq"].shape[2], plain["seq"].shape[2])
    for grp in range(2):
        assert np.array_equal(g["seq"][grp::2, :, :n], plain["seq"][:, :, :n])
        assert not g["seq"][grp::2, :, n:].any() and not plain["seq"][:, :, n:].any()
        assert np.allclose(g["score"][grp::2], plain["score"], rtol=1e-6, atol=1e-6)
