"""diverse_beam_groups / diverse_beam_strength end to end: transformer (the fused step driver) and rnnsearch (the recurrent one)
decode under the option what the reference search with groups of tests/diverse_ref.py decodes.

The tiny fixtures are those of tests/ngram_ref.py (H = 128, vocabularies 120 / 104, sources of 14, 5, 9 and 11 tokens) with the
seeds of diverse_ref.SEEDS; what the reference alone shows on them under diverse_ref.SETTINGS -- fp32 and float64 token- and
order-identical per group, gaps > 4 x the fp32 error, the fp32 reference within a quarter of the project's fp32 score tolerance
(rtol 1e-5 / atol 1e-6, which therefore is the score tolerance here: tests/rnnsearch_ref.score_tol), the sharpened model stable
under bf16 storage -- is asserted on the CPU by tests/test_diverse_host.py.
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_torch as rt  # noqa: E402
from tests import diverse_ref as D  # noqa: E402
from tests import rnnsearch_ref as R  # noqa: E402
from tests import shortlist_ref as SR  # noqa: E402
from tests import variant_gpu as G_  # noqa: E402
from tests import variant_ref as V  # noqa: E402
from zero_amd import shortlist  # noqa: E402
from zero_amd.config import SyntheticVocab  # noqa: E402
from zero_amd.models import load_all, model as registry  # noqa: E402
from zero_amd.models._factory import get_core, reset_cores  # noqa: E402

load_all()
TOL = R.score_tol(0.25, 0.0)            # (rtol, atol): the project's standard, see the module docstring
assert TOL == (D.RTOL, D.ATOL)
FIRST = D.SETTINGS[0]


@pytest.fixture(scope="module", params=list(D.MODELS))
def fx(request):
    model = request.param
    hp, src, Pn, fns = D.fixture(model)
    refs = {}

    def ref(st, sharp=False, fns_=None, key=None):
        """The fp32 reference search with groups; computed once per key and left unchanged."""
        k = (st, sharp, key)
        if k not in refs:
            refs[k] = D.search(fns if fns_ is None else fns_, hp, V.sharpen(hp, Pn) if sharp else Pn, src, st[0], st[1], st[2],
                               torch.float32)
        return refs[k]
    return dict(model=model, hp=hp, src=src, Pn=Pn, fns=fns, ref=ref)


def _hp(f, st, dtype, **kw):
    return G_.beam_hp(f["hp"], st[0], dtype, diverse_beam_groups=st[1], diverse_beam_strength=st[2], **kw)


def _close(scores, ref):
    fin = ref["score"] > -1e30
    print("largest score difference %.3e" % np.abs(scores - ref["score"])[fin].max())
    assert np.allclose(scores[fin], ref["score"][fin], rtol=TOL[0], atol=TOL[1]), np.abs(scores - ref["score"])[fin].max()


@pytest.mark.parametrize("st", D.SETTINGS, ids=str)
def test_fp32_mode_is_token_exact(fx, st):
    """Every beam of every group, in the merged order, token-equal to the reference search; scores within the tolerance; with
    the large lambda the first tokens of a sentence's hypotheses number at least G."""
    ref = fx["ref"](st)
    seqs, scores, core = G_.decode(_hp(fx, st, "float32"), fx["model"], fx["Pn"], fx["src"])
    assert seqs.shape[:2] == (fx["src"].shape[0], st[0])
    G_.assert_tokens(seqs, ref["seq"])
    _close(scores, ref)
    assert (np.diff(scores.astype(np.float64), axis=1) <= 0).all()            # the merge sorted them
    assert core.__dict__.get("_decode_step_launches", 0) > 0                   # the step ran from captured graphs
    if st[2] >= 8.0:
        assert all(len(set(seqs[b, :, 0].tolist())) >= st[1] for b in range(seqs.shape[0])), seqs[:, :, 0]


@pytest.mark.parametrize("st", [FIRST, D.SETTINGS[2]], ids=str)
def test_bf16_mode_best_hypotheses(fx, st):
    """Output distribution sharpened x 6: the best hypothesis of every sentence against the fp32 reference with groups."""
    from zero_amd.search import decode_hypothesis
    ref = fx["ref"](st, sharp=True)
    hp = _hp(fx, st, "bfloat16")
    seqs, scores, core = G_.decode(hp, fx["model"], V.sharpen(fx["hp"], fx["Pn"]), fx["src"])
    hyp, hyp_ref = decode_hypothesis(seqs, hp), rt.decode_hypothesis(ref["seq"], hp)
    assert hyp == hyp_ref, (hyp, hyp_ref)
    assert core.__dict__.get("_decode_step_launches", 0) > 0


ROUTES = {"host_book": {"ZERO_HIP_DECODE_DEVICE_BOOK": "0"}, "numpy_book": {"ZERO_HIP_DECODE_HOST_C": "0"},
          "eager": {"ZERO_HIP_DECODE_GRAPH": "0"}}


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_the_search_routes_agree_bit_for_bit(fx, monkeypatch, route, dtype):
    """Host bookkeeping in C, in numpy, and eager steps (where search.py launches the per-row top-k and the selection itself):
    steps, tokens and scores are the device-resident search's (K = 6, G = 3)."""
    hp = _hp(fx, D.SETTINGS[2], dtype)
    Pn = fx["Pn"] if dtype == "float32" else V.sharpen(fx["hp"], fx["Pn"])
    base = G_.decode(hp, fx["model"], Pn, fx["src"])
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    seqs, scores, core = G_.decode(hp, fx["model"], Pn, fx["src"])
    assert (core.__dict__.get("_decode_step_launches", 0) > 0) == (route != "eager")
    G_.assert_tokens(seqs, base[0])
    assert np.array_equal(scores, base[1]), np.abs(scores - base[1]).max()


def test_lambda_zero_equals_the_plain_beam_of_a_group(fx):
    """lambda = 0, K = 4, G = 2: both groups of a sentence are the plain search of beam 2, bit for bit; the merge (equal scores
    stay in group order) interleaves them."""
    plain = G_.decode(G_.beam_hp(fx["hp"], 2, "float32"), fx["model"], fx["Pn"], fx["src"])
    seqs, scores, _ = G_.decode(_hp(fx, (4, 2, 0.0), "float32"), fx["model"], fx["Pn"], fx["src"])
    for g in range(2):
        G_.assert_tokens(seqs[:, g::2], plain[0])
        assert np.array_equal(scores[:, g::2], plain[1]), np.abs(scores[:, g::2] - plain[1]).max()


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_one_group_is_the_option_absent(fx, dtype):
    """diverse_beam_groups = 1 (whatever the strength): tokens and scores bit-equal to hparams without the keys, and the
    captured step holds the same number of launches."""
    Pn = V.sharpen(fx["hp"], fx["Pn"])
    bare = G_.beam_hp(fx["hp"], 4, dtype)
    bare.del_hparam("diverse_beam_groups")
    bare.del_hparam("diverse_beam_strength")
    a = G_.decode(bare, fx["model"], Pn, fx["src"])
    la = a[2].__dict__["_decode_step_launches"]
    b = G_.decode(_hp(fx, (4, 1, 7.0), dtype), fx["model"], Pn, fx["src"])
    lb = b[2].__dict__["_decode_step_launches"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and la == lb
    c = G_.decode(_hp(fx, FIRST, dtype), fx["model"], Pn, fx["src"])
    assert not np.array_equal(a[0], c[0])


def test_step_graphs_are_reused_for_the_same_setting_only(fx):
    """A second batch of the same shape replays the first one's graphs; a run with another G, another lambda, or the option
    off, on the same engine adopts none of them and decodes what it decodes on a fresh engine."""
    from zero_amd import search
    model = fx["model"]
    hp = _hp(fx, FIRST, "float32")
    Pn = fx["Pn"]
    second = V.ragged((11, 14, 7, 9), hp.src_vocab.size(), 6, width=fx["src"].shape[1])
    G_.assert_graphs_reused(model, hp, Pn, fx["src"], second)
    for st in ((4, 4, FIRST[2]), (4, 2, 0.25), (4, 1, FIRST[2])):
        other = _hp(fx, st, "float32")
        fresh = G_.decode(other, model, Pn, fx["src"])
        reset_cores(); core = get_core(hp, model, Pn)
        enc, dec = registry.get_model(model).infer_fn(hp)
        search.beam_search({"source": fx["src"]}, enc, dec, hp)
        n0 = core.__dict__.get("_graph_adoptions", 0)
        enc, dec = registry.get_model(model).infer_fn(other)
        out = search.beam_search({"source": fx["src"]}, enc, dec, other)
        assert core.__dict__.get("_graph_adoptions", 0) == n0, st
        assert np.array_equal(np.asarray(out["seq"]), fresh[0]) and np.array_equal(np.asarray(out["score"]), fresh[1]), st


def test_search_mode_dev_selects_per_group_too():
    """search_mode=dev (the whole prefix through the training-path decoder each step; bf16): the eager per-row top-k and the
    selection on its logits.  The best hypotheses are the cached decode's under the same setting (sharpened model), the result
    has K sorted hypotheses per sentence, and it differs from the dev decode without groups."""
    from zero_amd.search import decode_hypothesis
    hp, src, Pn, _ = D.fixture("transformer")
    Pn = V.sharpen(hp, Pn)
    K, G, lam = FIRST
    out = {}
    for g in (1, G):
        h = G_.beam_hp(hp, K, "bfloat16", diverse_beam_groups=g, diverse_beam_strength=lam)
        h.search_mode = "dev"
        out[g] = G_.decode(h, "transformer", Pn, src)
    cached = G_.decode(G_.beam_hp(hp, K, "bfloat16", diverse_beam_groups=G, diverse_beam_strength=lam), "transformer", Pn, src)
    assert out[G][0].shape[:2] == (src.shape[0], K)
    assert decode_hypothesis(out[G][0], hp) == decode_hypothesis(cached[0], hp)
    assert (np.diff(out[G][1].astype(np.float64), axis=1) <= 0).all()
    assert not np.array_equal(out[G][0], out[1][0])


# ---------------------------------------------------------------------------------------------- combinations
def _forbidden(scores):
    """True when some hypothesis took an overwritten candidate (-1e8 over a length penalty; empty slots hold F32_MIN)."""
    return bool(((scores < -1e6) & (scores > -1e30)).any())


def _eager_equals(monkeypatch, hp, model, Pn, src, base):
    """The same decode with eager steps (ZERO_HIP_DECODE_GRAPH=0: search.py issues every launch of the tail itself): tokens and
    scores bit-equal to `base`."""
    monkeypatch.setenv("ZERO_HIP_DECODE_GRAPH", "0")
    seqs, scores, core = G_.decode(hp, model, Pn, src)
    monkeypatch.delenv("ZERO_HIP_DECODE_GRAPH")
    assert core.__dict__.get("_decode_step_launches", 0) == 0
    G_.assert_tokens(seqs, base[0])
    assert np.array_equal(scores, base[1]), np.abs(scores - base[1]).max()


@pytest.mark.parametrize("st, topk", [((4, 4, 0.5), 3), ((4, 2, 0.5), 3), ((6, 3, 0.5), 2)], ids=str)
def test_truncation_keeps_enough_for_the_lists_on_every_route(fx, monkeypatch, st, topk):
    """sampling_topk below the per-row list depth K + K/G: the truncation's min_keep = 2 * beam_size + 1 comes from the whole
    beam on every route, so the lists hold real candidates only.  Eager steps equal the captured ones bit for bit (fp32), no
    kept candidate carries the forbid value, and search_mode=dev (bf16, sharpened) gives the cached decode's best hypotheses."""
    from zero_amd.search import decode_hypothesis
    hp = _hp(fx, st, "float32", sampling_topk=topk)
    base = G_.decode(hp, fx["model"], fx["Pn"], fx["src"])
    assert not _forbidden(base[1])
    _eager_equals(monkeypatch, hp, fx["model"], fx["Pn"], fx["src"], base)
    if fx["model"] == "transformer":      # (the recurrent models decode with search_mode=cache only)
        Ps = V.sharpen(fx["hp"], fx["Pn"])
        hb = _hp(fx, st, "bfloat16", sampling_topk=topk)
        cached = G_.decode(hb, fx["model"], Ps, fx["src"])
        hd = copy.copy(hb)
        hd.search_mode = "dev"
        dev = G_.decode(hd, fx["model"], Ps, fx["src"])
        assert decode_hypothesis(dev[0], hb) == decode_hypothesis(cached[0], hb)
        assert not _forbidden(dev[1])


@pytest.mark.parametrize("kind", sorted(D.COMBOS))
def test_with_another_option(kind, monkeypatch):
    """diverse_ref.COMBOS, fp32, (K, G, lambda) = SETTINGS[0]: no_repeat_ngram_size = 2 on the transformer, sampling_topk = 5 on
    rnnsearch -- the reference search with groups around the wrapped decoding functions, token-exact; eager steps give the
    same, bit for bit."""
    model, value = D.COMBOS[kind]
    hp, src, Pn, fns = D.fixture(model)
    K, G, lam = FIRST
    ref = D.search(D.combo_fns(kind, fns, K), hp, Pn, src, K, G, lam, torch.float32)
    kw = dict(no_repeat_ngram_size=value) if kind == "ngram" else dict(sampling_topk=value)
    hp = G_.beam_hp(hp, K, "float32", diverse_beam_groups=G, diverse_beam_strength=lam, **kw)
    seqs, scores, _ = G_.decode(hp, model, Pn, src)
    G_.assert_tokens(seqs, ref["seq"])
    _close(scores, ref)
    _eager_equals(monkeypatch, hp, model, Pn, src, (seqs, scores))
    if kind == "ngram":
        from tests import ngram_ref as N
        for b in range(seqs.shape[0]):
            for k in range(seqs.shape[1]):
                assert not N.has_repeat(N.hypothesis(seqs[b, k], hp), value)


def test_two_member_ensemble():
    """transformer + transformer_aan, fp32, (K, G, lambda) = SETTINGS[0]: the rule on the combined log-probabilities, against
    the reference search with groups over the composed oracle (tests/ensemble_common.py: peaked toy members)."""
    from tests import ensemble_common as ec
    from zero_amd import search
    from zero_amd.models._ensemble import make_infer_fns, member_params
    models = ("transformer", "transformer_aan")
    K, G, lam = FIRST
    hps, Pns, src = ec.make_members(models, (3, 4))
    hps = ec.with_beam(hps, K, decode_dtype="float32", diverse_beam_groups=G, diverse_beam_strength=lam)
    enc, dec = ec.composed_infer_fn(hps, Pns, models)
    with torch.no_grad():
        ref = D.grouped_search(torch.tensor(src), enc, dec, hps[0], G, lam)
    reset_cores()
    for i, (hp, Pn, m) in enumerate(zip(hps, Pns, models)):
        get_core(member_params(hp, i), m, Pn)
    enc, dec, hp0 = make_infer_fns([registry.get_model(m) for m in models], hps)
    out = search.beam_search({"source": src}, enc, dec, hp0)
    seqs, scores = np.asarray(out["seq"]), np.asarray(out["score"])
    G_.assert_tokens(seqs, ref["seq"])
    _close(scores, ref)


VSRC, VT, FIRST_IDS, BEST, ROUND = 36, 41, 5, 2, 8


def _lex_lines():
    rng = np.random.default_rng(11)
    out = []
    for s in range(3, VSRC):
        out += ["%d %d %.3f" % (t, s, 0.9 - 0.2 * i) for i, t in enumerate(rng.choice(np.arange(FIRST_IDS, VT), 4, replace=False))]
    return out


def test_shortlist(tmp_path, monkeypatch):
    """Under a shortlist V is Vs: the run equals, bit for bit, the twin model (the rows S of the target-side tables as a
    vocabulary of its own, tests/test_gpu_shortlist_model.py) under the same groups, ids mapped back through S; and it differs
    from the shortlist decode without groups."""
    from tests.common import make_hp, perturb
    model = "transformer"
    path = tmp_path / "lex.txt"
    path.write_text("\n".join(_lex_lines()) + "\n")
    table = shortlist.parse_table(_lex_lines(), SyntheticVocab(VSRC), SyntheticVocab(VT))
    hp = make_hp(model, Vs=VSRC, Vt=VT, search_mode="cache")
    hp.scope_name = "t_diverse_sl_" + model
    hp.override_from_dict(dict(shortlist_file=str(path), shortlist_first=FIRST_IDS, shortlist_best=BEST, shortlist_round=ROUND))
    K, G, lam = FIRST
    plain_hp = G_.beam_hp(hp, K, "float32")
    hp = G_.beam_hp(hp, K, "float32", diverse_beam_groups=G, diverse_beam_strength=lam)
    Pn = perturb(rt.init_params(hp, model, seed=5), np.random.default_rng(6))
    src = V.ragged((6, 4, 5), VSRC, 5)
    ids, (_, Vs) = SR.build(src, table.off, table.ids, FIRST_IDS, BEST, VT, ROUND, VT)
    Sids = ids[:Vs].astype(np.int64)
    assert len(Sids) < VT
    seqs, scores, _ = G_.decode(hp, model, Pn, src)
    hp2 = copy.copy(hp)
    hp2.tgt_vocab, hp2.shortlist_file, hp2.scope_name = SyntheticVocab(len(Sids)), "", hp.scope_name + "_twin"
    Pn2 = dict(Pn)
    for name in {rt._emb_name(hp, "tgt"), rt._emb_name(hp, "softmax")}:
        Pn2[name] = np.ascontiguousarray(Pn[name][Sids])
    seqs2, scores2, _ = G_.decode(hp2, model, Pn2, src)
    G_.assert_tokens(seqs, Sids[seqs2])
    assert np.array_equal(scores, scores2), np.abs(scores - scores2).max()
    plain = G_.decode(plain_hp, model, Pn, src)
    assert not np.array_equal(plain[0], seqs)
    _eager_equals(monkeypatch, hp, model, Pn, src, (seqs, scores))
