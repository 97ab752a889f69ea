"""sampling_topk / sampling_topp end to end: transformer, transformer_aan (the fused step driver) and rnnsearch (the recurrent
one) decode under the truncation what the reference's search decodes with the rule of tests/sampling_ref.py (``truncated``: the
rule on the restated step's logits, after ngram_ref.constrained's ban where both are on).

The tiny fixtures are those of tests/ngram_ref.py (H = 128, vocabularies 120 / 104, sources of 14, 5, 9 and 11 tokens, the same
seeds); what the reference alone shows on them under sampling_ref.SETTINGS -- fp32 and float64 token- and order-identical, gaps
> 4 x the fp32 error, every threshold decision decided at 4 x the fp32 error, at least one sentence whose beams differ from the
untruncated search -- is asserted on the CPU by tests/test_sampling_host.py, including that the fp32 reference stays within a
quarter of the project's fp32 score tolerance, rtol 1e-5 / atol 1e-6, which therefore is the score tolerance here.  Beam 1 and 4.
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_torch as rt  # noqa: E402
from tests import ensemble_common as ec  # noqa: E402
from tests import ngram_ref as N  # noqa: E402
from tests import sampling_ref as S  # noqa: E402
from tests import shortlist_ref as SR  # noqa: E402
from tests import variant_gpu as G  # noqa: E402
from tests import variant_ref as V  # noqa: E402
from zero_amd import shortlist  # noqa: E402
from zero_amd.config import SyntheticVocab  # noqa: E402
from zero_amd.models import _decode, load_all, model as registry  # noqa: E402
from zero_amd.models._factory import get_core, reset_cores  # noqa: E402
from zero_amd.utils import dtype as zdtype  # noqa: E402

load_all()
TOL = (S.RTOL, S.ATOL)
BOTH = S.SETTINGS[-1]           # top-k and top-p together


@pytest.fixture(scope="module", params=list(S.MODELS))
def fx(request):
    model = request.param
    hp, src = N.fixture(model)
    Pn = N.MODELS[model]["init"](hp, N.SEEDS[model])
    refs = {}

    def ref(st, K, sharp=False, ngram=0):
        """The truncated fp32 reference; computed once per key and left unchanged."""
        key = (st, K, sharp, ngram)
        if key not in refs:
            refs[key] = V.search(S.fns_of(model, st[0], st[1], K, ngram=ngram), hp, V.sharpen(hp, Pn) if sharp else Pn, src, K,
                                 torch.float32)[0]
        return refs[key]
    return dict(model=model, hp=hp, src=src, Pn=Pn, ref=ref)


def _hp(f, K, dtype, st, **kw):
    return G.beam_hp(f["hp"], K, dtype, sampling_topk=st[0], sampling_topp=st[1], **kw)


def _close(scores, ref):
    fin = ref["score"] > -1e30
    print("largest score difference %.3e" % np.abs(scores - ref["score"])[fin].max())
    assert np.allclose(scores[fin], ref["score"][fin], rtol=TOL[0], atol=TOL[1]), np.abs(scores - ref["score"])[fin].max()


# ---------------------------------------------------------------------------------------------- noise off
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("st", S.SETTINGS, ids=str)
def test_fp32_mode_is_token_exact(fx, st, K):
    ref = fx["ref"](st, K)
    seqs, scores, core = G.decode(_hp(fx, K, "float32", st), fx["model"], fx["Pn"], fx["src"])
    G.assert_tokens(seqs, ref["seq"])
    _close(scores, ref)
    assert core.__dict__.get("_decode_step_launches", 0) > 0           # the step ran from captured graphs


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("st", S.SETTINGS, ids=str)
def test_bf16_mode_best_hypotheses(fx, st, K):
    """Output distribution sharpened x 6: the best hypothesis of every sentence against the truncated fp32 reference."""
    from zero_amd.search import decode_hypothesis
    ref = fx["ref"](st, K, sharp=True)
    hp = _hp(fx, K, "bfloat16", st)
    seqs, scores, core = G.decode(hp, fx["model"], V.sharpen(fx["hp"], fx["Pn"]), fx["src"])
    hyp, hyp_ref = decode_hypothesis(seqs, hp), rt.decode_hypothesis(ref["seq"], hp)
    assert hyp == hyp_ref, (hyp, hyp_ref)
    assert core.__dict__.get("_decode_step_launches", 0) > 0


def test_the_truncated_decode_differs_from_the_plain_one(fx):
    """What the reference shows on the CPU, on the device: under the nucleus some sentence's beams differ (fp32, beam 4), and
    every finished score does (the log-softmax renormalises over what is left)."""
    plain = G.decode(G.beam_hp(fx["hp"], 4, "float32"), fx["model"], fx["Pn"], fx["src"])
    trunc = G.decode(_hp(fx, 4, "float32", S.SETTINGS[1]), fx["model"], fx["Pn"], fx["src"])
    assert not np.array_equal(plain[0], trunc[0])
    assert (trunc[1][:, 0] > plain[1][:, 0]).all()


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_topp_one_is_inert_and_one_node_more(fx, dtype):
    """sampling_topp = 1.0 keeps every token: tokens and scores bit-equal to the option off (and to hparams without the keys),
    while the captured step holds exactly one launch more."""
    Pn = V.sharpen(fx["hp"], fx["Pn"])
    bare = G.beam_hp(fx["hp"], 4, dtype)
    bare.del_hparam("sampling_topk")
    bare.del_hparam("sampling_topp")
    a = G.decode(bare, fx["model"], Pn, fx["src"])
    la = a[2].__dict__["_decode_step_launches"]
    b = G.decode(_hp(fx, 4, dtype, (0, 0.0)), fx["model"], Pn, fx["src"])
    lb = b[2].__dict__["_decode_step_launches"]
    c = G.decode(_hp(fx, 4, dtype, (0, 1.0)), fx["model"], Pn, fx["src"])
    lc = c[2].__dict__["_decode_step_launches"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    assert la == lb and lc == lb + 1, (la, lb, lc)


ROUTES = {"host_book": {"ZERO_HIP_DECODE_DEVICE_BOOK": "0"}, "numpy_book": {"ZERO_HIP_DECODE_HOST_C": "0"},
          "eager": {"ZERO_HIP_DECODE_GRAPH": "0"}}


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_the_other_search_routes_equal_the_device_resident_one(fx, monkeypatch, route, dtype):
    """Host bookkeeping in C, in numpy, and eager steps (where search.py launches the truncation itself): steps, tokens and
    scores are the device-resident search's, bit for bit (top-k and top-p together, beam 4)."""
    hp = _hp(fx, 4, dtype, BOTH)
    Pn = fx["Pn"] if dtype == "float32" else V.sharpen(fx["hp"], fx["Pn"])
    base = G.decode(hp, fx["model"], Pn, fx["src"])
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    seqs, scores, core = G.decode(hp, fx["model"], Pn, fx["src"])
    assert (core.__dict__.get("_decode_step_launches", 0) > 0) == (route != "eager")
    G.assert_tokens(seqs, base[0])
    assert np.array_equal(scores, base[1]), np.abs(scores - base[1]).max()


def test_search_mode_dev_truncates_too():
    """search_mode=dev (the whole prefix through the training-path decoder each step; bf16): the eager truncation on its
    logits.  The best hypotheses are the cached decode's under the same setting, and the scores differ from the untruncated
    dev decode's."""
    from zero_amd.search import decode_hypothesis
    hp, src = N.fixture("transformer")
    Pn = V.sharpen(hp, N.MODELS["transformer"]["init"](hp, N.SEEDS["transformer"]))
    out = {}
    for st in ((0, 0.0), S.SETTINGS[1]):
        h = G.beam_hp(hp, 4, "bfloat16", sampling_topk=st[0], sampling_topp=st[1])
        h.search_mode = "dev"
        out[st] = G.decode(h, "transformer", Pn, src)
    cached = G.decode(G.beam_hp(hp, 4, "bfloat16", sampling_topk=0, sampling_topp=S.SETTINGS[1][1]), "transformer", Pn, src)
    assert decode_hypothesis(out[S.SETTINGS[1]][0], hp) == decode_hypothesis(cached[0], hp)
    assert (out[S.SETTINGS[1]][1][:, 0] > out[(0, 0.0)][1][:, 0]).all()


# ---------------------------------------------------------------------------------------------- combinations
@pytest.mark.parametrize("K", [1, 4])
def test_with_the_ngram_ban(fx, K):
    """sampling_ref.WITH_NGRAM (no_repeat_ngram_size = 3 and the nucleus), fp32: the reference with both wrappers (ban first),
    token-exact; no hypothesis repeats a 3-gram."""
    n, st = S.WITH_NGRAM
    assert n == 3
    ref = fx["ref"](st, K, ngram=n)
    seqs, scores, _ = G.decode(_hp(fx, K, "float32", st, no_repeat_ngram_size=n), fx["model"], fx["Pn"], fx["src"])
    G.assert_tokens(seqs, ref["seq"])
    _close(scores, ref)
    for b in range(seqs.shape[0]):
        for k in range(seqs.shape[1]):
            assert not N.has_repeat(N.hypothesis(seqs[b, k], fx["hp"]), 3)


def test_two_member_ensemble():
    """transformer + transformer_aan, fp32, beam 4: the rule on the combined log-probabilities, against the composed oracle
    under the same truncation."""
    from zero_amd import search
    from zero_amd.models._ensemble import make_infer_fns, member_params
    models = ("transformer", "transformer_aan")
    hps, Pns, src = ec.make_members(models, (3, 4))
    hps = ec.with_beam(hps, 4, decode_dtype="float32", sampling_topk=BOTH[0], sampling_topp=BOTH[1])
    fns = S.truncated(lambda hp, P: ec.composed_infer_fn(hps, Pns, models), BOTH[0], BOTH[1], 4)
    enc, dec = fns(hps[0], None)
    with torch.no_grad():
        ref = rt.beam_search({"source": torch.tensor(src)}, enc, dec, hps[0])
    reset_cores()
    for i, (hp, Pn, m) in enumerate(zip(hps, Pns, models)):
        get_core(member_params(hp, i), m, Pn)
    enc, dec, hp0 = make_infer_fns([registry.get_model(m) for m in models], hps)
    out = search.beam_search({"source": src}, enc, dec, hp0)
    seqs, scores = np.asarray(out["seq"]), np.asarray(out["score"])
    G.assert_tokens(seqs, ref["seq"])
    _close(scores, ref)


VSRC, VT, FIRST, BEST, ROUND = 36, 41, 5, 2, 8


def _lex_lines():
    rng = np.random.default_rng(11)
    out = []
    for s in range(3, VSRC):
        out += ["%d %d %.3f" % (t, s, 0.9 - 0.2 * i) for i, t in enumerate(rng.choice(np.arange(FIRST, VT), 4, replace=False))]
    return out


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("model", ["transformer", "rnnsearch"])
def test_shortlist(tmp_path, model, dtype):
    """Under a shortlist V is Vs: the run equals, bit for bit, the twin model (the rows S of the target-side tables as a
    vocabulary of its own, tests/test_gpu_shortlist_model.py) under the same truncation, ids mapped back through S; and it
    differs from the untruncated shortlist decode."""
    from tests.common import make_hp, perturb
    from tests import rnnsearch_ref as R
    path = tmp_path / "lex.txt"
    path.write_text("\n".join(_lex_lines()) + "\n")
    table = shortlist.parse_table(_lex_lines(), SyntheticVocab(VSRC), SyntheticVocab(VT))
    hp = R.fixture_hp(Vs=VSRC, Vt=VT) if model == "rnnsearch" else make_hp(model, Vs=VSRC, Vt=VT, search_mode="cache")
    hp.scope_name = "t_sample_sl_" + model
    hp.override_from_dict(dict(shortlist_file=str(path), shortlist_first=FIRST, shortlist_best=BEST, shortlist_round=ROUND))
    st = (0, 0.3)
    plain_hp = G.beam_hp(hp, 4, dtype)
    hp = G.beam_hp(hp, 4, dtype, sampling_topk=st[0], sampling_topp=st[1])
    Pn = R.init_params(hp, 5) if model == "rnnsearch" else perturb(rt.init_params(hp, model, seed=5), np.random.default_rng(6))
    src = V.ragged((6, 4, 5), VSRC, 5)
    ids, (_, Vs) = SR.build(src, table.off, table.ids, FIRST, BEST, VT, ROUND, VT)
    Sids = ids[:Vs].astype(np.int64)
    assert len(Sids) < VT
    seqs, scores, _ = G.decode(hp, model, Pn, src)
    hp2 = copy.copy(hp)
    hp2.tgt_vocab, hp2.shortlist_file, hp2.scope_name = SyntheticVocab(len(Sids)), "", hp.scope_name + "_twin"
    Pn2 = dict(Pn)
    for name in {rt._emb_name(hp, "tgt"), rt._emb_name(hp, "softmax")}:
        Pn2[name] = np.ascontiguousarray(Pn[name][Sids])
    seqs2, scores2, _ = G.decode(hp2, model, Pn2, src)
    G.assert_tokens(seqs, Sids[seqs2])
    assert np.array_equal(scores, scores2), np.abs(scores - scores2).max()
    plain = G.decode(plain_hp, model, Pn, src)
    assert (scores[:, 0] > plain[1][:, 0]).all()


def test_too_small_a_vocabulary_is_refused():
    """V_eff < 2 * beam_size + 1: encoding_fn names the sizes before any step runs."""
    from tests.common import make_hp
    hp = make_hp("transformer", Vs=40, Vt=8, search_mode="cache", scope_name="t_sample_small")
    hp = G.beam_hp(hp, 4, "float32", sampling_topk=3)
    Pn = rt.init_params(hp, "transformer", seed=2)
    src = V.ragged((14, 5), 40, 3)
    with pytest.raises(ValueError, match=r"sampling_topk=3.*2 \* beam_size \+ 1 = 9 candidates.*only 8"):
        G.decode(hp, "transformer", Pn, src)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_step_graphs_are_reused_for_the_same_setting_only(fx, dtype):
    """A second batch of the same shape replays the first one's graphs; a run with another k, another p, or the option off, on
    the same engine adopts none of them and decodes what it decodes on a fresh engine."""
    from zero_amd import search
    model = fx["model"]
    hp = _hp(fx, 4, dtype, BOTH)
    Pn = V.sharpen(fx["hp"], fx["Pn"])
    second = V.ragged((11, 14, 7, 9), hp.src_vocab.size(), 6, width=fx["src"].shape[1])
    G.assert_graphs_reused(model, hp, Pn, fx["src"], second)
    for st in ((BOTH[0] + 1, BOTH[1]), (BOTH[0], 0.5), (0, 0.0)):
        other = _hp(fx, 4, dtype, st)
        fresh = G.decode(other, model, Pn, fx["src"])
        reset_cores(); core = get_core(hp, model, Pn)
        enc, dec = registry.get_model(model).infer_fn(hp)
        search.beam_search({"source": fx["src"]}, enc, dec, hp)
        n0 = core.__dict__.get("_graph_adoptions", 0)
        enc, dec = registry.get_model(model).infer_fn(other)
        out = search.beam_search({"source": fx["src"]}, enc, dec, other)
        assert core.__dict__.get("_graph_adoptions", 0) == n0, st
        assert np.array_equal(np.asarray(out["seq"]), fresh[0]) and np.array_equal(np.asarray(out["score"]), fresh[1]), st


def test_the_call_recorder_shows_the_order(fx, monkeypatch):
    """Eager steps (ZERO_HIP_DECODE_GRAPH=0), where every launch of a step is a recorded call, with noise, ban and truncation
    on: per step zk_ngram_ban, zk_sample_truncate, zk_add_gumbel (and its seed advance), zk_beam_topk, in that order; with the
    truncation off the noise comes first, as it always did."""
    from tests import decode_trace as DT
    from zero_amd import search
    monkeypatch.setenv("ZERO_HIP_DECODE_GRAPH", "0")
    rec = DT.Recorder(monkeypatch)
    Pn = V.sharpen(fx["hp"], fx["Pn"])
    tail = ("zk_ngram_ban", "zk_sample_truncate", "zk_add_gumbel", "zk_seed_advance", "zk_beam_topk")

    def names(hp, phase):
        reset_cores(); get_core(hp, fx["model"], Pn)
        enc, dec = registry.get_model(fx["model"]).infer_fn(hp)
        with rec.phase(phase):
            out = search.beam_search({"source": fx["src"]}, enc, dec, hp)
        return [c[0] for c in rec.phases[phase] if c[0] in tail], out["steps"]
    on, steps = names(_hp(fx, 1, "bfloat16", BOTH, no_repeat_ngram_size=3, enable_noise_beam_search=True), "on")
    assert on == list(tail) * steps and steps > 0
    off, steps = names(_hp(fx, 1, "bfloat16", (0, 0.0), no_repeat_ngram_size=3, enable_noise_beam_search=True), "off")
    assert off == ["zk_add_gumbel", "zk_seed_advance", "zk_ngram_ban", "zk_beam_topk"] * steps and steps > 0


# ---------------------------------------------------------------------------------------------- noise on: sampling
@pytest.mark.parametrize("st", [(3, 0.0), (0, 0.4), (10, 0.4)], ids=str)
def test_samples_come_from_the_kept_set(fx, st):
    """Beam 1 with the Gumbel noise: one eager decoding_fn step per time step on a fixed state, its logits copied, then
    search_tail 20 times on a fresh copy (the seed advances with every draw).  Every returned candidate with a score above -1e7
    lies in the kept set of its row by the rule on the copied logits (undecided tokens either way).  With topk = min_keep = 3
    the distinct tokens of a row over all draws number at most 3."""
    K = 1
    hp = _hp(fx, K, "float32", st, enable_noise_beam_search=True)
    reset_cores(); core = get_core(hp, fx["model"], fx["Pn"])
    e = core.eng
    enc, dec = registry.get_model(fx["model"]).infer_fn(hp)
    state = enc(fx["src"], beam_size=K, max_steps=8)
    Vt = _decode.vocab_size(state)
    B = state["B"]
    mk = S.min_keep_of(K)
    tok = torch.tensor([0, 5, 7], dtype=torch.int32)
    for time in range(3):
        state["tok"].fill_(int(tok[time]))
        logits, state = dec(state["tok"], state, time)
        torch.cuda.synchronize()
        keep = logits.t.clone()
        x = logits.torch()[:, :Vt].cpu().numpy()
        yes, no = S.Band(x).classify(st[0], S.f32(st[1]), mk)
        assert int(no.sum()) > 0
        state["prev"].zero_()
        state["stepbuf"].copy_(torch.tensor([time, int(np.float32(1.0).view(np.int32)), -1, 0], dtype=torch.int32))
        seen = [set() for _ in range(B)]
        for draw in range(20):
            logits.t.copy_(keep)
            _decode.search_tail(state, core, logits, True, 1.0, zdtype.inf(), 0, st)
            torch.cuda.synchronize()
            ts, ti = state["ts"].cpu().numpy(), state["ti"].cpu().numpy()
            for b in range(B):
                for j in range(2 * K):
                    if ts[b, j] > -1e7:
                        beam, v = divmod(int(ti[b, j]), Vt)
                        assert beam == 0 and not no[b, v], (time, draw, b, j, v, ts[b, j])
                        seen[b].add(v)
        assert all(len(s) >= 1 for s in seen)
        if st == (3, 0.0):
            assert all(len(s) <= mk for s in seen), seen
        else:
            print("%s time %d: %s distinct tokens per row over 20 draws, %s kept by the rule"
                  % (fx["model"], time, [len(s) for s in seen], list((~no).sum(1))))
    _decode.startup_end(state)
