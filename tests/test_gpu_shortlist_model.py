"""Lexical shortlist decoding end to end (zero_amd/shortlist.py) on tiny models: target vocabulary 41, shortlist_first 5,
shortlist_best 2, shortlist_round 8, three short sentences -- the batch's shortlist is 24 of the 41 ids.

The definition the tests hold: decoding with shortlist S is decoding with the model whose target-side tables are restricted
to the rows S (a TWIN model with a target vocabulary of Vs ids and no shortlist), followed by mapping every id i to S[i].
S comes from the numpy reference (tests/shortlist_ref.py) over the table the CPU-tested loader parsed.

Twin         tokens equal on every beam, scores BIT-equal: the twin's step launches the same kernels on operands of the same
             shapes (tables of pad8(Vs) rows, logits with the leading dimension pad8(Vs)) holding the same values.
Full cover   shortlist_first = V: S is the whole vocabulary in order; hypotheses and scores bit-equal to shortlist off.
Oracle       transformer in fp32 against oracle.ref_torch on the restricted parameters (variant_gpu.assert_exact).
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_torch as rt  # noqa: E402
from tests import rnnsearch_ref as R  # noqa: E402
from tests import shortlist_ref as SR  # noqa: E402
from tests import variant_gpu as G  # noqa: E402
from tests import variant_ref as V  # noqa: E402
from tests.common import make_hp, perturb  # noqa: E402
from zero_amd import shortlist  # noqa: E402
from zero_amd.config import SyntheticVocab  # noqa: E402
from zero_amd.models import load_all  # noqa: E402
from zero_amd.models._factory import get_core, reset_cores  # noqa: E402

load_all()
MODELS = ["transformer", "transformer_aan", "transformer_rpr", "transformer_fuse", "rnnsearch"]
VSRC, VT = 36, 41
FIRST, BEST, ROUND = 5, 2, 8
LENGTHS = (6, 4, 5)


def _lines():
    """Four translations per source id 3 .. VSRC - 1 with falling probability (only the best two count), drawn from the
    ids the `first` rule does not cover; source id 7 translates to low ids only."""
    rng = np.random.default_rng(11)
    out = []
    for s in range(3, VSRC):
        tgt = rng.choice(np.arange(FIRST, VT), 4, replace=False)
        if s == 7:
            tgt = np.array([3, 4, 9, 10])
        out += ["%d %d %.3f" % (t, s, 0.9 - 0.2 * i) for i, t in enumerate(tgt)]
    return out


@pytest.fixture(scope="module")
def lex(tmp_path_factory):
    path = tmp_path_factory.mktemp("shortlist") / "lex.txt"
    path.write_text("\n".join(_lines()) + "\n")
    table = shortlist.parse_table(_lines(), SyntheticVocab(VSRC), SyntheticVocab(VT))
    return str(path), table


def _hp(model, lex, name="", **kw):
    if model == "rnnsearch":
        hp = R.fixture_hp(Vs=VSRC, Vt=VT)
        hp.override_from_dict(kw)
    else:
        hp = make_hp(model, Vs=VSRC, Vt=VT, search_mode="cache", **kw)
    hp.scope_name = "t_sl_%s%s" % (model, name)
    hp.override_from_dict(dict(shortlist_file=lex[0], shortlist_first=FIRST, shortlist_best=BEST, shortlist_round=ROUND))
    if hp.shared_source_target_embedding:
        hp.src_vocab = hp.tgt_vocab
    return hp


def _params(hp, model, seed=5):
    if model == "rnnsearch":
        return R.init_params(hp, seed)
    return perturb(rt.init_params(hp, model, seed=seed), np.random.default_rng(seed + 1))


def _src(seed=5, lengths=LENGTHS, width=None):
    return V.ragged(lengths, VSRC, seed, width=width)


def _S(lex, src, V_=VT, first=FIRST):
    ids, (n, Vs) = SR.build(src, lex[1].off, lex[1].ids, first, BEST, V_, ROUND, V_)
    return ids[:Vs].astype(np.int64)


def _twin(hp, Pn, S):
    """The model restricted to the rows S of its target-side tables: a target vocabulary of len(S) ids, no shortlist."""
    hp2 = copy.copy(hp)
    hp2.tgt_vocab = SyntheticVocab(len(S))
    hp2.shortlist_file = ""
    hp2.scope_name = hp.scope_name + "_twin"
    Pn2 = dict(Pn)
    for name in {rt._emb_name(hp, "tgt"), rt._emb_name(hp, "softmax")}:
        Pn2[name] = np.ascontiguousarray(Pn[name][S])
    return hp2, Pn2


def test_the_fixture_drops_about_half_the_vocabulary(lex):
    S = _S(lex, _src())
    assert len(S) == 24 and (S[:FIRST] == np.arange(FIRST)).all() and S[-1] > 24


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("model", MODELS)
def test_twin(lex, model, dtype, K):
    hp = G.beam_hp(_hp(model, lex), K, dtype)
    assert not hp.shared_source_target_embedding
    Pn, src = _params(hp, model), _src()
    S = _S(lex, src)
    seqs, scores, core = G.decode(hp, model, Pn, src)
    hp2, Pn2 = _twin(hp, Pn, S)
    seqs2, scores2, _ = G.decode(hp2, model, Pn2, src)
    assert seqs2.max() < len(S)
    G.assert_tokens(seqs, S[seqs2])
    assert np.isin(seqs, S).all()                        # every returned id is a member of S
    assert np.array_equal(scores, scores2), np.abs(scores - scores2).max()


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("model, kw", [("transformer", {}), ("transformer", {"shared_source_target_embedding": True}),
                                        ("transformer", {"shared_target_softmax_embedding": False}),
                                        ("transformer_aan", {"shared_target_softmax_embedding": False}),
                                        ("rnnsearch", {"shared_target_softmax_embedding": False}),
                                        ("rnnsearch", {"shared_source_target_embedding": True})],
                         ids=["plain", "shared_src_tgt", "own_softmax", "aan_own_softmax", "rnn_own_softmax", "rnn_shared"])
def test_full_cover_equals_shortlist_off(lex, model, kw, dtype):
    hp = G.beam_hp(_hp(model, lex, **kw), 4, dtype, shortlist_first=VT)
    Pn, src = _params(hp, model), _src()
    seqs, scores, _ = G.decode(hp, model, Pn, src)
    off = G.beam_hp(hp, 4, dtype, shortlist_file="")
    seqs0, scores0, _ = G.decode(off, model, Pn, src)
    assert np.array_equal(seqs, seqs0) and np.array_equal(scores, scores0)


@pytest.mark.parametrize("K", [1, 4])
def test_fp32_transformer_against_the_oracle_on_the_restricted_parameters(lex, K):
    model = "transformer"
    hp = G.beam_hp(_hp(model, lex), K, "float32")
    Pn, src = _params(hp, model), _src()
    S = _S(lex, src)
    hp2, Pn2 = _twin(hp, Pn, S)
    enc, dec = rt.infer_fn(hp2, rt.to_torch(Pn2), model)
    ref = rt.beam_search({"source": torch.tensor(src)}, enc, dec, hp2)
    ref = dict(ref, seq=S[ref["seq"]])
    seqs, scores, _ = G.decode(hp, model, Pn, src)
    G.assert_exact(seqs, scores, ref)


def test_source_padding_changes_nothing(lex, monkeypatch):
    hp = G.beam_hp(_hp("transformer", lex), 4, "float32")
    G.assert_padding_changes_nothing("transformer", hp, _params(hp, "transformer"), _src(), monkeypatch)


@pytest.mark.parametrize("model, dtype", [("transformer", "bfloat16"), ("transformer_aan", "float32"), ("rnnsearch", "bfloat16")])
def test_step_graphs_are_reused_across_shortlists_of_one_size(lex, model, dtype):
    """Two batches of one shape whose shortlists have the same size and different content: the second replays the first
    one's graphs (the tables' addresses and Vs are the same) and decodes what it decodes on a fresh engine."""
    hp = G.beam_hp(_hp(model, lex), 4, dtype)
    first, second = _src(), _src(6, (5, 6, 4))
    Sa, Sb = _S(lex, first), _S(lex, second)
    assert len(Sa) == len(Sb) and not np.array_equal(Sa, Sb)
    G.assert_graphs_reused(model, hp, _params(hp, model), first, second)


def test_two_shortlist_sizes_give_two_graph_sets(lex):
    from zero_amd import search
    from zero_amd.models import model as registry
    model = "transformer"
    hp = G.beam_hp(_hp(model, lex), 4, "bfloat16")
    big = _src()
    small = np.where(big > 2, 7, big)            # every word is source id 7, whose translations are low ids: a shortlist of 8
    assert len(_S(lex, small)) == 8 and len(_S(lex, big)) == 24
    reset_cores(); core = get_core(hp, model, _params(hp, model))

    def run(src):
        enc, dec = registry.get_model(model).infer_fn(hp)
        return search.beam_search({"source": src}, enc, dec, hp)
    a, b = run(big), run(small)
    assert core.__dict__.get("_graph_adoptions", 0) == 0
    keys = list(core._step_graph_cache)
    assert len(keys) == 2 and keys[0][:-1] == keys[1][:-1] and {k[-1] for k in keys} == {("shortlist", 24), ("shortlist", 8)}
    assert np.isin(b["seq"], _S(lex, small)).all() and np.isin(a["seq"], _S(lex, big)).all()
    c = run(big)
    assert core._graph_adoptions == 1 and np.array_equal(c["seq"], a["seq"]) and np.array_equal(c["score"], a["score"])


@pytest.mark.parametrize("model", ["transformer", "rnnsearch"])
def test_four_lanes_equal_one_lane(lex, model):
    from zero_amd.evalu import decode_many
    hp = G.beam_hp(_hp(model, lex), 4, "bfloat16")
    reset_cores(); get_core(hp, model, _params(hp, model))
    batches = [_src(10 + i, tuple(int(x) for x in np.random.default_rng(i).integers(3, 8, 3 + i % 2))) for i in range(6)]
    work = G.lane_worker(model, hp)
    one = decode_many(batches, work, streams=1)
    four = decode_many(batches, work, streams=4)
    for i, (a, b) in enumerate(zip(one, four)):
        assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), i
        assert np.isin(a[0], _S(lex, batches[i])).all()


@pytest.mark.parametrize("model", ["transformer", "rnnsearch"])
@pytest.mark.parametrize("mode", ["eager", "host_book"])
def test_the_other_bookkeeping_paths_map_back_too(lex, monkeypatch, model, mode):
    """ZERO_HIP_DECODE_GRAPH=0 (numpy bookkeeping, one step at a time) and ZERO_HIP_DECODE_DEVICE_BOOK=0 (graph step, host
    C bookkeeping) decode what the device-resident search decodes."""
    hp = G.beam_hp(_hp(model, lex), 4, "float32")
    Pn, src = _params(hp, model), _src()
    base = G.decode(hp, model, Pn, src)
    monkeypatch.setenv("ZERO_HIP_DECODE_GRAPH" if mode == "eager" else "ZERO_HIP_DECODE_DEVICE_BOOK", "0")
    seqs, scores, _ = G.decode(hp, model, Pn, src)
    G.assert_tokens(seqs, base[0])
    fin = base[1] > -1e30
    assert np.allclose(scores[fin], base[1][fin], rtol=1e-5, atol=1e-6)
    assert np.isin(seqs, _S(lex, src)).all()


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_noise_beam_search_stays_inside_the_shortlist(lex, dtype):
    hp = G.beam_hp(_hp("transformer", lex), 4, dtype, enable_noise_beam_search=True)
    src = _src()
    seqs, scores, _ = G.decode(hp, "transformer", _params(hp, "transformer"), src)
    assert np.isin(seqs, _S(lex, src)).all() and np.isfinite(scores[scores > -1e30]).all()
    assert (seqs != 0).any()
