"""no_repeat_ngram_size end to end: transformer, transformer_aan (the fused step driver) and rnnsearch (the recurrent one)
decode under the n-gram ban what the reference's search decodes with the ban of tests/ngram_ref.py (``constrained``: the ban on
the restated step's logits, the history carried in the state oracle.ref_torch.beam_search tiles and reorders).

The tiny fixtures of tests/ngram_ref.py (H = 128, vocabularies 120 / 104, sources of 14, 5, 9 and 11 tokens; seeds and what the
reference alone shows on them -- fp32 and float64 token- and order-identical, gaps > 4 x the fp32 error, every unconstrained
best hypothesis repeats an n-gram -- in that module's docstring; tests/test_ngram_host.py asserts them on the CPU, including
that the fp32 reference stays within a quarter of the project's fp32 score tolerance, rtol 1e-5 / atol 1e-6, which therefore is
the score tolerance here).  n = 2 and 3, beam 1 and 4.
"""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_torch as rt  # noqa: E402
from tests import ensemble_common as ec  # noqa: E402
from tests import ngram_ref as N  # noqa: E402
from tests import shortlist_ref as SR  # noqa: E402
from tests import variant_gpu as G  # noqa: E402
from tests import variant_ref as V  # noqa: E402
from zero_amd import shortlist  # noqa: E402
from zero_amd.config import SyntheticVocab  # noqa: E402
from zero_amd.models import load_all, model as registry  # noqa: E402
from zero_amd.models._factory import get_core, reset_cores  # noqa: E402

load_all()
TOL = (N.RTOL, N.ATOL)


@pytest.fixture(scope="module", params=["transformer", "transformer_aan", "rnnsearch"])
def fx(request):
    model = request.param
    hp, src = N.fixture(model)
    Pn = N.MODELS[model]["init"](hp, N.SEEDS[model])
    refs = {}

    def ref(n, K, sharp=False):
        """The constrained fp32 reference; computed once per key and left unchanged."""
        if (n, K, sharp) not in refs:
            refs[(n, K, sharp)] = V.search(N.constrained(N.MODELS[model]["fns"], n), hp, V.sharpen(hp, Pn) if sharp else Pn,
                                           src, K, torch.float32)[0]
        return refs[(n, K, sharp)]
    return dict(model=model, hp=hp, src=src, Pn=Pn, ref=ref)


def _no_repeats(seqs, hp, n):
    """The property the option guarantees, with no reference: no hypothesis of any beam holds an n-gram twice."""
    for b in range(seqs.shape[0]):
        for k in range(seqs.shape[1]):
            hyp = N.hypothesis(seqs[b, k], hp)
            assert not N.has_repeat(hyp, n), (b, k, hyp)


def _hp(f, K, dtype, n):
    return G.beam_hp(f["hp"], K, dtype, no_repeat_ngram_size=n)


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("n", [2, 3])
def test_fp32_mode_is_token_exact(fx, n, K):
    ref = fx["ref"](n, K)
    seqs, scores, core = G.decode(_hp(fx, K, "float32", n), fx["model"], fx["Pn"], fx["src"])
    G.assert_tokens(seqs, ref["seq"])
    fin = ref["score"] > -1e30
    print("%s n=%d K=%d: largest score difference %.3e" % (fx["model"], n, K, np.abs(scores - ref["score"])[fin].max()))
    assert np.allclose(scores[fin], ref["score"][fin], rtol=TOL[0], atol=TOL[1]), np.abs(scores - ref["score"])[fin].max()
    _no_repeats(seqs, fx["hp"], n)
    assert core.__dict__.get("_decode_step_launches", 0) > 0           # the step ran from captured graphs


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("n", [2, 3])
def test_bf16_mode_best_hypotheses(fx, n, K):
    """Output distribution sharpened x 6: the best hypothesis of every sentence against the constrained fp32 reference."""
    from zero_amd.search import decode_hypothesis
    ref = fx["ref"](n, K, sharp=True)
    hp = _hp(fx, K, "bfloat16", n)
    seqs, scores, core = G.decode(hp, fx["model"], V.sharpen(fx["hp"], fx["Pn"]), fx["src"])
    hyp, hyp_ref = decode_hypothesis(seqs, hp), rt.decode_hypothesis(ref["seq"], hp)
    assert hyp == hyp_ref, (hyp, hyp_ref)
    _no_repeats(seqs, fx["hp"], n)
    assert core.__dict__.get("_decode_step_launches", 0) > 0


def test_the_unconstrained_decode_repeats(fx):
    """What the option is for: without it the best hypothesis of some sentence holds a 2-gram twice (fp32, beam 4)."""
    seqs, _, _ = G.decode(G.beam_hp(fx["hp"], 4, "float32"), fx["model"], fx["Pn"], fx["src"])
    assert any(N.has_repeat(N.hypothesis(seqs[b, 0], fx["hp"]), 2) for b in range(seqs.shape[0]))


ROUTES = {"host_book": {"ZERO_HIP_DECODE_DEVICE_BOOK": "0"}, "numpy_book": {"ZERO_HIP_DECODE_HOST_C": "0"},
          "eager": {"ZERO_HIP_DECODE_GRAPH": "0"}}


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_the_other_search_modes_equal_the_device_resident_one(fx, monkeypatch, route, dtype):
    """The three history sources: the device-resident book's seq, the buffer the host refreshes before a replayed step (from
    the C bookkeeping's pinned sequences, or from the numpy loop's), and the same buffer with the time by value on eager
    steps.  Steps, tokens and scores are the device-resident search's, bit for bit (n = 3, beam 4)."""
    hp = _hp(fx, 4, dtype, 3)
    Pn = fx["Pn"] if dtype == "float32" else V.sharpen(fx["hp"], fx["Pn"])
    base = G.decode(hp, fx["model"], Pn, fx["src"])
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    seqs, scores, core = G.decode(hp, fx["model"], Pn, fx["src"])
    assert (core.__dict__.get("_decode_step_launches", 0) > 0) == (route != "eager")
    G.assert_tokens(seqs, base[0])
    assert np.array_equal(scores, base[1]), np.abs(scores - base[1]).max()


def test_search_mode_dev_bans_too():
    """search_mode=dev (the whole prefix through the training-path decoder each step; bf16): the eager ban on its logits.
    No hypothesis repeats a 2-gram, and the run differs from the unconstrained one."""
    hp, src = N.fixture("transformer")
    Pn = V.sharpen(hp, N.MODELS["transformer"]["init"](hp, N.SEEDS["transformer"]))
    out = []
    for n in (0, 2):
        h = G.beam_hp(hp, 4, "bfloat16", no_repeat_ngram_size=n)
        h.search_mode = "dev"
        out.append(G.decode(h, "transformer", Pn, src)[0])
    _no_repeats(out[1], hp, 2)
    assert any(N.has_repeat(N.hypothesis(out[0][b, 0], hp), 2) for b in range(src.shape[0]))


def test_four_lanes_equal_one_lane(fx):
    """Six batches through decode_many on one lane and on four (bf16, sharpened, n = 3): identical, and free of repeats."""
    from zero_amd.evalu import decode_many
    hp = _hp(fx, 4, "bfloat16", 3)
    reset_cores(); get_core(hp, fx["model"], V.sharpen(fx["hp"], fx["Pn"]))
    batches = [V.ragged(tuple(int(x) for x in np.random.default_rng(i).integers(5, 15, 3 + i % 2)), hp.src_vocab.size(), 10 + i)
               for i in range(6)]
    work = G.lane_worker(fx["model"], hp)
    one = decode_many(batches, work, streams=1)
    four = decode_many(batches, work, streams=4)
    for i, (a, b) in enumerate(zip(one, four)):
        assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), i
        _no_repeats(a[0], fx["hp"], 3)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_step_graphs_are_reused_for_the_same_n_only(fx, dtype):
    """A second batch of the same shape replays the first one's graphs (variant_gpu.assert_graphs_reused); a run with another
    n, or with the option off, on the same engine adopts none of them and decodes what it decodes on a fresh engine."""
    from zero_amd import search
    model = fx["model"]
    hp = _hp(fx, 4, dtype, 3)
    Pn = V.sharpen(fx["hp"], fx["Pn"])
    second = V.ragged((11, 14, 7, 9), hp.src_vocab.size(), 6, width=fx["src"].shape[1])
    G.assert_graphs_reused(model, hp, Pn, fx["src"], second)
    for n in (2, 0):
        other = _hp(fx, 4, dtype, n)
        fresh = G.decode(other, model, Pn, fx["src"])
        reset_cores(); core = get_core(hp, model, Pn)
        enc, dec = registry.get_model(model).infer_fn(hp)
        search.beam_search({"source": fx["src"]}, enc, dec, hp)
        n0 = core.__dict__.get("_graph_adoptions", 0)
        enc, dec = registry.get_model(model).infer_fn(other)
        out = search.beam_search({"source": fx["src"]}, enc, dec, other)
        assert core.__dict__.get("_graph_adoptions", 0) == n0, n
        assert np.array_equal(np.asarray(out["seq"]), fresh[0]) and np.array_equal(np.asarray(out["score"]), fresh[1]), n
        if n:
            _no_repeats(np.asarray(out["seq"]), fx["hp"], n)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_n_0_is_the_decode_without_the_hparam(fx, dtype):
    """no_repeat_ngram_size = 0 against hparams that do not have the key at all: tokens and scores bit-equal, and the same
    number of launches in the captured step; n = 3 adds exactly one."""
    Pn = V.sharpen(fx["hp"], fx["Pn"])
    bare = G.beam_hp(fx["hp"], 4, dtype)
    bare.del_hparam("no_repeat_ngram_size")
    assert not hasattr(bare, "no_repeat_ngram_size")
    a = G.decode(bare, fx["model"], Pn, fx["src"])
    la = a[2].__dict__["_decode_step_launches"]
    b = G.decode(_hp(fx, 4, dtype, 0), fx["model"], Pn, fx["src"])
    lb = b[2].__dict__["_decode_step_launches"]
    c = G.decode(_hp(fx, 4, dtype, 3), fx["model"], Pn, fx["src"])
    lc = c[2].__dict__["_decode_step_launches"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert la == lb and lc == lb + 1, (la, lb, lc)


def _recorded(hp, model, Pn, src, rec):
    """The names of every library call of one eager decode (each step issues its launches), by tests/decode_trace.Recorder."""
    from zero_amd import search
    reset_cores(); get_core(hp, model, Pn)
    enc, dec = registry.get_model(model).infer_fn(hp)
    with rec.phase("search"):
        out = search.beam_search({"source": src}, enc, dec, hp)
    return [c[0] for c in rec.phases["search"]], out["steps"]


def test_the_call_recorder_shows_one_launch_more_per_step(fx, monkeypatch):
    """Eager steps (ZERO_HIP_DECODE_GRAPH=0), where every launch of a step is a recorded call: with the option on there is one
    zk_ngram_ban per step, directly ahead of the step's zk_beam_topk, and without those calls the sequence of entry points is
    the one of the run with the option off, which holds no such call.  (On captured steps test_n_0_... counts the nodes.)"""
    from tests import decode_trace as DT
    monkeypatch.setenv("ZERO_HIP_DECODE_GRAPH", "0")
    rec = DT.Recorder(monkeypatch)
    Pn = V.sharpen(fx["hp"], fx["Pn"])
    off, steps0 = _recorded(_hp(fx, 4, "bfloat16", 0), fx["model"], Pn, fx["src"], rec)
    on, steps = _recorded(_hp(fx, 4, "bfloat16", 3), fx["model"], Pn, fx["src"], rec)
    assert "zk_ngram_ban" not in off and off.count("zk_beam_topk") == steps0
    assert on.count("zk_ngram_ban") == steps == on.count("zk_beam_topk")
    assert all(on[i + 1] == "zk_beam_topk" for i, x in enumerate(on) if x == "zk_ngram_ban")
    rest = [x for x in on if x != "zk_ngram_ban"]
    m = min(len(rest), len(off))
    assert rest[:m] == off[:m] and m > 0.5 * len(off)


def test_two_member_ensemble():
    """transformer + transformer_aan, fp32, beam 4, n = 3: the ban on the combined log-probabilities, against the composed
    oracle under the same ban; every search route gives the same result."""
    from zero_amd import search
    from zero_amd.models._ensemble import make_infer_fns, member_params
    models = ("transformer", "transformer_aan")
    hps, Pns, src = ec.make_members(models, (3, 4))
    hps = ec.with_beam(hps, 4, decode_dtype="float32", no_repeat_ngram_size=3)
    fns = N.constrained(lambda hp, P: ec.composed_infer_fn(hps, Pns, models), 3)
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
    fin = ref["score"] > -1e30
    assert np.allclose(scores[fin], ref["score"][fin], rtol=1e-5, atol=1e-6), np.abs(scores - ref["score"])[fin].max()
    _no_repeats(seqs, hps[0], 3)


# ---------------------------------------------------------------------------------------------- shortlist
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
    """Under a shortlist the history and the logits are both in shortlist ids: the run equals, bit for bit, the twin model
    (the rows S of the target-side tables as a vocabulary of its own, tests/test_gpu_shortlist_model.py) under the same ban,
    ids mapped back through S; no hypothesis repeats a 3-gram."""
    from tests.common import make_hp, perturb
    from tests import rnnsearch_ref as R
    path = tmp_path / "lex.txt"
    path.write_text("\n".join(_lex_lines()) + "\n")
    table = shortlist.parse_table(_lex_lines(), SyntheticVocab(VSRC), SyntheticVocab(VT))
    hp = R.fixture_hp(Vs=VSRC, Vt=VT) if model == "rnnsearch" else make_hp(model, Vs=VSRC, Vt=VT, search_mode="cache")
    hp.scope_name = "t_ngram_sl_" + model
    hp.override_from_dict(dict(shortlist_file=str(path), shortlist_first=FIRST, shortlist_best=BEST, shortlist_round=ROUND))
    hp = G.beam_hp(hp, 4, dtype, no_repeat_ngram_size=3)
    Pn = R.init_params(hp, 5) if model == "rnnsearch" else perturb(rt.init_params(hp, model, seed=5), np.random.default_rng(6))
    src = V.ragged((6, 4, 5), VSRC, 5)
    ids, (_, Vs) = SR.build(src, table.off, table.ids, FIRST, BEST, VT, ROUND, VT)
    S = ids[:Vs].astype(np.int64)
    assert len(S) < VT
    seqs, scores, _ = G.decode(hp, model, Pn, src)
    hp2 = copy.copy(hp)
    hp2.tgt_vocab, hp2.shortlist_file, hp2.scope_name = SyntheticVocab(len(S)), "", hp.scope_name + "_twin"
    Pn2 = dict(Pn)
    for name in {rt._emb_name(hp, "tgt"), rt._emb_name(hp, "softmax")}:
        Pn2[name] = np.ascontiguousarray(Pn[name][S])
    seqs2, scores2, _ = G.decode(hp2, model, Pn2, src)
    G.assert_tokens(seqs, S[seqs2])
    assert np.array_equal(scores, scores2), np.abs(scores - scores2).max()
    _no_repeats(seqs, hp, 3)


def test_too_small_a_vocabulary_is_refused():
    """V - Tmax < 2 * beam_size: encoding_fn names the three sizes before any step runs."""
    from tests.common import make_hp
    hp = make_hp("transformer", Vs=40, Vt=30, search_mode="cache", scope_name="t_ngram_small")
    hp = G.beam_hp(hp, 4, "float32", no_repeat_ngram_size=2)
    Pn = rt.init_params(hp, "transformer", seed=2)
    src = V.ragged((14, 5), 40, 3)
    with pytest.raises(ValueError, match=r"no_repeat_ngram_size=2.*24 tokens.*= 8 of the 30 candidates"):
        G.decode(hp, "transformer", Pn, src)
    hp.no_repeat_ngram_size = 0
    seqs, scores, _ = G.decode(hp, "transformer", Pn, src)
    assert np.isfinite(scores[:, 0]).all()


def test_cli_mode_test(tmp_path):
    """`run.py --mode test` with no_repeat_ngram_size=3 in a fresh interpreter, both decode modes: one translation per source
    line and none of them holds a 3-gram twice.  (variant_gpu.cli_mode_test's files with a vocabulary of 40 words instead of
    12: with 12 the option refuses the run, 15 candidates - 16 cache positions < 2 * beam_size.)"""
    rng = np.random.default_rng(3)
    words = ["w%d" % i for i in range(40)]
    (tmp_path / "vocab.txt").write_text("\n".join(words) + "\n")
    lines = [" ".join(rng.choice(words, size=int(rng.integers(2, 7)))) for _ in range(8)]
    for name in ("test.src", "test.tgt"):
        (tmp_path / name).write_text("\n".join(lines) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    common = "model_name=transformer,scope_name=transformer,hidden_size=64,embed_size=64,filter_size=128,num_heads=1," \
        "num_encoder_layer=1,num_decoder_layer=1,no_repeat_ngram_size=3,eval_batch_size=3,beam_size=2,decode_length=4," \
        "initializer=uniform_unit_scaling,initializer_gain=1.0,output_dir=%s," % (tmp_path / "out") + \
        ",".join("%s=%s" % (k, tmp_path / v) for k, v in dict(
            src_vocab_file="vocab.txt", tgt_vocab_file="vocab.txt", src_test_file="test.src", tgt_test_file="test.tgt").items())
    for dtype in ("bfloat16", "float32"):
        out = tmp_path / ("t_%s.txt" % dtype)
        r = subprocess.run([sys.executable, "-m", "zero_amd.run", "--mode", "test", "--parameters",
                            common + ",decode_dtype=%s,test_output=%s" % (dtype, out)],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "bleu" in r.stdout
        hyps = out.read_text().splitlines()
        assert len(hyps) == 8
        for h in hyps:
            assert not N.has_repeat(h.split(), 3), h
