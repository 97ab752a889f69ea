"""tgt_prefix_file end to end: transformer, transformer_aan (the fused step driver) and rnnsearch (the recurrent one) decode
under forced prefixes what the reference's search decodes with the rule of tests/prefix_ref.py (``constrained``: the rule on the
restated step's logits).

The tiny fixtures of tests/prefix_ref.py (ngram_ref's models, H = 128, vocabularies 120 / 104, sources of 14, 5, 9 and 11 tokens,
prefixes of 0, 1, 3 and 2 tokens; seeds and what the reference alone shows on them -- fp32 and float64 identical on every beam,
free gaps > 4 x the fp32 error, forced steps adding exactly 0 -- in that module's docstring; tests/test_prefix_checker.py asserts
them on the CPU, including that the fp32 reference stays within a quarter of the project's fp32 score tolerance, rtol 1e-5 /
atol 1e-6, which therefore is the score tolerance here: forced steps add no rounding).  Beam 1 and 4.
"""
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
from tests import prefix_ref as PR  # noqa: E402
from tests import variant_gpu as G  # noqa: E402
from tests import variant_ref as V  # noqa: E402
from zero_amd.models import load_all, model as registry  # noqa: E402
from zero_amd.models._factory import get_core, reset_cores  # noqa: E402

load_all()
TOL = (PR.RTOL, PR.ATOL)


def _search(hp, model, src, prefix):
    """One search on the present cores -> (seqs, scores, steps)."""
    from zero_amd import search
    enc, dec = registry.get_model(model).infer_fn(hp)
    feats = {"source": src}
    if prefix is not None:
        feats["prefix"] = prefix
    out = search.beam_search(feats, enc, dec, hp)
    return np.asarray(out["seq"]).copy(), np.asarray(out["score"]).copy(), out["steps"]


def _decode(hp, model, Pn, src, prefix):
    """-> (seqs, scores, core) on a fresh core holding Pn."""
    reset_cores()
    core = get_core(hp, model, Pn)
    seqs, scores, _ = _search(hp, model, src, prefix)
    return seqs, scores, core


@pytest.fixture(scope="module", params=["transformer", "transformer_aan", "rnnsearch"])
def fx(request):
    model = request.param
    hp, src, prefix = PR.fixture(model)
    Pn = PR.MODELS[model]["init"](hp, PR.SEEDS[model])
    refs = {}

    def ref(K, sharp=False):
        """The constrained fp32 reference; computed once per key and left unchanged."""
        if (K, sharp) not in refs:
            refs[(K, sharp)] = V.search(PR.constrained(PR.MODELS[model]["fns"], prefix, K), hp,
                                        V.sharpen(hp, Pn) if sharp else Pn, src, K, torch.float32)[0]
        return refs[(K, sharp)]
    return dict(model=model, hp=hp, src=src, prefix=prefix, Pn=Pn, ref=ref)


def _holds(seqs, scores, prefix, hp):
    """The properties the option guarantees, with no reference: every hypothesis of every beam starts with its prefix, none
    ends inside it, and none scores like a filler."""
    for b in range(seqs.shape[0]):
        for k in range(seqs.shape[1]):
            if scores[b, k] > -1e30:
                assert scores[b, k] > PR.REAL, (b, k, scores[b, k])
                assert PR.starts_with(seqs[b, k], prefix[b], hp), (b, k, seqs[b, k], prefix[b])
                assert not PR.ends_inside(seqs[b, k], prefix[b], hp), (b, k)


@pytest.mark.parametrize("K", [1, 4])
def test_fp32_mode_is_token_exact(fx, K):
    ref = fx["ref"](K)
    seqs, scores, core = _decode(G.beam_hp(fx["hp"], K, "float32"), fx["model"], fx["Pn"], fx["src"], fx["prefix"])
    G.assert_tokens(seqs, ref["seq"])
    fin = ref["score"] > -1e30
    print("%s K=%d: largest score difference %.3e" % (fx["model"], K, np.abs(scores - ref["score"])[fin].max()))
    assert np.allclose(scores[fin], ref["score"][fin], rtol=TOL[0], atol=TOL[1]), np.abs(scores - ref["score"])[fin].max()
    _holds(seqs, scores, fx["prefix"], fx["hp"])
    assert core.__dict__.get("_decode_step_launches", 0) > 0           # the step ran from captured graphs


@pytest.mark.parametrize("K", [1, 4])
def test_bf16_mode_best_hypotheses(fx, K):
    """Output distribution sharpened x 6: the best hypothesis of every sentence against the constrained fp32 reference."""
    from zero_amd.search import decode_hypothesis
    ref = fx["ref"](K, sharp=True)
    hp = G.beam_hp(fx["hp"], K, "bfloat16")
    seqs, scores, core = _decode(hp, fx["model"], V.sharpen(fx["hp"], fx["Pn"]), fx["src"], fx["prefix"])
    hyp, hyp_ref = decode_hypothesis(seqs, hp), rt.decode_hypothesis(ref["seq"], hp)
    assert hyp == hyp_ref, (hyp, hyp_ref)
    _holds(seqs, scores, fx["prefix"], fx["hp"])
    assert core.__dict__.get("_decode_step_launches", 0) > 0


def test_the_unconstrained_decode_does_not_start_with_the_prefix(fx):
    seqs, _, _ = _decode(G.beam_hp(fx["hp"], 4, "float32"), fx["model"], fx["Pn"], fx["src"], None)
    for b in range(seqs.shape[0]):
        if fx["prefix"][b].any():
            assert not PR.starts_with(seqs[b, 0], fx["prefix"][b], fx["hp"]), b


ROUTES = {"host_book": {"ZERO_HIP_DECODE_DEVICE_BOOK": "0"}, "numpy_book": {"ZERO_HIP_DECODE_HOST_C": "0"},
          "eager": {"ZERO_HIP_DECODE_GRAPH": "0"}}


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_the_other_search_modes_equal_the_device_resident_one(fx, monkeypatch, route, dtype):
    """The replayed step with the host's C or numpy bookkeeping (the force node reads the time word) and the eager steps (the
    time by value): steps, tokens and scores are the device-resident search's, bit for bit (beam 4)."""
    hp = G.beam_hp(fx["hp"], 4, dtype)
    Pn = fx["Pn"] if dtype == "float32" else V.sharpen(fx["hp"], fx["Pn"])
    base = _decode(hp, fx["model"], Pn, fx["src"], fx["prefix"])
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    seqs, scores, core = _decode(hp, fx["model"], Pn, fx["src"], fx["prefix"])
    assert (core.__dict__.get("_decode_step_launches", 0) > 0) == (route != "eager")
    G.assert_tokens(seqs, base[0])
    assert np.array_equal(scores, base[1]), np.abs(scores - base[1]).max()


def test_search_mode_dev_forces_too():
    """search_mode=dev (the whole prefix through the training-path decoder each step; bf16): the eager force on its logits."""
    hp, src, prefix = PR.fixture("transformer")
    Pn = V.sharpen(hp, PR.MODELS["transformer"]["init"](hp, PR.SEEDS["transformer"]))
    h = G.beam_hp(hp, 4, "bfloat16")
    h.search_mode = "dev"
    seqs, scores, _ = _decode(h, "transformer", Pn, src, prefix)
    _holds(seqs, scores, prefix, hp)
    plain, _, _ = _decode(h, "transformer", Pn, src, None)
    assert any(not PR.starts_with(plain[b, 0], prefix[b], hp) for b in range(src.shape[0]))


def test_four_lanes_equal_one_lane(fx):
    """Six batches with prefixes through decode_many on one lane and on four (bf16, sharpened): identical."""
    from zero_amd.evalu import decode_many
    hp = G.beam_hp(fx["hp"], 4, "bfloat16")
    reset_cores(); get_core(hp, fx["model"], V.sharpen(fx["hp"], fx["Pn"]))
    batches = []
    for i in range(6):
        lens = tuple(int(x) for x in np.random.default_rng(i).integers(5, 15, 3 + i % 2))
        batches.append((V.ragged(lens, hp.src_vocab.size(), 10 + i),
                        PR.prefixes(hp.tgt_vocab.size(), tuple((i + j) % 4 for j in range(len(lens))), seed=20 + i)))
    import threading
    tl = threading.local()

    def work(item):
        from zero_amd.search import beam_search
        if not hasattr(tl, "fns"):
            tl.fns = registry.get_model(fx["model"]).infer_fn(hp)
        out = beam_search({"source": item[0], "prefix": item[1]}, tl.fns[0], tl.fns[1], hp)
        return np.asarray(out["seq"]).copy(), np.asarray(out["score"]).copy(), out["steps"]
    one = decode_many(batches, work, streams=1)
    four = decode_many(batches, work, streams=4)
    for i, (a, b) in enumerate(zip(one, four)):
        assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), i
        _holds(a[0], a[1], batches[i][1], fx["hp"])


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_empty_prefixes_are_the_decode_without_the_feature(fx, dtype):
    """A table of zeros against features without the key: tokens and scores bit-equal, and the same number of launches in the
    captured step; a table with prefixes adds exactly one."""
    Pn = V.sharpen(fx["hp"], fx["Pn"])
    hp = G.beam_hp(fx["hp"], 4, dtype)
    a = _decode(hp, fx["model"], Pn, fx["src"], None)
    la = a[2].__dict__["_decode_step_launches"]
    b = _decode(hp, fx["model"], Pn, fx["src"], np.zeros_like(fx["prefix"]))
    lb = b[2].__dict__["_decode_step_launches"]
    c = _decode(hp, fx["model"], Pn, fx["src"], fx["prefix"])
    lc = c[2].__dict__["_decode_step_launches"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert la == lb and lc == lb + 1, (la, lb, lc)
    bare = G.beam_hp(fx["hp"], 4, dtype)
    bare.del_hparam("tgt_prefix_file")
    d = _decode(bare, fx["model"], Pn, fx["src"], None)
    assert np.array_equal(a[0], d[0]) and np.array_equal(a[1], d[1]) and d[2].__dict__["_decode_step_launches"] == la


def _recorded(hp, model, Pn, src, prefix, rec):
    """The names of every library call of one eager decode (each step issues its launches), by tests/decode_trace.Recorder."""
    reset_cores(); get_core(hp, model, Pn)
    with rec.phase("search"):
        _, _, steps = _search(hp, model, src, prefix)
    return [c[0] for c in rec.phases["search"]], steps


def test_the_call_recorder_shows_one_launch_more_per_step(fx, monkeypatch):
    """Eager steps (ZERO_HIP_DECODE_GRAPH=0), where every launch of a step is a recorded call: with a table there is one
    zk_prefix_force per step, directly ahead of the step's zk_beam_topk, and without those calls the sequence of entry points
    is the one of the run without the feature, which holds no such call."""
    from tests import decode_trace as DT
    monkeypatch.setenv("ZERO_HIP_DECODE_GRAPH", "0")
    rec = DT.Recorder(monkeypatch)
    Pn = V.sharpen(fx["hp"], fx["Pn"])
    hp = G.beam_hp(fx["hp"], 4, "bfloat16")
    off, steps0 = _recorded(hp, fx["model"], Pn, fx["src"], None, rec)
    on, steps = _recorded(hp, fx["model"], Pn, fx["src"], fx["prefix"], rec)
    assert "zk_prefix_force" not in off and off.count("zk_beam_topk") == steps0
    assert on.count("zk_prefix_force") == steps == on.count("zk_beam_topk")
    assert all(on[i + 1] == "zk_beam_topk" for i, x in enumerate(on) if x == "zk_prefix_force")
    rest = [x for x in on if x != "zk_prefix_force"]
    m = min(len(rest), len(off))
    assert rest[:m] == off[:m] and m > 0.5 * len(off)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_step_graphs_are_reused_with_tables_and_not_across(fx, dtype):
    """A second batch of the same shape with other prefixes replays the first one's graphs (the table's address is the same);
    a run without prefixes on the same engine adopts none of them, and each decodes what it decodes on a fresh engine."""
    model = fx["model"]
    hp = G.beam_hp(fx["hp"], 4, dtype)
    Pn = V.sharpen(fx["hp"], fx["Pn"])
    second = V.ragged((11, 14, 7, 9), hp.src_vocab.size(), 6, width=fx["src"].shape[1])
    prefix2 = PR.prefixes(hp.tgt_vocab.size(), (2, 1, 0, 3), seed=5)
    fresh = [_decode(hp, model, Pn, s, p)[:2] for s, p in ((fx["src"], fx["prefix"]), (second, prefix2), (second, None))]
    assert not np.array_equal(fresh[1][0], fresh[2][0])
    reset_cores(); core = get_core(hp, model, Pn)
    a = _search(hp, model, fx["src"], fx["prefix"])
    n0 = core.__dict__.get("_graph_adoptions", 0)
    b = _search(hp, model, second, prefix2)
    assert core.__dict__.get("_graph_adoptions", 0) == n0 + 1
    c = _search(hp, model, second, None)
    assert core.__dict__.get("_graph_adoptions", 0) == n0 + 1            # with a table / without: not the same launch sequence
    d = _search(hp, model, second, np.zeros_like(prefix2))
    assert core.__dict__.get("_graph_adoptions", 0) == n0 + 2            # empty prefixes: the plain step's graphs
    for got, want in ((a, fresh[0]), (b, fresh[1]), (c, fresh[2]), (d, fresh[2])):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    _holds(b[0], b[1], prefix2, fx["hp"])


def test_two_member_ensemble():
    """transformer + transformer_aan, fp32, beam 4: the rule on the combined log-probabilities, against the composed oracle
    under the same rule."""
    from zero_amd import search
    from zero_amd.models._ensemble import make_infer_fns, member_params
    models = ("transformer", "transformer_aan")
    hps, Pns, src = ec.make_members(models, (3, 4))
    hps = ec.with_beam(hps, 4, decode_dtype="float32")
    prefix = PR.prefixes(hps[0].tgt_vocab.size(), tuple(PR.PREFIX_LENGTHS[b % 4] for b in range(src.shape[0])))
    fns = PR.constrained(lambda hp, P: ec.composed_infer_fn(hps, Pns, models), prefix, 4)
    enc, dec = fns(hps[0], None)
    with torch.no_grad():
        ref = rt.beam_search({"source": torch.tensor(src)}, enc, dec, hps[0])
    reset_cores()
    for i, (hp, Pn, m) in enumerate(zip(hps, Pns, models)):
        get_core(member_params(hp, i), m, Pn)
    enc, dec, hp0 = make_infer_fns([registry.get_model(m) for m in models], hps)
    out = search.beam_search({"source": src, "prefix": prefix}, enc, dec, hp0)
    seqs, scores = np.asarray(out["seq"]), np.asarray(out["score"])
    G.assert_tokens(seqs, ref["seq"])
    fin = ref["score"] > -1e30
    assert np.allclose(scores[fin], ref["score"][fin], rtol=1e-5, atol=1e-6), np.abs(scores - ref["score"])[fin].max()
    _holds(seqs, scores, prefix, hps[0])


# ---------------------------------------------------------------------------------------------- with the other options
def _two_routes(hp, model, Pn, src, prefix, monkeypatch):
    base = _decode(hp, model, Pn, src, prefix)
    monkeypatch.setenv("ZERO_HIP_DECODE_GRAPH", "0")
    eager = _decode(hp, model, Pn, src, prefix)
    monkeypatch.delenv("ZERO_HIP_DECODE_GRAPH")
    G.assert_tokens(eager[0], base[0])
    assert np.array_equal(eager[1], base[1])
    return base


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_with_the_ngram_ban(fx, monkeypatch, dtype):
    """no_repeat_ngram_size = 2: every hypothesis starts with its prefix and holds no 2-gram twice, the prefix's own 2-grams
    included; in fp32 the hypotheses are those of the reference under both rules (tests/prefix_ref.with_ngram); the eager route
    equals the captured one bit for bit.  A prefix that holds a 2-gram twice is refused before the encoder pass."""
    hp = G.beam_hp(fx["hp"], 4, dtype, no_repeat_ngram_size=2)
    Pn = fx["Pn"] if dtype == "float32" else V.sharpen(fx["hp"], fx["Pn"])
    seqs, scores, _ = _two_routes(hp, fx["model"], Pn, fx["src"], fx["prefix"], monkeypatch)
    _holds(seqs, scores, fx["prefix"], fx["hp"])
    for b in range(seqs.shape[0]):
        for k in range(4):
            if scores[b, k] > -1e30:
                assert not N.has_repeat(N.hypothesis(seqs[b, k], fx["hp"]), 2), (b, k)
    # prefix_ref.free_margin on the reference under both rules at beam 4 (CPU): transformer gap 1.33e-04 against err 5.7e-06,
    # transformer_aan 2.29e-05 against 3.8e-06 -- more than 4 x, so the fp32 mode must reproduce the best hypotheses;
    # rnnsearch 3.8e-06 against 7.6e-06: the reference alone is too close to a tie there, and only the properties are held
    if dtype == "float32" and fx["model"] != "rnnsearch":
        ref = V.search(PR.with_ngram(PR.MODELS[fx["model"]]["fns"], fx["prefix"], 4, 2), fx["hp"], Pn, fx["src"], 4,
                       torch.float32)[0]
        assert [N.hypothesis(r[0], fx["hp"]) for r in seqs] == [N.hypothesis(r[0], fx["hp"]) for r in ref["seq"]]
    twice = np.zeros((fx["src"].shape[0], 4), dtype=np.int64)
    twice[0] = [5, 6, 5, 6]
    with pytest.raises(ValueError, match=r"no_repeat_ngram_size=2: the 2-gram \(5, 6\)"):
        _search(hp, fx["model"], fx["src"], twice)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_with_sampling_topk(fx, monkeypatch, dtype):
    """sampling_topk = 3 without noise (the truncation keeps 2 * beam_size + 1 = 3 entries of a row of 104 or more: the forced
    tokens are outside): the step forces ahead of the truncation and ahead of the tail (tests/prefix_ref.step_truncated), so a
    forced token is still the step's only real candidate; routes bit-equal."""
    hp = G.beam_hp(fx["hp"], 1, dtype, sampling_topk=3)
    Pn = V.sharpen(fx["hp"], fx["Pn"])
    seqs, scores, _ = _two_routes(hp, fx["model"], Pn, fx["src"], fx["prefix"], monkeypatch)
    _holds(seqs, scores, fx["prefix"], fx["hp"])


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_with_diverse_beam_groups(fx, monkeypatch, dtype):
    """diverse_beam_groups = 2 at beam 4: the rows of a sentence are the whole beam, so every group starts with the prefix
    (the Hamming penalty lowers a later group's forced token by lambda, which is nothing beside 1e8); routes bit-equal."""
    hp = G.beam_hp(fx["hp"], 4, dtype, diverse_beam_groups=2, diverse_beam_strength=0.5)
    Pn = V.sharpen(fx["hp"], fx["Pn"])
    seqs, scores, _ = _two_routes(hp, fx["model"], Pn, fx["src"], fx["prefix"], monkeypatch)
    _holds(seqs, scores, fx["prefix"], fx["hp"])
    assert (scores[:, :2] > -1e30).all()          # at least one hypothesis of each group came out, and _holds saw them


def test_cli_mode_test(tmp_path):
    """`run.py --mode test` with tgt_prefix_file in a fresh interpreter, both decode modes: one translation per source line,
    each starting with its line of the prefix file (an empty line: any translation)."""
    rng = np.random.default_rng(3)
    words = ["w%d" % i for i in range(40)]
    (tmp_path / "vocab.txt").write_text("\n".join(words) + "\n")
    lines = [" ".join(rng.choice(words, size=int(rng.integers(2, 7)))) for _ in range(8)]
    for name in ("test.src", "test.tgt"):
        (tmp_path / name).write_text("\n".join(lines) + "\n")
    prefixes = ["w7", "", "w9 w11", "w3", "", "w30 w31", "w12", "w5"]
    (tmp_path / "prefix.txt").write_text("\n".join(prefixes) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    common = "model_name=transformer,scope_name=transformer,hidden_size=64,embed_size=64,filter_size=128,num_heads=1," \
        "num_encoder_layer=1,num_decoder_layer=1,eval_batch_size=3,beam_size=2,decode_length=4," \
        "initializer=uniform_unit_scaling,initializer_gain=1.0,output_dir=%s," % (tmp_path / "out") + \
        ",".join("%s=%s" % (k, tmp_path / v) for k, v in dict(
            src_vocab_file="vocab.txt", tgt_vocab_file="vocab.txt", src_test_file="test.src", tgt_test_file="test.tgt",
            tgt_prefix_file="prefix.txt").items())
    for dtype in ("bfloat16", "float32"):
        out = tmp_path / ("t_%s.txt" % dtype)
        r = subprocess.run([sys.executable, "-m", "zero_amd.run", "--mode", "test", "--parameters",
                            common + ",decode_dtype=%s,test_output=%s" % (dtype, out)],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "bleu" in r.stdout
        hyps = out.read_text().splitlines()
        assert len(hyps) == 8
        for h, p in zip(hyps, prefixes):
            assert h.split()[:len(p.split())] == p.split(), (h, p)
