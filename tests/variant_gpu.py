"""What the GPU decode tests of the variant models share (a plain module; imported only by tests marked gpu):
tests/test_gpu_{rela,fixup,l0drop,rnnsearch,deepatt,deepnmt,lrn}_model.py keep their cases, docstrings and whatever one of
them alone checks.

``beam_hp`` / ``decode``        the hparams of one decode and the decode itself on a fresh core
``Reference``                   variant_ref.search in fp32, computed once per key and left unchanged
``assert_tokens`` / ``assert_exact``   token-equal hypotheses; scores within the project's fp32 standard
``lane_worker``                 the per-thread infer_fn closure that zero_amd.evalu.decode_many runs on its lanes
``assert_padding_changes_nothing`` / ``assert_graphs_reused``   two whole test bodies that several variants share
``fp32_exact`` / ``bf16_best`` / ``assert_padding_within_tol`` / ``assert_four_lanes_equal_one`` /
``assert_search_mode_equals_device`` / ``cli_mode_test``   the test bodies the recurrent models share; f is a model test's fixture:
                                a dict with hp, Pn, src, ref (a Reference) and tol = (rtol, atol)
"""
import copy
import threading

import numpy as np
import torch

from tests import variant_ref as V
from zero_amd.models import model as registry
from zero_amd.models._factory import get_core, reset_cores


def beam_hp(hp, K, dtype, **kw):
    hp = copy.copy(hp)
    hp.beam_size, hp.decode_dtype, hp.search_mode = K, dtype, "cache"
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def decode(hp, model, Pn, src):
    """-> (seqs, scores, core) of tower_infer_graph on a fresh core holding Pn."""
    from zero_amd.main import tower_infer_graph
    reset_cores()
    core = get_core(hp, model, Pn)
    seqs, scores = tower_infer_graph({"source": src}, registry.get_model(model), hp)
    return np.asarray(seqs), np.asarray(scores), core


class Reference(object):
    """rt.beam_search with the restated model in fp32 (variant_ref.search); computed once per key and left unchanged."""

    def __init__(self, decoding_fns, hp, Pn, src):
        self.decoding_fns, self.hp, self.Pn, self.src, self.refs = decoding_fns, hp, Pn, src, {}

    def __call__(self, K, Pn=None, src=None, key=None):
        if key is not None and key in self.refs:
            return self.refs[key]
        ref, _ = V.search(self.decoding_fns, self.hp, self.Pn if Pn is None else Pn, self.src if src is None else src, K,
                          torch.float32)
        if key is not None:
            self.refs[key] = ref
        return ref


def assert_tokens(seqs, ref_seq):
    n = min(seqs.shape[2], ref_seq.shape[2])
    assert np.array_equal(seqs[:, :, :n], ref_seq[:, :, :n]), (seqs, ref_seq)
    assert not seqs[:, :, n:].any() and not ref_seq[:, :, n:].any()


def assert_exact(seqs, scores, ref):
    """Every hypothesis of every beam token-equal, scores within rtol 1e-5 / atol 1e-6 (tests/test_gpu_decode_f32.py)."""
    assert_tokens(seqs, ref["seq"])
    fin = ref["score"] > -1e30
    print("largest score difference %.3e" % np.abs(scores - ref["score"])[fin].max())
    assert np.allclose(scores[fin], ref["score"][fin], rtol=1e-5, atol=1e-6), np.abs(scores - ref["score"])[fin].max()


def lane_worker(model, hp):
    """-> work(src) for decode_many: every lane (thread) builds its own infer_fn pair once."""
    from zero_amd.search import beam_search
    graph = registry.get_model(model)
    tl = threading.local()

    def work(src):
        if not hasattr(tl, "fns"):
            tl.fns = graph.infer_fn(hp)
        out = beam_search({"source": src}, tl.fns[0], tl.fns[1], hp)
        return np.asarray(out["seq"]).copy(), np.asarray(out["score"]).copy(), out["steps"]
    return work


def assert_padding_changes_nothing(model, hp, Pn, src, monkeypatch):
    """ZERO_HIP_DECODE_PAD_LEN = 1 and = 8: tokens AND scores are identical."""
    out = []
    for pad in ("1", "8"):
        monkeypatch.setenv("ZERO_HIP_DECODE_PAD_LEN", pad)
        seqs, scores, _ = decode(hp, model, Pn, src)
        out.append((seqs, scores))
    assert_tokens(out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1])


def assert_graphs_reused(model, hp, Pn, first, second):
    """Two batches of one shape with different content, one after the other on one engine: the second adopts the first
    one's graphs and each decodes what it decodes on a fresh engine.  -> the two runs (seqs, scores) on the shared engine."""
    from zero_amd import search

    def run(src):
        enc, dec = registry.get_model(model).infer_fn(hp)
        out = search.beam_search({"source": src}, enc, dec, hp)
        return np.asarray(out["seq"]).copy(), np.asarray(out["score"]).copy()
    fresh = []
    for src in (first, second):
        reset_cores(); get_core(hp, model, Pn)
        fresh.append(run(src))
    assert not np.array_equal(fresh[0][0], fresh[1][0])
    reset_cores(); core = get_core(hp, model, Pn)
    a = run(first)
    n0 = core.__dict__.get("_graph_adoptions", 0)
    b = run(second)
    assert core.__dict__.get("_graph_adoptions", 0) == n0 + 1
    assert np.array_equal(a[0], fresh[0][0]) and np.array_equal(a[1], fresh[0][1])
    assert np.array_equal(b[0], fresh[1][0]) and np.array_equal(b[1], fresh[1][1])
    return a, b


def fp32_exact(f, model, K, label=""):
    """The fp32 mode: every hypothesis of every beam token-equal, scores within f["tol"].  -> the core."""
    ref = f["ref"](K, key=("plain", K))
    seqs, scores, core = decode(beam_hp(f["hp"], K, "float32"), model, f["Pn"], f["src"])
    assert_tokens(seqs, ref["seq"])
    fin = ref["score"] > -1e30
    rtol, atol = f["tol"]
    print("%sK=%d: largest score difference %.3e" % (label, K, np.abs(scores - ref["score"])[fin].max()))
    assert np.allclose(scores[fin], ref["score"][fin], rtol=rtol, atol=atol), np.abs(scores - ref["score"])[fin].max()
    return core


def bf16_best(f, model, K, label=""):
    """The bf16 mode, output distribution sharpened x 6: the best hypothesis of every sentence against the fp32 reference.
    -> the core (core._decode_step_launches: the nodes of the captured step)."""
    from oracle import ref_torch as rt
    from zero_amd.search import decode_hypothesis
    Pn = V.sharpen(f["hp"], f["Pn"])
    ref = f["ref"](K, Pn=Pn, key=("sharp", K))
    hp = beam_hp(f["hp"], K, "bfloat16")
    seqs, scores, core = decode(hp, model, Pn, f["src"])
    print("%sK=%d: %d launches per captured step, top score diff %.3e"
          % (label, K, core.__dict__.get("_decode_step_launches", 0), np.abs(scores[:, 0] - ref["score"][:, 0]).max()))
    hyp, hyp_ref = decode_hypothesis(seqs, hp), rt.decode_hypothesis(ref["seq"], hp)
    assert hyp == hyp_ref, (hyp, hyp_ref)
    return core


def assert_padding_within_tol(f, model, monkeypatch):
    """ZERO_HIP_DECODE_PAD_LEN = 1 and = 8 in the fp32 mode: tokens equal, scores within f["tol"] -- not bitwise where the
    encoder's products have B * Ls rows: the K-slicing of the fp32 GEMM depends on its row count."""
    out = []
    for pad in ("1", "8"):
        monkeypatch.setenv("ZERO_HIP_DECODE_PAD_LEN", pad)
        seqs, scores, _ = decode(beam_hp(f["hp"], 4, "float32"), model, f["Pn"], f["src"])
        out.append((seqs, scores))
    assert_tokens(out[0][0], out[1][0])
    fin = out[0][1] > -1e30
    rtol, atol = f["tol"]
    print("largest score difference between the paddings %.3e" % np.abs(out[0][1] - out[1][1])[fin].max())
    assert np.array_equal(fin, out[1][1] > -1e30) and np.allclose(out[0][1][fin], out[1][1][fin], rtol=rtol, atol=atol)


def assert_four_lanes_equal_one(f, model):
    """Six batches through decode_many on one lane and on four (bf16, sharpened model): steps, tokens and scores identical."""
    from zero_amd.evalu import decode_many
    hp = beam_hp(f["hp"], 4, "bfloat16")
    reset_cores(); get_core(hp, model, V.sharpen(f["hp"], f["Pn"]))
    batches = [V.ragged(tuple(int(x) for x in np.random.default_rng(i).integers(5, 15, 3 + i % 2)), hp.src_vocab.size(), 10 + i)
               for i in range(6)]
    work = lane_worker(model, hp)
    one = decode_many(batches, work, streams=1)
    four = decode_many(batches, work, streams=4)
    for i, (a, b) in enumerate(zip(one, four)):
        assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), i


def assert_search_mode_equals_device(f, model, monkeypatch, mode):
    """mode "eager": the step without graphs (decoding_fn + state.reorder per step); "host_book": the graph step with the
    bookkeeping on the host.  Either decodes what the device-resident search decodes (fp32, beam 4)."""
    hp = beam_hp(f["hp"], 4, "float32")
    base = decode(hp, model, f["Pn"], f["src"])
    monkeypatch.setenv("ZERO_HIP_DECODE_GRAPH" if mode == "eager" else "ZERO_HIP_DECODE_DEVICE_BOOK", "0")
    seqs, scores, _ = decode(hp, model, f["Pn"], f["src"])
    assert_tokens(seqs, base[0])
    fin = base[1] > -1e30
    assert np.allclose(scores[fin], base[1][fin], rtol=f["tol"][0], atol=f["tol"][1])


def cli_mode_test(tmp_path, model_params):
    """The reference's command line in a fresh interpreter: `--mode test` on files of 8 lines with freshly initialised weights
    (there is no training to make a checkpoint), in both decode modes; the evaluation loop decodes its batches on lanes and
    writes one translation per source line.  model_params: "model_name=...,scope_name=...,<sizes>"."""
    import os
    import subprocess
    import sys
    rng = np.random.default_rng(3)
    words = ["w%d" % i for i in range(12)]
    (tmp_path / "vocab.txt").write_text("\n".join(words) + "\n")
    lines = [" ".join(rng.choice(words, size=int(rng.integers(2, 7)))) for _ in range(8)]
    for name in ("test.src", "test.tgt"):
        (tmp_path / name).write_text("\n".join(lines) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    common = model_params + ",eval_batch_size=3,beam_size=2," \
        "decode_length=4,initializer=uniform_unit_scaling,initializer_gain=1.0,output_dir=%s," % (tmp_path / "out") + \
        ",".join("%s=%s" % (k, tmp_path / v) for k, v in dict(
            src_vocab_file="vocab.txt", tgt_vocab_file="vocab.txt", src_test_file="test.src", tgt_test_file="test.tgt").items())
    for dtype in ("bfloat16", "float32"):
        out = tmp_path / ("t_%s.txt" % dtype)
        r = subprocess.run([sys.executable, "-m", "zero_amd.run", "--mode", "test", "--parameters",
                            common + ",decode_dtype=%s,test_output=%s" % (dtype, out)],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "bleu" in r.stdout
        assert len(out.read_text().splitlines()) == 8
