"""What the GPU decode tests of the variant models share (a plain module; imported only by tests marked gpu):
tests/test_gpu_{rela,fixup,l0drop,rnnsearch}_model.py keep their cases, docstrings and whatever one of them alone checks.

``beam_hp`` / ``decode``        the hparams of one decode and the decode itself on a fresh core
``Reference``                   variant_ref.search in fp32, computed once per key and left unchanged
``assert_tokens`` / ``assert_exact``   token-equal hypotheses; scores within the project's fp32 standard
``lane_worker``                 the per-thread infer_fn closure that zero_amd.evalu.decode_many runs on its lanes
``assert_padding_changes_nothing`` / ``assert_graphs_reused``   two whole test bodies that several variants share
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
