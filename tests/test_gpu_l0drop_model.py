"""transformer_l0drop decoding end to end against the reference restated in tests/l0drop_ref.py (ref_torch's encoder,
self-attention, feed-forward and beam search; the gate, the compaction and the count-weighted cross-attention restated).

Tiny model: H = 128, 2 heads, 2 + 2 layers, vocabularies of 120 / 104, B = 4 sources of 14, 5, 9 and 11 tokens, beam 1
and 4; rt.init_params + perturbed biases + a source_pruning pair that l0drop_ref.make_fixture scales and shifts until
between a quarter and three quarters of the valid positions are kept (here 22 of 39).  Measured by the builder on the CPU
(and asserted there, so a change of the fixture cannot silently lose the margin):

    min |log_alpha - log(1/11)| over the valid positions                       0.271
    max |log_alpha_fp32 - log_alpha_float64|                                   3.6e-06   (margin >= 4 x: fp32 mode)
    max |log_alpha(bf16 storage) - log_alpha(fp32)| of ref_torch               0.054     (margin >= 4 x: bf16 mode)

so the kept sets of both modes must equal the reference's exactly.  fp32 mode: every hypothesis of every beam
token-equal, scores within rtol 1e-5 / atol 1e-6 (tests/test_gpu_decode_f32.py).  bf16 mode: the hypotheses compared as
tests/test_gpu_model.py::test_beam_search_token_ids compares them (output distribution sharpened x 6, best hypothesis
of every sentence against the fp32 reference).
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_torch as rt  # noqa: E402
from tests import l0drop_ref as L  # noqa: E402
from tests.common import make_hp  # noqa: E402
from zero_amd.models import model as registry, load_all  # noqa: E402
from zero_amd.models._factory import get_core, reset_cores  # noqa: E402

load_all()
MODEL = "transformer_l0drop"
LENGTHS = (14, 5, 9, 11)


def _source(hp, lengths=LENGTHS, seed=5, width=None):
    rng = np.random.default_rng(seed)
    src = np.zeros((len(lengths), width or max(lengths)), dtype=np.int64)
    for b, n in enumerate(lengths):
        src[b, :n - 1] = rng.integers(3, hp.src_vocab.size(), n - 1)
        src[b, n - 1] = 2
    return src


@pytest.fixture(scope="module")
def fx():
    hp = make_hp(MODEL, search_mode="cache")
    src = _source(hp)
    f = L.make_fixture(hp, src, 41)
    print("fixture: kept %.0f %% of the valid positions, margin %.3f, fp32 error %.2e, bf16-storage error %.3f"
          % (100 * f["frac"], f["margin"], f["err_f32"], f["err_bf16"]))
    f.update(hp=hp, src=src, refs={})
    return f


def _hp(fx, K, dtype, **kw):
    hp = copy.copy(fx["hp"])
    hp.beam_size, hp.decode_dtype, hp.search_mode = K, dtype, "cache"
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def _reference(fx, K, Pn=None, src=None, key=None):
    """rt.beam_search with the restated decoder; computed once per key and left unchanged."""
    if key is not None and key in fx["refs"]:
        return fx["refs"][key]
    hp = _hp(fx, K, "float32")
    enc, dec = L.decoding_fns(hp, rt.to_torch(fx["Pn"] if Pn is None else Pn))
    ref = rt.beam_search({"source": torch.tensor(fx["src"] if src is None else src)}, enc, dec, hp)
    if key is not None:
        fx["refs"][key] = ref
    return ref


def _decode(hp, Pn, src, model=MODEL):
    from zero_amd.main import tower_infer_graph
    reset_cores()
    core = get_core(hp, model, Pn)
    seqs, scores = tower_infer_graph({"source": src}, registry.get_model(model), hp)
    return np.asarray(seqs), np.asarray(scores), core


def _kept(core, f32, B, Ls=16):
    """The kept positions per sentence as the device left them (engine buffers of models/_l0drop.py) by the last batch of
    B sentences padded to Ls positions (every source here is 14 wide: 16 with ZERO_HIP_DECODE_PAD_LEN = 8)."""
    pre = "dq." if f32 else "dc."
    torch.cuda.synchronize()
    cnt = core.eng.bufs[pre + "l0.cnt"][:2 * B].view(2, B).cpu().numpy()
    pos = core.eng.bufs[pre + "l0.pos"][:B * Ls].view(B, Ls).cpu().numpy()
    return [set(pos[b, :cnt[0, b]].tolist()) for b in range(B)]


def _assert_exact(seqs, scores, ref):
    n = min(seqs.shape[2], ref["seq"].shape[2])
    assert np.array_equal(seqs[:, :, :n], ref["seq"][:, :, :n]), (seqs, ref["seq"])
    assert not seqs[:, :, n:].any() and not ref["seq"][:, :, n:].any()
    fin = ref["score"] > -1e30
    assert np.allclose(scores[fin], ref["score"][fin], rtol=1e-5, atol=1e-6), np.abs(scores - ref["score"])[fin].max()


@pytest.mark.parametrize("K", [1, 4])
def test_fp32_mode_is_token_exact(fx, K):
    ref = _reference(fx, K, key=("plain", K))
    seqs, scores, core = _decode(_hp(fx, K, "float32"), fx["Pn"], fx["src"])
    kept = _kept(core, True, len(LENGTHS))
    assert kept == [set(np.nonzero(r)[0].tolist()) for r in fx["kept"]], kept
    _assert_exact(seqs, scores, ref)


@pytest.mark.parametrize("K", [1, 4])
def test_bf16_mode(fx, K):
    from zero_amd.search import decode_hypothesis
    Pn = dict(fx["Pn"])
    # sharpen the output distribution so that bf16 noise cannot flip near-ties of a random model (the encoder, and with it
    # the fixture's keep margins, does not read this table)
    Pn["tgt_embedding"] = (Pn["tgt_embedding"] * 6.0).astype(np.float32)
    ref = _reference(fx, K, Pn=Pn, key=("sharp", K))
    hp = _hp(fx, K, "bfloat16")
    seqs, scores, core = _decode(hp, Pn, fx["src"])
    kept = _kept(core, False, len(LENGTHS))
    assert kept == [set(np.nonzero(r)[0].tolist()) for r in fx["kept"]], kept
    assert core.__dict__.get("_decode_step_launches", 0) > 0           # the step ran from captured graphs
    hyp, hyp_ref = decode_hypothesis(seqs, hp), rt.decode_hypothesis(ref["seq"], hp)
    print("K=%d: top score diff %.3e" % (K, np.abs(scores[:, 0] - ref["score"][:, 0]).max()))
    assert hyp == hyp_ref, (hyp, hyp_ref)


def test_all_kept_equals_the_plain_transformer(fx):
    """b_0 = +20: every gate is exactly 1, nothing is dropped, the zero slot is masked: the tokens of `transformer` on the
    same weights, scores inside the fp32 bound."""
    Pn = L.with_pruning(fx["Pn"], fx["Pn"]["source_pruning/W_0_0"] * 0.0, 20.0)
    base = {k: v for k, v in Pn.items() if not k.startswith("source_pruning/")}
    hp = _hp(fx, 4, "float32")
    seqs, scores, core = _decode(hp, Pn, fx["src"])
    gate = core.eng.bufs["dq.l0.gate"][:fx["src"].size].cpu().numpy()
    assert (gate == 1.0).all()
    hp_t = _hp(fx, 4, "float32", model_name="transformer", scope_name="t_l0_plain")
    seqs_t, scores_t, _ = _decode(hp_t, base, fx["src"], model="transformer")
    _assert_exact(seqs, scores, {"seq": seqs_t, "score": scores_t})


def test_all_dropped_attends_to_the_counting_slot_only(fx):
    """b_0 = -20: every gate is 0; each sentence attends to the zero slot alone; the decode finishes and equals the
    reference."""
    Pn = L.with_pruning(fx["Pn"], fx["Pn"]["source_pruning/W_0_0"] * 0.0, -20.0)
    ref = _reference(fx, 4, Pn=Pn)
    seqs, scores, core = _decode(_hp(fx, 4, "float32"), Pn, fx["src"])
    assert _kept(core, True, len(LENGTHS)) == [set()] * len(LENGTHS)
    _assert_exact(seqs, scores, ref)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_step_graphs_are_reused_across_batches_with_other_kept_sets(fx, dtype):
    """Two batches of equal (B, Lm, Tmax) with different kept sets, one after the other on one engine with the step-graph
    cache on: the second replays the first one's graphs and must decode what it decodes on a fresh engine (a stale kbias
    or mask pointer would show)."""
    from zero_amd import search
    hp = _hp(fx, 4, dtype)
    Pn = dict(fx["Pn"])
    Pn["tgt_embedding"] = (Pn["tgt_embedding"] * 6.0).astype(np.float32)
    first = fx["src"]
    second = _source(hp, (11, 14, 7, 9), seed=6, width=first.shape[1])

    def run(src):
        enc, dec = registry.get_model(MODEL).infer_fn(hp)
        out = search.beam_search({"source": src}, enc, dec, hp)
        return np.asarray(out["seq"]).copy(), np.asarray(out["score"]).copy()
    fresh = []
    for src in (first, second):
        reset_cores(); core = get_core(hp, MODEL, Pn)
        fresh.append(run(src) + (_kept(core, dtype == "float32", 4), core.eng.bufs[("dq." if dtype == "float32" else "dc.") + "kbias"].numel()))
    assert fresh[0][2] != fresh[1][2]
    reset_cores(); core = get_core(hp, MODEL, Pn)
    a = run(first)
    n0 = core.__dict__.get("_graph_adoptions", 0)
    b = run(second)
    assert fresh[0][3] == fresh[1][3]       # equal Lm (kept at most 8 and 11 -> 16 slots): the second batch adopts the graphs
    assert core.__dict__.get("_graph_adoptions", 0) == n0 + 1
    assert np.array_equal(a[0], fresh[0][0]) and np.array_equal(a[1], fresh[0][1])
    assert np.array_equal(b[0], fresh[1][0]) and np.array_equal(b[1], fresh[1][1])
    if dtype == "float32":
        ref = _reference(fx, 4, Pn=Pn, src=second)
        _assert_exact(b[0], b[1], ref)


def test_four_lanes_equal_one_lane(fx):
    from zero_amd.evalu import decode_many
    from zero_amd.search import beam_search
    import threading
    hp = _hp(fx, 4, "bfloat16")
    Pn = dict(fx["Pn"])
    Pn["tgt_embedding"] = (Pn["tgt_embedding"] * 6.0).astype(np.float32)
    reset_cores(); get_core(hp, MODEL, Pn)
    batches = [_source(hp, tuple(int(x) for x in np.random.default_rng(i).integers(5, 15, 3 + i % 2)), seed=10 + i)
               for i in range(6)]
    graph = registry.get_model(MODEL)
    tl = threading.local()

    def work(s_):
        if not hasattr(tl, "fns"):
            tl.fns = graph.infer_fn(hp)
        out = beam_search({"source": s_}, tl.fns[0], tl.fns[1], hp)
        return np.asarray(out["seq"]).copy(), np.asarray(out["score"]).copy(), out["steps"]
    one = decode_many(batches, work, streams=1)
    four = decode_many(batches, work, streams=4)
    for i, (a, b) in enumerate(zip(one, four)):
        assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), i


def test_bf16_mode_names_its_limit(fx, monkeypatch):
    hp = _hp(fx, 4, "bfloat16")
    monkeypatch.setenv("ZERO_HIP_DECODE_FUSE_ATT", "0")
    with pytest.raises(ValueError, match="decode_dtype=float32"):
        _decode(hp, fx["Pn"], fx["src"])
