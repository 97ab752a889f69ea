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
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_torch as rt  # noqa: E402
from tests import l0drop_ref as L  # noqa: E402
from tests import variant_gpu as G  # noqa: E402
from tests import variant_ref as V  # noqa: E402
from tests.common import make_hp  # noqa: E402
from zero_amd.models import model as registry, load_all  # noqa: E402
from zero_amd.models._factory import get_core, reset_cores  # noqa: E402

load_all()
MODEL = "transformer_l0drop"
LENGTHS = (14, 5, 9, 11)


@pytest.fixture(scope="module")
def fx():
    hp = make_hp(MODEL, search_mode="cache")
    src = V.ragged(LENGTHS, hp.src_vocab.size(), 5)
    f = L.make_fixture(hp, src, 41)
    print("fixture: kept %.0f %% of the valid positions, margin %.3f, fp32 error %.2e, bf16-storage error %.3f"
          % (100 * f["frac"], f["margin"], f["err_f32"], f["err_bf16"]))
    f.update(hp=hp, src=src, ref=G.Reference(L.decoding_fns, hp, f["Pn"], src))
    return f


def _kept(core, f32, B, Ls=16):
    """The kept positions per sentence as the device left them (engine buffers of models/_l0drop.py) by the last batch of
    B sentences padded to Ls positions (every source here is 14 wide: 16 with ZERO_HIP_DECODE_PAD_LEN = 8)."""
    pre = "dq." if f32 else "dc."
    torch.cuda.synchronize()
    cnt = core.eng.bufs[pre + "l0.cnt"][:2 * B].view(2, B).cpu().numpy()
    pos = core.eng.bufs[pre + "l0.pos"][:B * Ls].view(B, Ls).cpu().numpy()
    return [set(pos[b, :cnt[0, b]].tolist()) for b in range(B)]


@pytest.mark.parametrize("K", [1, 4])
def test_fp32_mode_is_token_exact(fx, K):
    ref = fx["ref"](K, key=("plain", K))
    seqs, scores, core = G.decode(G.beam_hp(fx["hp"], K, "float32"), MODEL, fx["Pn"], fx["src"])
    kept = _kept(core, True, len(LENGTHS))
    assert kept == [set(np.nonzero(r)[0].tolist()) for r in fx["kept"]], kept
    G.assert_exact(seqs, scores, ref)


@pytest.mark.parametrize("K", [1, 4])
def test_bf16_mode(fx, K):
    from zero_amd.search import decode_hypothesis
    # (the encoder, and with it the fixture's keep margins, does not read the sharpened table)
    Pn = V.sharpen(fx["hp"], fx["Pn"])
    ref = fx["ref"](K, Pn=Pn, key=("sharp", K))
    hp = G.beam_hp(fx["hp"], K, "bfloat16")
    seqs, scores, core = G.decode(hp, MODEL, Pn, fx["src"])
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
    hp = G.beam_hp(fx["hp"], 4, "float32")
    seqs, scores, core = G.decode(hp, MODEL, Pn, fx["src"])
    gate = core.eng.bufs["dq.l0.gate"][:fx["src"].size].cpu().numpy()
    assert (gate == 1.0).all()
    hp_t = G.beam_hp(fx["hp"], 4, "float32", model_name="transformer", scope_name="t_l0_plain")
    seqs_t, scores_t, _ = G.decode(hp_t, "transformer", base, fx["src"])
    G.assert_exact(seqs, scores, {"seq": seqs_t, "score": scores_t})


def test_all_dropped_attends_to_the_counting_slot_only(fx):
    """b_0 = -20: every gate is 0; each sentence attends to the zero slot alone; the decode finishes and equals the
    reference."""
    Pn = L.with_pruning(fx["Pn"], fx["Pn"]["source_pruning/W_0_0"] * 0.0, -20.0)
    ref = fx["ref"](4, Pn=Pn)
    seqs, scores, core = G.decode(G.beam_hp(fx["hp"], 4, "float32"), MODEL, Pn, fx["src"])
    assert _kept(core, True, len(LENGTHS)) == [set()] * len(LENGTHS)
    G.assert_exact(seqs, scores, ref)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_step_graphs_are_reused_across_batches_with_other_kept_sets(fx, dtype):
    """Two batches of equal (B, Lm, Tmax) with different kept sets, one after the other on one engine with the step-graph
    cache on: the second replays the first one's graphs and must decode what it decodes on a fresh engine (a stale kbias
    or mask pointer would show)."""
    from zero_amd import search
    hp = G.beam_hp(fx["hp"], 4, dtype)
    Pn = V.sharpen(fx["hp"], fx["Pn"])
    first = fx["src"]
    second = V.ragged((11, 14, 7, 9), hp.src_vocab.size(), 6, width=first.shape[1])

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
        ref = fx["ref"](4, Pn=Pn, src=second)
        G.assert_exact(b[0], b[1], ref)


def test_four_lanes_equal_one_lane(fx):
    from zero_amd.evalu import decode_many
    hp = G.beam_hp(fx["hp"], 4, "bfloat16")
    reset_cores(); get_core(hp, MODEL, V.sharpen(fx["hp"], fx["Pn"]))
    batches = [V.ragged(tuple(int(x) for x in np.random.default_rng(i).integers(5, 15, 3 + i % 2)), hp.src_vocab.size(), 10 + i)
               for i in range(6)]
    work = G.lane_worker(MODEL, hp)
    one = decode_many(batches, work, streams=1)
    four = decode_many(batches, work, streams=4)
    for i, (a, b) in enumerate(zip(one, four)):
        assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), i


def test_bf16_mode_names_its_limit(fx, monkeypatch):
    hp = G.beam_hp(fx["hp"], 4, "bfloat16")
    monkeypatch.setenv("ZERO_HIP_DECODE_FUSE_ATT", "0")
    with pytest.raises(ValueError, match="decode_dtype=float32"):
        G.decode(hp, MODEL, fx["Pn"], fx["src"])
