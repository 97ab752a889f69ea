"""transformer_rela decoding end to end against the reference restated in tests/rela_ref.py (ref_torch's linear, LayerNorm,
feed-forward, embedding, timing and beam search; dot_attention + gated_rms_norm of modules/rela.py restated in the encoder
and in both decoder attentions).

Tiny model: H = 128, 2 heads, 2 + 2 layers, vocabularies of 120 / 104, B = 4 sources of 14, 5, 9 and 11 tokens, beam 1
and 4; rela_ref.init_params (rt.init_params + perturbed biases + post/scale around 1, post/gate from the initialiser).
ReLA has a discontinuity softmax lacks (a row whose only positive score is barely positive is normalised up to O(1)), so
rela_ref.make_fixture measures on the CPU, and asserts there, that the reference alone is far from it on this fixture
(seed 49, chosen among 41 .. 59 for the widest margin):

    float64 and fp32 reference: identical hypotheses on every beam, identical candidate order at every step
    smallest gap between a kept candidate and its runner-up (float64 run)      1.23e-03
    largest |score_fp32 - score_float64| over the kept candidates               2.9e-06      (gap > 4 x: here 430 x)

fp32 mode: every hypothesis of every beam token-equal, scores within rtol 1e-5 / atol 1e-6 (tests/test_gpu_decode_f32.py).
bf16 mode: compared as tests/test_gpu_model.py::test_beam_search_token_ids compares (output distribution sharpened x 6, best
hypothesis of every sentence against the fp32 reference).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import ref_torch as rt  # noqa: E402
from tests import rela_ref as R  # noqa: E402
from tests import variant_gpu as G  # noqa: E402
from tests import variant_ref as V  # noqa: E402
from tests.common import make_hp  # noqa: E402
from zero_amd.models import load_all  # noqa: E402
from zero_amd.models._factory import get_core, reset_cores  # noqa: E402

load_all()
MODEL = "transformer_rela"
LENGTHS = (14, 5, 9, 11)
SEED = 49


@pytest.fixture(scope="module")
def fx():
    hp = make_hp(MODEL, search_mode="cache")
    src = V.ragged(LENGTHS, hp.src_vocab.size(), 5)
    f = R.make_fixture(hp, src, SEED)
    print("fixture: smallest candidate gap %.3e, largest fp32 - float64 score difference %.3e (x %.0f)"
          % (f["gap"], f["err"], f["gap"] / f["err"]))
    f.update(hp=hp, src=src, ref=G.Reference(R.decoding_fns, hp, f["Pn"], src))
    return f


@pytest.mark.parametrize("K", [1, 4])
def test_fp32_mode_is_token_exact(fx, K):
    ref = fx["ref"](K, key=("plain", K))
    seqs, scores, _ = G.decode(G.beam_hp(fx["hp"], K, "float32"), MODEL, fx["Pn"], fx["src"])
    G.assert_exact(seqs, scores, ref)


@pytest.mark.parametrize("K", [1, 4])
def test_bf16_mode(fx, K):
    from zero_amd.search import decode_hypothesis
    Pn = V.sharpen(fx["hp"], fx["Pn"])
    ref = fx["ref"](K, Pn=Pn, key=("sharp", K))
    hp = G.beam_hp(fx["hp"], K, "bfloat16")
    seqs, scores, core = G.decode(hp, MODEL, Pn, fx["src"])
    assert core.__dict__.get("_decode_step_launches", 0) > 0           # the step ran from captured graphs
    hyp, hyp_ref = decode_hypothesis(seqs, hp), rt.decode_hypothesis(ref["seq"], hp)
    print("K=%d: top score diff %.3e" % (K, np.abs(scores[:, 0] - ref["score"][:, 0]).max()))
    assert hyp == hyp_ref, (hyp, hyp_ref)


def test_fp32_source_padding_changes_nothing(fx, monkeypatch):
    """ZERO_HIP_DECODE_PAD_LEN = 1 (14 source positions) and = 8 (16): the masked keys contribute exact zeros, in the
    encoder and in every cross-attention, so tokens AND scores are identical."""
    G.assert_padding_changes_nothing(MODEL, G.beam_hp(fx["hp"], 4, "float32"), fx["Pn"], fx["src"], monkeypatch)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_step_graphs_are_reused_across_batches(fx, dtype):
    """Two batches of one shape with different content, one after the other on one engine: the second replays the first
    one's graphs and decodes what it decodes on a fresh engine."""
    hp = G.beam_hp(fx["hp"], 4, dtype)
    second = V.ragged((11, 14, 7, 9), hp.src_vocab.size(), 6, width=fx["src"].shape[1])
    G.assert_graphs_reused(MODEL, hp, V.sharpen(fx["hp"], fx["Pn"]), fx["src"], second)


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


def _small(H, name):
    hp = make_hp(MODEL, H=H, F=2 * H, heads=2, layers=1, Vs=40, Vt=36, search_mode="cache", scope_name=name)
    return hp, R.init_params(hp, 3), V.ragged((6, 3, 5), hp.src_vocab.size(), 2)


def test_bf16_mode_names_its_limit_and_fp32_decodes_the_same_model():
    """H = 24 with 2 heads is a head size of 12: outside the bf16 form (16-byte key loads need d % 8 == 0), so encoding_fn
    refuses before the encoder pass and names decode_dtype=float32, which decodes the same model.  H = 16 with 2 heads
    (d = 8) is the smallest shape the fp32 form is built for; it decodes there as well."""
    hp, Pn, src = _small(24, "t_rela_h24")
    hp.beam_size = 2
    hp.decode_dtype = "bfloat16"
    with pytest.raises(ValueError, match="multiple of 8.*decode_dtype=float32"):
        G.decode(hp, MODEL, Pn, src)
    for H, name in ((24, "t_rela_h24"), (16, "t_rela_h16")):
        hp, Pn, src = _small(H, name)
        hp.beam_size = 2
        hp.decode_dtype = "float32"
        seqs, scores, _ = G.decode(hp, MODEL, Pn, src)
        assert seqs.shape[:2] == (3, 2) and np.isfinite(scores[:, 0]).all() and (seqs[:, 0] != 0).any()
