"""rnnsearch decoding end to end against the reference restated in tests/rnnsearch_ref.py (ref_torch's linear,
remove_invalid_seq, storage sites and beam search around the restated ATR scans and additive attention).

Tiny model: hidden_size 128, embed_size 64, vocabularies of 120 / 104, B = 4 sources of 14, 5, 9 and 11 tokens, beam 1 and 4,
both encoder forms (caencoder on / off).  rnnsearch_ref.make_fixture measures on the CPU, and asserts there, what the
reference alone shows on this fixture (seeds 37 / 9; figures in the docstring of tests/rnnsearch_ref.py): float64 and fp32
reference token- and order-identical, the smallest candidate gap 34 x / 51 x the largest fp32 - float64 score difference
(required: 4 x), that difference under 0.03 of the project's fp32 score tolerance (required: at most a quarter).

fp32 mode: every hypothesis of every beam token-equal, scores within rtol 1e-5 / atol 1e-6 (rnnsearch_ref.score_tol).
bf16 mode: output distribution sharpened x 6, best hypothesis of every sentence against the fp32 reference.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import rnnsearch_ref as R  # noqa: E402
from tests import variant_gpu as G  # noqa: E402
from tests import variant_ref as V  # noqa: E402
from zero_amd.models import load_all  # noqa: E402

load_all()
MODEL = "rnnsearch"


@pytest.fixture(scope="module", params=[True, False], ids=["caencoder", "bidirectional"])
def fx(request):
    ca = request.param
    hp = R.fixture_hp(ca)
    src = V.ragged(R.LENGTHS, hp.src_vocab.size(), 5)
    f = R.make_fixture(hp, src, R.SEEDS[ca])
    print("fixture caencoder=%s: smallest candidate gap %.3e, largest fp32 - float64 score difference %.3e (x %.0f), %.3f of "
          "the fp32 score tolerance" % (ca, f["gap"], f["err"], f["gap"] / f["err"], f["rel"]))
    f.update(hp=hp, src=src, ref=G.Reference(R.decoding_fns, hp, f["Pn"], src), tol=R.score_tol(f["rel"], f["err"]))
    return f


@pytest.mark.parametrize("K", [1, 4])
def test_fp32_mode_is_token_exact(fx, K):
    G.fp32_exact(fx, MODEL, K)


@pytest.mark.parametrize("K", [1, 4])
def test_bf16_mode(fx, K):
    core = G.bf16_best(fx, MODEL, K)
    assert core.__dict__.get("_decode_step_launches", 0) > 0           # the step ran from captured graphs


def test_fp32_source_padding(fx, monkeypatch):
    """ZERO_HIP_DECODE_PAD_LEN = 1 (14 source positions) and = 8 (16): a padded position has mask 0, so both scans carry the
    state over it and the attention gives it the weight 0.  Tokens equal, scores within the fp32 tolerance -- not bitwise:
    the K-slicing of the fp32 GEMM depends on its row count, and the encoder's products have B * Ls rows."""
    G.assert_padding_within_tol(fx, MODEL, monkeypatch)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_step_graphs_are_reused_across_batches(fx, dtype):
    """Two batches of one shape with different content, one after the other on one engine: the second replays the first
    one's graphs and decodes what it decodes on a fresh engine."""
    hp = G.beam_hp(fx["hp"], 4, dtype)
    second = V.ragged((11, 14, 7, 9), hp.src_vocab.size(), 6, width=fx["src"].shape[1])
    G.assert_graphs_reused(MODEL, hp, V.sharpen(fx["hp"], fx["Pn"]), fx["src"], second)


def test_four_lanes_equal_one_lane(fx):
    G.assert_four_lanes_equal_one(fx, MODEL)


@pytest.mark.parametrize("mode", ["eager", "host_book"])
def test_the_other_search_modes_equal_the_device_resident_one(fx, monkeypatch, mode):
    """The step without graphs (decoding_fn + state.reorder per step) and the graph step with the bookkeeping on the host
    decode what the device-resident search decodes: reorder() / bind_caches() of the ping-pong state serve all three."""
    G.assert_search_mode_equals_device(fx, MODEL, monkeypatch, mode)


def _small(H, E, name, ca=True):
    from tests.common import make_hp
    hp = make_hp(MODEL, H=H, Vs=40, Vt=36, search_mode="cache", scope_name=name, cell="atr", caencoder=ca, layer_norm=False)
    hp.embed_size = E
    return hp, R.init_params(hp, 3), V.ragged((6, 3, 5), hp.src_vocab.size(), 2)


def test_bf16_mode_names_its_limit_and_fp32_decodes_the_same_model():
    """hidden_size 20, embed_size 12: outside the bf16 form (rows are loaded 16 bytes at a time), so encoding_fn refuses
    before the encoder pass and names decode_dtype=float32, which decodes the same model."""
    hp, Pn, src = _small(20, 12, "t_rnn_h20")
    hp.beam_size = 2
    hp.decode_dtype = "bfloat16"
    with pytest.raises(ValueError, match="multiples of 8.*decode_dtype=float32"):
        G.decode(hp, MODEL, Pn, src)
    hp.decode_dtype = "float32"
    seqs, scores, _ = G.decode(hp, MODEL, Pn, src)
    assert seqs.shape[:2] == (3, 2) and np.isfinite(scores[:, 0]).all() and (seqs[:, 0] != 0).any()


def test_cli_mode_test(tmp_path):
    """The reference's command line in a fresh interpreter: `--mode test` on files with model_name=rnnsearch (freshly
    initialised weights: there is no training to make a checkpoint), hidden_size != embed_size, in both decode modes; the
    evaluation loop decodes its batches on lanes and writes one translation per source line."""
    G.cli_mode_test(tmp_path, "model_name=rnnsearch,scope_name=rnnsearch,hidden_size=32,embed_size=24")
