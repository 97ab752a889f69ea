"""rnnsearch_deepatt decoding end to end against the reference restated in tests/deepatt_ref.py (ref_torch's linear,
remove_invalid_seq, storage sites and beam search around the restated encoder stack, cells and deep-attention step).

Tiny model: hidden_size 128, embed_size 64, vocabularies of 120 / 104, B = 4 sources of 14, 5, 9 and 11 tokens, two
conditional encoder layers (a forward, a reversed and an un-reversed conditional scan all occur), two attention layers, beam 1
and 4, both cells (atr, gru).  deepatt_ref.make_fixture measures on the CPU, and asserts there, what the reference alone shows on
this fixture (seeds and figures in the docstring of tests/deepatt_ref.py): float64 and fp32 reference token- and
order-identical, the smallest candidate gap more than 4 x the largest fp32 - float64 score difference, that difference at most a
quarter of the project's fp32 score tolerance.

fp32 mode: every hypothesis of every beam token-equal, scores within rtol 1e-5 / atol 1e-6 (deepatt_ref.score_tol).
bf16 mode: output distribution sharpened x 6, best hypothesis of every sentence against the fp32 reference.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import deepatt_ref as D  # noqa: E402
from tests import variant_gpu as G  # noqa: E402
from tests import variant_ref as V  # noqa: E402
from zero_amd.models import load_all  # noqa: E402

load_all()
MODEL = "rnnsearch_deepatt"
STEP_LAUNCHES = {"atr": 6 + 4 * 2, "gru": 8 + 6 * 2}       # the model's own launches of a step with D = 2 (models/_deepatt.py)


@pytest.fixture(scope="module", params=["atr", "gru"])
def fx(request):
    cell = request.param
    hp = D.fixture_hp(cell)
    src = V.ragged(D.LENGTHS, hp.src_vocab.size(), 5)
    f = D.make_fixture(hp, src, D.SEEDS[cell])
    print("fixture cell=%s: smallest candidate gap %.3e, largest fp32 - float64 score difference %.3e (x %.0f), %.3f of "
          "the fp32 score tolerance" % (cell, f["gap"], f["err"], f["gap"] / f["err"], f["rel"]))
    f.update(hp=hp, cell=cell, src=src, ref=G.Reference(D.decoding_fns, hp, f["Pn"], src), tol=D.score_tol(f["rel"], f["err"]))
    return f


@pytest.mark.parametrize("K", [1, 4])
def test_fp32_mode_is_token_exact(fx, K):
    G.fp32_exact(fx, MODEL, K)


@pytest.mark.parametrize("K", [1, 4])
def test_bf16_mode(fx, K):
    core = G.bf16_best(fx, MODEL, K, "%d launches of the model's own, " % STEP_LAUNCHES[fx["cell"]])
    assert core.__dict__.get("_decode_step_launches", 0) >= STEP_LAUNCHES[fx["cell"]]      # the step ran from captured graphs


def test_fp32_source_padding(fx, monkeypatch):
    """ZERO_HIP_DECODE_PAD_LEN = 1 (14 source positions) and = 8 (16): a padded position has mask 0, so every scan of the
    encoder stack carries the state over it -- in either direction -- and the attentions give it the weight 0.  Tokens equal,
    scores within the fp32 tolerance -- not bitwise: the K-slicing of the fp32 GEMM depends on its row count, and the encoder's
    products have B * Ls rows."""
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


def _small(H, E, name, cell):
    from tests.common import make_hp
    hp = make_hp(MODEL, H=H, heads=1, Vs=40, Vt=36, search_mode="cache", scope_name=name, cell=cell, layer_norm=False,
                 num_encoder_layer=1, num_decoder_layer=1)
    hp.embed_size = E
    return hp, D.init_params(hp, 3), V.ragged((6, 3, 5), hp.src_vocab.size(), 2)


@pytest.mark.parametrize("cell", ["atr", "gru"])
def test_bf16_mode_names_its_limit_and_fp32_decodes_the_same_model(cell):
    """hidden_size 20, embed_size 12: outside the bf16 forms (rows are loaded 16 bytes at a time), so encoding_fn refuses
    before the encoder pass and names decode_dtype=float32, which decodes the same model (one conditional encoder layer: the
    feature comes from position 0)."""
    hp, Pn, src = _small(20, 12, "t_deepatt_h20_" + cell, cell)
    hp.beam_size = 2
    hp.decode_dtype = "bfloat16"
    with pytest.raises(ValueError, match="multiples of 8.*decode_dtype=float32"):
        G.decode(hp, MODEL, Pn, src)
    hp.decode_dtype = "float32"
    seqs, scores, _ = G.decode(hp, MODEL, Pn, src)
    assert seqs.shape[:2] == (3, 2) and np.isfinite(scores[:, 0]).all() and (seqs[:, 0] != 0).any()


def test_cli_mode_test(tmp_path):
    """The reference's command line in a fresh interpreter: `--mode test` on files with model_name=rnnsearch_deepatt and
    cell=gru (freshly initialised weights: there is no training to make a checkpoint), hidden_size != embed_size, in both
    decode modes; the evaluation loop decodes its batches on lanes and writes one translation per source line."""
    G.cli_mode_test(tmp_path, "model_name=rnnsearch_deepatt,scope_name=deepatt,cell=gru,num_heads=1,num_encoder_layer=2,"
                              "num_decoder_layer=2,hidden_size=32,embed_size=24")
