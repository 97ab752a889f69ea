"""deepnmt decoding end to end against the reference restated in tests/deepnmt_ref.py (ref_torch's remove_invalid_seq, storage
sites and beam search around the restated encoder stack, cells, attention and the fp32 residual stream).

Three tiny configurations, vocabularies of 120 / 104, B = 4 sources of 14, 5, 9 and 11 tokens, beam 1 and 4:
    (A) atr, caencoder, dl4mt_redict, NE 2, ND 3, H 128, E 64     the defaults' form: one-to-one layers, x_map + LayerNorm
    (B) atr, no switch,               NE 1, ND 2, H 64,  E 64     z is 2 H wide, the plain-form layer, feature = x
    (C) gru, caencoder, use_deep_att, dl4mt_redict, NE 2, ND 2, H 128, E 128     a projected memory per layer
deepnmt_ref.make_fixture measures on the CPU, and asserts there, what the reference alone shows on each (seeds and figures in
the docstring of tests/deepnmt_ref.py): float64 and fp32 reference token- and order-identical, the smallest candidate gap more
than 4 x the largest fp32 - float64 score difference.

fp32 mode: every hypothesis of every beam token-equal, scores within deepnmt_ref.score_tol.
bf16 mode: output distribution sharpened x 6, best hypothesis of every sentence against the fp32 reference.
Once, on (A): source padding, step graphs reused across batches, four lanes against one, the other search modes, the command
line, and the bf16 size limit at embed_size 620.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import deepnmt_ref as D  # noqa: E402
from tests import variant_gpu as G  # noqa: E402
from tests import variant_ref as V  # noqa: E402
from zero_amd.models import load_all  # noqa: E402

load_all()
MODEL = "deepnmt"


def step_launches(hp, f32):
    """The model's own launches of a captured step (the formula of zero_amd/models/_deepnmt.py)."""
    n = 1 if str(hp.cell).lower() == "atr" else 2                 # n_p = n_c
    per = {"att": 4 * n + 3, "one2one": 4 * n + 1, "plain": 2 * n + 1}
    return (1 if f32 else 2) + sum(per[D.form_of(hp, l)] for l in range(hp.num_decoder_layer)) + (3 if hp.dl4mt_redict else 1)


@functools.lru_cache(maxsize=None)
def _fixture(config):
    hp = D.fixture_hp(config)
    src = V.ragged(D.LENGTHS, hp.src_vocab.size(), 5)
    f = D.make_fixture(hp, src, D.SEEDS[config])
    print("fixture (%s): smallest candidate gap %.3e, largest fp32 - float64 score difference %.3e (x %.0f), %.3f of the fp32 "
          "score tolerance" % (config, f["gap"], f["err"], f["gap"] / f["err"], f["rel"]))
    f.update(hp=hp, config=config, src=src, ref=G.Reference(D.decoding_fns, hp, f["Pn"], src), tol=D.score_tol(f["rel"], f["err"]))
    return f


@pytest.fixture(scope="module", params=sorted(D.CONFIGS))
def fx(request):
    return _fixture(request.param)


@pytest.fixture(scope="module")
def fa():
    return _fixture("A")


def test_step_launch_formula():
    assert [step_launches(D.fixture_hp(c), False) for c in "ABC"] == [22, 13, 27]
    assert [step_launches(D.fixture_hp(c), True) for c in "ABC"] == [21, 12, 26]


@pytest.mark.parametrize("K", [1, 4])
def test_fp32_mode_is_token_exact(fx, K):
    core = G.fp32_exact(fx, MODEL, K, "(%s) " % fx["config"])
    assert core.__dict__.get("_decode_step_launches", 0) >= step_launches(fx["hp"], True)


@pytest.mark.parametrize("K", [1, 4])
def test_bf16_mode(fx, K):
    own = step_launches(fx["hp"], False)
    core = G.bf16_best(fx, MODEL, K, "(%s) %d launches of the model's own, " % (fx["config"], own))
    assert core.__dict__.get("_decode_step_launches", 0) >= own                  # the step ran from captured graphs


def test_fp32_source_padding(fa, monkeypatch):
    """ZERO_HIP_DECODE_PAD_LEN = 1 (14 source positions) and = 8 (16): a padded position has mask 0, so every scan of the
    encoder stack carries the state over it -- in either direction -- and the attention gives it the weight 0; its rows of the
    residual stream are computed and never read.  Tokens equal, scores within the fp32 tolerance -- not bitwise: the K-slicing
    of the fp32 GEMM depends on its row count, and the encoder's products have B * Ls rows."""
    G.assert_padding_within_tol(fa, MODEL, monkeypatch)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_step_graphs_are_reused_across_batches(fa, dtype):
    """Two batches of one shape with different content, one after the other on one engine: the second replays the first
    one's graphs and decodes what it decodes on a fresh engine."""
    hp = G.beam_hp(fa["hp"], 4, dtype)
    second = V.ragged((11, 14, 7, 9), hp.src_vocab.size(), 6, width=fa["src"].shape[1])
    G.assert_graphs_reused(MODEL, hp, V.sharpen(fa["hp"], fa["Pn"]), fa["src"], second)


def test_four_lanes_equal_one_lane(fa):
    G.assert_four_lanes_equal_one(fa, MODEL)


@pytest.mark.parametrize("mode", ["eager", "host_book"])
@pytest.mark.parametrize("config", ["A", "B"])
def test_the_other_search_modes_equal_the_device_resident_one(monkeypatch, mode, config):
    """The step without graphs (decoding_fn + state.reorder per step) and the graph step with the bookkeeping on the host
    decode what the device-resident search decodes: reorder() / bind_caches() of the per-layer ping-pong state serve all three.
    (B) has the plain-form layer, whose single cell launch must never run in place: the eager search's first step follows no
    reorder."""
    G.assert_search_mode_equals_device(_fixture(config), MODEL, monkeypatch, mode)


def test_bf16_mode_names_its_limit_and_fp32_decodes_the_same_model():
    """(A) with embed_size 620, the recipe's: no multiple of 8, so the bf16 mode refuses before the encoder pass and names
    decode_dtype=float32, which decodes the same model."""
    hp = D.fixture_hp("A", scope_name="t_deepnmt_e620")
    hp.embed_size = 620
    Pn = D.init_params(hp, 3)
    src = V.ragged((6, 3, 5), hp.src_vocab.size(), 2)
    hp.beam_size = 2
    hp.decode_dtype = "bfloat16"
    with pytest.raises(ValueError, match="deepnmt in bf16.*multiples of 8.*decode_dtype=float32"):
        G.decode(hp, MODEL, Pn, src)
    hp.decode_dtype = "float32"
    seqs, scores, _ = G.decode(hp, MODEL, Pn, src)
    assert seqs.shape[:2] == (3, 2) and np.isfinite(scores[:, 0]).all() and (seqs[:, 0] != 0).any()


def test_cli_mode_test(tmp_path):
    """The reference's command line in a fresh interpreter: `--mode test` on files with model_name=deepnmt (freshly
    initialised weights: there is no training to make a checkpoint), hidden_size != embed_size, three decoder layers, in both
    decode modes; the evaluation loop decodes its batches on lanes and writes one translation per source line."""
    G.cli_mode_test(tmp_path, "model_name=deepnmt,scope_name=deepnmt,cell=atr,num_heads=1,num_encoder_layer=2,"
                              "num_decoder_layer=3,hidden_size=32,embed_size=24")
