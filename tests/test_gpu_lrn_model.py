"""rnnsearch_deepatt and deepnmt decoding with the lrn / olrn cells, end to end against the references restated in
tests/deepatt_ref.py and tests/deepnmt_ref.py, whose cell dispatch runs all four cells (fixtures: tests/lrn_ref.py).

Fixtures (vocabularies 120 / 104, B = 4 sources of 14, 5, 9 and 11 tokens):
    rnnsearch_deepatt, lrn and olrn: the sizes of tests/test_gpu_deepatt_model.py (H 128, E 64, NE = D = 2) -- a forward, a
        reversed paired and an un-reversed paired scan all occur;
    deepnmt olrn_ca: configuration (A) of tests/deepnmt_ref.py (caencoder, dl4mt_redict, NE 2, ND 3): the reversed paired scan of
        the encoder and the paired one-step launches of the one-to-one decoder layers run;
    deepnmt lrn_plain: configuration (B) (NE 1, ND 2, H = E = 64): the plain backward scan into a column slice, the [x | c] layer.
make_fixture measures on the CPU, and asserts there, what the reference alone shows on each (seeds and figures in
the docstring of tests/lrn_ref.py).

fp32 mode: every hypothesis of every beam token-equal, scores within score_tol.  bf16 mode: output distribution sharpened x 6,
best hypothesis of every sentence against the fp32 reference.  On rnnsearch_deepatt also: source padding, graph reuse, four lanes
against one, the other search modes, the command line; and the launch structure through the call recorder of
tests/decode_trace.py: 1 + NE scan launches per encoder pass whatever Ls, 6 + 4 D launches per step, none of them for cell=atr.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import deepatt_ref as DA  # noqa: E402
from tests import deepnmt_ref as DN  # noqa: E402
from tests import decode_trace as DT  # noqa: E402
from tests import lrn_ref as L  # noqa: E402
from tests import variant_gpu as G  # noqa: E402
from tests import variant_ref as V  # noqa: E402
from zero_amd.models import load_all, model as registry  # noqa: E402
from zero_amd.models._factory import get_core, reset_cores  # noqa: E402

load_all()
SCANS = ("zk_rnn_lrn_scan", "zk_f32_rnn_lrn_scan")
NE = D = 2
STEP_LAUNCHES = 6 + 4 * D           # embed, projection, lower cell, D x (feed_query, attention, projection, higher cell), ff, tanh, logits


@functools.lru_cache(maxsize=None)
def _fixture(name):
    if name.startswith("deepatt_"):
        model, hp, M = "rnnsearch_deepatt", L.deepatt_hp(name[len("deepatt_"):]), DA
    else:
        model, hp, M = "deepnmt", L.deepnmt_hp(name[len("deepnmt_"):]), DN
    src = V.ragged(L.LENGTHS, hp.src_vocab.size(), 5)
    f = M.make_fixture(hp, src, L.SEEDS[name])
    print("fixture %s: smallest candidate gap %.3e, largest fp32 - float64 score difference %.3e (x %.0f), %.3f of the fp32 "
          "score tolerance" % (name, f["gap"], f["err"], f["gap"] / f["err"], f["rel"]))
    f.update(hp=hp, name=name, model=model, src=src, ref=G.Reference(M.decoding_fns, hp, f["Pn"], src),
             tol=L.score_tol(f["rel"], f["err"]))
    return f


@pytest.fixture(scope="module", params=["deepatt_lrn", "deepatt_olrn"])
def fx(request):
    return _fixture(request.param)


@pytest.fixture(scope="module", params=["deepnmt_olrn_ca", "deepnmt_lrn_plain"])
def fn(request):
    return _fixture(request.param)


# ---------------------------------------------------------------------------------------------- rnnsearch_deepatt
@pytest.mark.parametrize("K", [1, 4])
def test_deepatt_fp32_mode_is_token_exact(fx, K):
    G.fp32_exact(fx, fx["model"], K, fx["name"] + " ")


@pytest.mark.parametrize("K", [1, 4])
def test_deepatt_bf16_mode(fx, K):
    core = G.bf16_best(fx, fx["model"], K, fx["name"] + " ")
    assert core.__dict__.get("_decode_step_launches", 0) >= STEP_LAUNCHES       # the step ran from captured graphs


def test_deepatt_fp32_source_padding(fx, monkeypatch):
    """ZERO_HIP_DECODE_PAD_LEN = 1 (14 source positions) and = 8 (16): a padded position has mask 0, so every scan carries the
    state over it -- the reversed scans meet the padding FIRST -- and the attentions give it the weight 0.  Tokens equal, scores
    within the fp32 tolerance (not bitwise: the K-slicing of the fp32 GEMM depends on its row count)."""
    G.assert_padding_within_tol(fx, fx["model"], monkeypatch)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_deepatt_step_graphs_are_reused_across_batches(fx, dtype):
    hp = G.beam_hp(fx["hp"], 4, dtype)
    second = V.ragged((11, 14, 7, 9), hp.src_vocab.size(), 6, width=fx["src"].shape[1])
    G.assert_graphs_reused(fx["model"], hp, V.sharpen(fx["hp"], fx["Pn"]), fx["src"], second)


def test_deepatt_four_lanes_equal_one_lane(fx):
    G.assert_four_lanes_equal_one(fx, fx["model"])


@pytest.mark.parametrize("mode", ["eager", "host_book"])
def test_deepatt_other_search_modes_equal_the_device_resident_one(fx, monkeypatch, mode):
    G.assert_search_mode_equals_device(fx, fx["model"], monkeypatch, mode)


def test_cli_mode_test(tmp_path):
    """`--mode test` in a fresh interpreter with model_name=rnnsearch_deepatt and cell=lrn (freshly initialised weights),
    hidden_size 32 / embed_size 24, in both decode modes: one translation per source line."""
    G.cli_mode_test(tmp_path, "model_name=rnnsearch_deepatt,scope_name=deepatt_lrn,cell=lrn,num_heads=1,num_encoder_layer=2,"
                              "num_decoder_layer=2,hidden_size=32,embed_size=24")


# ---------------------------------------------------------------------------------------------- the launch structure
def _record(hp, model, Pn, src, patch, pad):
    """-> the recorded calls of one encoder pass and one eager decoder step (tests/decode_trace.py's recorder)."""
    import torch
    patch.setenv("ZERO_HIP_DECODE_PAD_LEN", pad)
    reset_cores()
    core = get_core(hp, model, Pn)
    enc, dec = registry.get_model(model).infer_fn(hp)
    tok = torch.full((src.shape[0] * hp.beam_size,), 5, dtype=torch.int32, device=core.eng.device)
    rec = DT.Recorder(patch)
    with rec.phase("encode"):
        state = enc(src)
    with rec.phase("step"):
        dec(tok, state, 0)
    torch.cuda.synchronize()
    reset_cores()
    return rec.phases, state["Ls"]


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_encoder_pass_is_one_scan_launch_per_layer_whatever_ls(fx, monkeypatch, dtype):
    hp = G.beam_hp(fx["hp"], 4, dtype)
    counts = {}
    for pad, Ls in (("1", 14), ("8", 16)):
        with monkeypatch.context() as patch:
            phases, got_ls = _record(hp, fx["model"], fx["Pn"], fx["src"], patch, pad)
        assert got_ls == Ls
        scans = [a for n, a in phases["encode"] if n in SCANS]
        assert len(scans) == 1 + NE, [n for n, _ in phases["encode"]]
        assert [a[-4] for a in scans] == [Ls] * (1 + NE)                          # T: every scan walks all Ls positions
        assert [a[-3] for a in scans] == [0, 1, 0]                                 # forward, reversed pair, un-reversed pair
        assert [a[7] is not None for a in scans] == [False, True, True]           # hi: the single form, then the pairs
        assert not any(n.endswith(("rnn_atr_step", "rnn_gru_gates", "rnn_gru_out")) for n, _ in phases["encode"])
        step = [n for n, _ in phases["step"]]
        assert len(step) == STEP_LAUNCHES, step
        assert sum(n in SCANS for n in step) == 1 + D
        counts[Ls] = len(phases["encode"])
    assert counts[14] == counts[16]                                                # the whole pass: independent of Ls


def test_atr_issues_no_scan_launch(monkeypatch):
    hp = G.beam_hp(DA.fixture_hp("atr"), 4, "bfloat16")
    src = V.ragged(L.LENGTHS, hp.src_vocab.size(), 5)
    with monkeypatch.context() as patch:
        phases, Ls = _record(hp, "rnnsearch_deepatt", DA.init_params(hp, DA.SEEDS["atr"]), src, patch, "1")
    names = [n for ph in phases.values() for n, _ in ph]
    assert not any(n in SCANS for n in names)
    assert sum(n == "zk_rnn_atr_step" for n, _ in phases["encode"]) == (1 + 2 * NE) * Ls
    assert len(phases["step"]) == STEP_LAUNCHES


# ---------------------------------------------------------------------------------------------- deepnmt
def test_deepnmt_fp32_mode_is_token_exact(fn):
    G.fp32_exact(fn, fn["model"], 4, fn["name"] + " ")


def test_deepnmt_bf16_mode(fn):
    G.bf16_best(fn, fn["model"], 4, fn["name"] + " ")


def test_deepnmt_one_to_one_layers_are_one_paired_launch(monkeypatch):
    f = _fixture("deepnmt_olrn_ca")
    hp = G.beam_hp(f["hp"], 4, "bfloat16")
    with monkeypatch.context() as patch:
        phases, Ls = _record(hp, "deepnmt", f["Pn"], f["src"], patch, "1")
    enc = [a for n, a in phases["encode"] if n in SCANS]
    # layer 0: the forward scan and the reversed pair; layer 1: the forward scan
    assert [(a[-4], a[-3], a[7] is not None) for a in enc] == [(Ls, 0, False), (Ls, 1, True), (Ls, 0, False)]
    step = [a for n, a in phases["step"] if n in SCANS]
    # layer 0 (attention form): lower, higher; layers 1 and 2 (one-to-one): ONE paired launch each
    assert [(a[-4], a[7] is not None) for a in step] == [(1, False), (1, False), (1, True), (1, True)]
    assert all(a[-2] == 1 for a in enc + step)                                     # gated: olrn
