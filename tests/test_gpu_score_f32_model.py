"""The fp32 scorer end to end (score_dtype = float32; zero_amd/models/_score_f32.py) against oracle.ref_torch.

Tiny models of tests.common.make_hp (H = 128, 2 heads, 2 + 2 layers, vocabularies 120 / 104), padded sources of 14, 5, 9, 11
and targets of 10, 4, 7, 6 tokens (score_f32_ref.model_fixture).

  parity     score_fn against rt.score_fn in float64, relative, within 4 x ORACLE_FLOOR (the float32 oracle's own distance
             from the float64 one on the same inputs, measured on the CPU: 1.259e-07, so 5.0e-07) -- the bf16 scorer is
             granted 5e-3 by tests/test_gpu_model.py and misses this by orders of magnitude
  identity   a hypothesis the fp32 decoder found, force-decoded by the fp32 scorer, gives back the beam score:
             -score n / ((5 + n) / 6)^alpha == beam score
  default    score_dtype unset: the launches of score_fn are those of the bf16 forward, one for one
  refusals, B = 0, and run.py --mode score in a fresh interpreter
"""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import decode_trace as DT  # noqa: E402
from tests import score_f32_ref as R  # noqa: E402
from tests.common import make_hp  # noqa: E402
from zero_amd.models import model as registry, load_all  # noqa: E402
from zero_amd.models._factory import get_core, reset_cores  # noqa: E402
from zero_amd.variables import reset_stores  # noqa: E402

load_all()
BF16_ENTRY_POINTS = ("zk_gemm", "zk_attn_fwd", "zk_attn_out_ln", "zk_proj_attn_out_ln", "zk_add_ln_fwd", "zk_embed_fwd",
                     "zk_aan_fwd", "zk_cumavg_add_fwd")


def _score(hp, model, Pn, src, tgt, patch=None):
    """-> (scores float64 [B], names of the library entry points score_fn called)."""
    reset_cores()
    get_core(hp, model, Pn)
    names = []
    if patch is not None:
        rec = DT.Recorder(patch)
        with rec.phase("score"):
            out = registry.get_model(model).score_fn({"source": src, "target": tgt}, hp)
        names = rec.phases["score"]
    else:
        out = registry.get_model(model).score_fn({"source": src, "target": tgt}, hp)
    torch.cuda.synchronize()
    return out["score"].float().cpu().numpy().astype(np.float64), names


@pytest.mark.parametrize("case", sorted(R.MODEL_CASES))
def test_parity_with_the_float64_oracle(case, monkeypatch):
    hp, Pn, src, tgt = R.model_fixture(case)
    model = R.MODEL_CASES[case][0]
    want = R.oracle_scores(hp, Pn, model, src, tgt, torch.float64)
    hp.score_dtype = "float32"
    got, calls = _score(hp, model, Pn, src, tgt, monkeypatch)
    rel = np.abs(got / want - 1)
    print("%s: largest relative error %.3e (oracle floor %.3e, allowed %.3e)" % (case, rel.max(), R.ORACLE_FLOOR,
                                                                               4 * R.ORACLE_FLOOR))
    names = [c[0] for c in calls]
    assert "zk_f32_attn_seq" in names, names
    assert not [n for n in names if n.startswith(BF16_ENTRY_POINTS)], names
    assert "zk_f32_attn" not in names and "zk_f32_attn_kb" not in names
    assert np.isfinite(got).all() and rel.max() <= 4 * R.ORACLE_FLOOR, (got, want, rel)


def test_default_scorer_runs_the_bf16_launches(monkeypatch):
    """score_dtype unset: none of the fp32 launches run.  The distance of the bf16 forward from the float64 oracle on this
    fixture is printed next to the fp32 scorer's allowance (9.4e-04 against 5.0e-07 when this was written): a figure, not
    a condition -- the bf16 forward's own bound is tests/test_gpu_model.py's."""
    hp, Pn, src, tgt = R.model_fixture("transformer")
    want = R.oracle_scores(hp, Pn, "transformer", src, tgt, torch.float64)
    got, calls = _score(hp, "transformer", Pn, src, tgt, monkeypatch)
    rel = np.abs(got / want - 1).max()
    print("bf16 score_fn: largest relative error %.3e (the fp32 scorer is allowed %.3e)" % (rel, 4 * R.ORACLE_FLOOR))
    names = [c[0] for c in calls]
    assert not [n for n in names if n.startswith("zk_f32_")], names
    assert [n for n in names if n.startswith(BF16_ENTRY_POINTS)]


@pytest.fixture(scope="module")
def ident():
    hp, Pn, src = R.identity_fixture()
    return dict(hp=hp, Pn=Pn, src=src)


@pytest.mark.parametrize("K", [1, 4])
def test_forced_decoding_identity(ident, K):
    """Decode with decode_dtype = float32, then score the top hypothesis of EVERY sentence (n tokens including its EOS) with
    score_dtype = float32.  Tolerance: the larger of 4 x IDENTITY_FLOOR (the identity with the float32 oracle alone,
    2.636e-07 relative) and the rtol 1e-5 / atol 1e-6 tests/test_gpu_decode_f32.py grants fp32 beam scores."""
    from zero_amd.main import tower_infer_graph
    hp = copy.copy(ident["hp"])
    hp.beam_size, hp.decode_dtype, hp.score_dtype = K, "float32", "float32"
    reset_cores()
    get_core(hp, R.IDENTITY_MODEL, ident["Pn"])
    graph = registry.get_model(R.IDENTITY_MODEL)
    seqs, scores = tower_infer_graph({"source": ident["src"]}, graph, hp)
    hyps = R.top_hypotheses(np.asarray(seqs), np.asarray(scores), hp.tgt_vocab.eos())
    assert len(hyps) == ident["src"].shape[0]
    # (the fixture condition, checked on the CPU in tests/test_score_f32_checker.py: these are the oracle's hypotheses)
    _, _, want = R.oracle_identity(ident["hp"], ident["Pn"], ident["src"], K, torch.float32)
    assert [h for h, _ in hyps] == [h for h, _ in want]

    def score_of(toks):
        out = graph.score_fn({"source": ident["src"], "target": R.pad_targets([(t, 0) for t in toks])}, hp)
        return out["score"].float().cpu().numpy()
    lhs, rhs = R.identity_sides(hyps, score_of, hp.decode_alpha)
    tol = np.maximum(4 * R.IDENTITY_FLOOR * np.abs(rhs), 1e-6 + 1e-5 * np.abs(rhs))
    print("K=%d: lengths %s, beam scores %s, largest |lhs - rhs| %.3e (allowed %.3e)" %
          (K, [len(h) for h, _ in hyps], np.round(rhs, 4), np.abs(lhs - rhs).max(), tol.min()))
    assert (np.abs(lhs - rhs) <= tol).all(), (lhs, rhs)


@pytest.mark.parametrize("model", ["transformer", "transformer_aan"])
def test_default_launches_are_unchanged(model, monkeypatch):
    """score_dtype unset (and decode_dtype = float32 set: it must not leak into scoring): score_fn issues exactly the
    launches of the bf16 forward it issued before the dispatch existed -- restated here as the bypass."""
    from zero_amd.models._factory import closing_dropout
    hp, Pn, src, tgt = R.model_fixture(model)
    hp.decode_dtype = "float32"
    reset_cores()
    get_core(hp, model, Pn)
    registry.get_model(model).score_fn({"source": src, "target": tgt}, hp)      # (an engine's first forward sets up its state)
    rec = DT.Recorder(monkeypatch)
    with rec.phase("score_fn"):
        a = registry.get_model(model).score_fn({"source": src, "target": tgt}, hp)["score"].float().cpu().numpy()
    with rec.phase("bypass"):
        p = closing_dropout(copy.copy(hp))
        p.label_smooth = 0.0
        core = get_core(p, model)
        _, per_sample, _ = core.forward(core.upload(src, tgt), train=False, save=False, label_smooth=0.0)
        b = per_sample.float().cpu().numpy()
    assert len(rec.phases["bypass"]) > 10
    msgs = DT.diff({"x": rec.phases["bypass"]}, {"x": rec.phases["score_fn"]})
    assert not msgs, msgs[:5]
    assert np.array_equal(a, b)


def test_refusals():
    hp = make_hp("transformer_fixup", score_dtype="float32", scope_name="t_sf32_fixup")
    src, tgt = np.array([[5, 6, 2]]), np.array([[7, 2]])
    with pytest.raises(NotImplementedError, match="transformer_fixup"):
        registry.get_model("transformer_fixup").score_fn({"source": src, "target": tgt}, hp)
    for model in ("transformer_rela", "transformer_l0drop"):          # unchanged: refused whatever score_dtype says
        for dt in ("bfloat16", "float32"):
            hp = make_hp(model, score_dtype=dt, scope_name="t_sf32_" + model)
            with pytest.raises(NotImplementedError, match="decode only"):
                registry.get_model(model).score_fn({"source": src, "target": tgt}, hp)


def test_no_sentences_gives_an_empty_score():
    hp, Pn, src, tgt = R.model_fixture("transformer")
    hp.score_dtype = "float32"
    reset_cores()
    out = registry.get_model("transformer").score_fn({"source": src[:0], "target": tgt[:0]}, hp, initializer=Pn)
    assert out["score"].shape == (0,) and out["score"].dtype == torch.float32


def test_cli_score_reaches_the_fp32_path(tmp_path):
    """run.py --mode score --parameters score_dtype=float32 in a fresh interpreter writes the scores of the in-process
    scorer with score_dtype = float32, and they differ from the bf16 scorer's."""
    import subprocess
    import sys
    from tests.test_gpu_loops import _write_bitext
    from zero_amd import main as loops, run as cli
    reset_cores(); reset_stores()
    _write_bitext(tmp_path, n=16)
    out = tmp_path / "out"
    kv = dict(hidden_size=32, embed_size=32, filter_size=64, num_heads=2, num_encoder_layer=1, num_decoder_layer=1,
              dropout=0.0, relu_dropout=0.0, residual_dropout=0.0, attention_dropout=0.0, label_smooth=0.1,
              model_name="transformer", scope_name="transformer", batch_or_token="batch", batch_size=16,
              eval_batch_size=8, max_training_steps=4, epoches=1000, disp_freq=20, save_freq=2, eval_freq=1000,
              lrate=0.3, lrate_strategy="noam", warmup_steps=20, beam_size=2, decode_length=4, process_num=1,
              buffer_size=100, shuffle_batch=False, ema_decay=-1.0, checkpoints=2, best_checkpoints=1,
              src_vocab_file=str(tmp_path / "vocab.txt"), tgt_vocab_file=str(tmp_path / "vocab.txt"),
              src_train_file=str(tmp_path / "train.src"), tgt_train_file=str(tmp_path / "train.tgt"),
              src_dev_file=str(tmp_path / "dev.src"), tgt_dev_file=str(tmp_path / "dev.tgt"),
              src_test_file=str(tmp_path / "dev.src"), tgt_test_file=str(tmp_path / "dev.tgt"),
              output_dir=str(out), test_output=str(out / "test.trans.txt"), random_seed=7)
    params = cli.setup(cli.build_params(",".join("%s=%s" % (k, v) for k, v in kv.items())))
    cli.save_parameters(params, params.output_dir)
    cli.setup_recorder(params)
    loops.train(params)
    texts = {}
    for dt in ("float32", "bfloat16"):
        reset_cores(); reset_stores()
        p = cli.setup(cli.build_params("output_dir=%s,test_output=%s,score_dtype=%s" % (out, out / ("s_%s.txt" % dt), dt)))
        loops.scorer(p)
        texts[dt] = (out / ("s_%s.txt" % dt)).read_text()
    assert len(texts["float32"].split()) == 8 and texts["float32"] != texts["bfloat16"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "zero_amd.run", "--mode", "score", "--parameters",
                        "output_dir=%s,test_output=%s,score_dtype=float32" % (out, out / "s_cli.txt")],
                       env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (out / "s_cli.txt").read_text() == texts["float32"]
    reset_cores(); reset_stores()
