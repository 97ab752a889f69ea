"""alignment_file end to end (zero_amd/align.py, zero_amd/models/_align.py) against the model restated on oracle.ref_torch
(tests/align_ref.py model_probs: teacher-forced, shifted input, the chosen layer's cross-attention weights averaged over heads).

Tiny models of the three built types (H = 128, 2 heads, vocabularies 120 / 104), sources of 14, 5, 9 and 11 tokens, targets of
12, 4, 7 and 9 tokens, alignment_layer -1 and 0.

  float32   probabilities within 4 x F32_MODEL_FLOOR (the float32 restatement's own distance from the float64 one, measured
            on the CPU: 6.47e-07, so 2.6e-06 -- the margin the fp32 scorer's tests use); every hard alignment equal where
            the float64 gap exceeds that tolerance
  bf16      hard alignments equal to the float64 reference's on every DECISIVE row (gap > 4 x BF16_MODEL_FLOOR = 0.036);
            at most 25 % of the rows are not decisive (the fixture meets that from the reference alone,
            tests/test_align_checker.py)
  padding (ZERO_HIP_PAD_LEN=8), run.py --mode test / --mode score in a fresh interpreter, replace_unk
"""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import align_ref as R  # noqa: E402
from tests import decode_trace as DT  # noqa: E402
from zero_amd import align as zalign  # noqa: E402
from zero_amd.models import load_all  # noqa: E402
from zero_amd.models._factory import reset_cores  # noqa: E402
from zero_amd.variables import reset_stores  # noqa: E402

load_all()
_REFS = {}


def _ref(model, layer):
    """the float64 reference of a (model, layer), computed once"""
    if (model, layer) not in _REFS:
        hp, Pn, src, tgt = R.model_fixture(model)
        _REFS[model, layer] = dict(hp=hp, Pn=Pn, src=src, tgt=tgt, P=R.model_probs(hp, Pn, model, src, tgt, layer),
                                   am=R.eligible(src), live=R.live_rows(tgt))
    return _REFS[model, layer]


def _run(fx, model, layer, dtype, patch=None):
    hp = copy.copy(fx["hp"])
    hp.alignment_layer, hp.score_dtype = layer, dtype
    reset_cores()
    names = []
    feats = {"source": fx["src"], "target": fx["tgt"]}
    if patch is not None:
        rec = DT.Recorder(patch)
        with rec.phase("align"):
            out = zalign.align_fn(feats, hp, model, initializer=fx["Pn"], want_probs=True)
        names = [c[0] for c in rec.phases["align"]]
    else:
        out = zalign.align_fn(feats, hp, model, initializer=fx["Pn"], want_probs=True)
    torch.cuda.synchronize()
    B, Lt, Ls = fx["P"].shape
    return out["best"].cpu().numpy()[:, :Lt], out["probs"].cpu().numpy().astype(np.float64)[:, :Lt, :Ls], names


@pytest.mark.parametrize("layer", R.MODEL_LAYERS)
@pytest.mark.parametrize("model", R.MODEL_CASES)
def test_float32_pass_against_the_float64_reference(model, layer, monkeypatch):
    fx = _ref(model, layer)
    best, P, names = _run(fx, model, layer, "float32", monkeypatch)
    tol = 4 * R.F32_MODEL_FLOOR
    err = np.abs(P - fx["P"]).max()
    print("%s layer %d: largest |P - P64| %.3e (allowed %.3e)" % (model, layer, err, tol))
    assert names.count("zk_f32_align_probs") == 1 and "zk_align_probs" not in names, names
    assert "zk_ce_fused" not in names and "zk_loss_reduce" not in names          # no logits, no loss
    assert np.isfinite(P).all() and err <= tol
    want = R.hard_align(fx["P"], fx["am"])
    sure = R.row_gaps(fx["P"], fx["am"]) > tol
    assert sure[fx["live"]].mean() > 0.9
    assert (best[sure] == want[sure]).all(), (best, want)
    assert (np.take_along_axis(fx["am"], best.astype(np.int64), 1) == 1).all()         # never a pad, never the source's EOS


@pytest.mark.parametrize("layer", R.MODEL_LAYERS)
@pytest.mark.parametrize("model", R.MODEL_CASES)
def test_bf16_pass_on_the_decisive_rows(model, layer, monkeypatch):
    fx = _ref(model, layer)
    best, P, names = _run(fx, model, layer, "bfloat16", monkeypatch)
    assert names.count("zk_align_probs") == 1 and "zk_f32_align_probs" not in names, names
    assert "zk_ce_fused" not in names and "zk_loss_reduce" not in names
    live = fx["live"]
    decisive = (R.row_gaps(fx["P"], fx["am"]) > 4 * R.BF16_MODEL_FLOOR) & live
    want = R.hard_align(fx["P"], fx["am"])
    print("%s layer %d: %d of %d rows decisive, largest |P - P64| %.3e" %
          (model, layer, decisive.sum(), live.sum(), np.abs(P - fx["P"]).max()))
    assert 1.0 - decisive.sum() / float(live.sum()) <= R.DECISIVE_CAP
    assert (best[decisive] == want[decisive]).all(), (best, want, decisive)
    assert (np.take_along_axis(fx["am"], best.astype(np.int64), 1)[live] == 1).all()
    assert np.allclose(P.sum(-1), 1.0, atol=1e-5) and (P[np.broadcast_to((fx["src"] == 0)[:, None, :], P.shape)] == 0).all()


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_source_padding_gives_the_same_alignments(dtype, monkeypatch):
    fx = _ref("transformer", -1)
    a, _, _ = _run(fx, "transformer", -1, dtype)
    monkeypatch.setenv("ZERO_HIP_PAD_LEN", "8")
    b, Pb, _ = _run(fx, "transformer", -1, dtype)
    assert Pb.shape == fx["P"].shape
    assert np.array_equal(a[fx["live"]], b[fx["live"]])


def test_refusals_come_from_the_new_paths_only():
    from tests.common import make_hp
    src, tgt = np.array([[5, 6, 2]]), np.array([[7, 2]])
    for model in ("transformer_rpr", "transformer_rela", "transformer_l0drop", "transformer_fixup", "rnnsearch"):
        hp = make_hp(model, scope_name="t_align_refused_" + model, alignment_file="a.txt")
        with pytest.raises(NotImplementedError, match="alignment_file.*" + model):
            zalign.align_fn({"source": src, "target": tgt}, hp, model)
    hp = make_hp("transformer", scope_name="t_align_layer", alignment_layer=2)
    with pytest.raises(ValueError, match="alignment_layer=2"):
        zalign.align_fn({"source": src, "target": tgt}, hp, "transformer")
    hp = make_hp("transformer", H=96, heads=2, scope_name="t_align_d48")       # d = 48: the bf16 form refuses, fp32 runs
    reset_cores()
    with pytest.raises(ValueError, match="score_dtype=float32"):
        zalign.align_fn({"source": src, "target": tgt}, hp, "transformer")
    hp.score_dtype = "float32"
    out = zalign.align_fn({"source": src, "target": tgt}, hp, "transformer")
    assert out["best"].shape == (1, 2) and out["probs"] is None
    hp = make_hp("transformer", scope_name="t_align_long")
    reset_cores()
    long_src = np.full((1, R.MAX_LK + 1), 5)
    with pytest.raises(ValueError, match="%d.*%d" % (R.MAX_LK + 1, R.MAX_LK)):
        zalign.align_fn({"source": long_src, "target": tgt}, hp, "transformer")
    reset_cores()


def _pairs_of(best, src_lens, tgt_lens):
    return [zalign.format_pairs(zalign.hard_pairs(best[b], src_lens[b], tgt_lens[b])) for b in range(len(src_lens))]


def test_cli_test_and_score_modes(tmp_path):
    """run.py --mode test (bf16) and --mode score (float32) in a fresh interpreter with alignment_file: one line per source
    line, every pair inside its sentence and hypothesis, and the file equals align_fn on the same pairs.  Then replace_unk in
    process on a source with an out-of-vocabulary word (the forced prefix <unk> puts the token into every hypothesis)."""
    from zero_amd import main as loops, run as cli
    rng = np.random.default_rng(3)
    words = ["w%d" % i for i in range(40)]
    (tmp_path / "vocab.txt").write_text("\n".join(words) + "\n")
    lines = [" ".join(rng.choice(words, size=int(rng.integers(2, 7)))) for _ in range(8)]
    lines[2] = "Zürich " + lines[2]                 # an out-of-vocabulary source word
    for name in ("test.src", "test.tgt"):
        (tmp_path / name).write_text("\n".join(lines) + "\n")
    (tmp_path / "prefix.txt").write_text("\n".join(["<unk>"] * 8) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    common = "model_name=transformer,scope_name=transformer,hidden_size=64,embed_size=64,filter_size=128,num_heads=2," \
        "num_encoder_layer=1,num_decoder_layer=2,eval_batch_size=3,beam_size=2,decode_length=4," \
        "initializer=uniform_unit_scaling,initializer_gain=1.0,output_dir=%s," % (tmp_path / "out") + \
        ",".join("%s=%s" % (k, tmp_path / v) for k, v in dict(
            src_vocab_file="vocab.txt", tgt_vocab_file="vocab.txt", src_test_file="test.src", tgt_test_file="test.tgt").items())
    for mode, dtype in (("test", "bfloat16"), ("score", "float32")):
        out, ali = tmp_path / ("o_%s.txt" % mode), tmp_path / ("a_%s.txt" % mode)
        extra = ",score_dtype=%s,test_output=%s,alignment_file=%s" % (dtype, out, ali)
        r = subprocess.run([sys.executable, "-m", "zero_amd.run", "--mode", mode, "--parameters", common + extra],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got = ali.read_text().split("\n")[:-1]
        hyps = out.read_text().splitlines() if mode == "test" else lines
        assert len(got) == 8 and len(hyps) == 8
        for g, s, h in zip(got, lines, hyps):
            ts = [int(p.split("-")[1]) for p in g.split()]
            assert ts == sorted(ts) and len(set(ts)) == len(ts)
            assert all(0 <= int(p.split("-")[0]) < len(s.split()) and 0 <= int(p.split("-")[1]) < len(h.split()) for p in g.split())
        # the same pairs through align_fn in this process (the same seeded initialisation, no checkpoint)
        reset_cores(); reset_stores()
        params = cli.setup(cli.build_params(common + extra))
        loops._eval_trainer(params)
        src = [params.src_vocab.to_id(s.split()) for s in lines]
        tgt = [params.tgt_vocab.to_id(h.split()) for h in hyps]
        pad = lambda rows: np.array([r + [0] * (max(map(len, rows)) - len(r)) for r in rows])
        best = zalign.align_fn({"source": pad(src), "target": pad(tgt)}, params, "transformer")["best"].cpu().numpy()
        assert _pairs_of(best, [len(s) - 1 for s in src], [len(t) - 1 for t in tgt]) == got
    # replace_unk: every hypothesis starts with the forced <unk>; it becomes the raw source word it is aligned to
    reset_cores(); reset_stores()
    out, ali = tmp_path / "o_unk.txt", tmp_path / "a_unk.txt"
    params = cli.setup(cli.build_params(common + ",test_output=%s,alignment_file=%s,replace_unk=True,tgt_prefix_file=%s"
                                        % (out, ali, tmp_path / "prefix.txt")))
    loops.evaluate(params)
    hyps, got = out.read_text().splitlines(), ali.read_text().split("\n")[:-1]
    assert len(hyps) == 8 and len(got) == 8
    for h, g, s in zip(hyps, got, lines):
        first = [p for p in g.split() if p.endswith("-0")]
        assert len(first) == 1
        assert h.split()[0] == s.split()[int(first[0].split("-")[0])] and "<unk>" not in h.split()[:1]
    reset_cores(); reset_stores()
