"""Host side of ensemble decoding (no GPU): per-directory parameters of ``--mode ensemble``, checkpoint renaming into the
member scopes, and the composed oracle the GPU tests compare against."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import ref_torch as rt  # noqa: E402
from tests.common import make_hp  # noqa: E402
from tests import ensemble_common as ec  # noqa: E402


def _write_param_json(directory, **values):
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "param.json"), "w") as w:
        w.write(json.dumps(values))


def test_parameter_priority_per_directory(tmp_path):
    """run.py:322-343: command line > the directory's param.json > --config > defaults, one set per directory."""
    from zero_amd.run import build_ensemble_params
    from zero_amd.models._ensemble import member_params, member_scope
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _write_param_json(a, model_name="transformer", hidden_size=128, num_heads=2, beam_size=7, scope_name="nmt")
    _write_param_json(b, model_name="transformer_aan", hidden_size=256, num_heads=4, beam_size=9, scope_name="nmt")
    cfg = tmp_path / "cfg.py"
    cfg.write_text("dict(num_heads=16, filter_size=999, decode_length=33)")
    ps = build_ensemble_params("%s;%s" % (a, b), parameters="beam_size=3,decode_alpha=0.25", config=str(cfg))
    assert len(ps) == 2
    assert [p.model_name for p in ps] == ["transformer", "transformer_aan"]       # the directory's own
    assert [p.hidden_size for p in ps] == [128, 256]
    assert [p.beam_size for p in ps] == [3, 3]                                      # the command line wins in both
    assert [p.decode_alpha for p in ps] == [0.25, 0.25]
    assert [p.num_heads for p in ps] == [16, 16]            # run.py:338-339: --config is applied again over param.json
    assert [p.filter_size for p in ps] == [999, 999]        # --config over the defaults
    assert [p.output_dir for p in ps] == [os.path.abspath(a), os.path.abspath(b)]
    assert [member_scope(p, i) for i, p in enumerate(ps)] == ["nmt_ensembler_0", "nmt_ensembler_1"]
    hp1 = member_params(ps[1], 1)
    assert hp1.scope_name == "nmt_ensembler_1" and ps[1].scope_name == "nmt" and hp1.hidden_size == 256
    # without --config the saved value stands
    ps = build_ensemble_params("%s;%s" % (a, b), parameters="beam_size=3")
    assert [p.num_heads for p in ps] == [2, 4]


def test_run_docstring_no_longer_disclaims_the_mode():
    import zero_amd.run as run
    assert "not provided" not in run.__doc__ and "ensemble" in run.__doc__


@pytest.mark.parametrize("ema", [False, True])
def test_checkpoint_is_renamed_into_the_member_scope(tmp_path, ema):
    """A checkpoint the existing Saver wrote under scope ``model`` comes back as the tensors of ``model_ensembler_1``;
    with ema_decay > 0 the ExponentialMovingAverage entries replace the plain ones (main.py:660-714)."""
    from zero_amd.models._ensemble import member_params, member_scope, member_tensors
    from zero_amd.utils.saver import Saver, assign_tensors, collect_tensors
    from zero_amd.variables import VariableStore
    hp = make_hp("transformer", H=16, F=32, heads=2, Vs=13, Vt=11, scope_name="model")
    src = VariableStore(hp, "transformer", "cpu")
    values = rt.init_params(hp, "transformer", seed=9)
    src.load(values)
    shadows = src.master * 0.5 + 0.25            # a flat buffer laid out like the parameters, as TrainOp's EMA is
    saver = Saver(checkpoints=2, output_dir=str(tmp_path))
    saver.save(collect_tensors(src, "model", 12, hp, ema=shadows), 12)
    tensors = Saver(checkpoints=2, output_dir=str(tmp_path)).restore(str(tmp_path))
    assert "model/encoder/layer_0/feed_forward/ffn_layer/enlarge/W_0_0" in tensors
    renamed = member_tensors(tensors, 1, ema=ema)
    assert "model_ensembler_1/encoder/layer_0/feed_forward/ffn_layer/enlarge/W_0_0" in renamed
    assert not any(k.startswith("model/") for k in renamed)
    assert int(renamed["global_step"]) == 12
    hp1 = member_params(hp, 1)
    assert member_scope(hp, 1) == hp1.scope_name == "model_ensembler_1"
    dst = VariableStore(hp1, "transformer", "cpu")
    got, missing, _ = assign_tensors(dst, hp1.scope_name, renamed)
    assert not missing and len(got) == len(values)
    want = src.export(shadows) if ema else src.export("master")
    have = dst.export("master")
    for name in want:
        assert np.array_equal(have[name], want[name]), name
    # the plain restore under the old scope name finds nothing: the renaming is what makes the member's scope match
    _, missing, _ = assign_tensors(VariableStore(hp1, "transformer", "cpu"), hp1.scope_name, tensors)
    assert len(missing) == len(values)


def test_members_are_checked_before_any_device_work():
    """No member, mismatched target vocabularies, mixed decode_dtype: refused from the parameters alone."""
    from zero_amd.hip import ZeroHipError
    from zero_amd.config import SyntheticVocab
    from zero_amd.models._ensemble import check_members
    with pytest.raises(ZeroHipError, match="at least one member"):
        check_members([])
    a, b = make_hp("transformer"), make_hp("transformer_aan")
    check_members([a, b])
    b.tgt_vocab = SyntheticVocab(105)
    with pytest.raises(ZeroHipError, match="target vocabulary"):
        check_members([a, b])
    b = make_hp("transformer_aan")
    b.decode_dtype = "float32"
    with pytest.raises(ZeroHipError, match="decode_dtype.*0: bfloat16, 1: float32"):
        check_members([a, b])
    with pytest.raises(ZeroHipError, match="at most 8 members"):
        check_members([a] * 9)


def test_composed_oracle_probe():
    """The GPU tests' oracle, checked on its own: three different toy members (seeds 3/4/5), beam 4, cache mode, a 5 x 9
    source.  It ends after 15 steps with finite scores, and its beam-0 hypotheses are NOT those of any single member, so
    a decode that silently used one member cannot pass the comparison."""
    models = ("transformer", "transformer_aan", "transformer_rpr")
    hps, Pns, src = ec.make_members(models, (3, 4, 5))
    assert src.shape == (5, 9)
    out = ec.composed_oracle(hps, Pns, models, src)
    assert out["steps"] == 15
    assert np.isfinite(out["score"]).all()
    best = rt.decode_hypothesis(out["seq"], hps[0])
    for hp, Pn, m in zip(hps, Pns, models):
        single = rt.decode_hypothesis(ec.single_oracle(hp, Pn, m, src)["seq"], hp)
        same = sum(a == b for a, b in zip(best, single))
        print("composed oracle vs %s alone: %d of %d beam-0 hypotheses equal" % (m, same, len(best)))
        assert same < len(best), m


def test_composed_oracle_with_one_member_is_the_single_oracle():
    """M = 1: log(softmax) then the search's own log-softmax -- the same hypotheses as the single-model oracle."""
    hps, Pns, src = ec.make_members(("transformer_aan",), (4,))
    one = ec.composed_oracle(hps, Pns, ("transformer_aan",), src)
    ref = ec.single_oracle(hps[0], Pns[0], "transformer_aan", src)
    assert np.array_equal(one["seq"], ref["seq"]) and one["steps"] == ref["steps"]
    np.testing.assert_allclose(one["score"], ref["score"], rtol=1e-5, atol=1e-6)
