"""The checker of the fp32 scorer's tests, on the CPU (tests/score_f32_ref.py): a correct float32 computation in another
summation order stays inside the derived bounds on every case, every planted defect leaves them on at least one element of
at least one case, the floors written into score_f32_ref.py are re-measured, and the fixture of the forced-decoding identity
is shown to end every top hypothesis in EOS under the oracle."""
import numpy as np
import pytest
import torch

from tests import score_f32_ref as R


@pytest.fixture(scope="module")
def attn():
    out = {}
    for name in R.ATTN_CASES:
        x = R.attn_inputs(name)
        out[name] = (x, R.attn_reference(name, x).numpy(), R.attn_bound(name, x))
    return out


def test_restatement_equals_attn_math(attn):
    """attn_f64 (which carries the defects and feeds the bound) is parity.attn_math where both are defined."""
    for name, (x, ref, _) in attn.items():
        mine = R.attn_f64(name, x)["out"]
        assert np.abs(mine - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), name


@pytest.mark.parametrize("name", sorted(R.ATTN_CASES))
def test_attention_standin_within_bound(attn, name):
    x, ref, bound = attn[name]
    ratio = R.worst_ratio(R.attn_standin(name, x).numpy(), ref, bound)
    print("%s: float32 stand-in, largest |err| / bound = %.3f" % (name, ratio))
    assert ratio <= 1.0, (name, ratio)


def test_attention_bound_is_small(attn):
    """The bound is a rounding-sized quantity, not a licence: against HOT_VALUE-sized outputs it stays below 1e-2 of them."""
    for name, (x, ref, bound) in attn.items():
        assert float((bound / np.maximum(np.abs(ref), 1.0)).max()) < 1e-2, name


@pytest.mark.parametrize("defect", R.ATTN_DEFECTS)
def test_attention_defects_exceed_bound(attn, defect):
    seen = {}
    for name, (x, ref, bound) in attn.items():
        bad = R.attn_f64(name, x, defect=defect)["out"]
        seen[name] = R.worst_ratio(bad, ref, bound)
    print("%s: largest |err| / bound per case: %s" % (defect, {k: "%.3g" % v for k, v in seen.items()}))
    assert max(seen.values()) > 1.0, (defect, seen)


def test_hot_last_key_makes_off_by_one_large(attn):
    """In the causal cases with more than one key an off-by-one is wrong by O(HOT_VALUE) somewhere, not by a rounding."""
    for name, (x, ref, bound) in attn.items():
        if R.ATTN_CASES[name].get("causal") and R.ATTN_CASES[name]["Lk"] > 1:
            for defect in ("causal_plus_one", "causal_minus_one"):
                err = np.abs(R.attn_f64(name, x, defect=defect)["out"] - ref).max()
                assert err > 1.0, (name, defect, err)


@pytest.mark.parametrize("use_mask", [1, 0])
@pytest.mark.parametrize("with_add", [False, True])
def test_cumavg_checker(use_mask, with_add):
    x = R.cumavg_inputs()
    add = x["add"] if with_add else None
    ref, bound = R.cumavg_reference(x["x"], x["mask"], use_mask, add)
    ratio = R.worst_ratio(R.cumavg_standin(x["x"], x["mask"], use_mask, add).numpy(), ref, bound)
    print("cumavg use_mask=%d add=%s: float32 stand-in, largest |err| / bound = %.3f" % (use_mask, with_add, ratio))
    assert ratio <= 1.0
    for defect in R.CUMAVG_DEFECTS:
        bad, _ = R.cumavg_reference(x["x"], x["mask"], use_mask, add, defect=defect)
        assert R.worst_ratio(bad, ref, bound) > 1.0, defect


def test_embed_checker():
    from zero_amd.func import timing_table
    x = R.embed_inputs()
    tim = torch.from_numpy(timing_table(R.EMBED_SHAPE["L"] + 1, R.EMBED_SHAPE["H"]))
    ref, bound = R.embed_reference(x["ids"], x["table"], x["bias"], tim)
    ratio = R.worst_ratio(R.embed_standin(x["ids"], x["table"], x["bias"], tim).numpy(), ref, bound)
    print("embed_shift: float32 stand-in, largest |err| / bound = %.3f" % ratio)
    assert ratio <= 1.0
    for defect in R.EMBED_DEFECTS:
        bad, _ = R.embed_reference(x["ids"], x["table"], x["bias"], tim, defect=defect)
        assert R.worst_ratio(bad, ref, bound) > 1.0, defect


def test_oracle_floor():
    """The float32 oracle against the float64 oracle on the model fixtures: the floor the device is held to 4 x of."""
    worst = 0.0
    for case in R.MODEL_CASES:
        hp, Pn, src, tgt = R.model_fixture(case)
        model = R.MODEL_CASES[case][0]
        s64 = R.oracle_scores(hp, Pn, model, src, tgt, torch.float64)
        s32 = R.oracle_scores(hp, Pn, model, src, tgt, torch.float32)
        rel = float(np.abs(s32 / s64 - 1).max())
        print("%s: scores %s, float32 against float64 oracle: largest relative difference %.3e" % (case, np.round(s64, 3), rel))
        worst = max(worst, rel)
    print("oracle floor %.3e (recorded %.3e)" % (worst, R.ORACLE_FLOOR))
    assert R.ORACLE_FLOOR / 2 <= worst <= R.ORACLE_FLOOR * 2, (worst, R.ORACLE_FLOOR)


def test_identity_floor_and_fixture():
    """Under the oracle (float32 and float64, beam 1 and 4) the top hypothesis of EVERY sentence of the identity fixture ends
    in EOS (top_hypotheses asserts it), both precisions find the same hypotheses, and the identity holds with the oracle
    alone to the recorded floor."""
    hp, Pn, src = R.identity_fixture()
    worst = 0.0
    for K in (1, 4):
        lhs, rhs, hyps = R.oracle_identity(hp, Pn, src, K, torch.float32)
        l64, r64, h64 = R.oracle_identity(hp, Pn, src, K, torch.float64)
        assert [h for h, _ in hyps] == [h for h, _ in h64], K
        assert len(hyps) == src.shape[0]
        assert np.abs(l64 / r64 - 1).max() < 1e-6          # (the identity itself; the beam's penalty is float32)
        rel = float(np.abs(lhs / rhs - 1).max())
        print("K=%d: lengths %s, beam scores %s, identity off by %.3e (float32 oracle)" %
              (K, [len(h) for h, _ in hyps], np.round(rhs, 4), rel))
        worst = max(worst, rel)
    print("identity floor %.3e (recorded %.3e)" % (worst, R.IDENTITY_FLOOR))
    assert R.IDENTITY_FLOOR / 2 <= worst <= R.IDENTITY_FLOOR * 2, (worst, R.IDENTITY_FLOOR)


def test_score_dtype_is_a_build_parameter():
    from zero_amd.config import default_params
    from zero_amd.models import _score_f32
    hp = default_params()
    assert hp.score_dtype == "bfloat16" and not _score_f32.wanted(hp)
    for s in ("float32", "fp32", "f32", "FLOAT32"):
        hp.score_dtype = s
        assert _score_f32.wanted(hp)
    hp.score_dtype, hp.decode_dtype = "bfloat16", "float32"
    assert not _score_f32.wanted(hp)          # decode_dtype keeps meaning decoding only
