"""The alignment checker checked on the CPU (tests/align_ref.py): the stand-in of a correct kernel stays inside every bound on
every kernel case, every planted defect fails on the case named for it, the arg-max acceptance rule holds from the reference
alone, and the model fixtures meet the conditions tests/test_gpu_align_model.py relies on (floors, decisive rows)."""
import numpy as np
import pytest

from tests import align_ref as R


def _check(x, form, defect=None):
    """-> (worst |P - P_ref| / bound, arg-max violations) of the stand-in (with a defect planted) against the reference."""
    ref = R.case_reference(x)
    bound = R.align_bound(ref, form)
    km = None if x["kmask"] is None else x["kmask"].numpy()
    am = None if x["amask"] is None else x["amask"].numpy()
    P, best = R.align_standin(x["q"].numpy(), x["k"].numpy(), km, x["nh"], form, inf_const=x["inf"], amask=am, defect=defect)
    return R.worst_ratio(P, ref["P"], bound), R.accept_best(best, ref["P"], bound, ref["amask"]), ref, best


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_standin_stays_inside_every_bound(case, form):
    x = R.case_inputs(case, form)
    ratio, bad, ref, best = _check(x, form)
    print("%s %s: worst |err| / bound %.3f" % (case, form, ratio))
    assert ratio <= 1.0
    assert not bad, bad[:3]
    assert np.allclose(ref["P"].sum(-1), 1.0, atol=1e-12)
    if x["kmask"] is not None and x["inf"] == R.MASK_INF:
        assert (ref["P"][np.broadcast_to((x["kmask"].numpy() == 0)[:, None, :], ref["P"].shape)] == 0.0).all()


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("defect", sorted(R.DEFECTS))
def test_every_defect_fails_on_its_case(defect, form):
    x = R.case_inputs(R.DEFECTS[defect], form)
    ratio, bad, _, _ = _check(x, form, defect)
    print("%s on %s %s: worst |err| / bound %.3g, %d arg-max violations" % (defect, R.DEFECTS[defect], form, ratio, len(bad)))
    if defect == "tie_later":
        # equal values: both indices pass the acceptance rule; the explicit tie assertion of the kernel test catches it
        cs = R.CASES["ties"]
        ref = R.case_reference(x)
        got = R.case_reference(x, defect)["best"]
        assert (ref["best"] == cs["tie"][0]).all() and (got == cs["tie"][1]).all()
        return
    assert ratio > 1.0 or bad


def test_one_valid_key_and_ties_in_the_reference():
    x = R.case_inputs("q15_k15_ragged", "fp32")
    P = R.case_reference(x)["P"]
    assert (P[2, :, 0] == 1.0).all() and (P[2, :, 1:] == 0.0).all()
    x = R.case_inputs("ties", "bf16")
    ref = R.case_reference(x)
    j1, j2 = R.CASES["ties"]["tie"]
    assert (ref["P"][:, :, j1] == ref["P"][:, :, j2]).all() and (ref["best"] == j1).all()


def test_acceptance_rule_from_the_reference_alone():
    """The reference's own arg-max is accepted; an ineligible index, a -1 on a row with eligible positions and an index whose
    probability is more than two bounds below the best are refused; -1 is demanded where nothing is eligible."""
    x = R.case_inputs("q16_k64_last", "fp32")
    ref = R.case_reference(x)
    bound = R.align_bound(ref, "fp32")
    am = ref["amask"]
    assert not R.accept_best(ref["best"], ref["P"], bound, am)
    worst = np.where(am[:, None, :] != 0, ref["P"], np.inf).argmin(-1).astype(np.int32)
    gap = np.take_along_axis(ref["P"], ref["best"][..., None].astype(np.int64), -1)[..., 0] - \
        np.take_along_axis(ref["P"], worst[..., None].astype(np.int64), -1)[..., 0]
    assert (gap[:2] > 4 * bound.max()).all()
    bad = R.accept_best(worst, ref["P"], bound, am)
    assert len(bad) >= 2 * ref["P"].shape[1]
    masked = np.full_like(ref["best"], x["kmask"].shape[1] - 1)           # sentence 1 and 2: a masked position
    assert len(R.accept_best(masked, ref["P"], bound, am)) >= 2 * ref["P"].shape[1]
    assert len(R.accept_best(np.full_like(ref["best"], -1), ref["P"], bound, am)) == ref["best"].size
    assert len(R.accept_best(ref["best"], ref["P"], bound, np.zeros_like(am))) == ref["best"].size
    assert not R.accept_best(np.full_like(ref["best"], -1), ref["P"], bound, np.zeros_like(am))


# ---------------------------------------------------------------------------------------------- the model fixtures
@pytest.fixture(scope="module")
def model_refs():
    import torch
    out = {}
    for model in R.MODEL_CASES:
        hp, Pn, src, tgt = R.model_fixture(model)
        for layer in R.MODEL_LAYERS:
            out[model, layer] = dict(
                src=src, tgt=tgt, P64=R.model_probs(hp, Pn, model, src, tgt, layer),
                P32=R.model_probs(hp, Pn, model, src, tgt, layer, dtype=torch.float32),
                Pbf=R.model_probs(hp, Pn, model, src, tgt, layer, dtype=torch.float32, store_bf16=True))
    return out


def test_model_floors_are_the_quoted_ones(model_refs):
    f32 = max(np.abs(r["P32"] - r["P64"]).max() for r in model_refs.values())
    bf = max(np.abs(r["Pbf"] - r["P64"]).max() for r in model_refs.values())
    print("float32 restatement: %.3e (quoted %.3e); bf16-storage restatement: %.3e (quoted %.3e)" %
          (f32, R.F32_MODEL_FLOOR, bf, R.BF16_MODEL_FLOOR))
    assert 0.5 * R.F32_MODEL_FLOOR <= f32 <= R.F32_MODEL_FLOOR
    assert 0.5 * R.BF16_MODEL_FLOOR <= bf <= R.BF16_MODEL_FLOOR


def test_reference_alone_meets_the_decisive_cap(model_refs):
    for (model, layer), r in sorted(model_refs.items()):
        am, live = R.eligible(r["src"]), R.live_rows(r["tgt"])
        gaps = R.row_gaps(r["P64"], am)[live]
        frac = float((gaps <= 4 * R.BF16_MODEL_FLOOR).mean())
        print("%s layer %d: %d rows, %.0f %% non-decisive" % (model, layer, gaps.size, 100 * frac))
        assert gaps.size == sum(n - 1 for n in R.TARGET_LENGTHS)
        assert frac <= R.DECISIVE_CAP
        # a masked source position and the source's EOS are never the reference's alignment
        best = R.hard_align(r["P64"], am)
        assert (np.take_along_axis(am, best.astype(np.int64), 1)[live] == 1).all()
        assert (r["P64"][np.broadcast_to((r["src"] == 0)[:, None, :], r["P64"].shape)] == 0).all()
