"""transformer_fixup on the CPU: the registry, the variable layout and initial values, the refusals, the check of
tests/test_gpu_fixup_kernels.py shown to pass a correct stand-in and to reject every planted defect, the two paths of the
restated reference against each other, and the fixture of tests/test_gpu_fixup_model.py.

Stand-ins (fixup_ref.standin_*: torch float32, another evaluation order, one rounding to the storage type) lie within the
bounds on every kernel case.  Planted defects (fixup_ref.RES_DEFECTS, FFN_DEFECTS), each outside the bound on at least one
case; host_baked applies where every scalar is passed, xs_from_rounded shows in the bf16 form only (in the fp32 form the
storage type IS the stream's type).
"""
import copy

import numpy as np
import pytest
import torch

from oracle import ref_torch as rt
from tests import fixup_ref as R
from tests import variant_ref as V
from tests.common import make_hp

MODEL = "transformer_fixup"
FORMS = ("bf16", "fp32")


# ---------------------------------------------------------------------------------------------- registry and layout
def test_the_registry_has_the_triple():
    from zero_amd.models import model as registry, load_all
    load_all()
    triple = registry.get_model(MODEL)
    assert callable(triple.train_fn) and callable(triple.score_fn) and callable(triple.infer_fn)


@pytest.mark.parametrize("shared,softmax_shared", [(False, True), (False, False), (True, True)])
def test_variable_specs(shared, softmax_shared):
    from zero_amd.variables import variable_specs
    hp = make_hp(MODEL, shared_source_target_embedding=shared, shared_target_softmax_embedding=softmax_shared)
    if shared:
        hp.tgt_vocab = hp.src_vocab
    specs = variable_specs(hp, MODEL)
    want = R.param_names(hp)
    assert [s[0] for s in specs] == [w[0] for w in want]
    assert [tuple(s[1]) for s in specs] == [tuple(w[1]) for w in want]
    names = [s[0] for s in specs]
    assert not [n for n in names if n.endswith("/b_0") or "layer_norm" in n]
    assert ("softmax_embedding" in names) == (not shared and not softmax_shared)
    NE, ND = hp.num_encoder_layer, hp.num_decoder_layer
    assert len([n for n in names if n.endswith("shift/offset")]) == 2 * NE + 3 * ND + 2
    assert len([n for n in names if n.endswith("scale/scale")]) == 2 * NE + 3 * ND + 1
    assert names.index("encoder/scale/scale") == names.index("encoder/shift/offset") + 1 < names.index("decoder/layer_0/self_attention/shift/offset")
    assert names[-1 if shared or softmax_shared else -2] == "decoder/shift/offset"


def test_initial_values():
    from zero_amd.variables import initial_values
    hp = make_hp(MODEL, shared_target_softmax_embedding=False)
    L = 2 * hp.num_encoder_layer + 3 * hp.num_decoder_layer
    vals = initial_values(hp, MODEL, 11)
    base = initial_values(hp, "transformer", 11)
    for n, v in vals.items():
        if n.endswith("shift/offset"):
            assert v.shape == (1,) and v[0] == 0, n
        elif n.endswith("scale/scale"):
            assert v.shape == (1,) and v[0] == 1, n
        elif n.endswith("o_map/W_0_0") or n.endswith("output/W_0_0") or n == "softmax_embedding":
            assert not v.any(), n
        elif n.endswith("enlarge/W_0_0"):
            assert np.allclose(v, base[n] * L ** -0.5, rtol=1e-6, atol=0) and v.any(), n
        elif n.endswith("_map/W_0_0"):
            assert np.allclose(v, base[n] * L ** (-1.0 / 6.0), rtol=1e-6, atol=0) and v.any(), n
        else:
            assert np.array_equal(v, base[n]), n          # embeddings and `bias` as for `transformer`


def test_refusals_touch_no_device(monkeypatch):
    from zero_amd.models import model as registry, load_all, _factory
    load_all()
    monkeypatch.setattr(_factory, "get_core", lambda *a, **k: pytest.fail("a refusal built a core"))
    triple = registry.get_model(MODEL)
    hp = make_hp(MODEL)
    feats = {"source": np.ones((1, 2)), "target": np.ones((1, 2))}
    with pytest.raises(NotImplementedError, match="transformer_fixup.*backward of the scalar"):
        triple.train_fn(feats, hp)
    hp.search_mode = "dev"
    with pytest.raises(NotImplementedError, match="transformer_fixup.*re-encoding decode mode"):
        triple.infer_fn(hp)
    from zero_amd.models import _ensemble
    with pytest.raises(NotImplementedError, match="transformer_fixup.*untested member type"):
        _ensemble.check_members([make_hp("transformer"), make_hp(MODEL)])


# ---------------------------------------------------------------------------------------------- the kernel check
RUNS = [(name, form) for name in R.CASES for form in FORMS]
FFN_RUNS = [(name, form) for name in R.FFN_CASES for form in FORMS]


def _check_residual(got_x, got_xs, ref, x, form, what):
    bx, bxs = R.residual_bound(ref, V.STORAGE[form])
    r = 0.0
    if got_x is not None:
        r = max(r, V.assert_within(got_x, ref["x_out"], bx, what + " x_out"))
    if got_xs is not None:
        r = max(r, V.assert_within(got_xs, ref["xs"], bxs, what + " xs_out"))
    return r


def test_standins_are_within_the_bounds_on_every_case():
    worst = dict.fromkeys(FORMS, 0.0)
    for name, form in RUNS:
        x = R.case_inputs(name, form)
        ref = R.case_reference(name, x, form)
        gx, gxs = R.standin_residual(x["x"], x["y"], x["a"], x["o"], x["b"], V.STORAGE[form])
        worst[form] = max(worst[form], _check_residual(gx.double().numpy(), gxs.double().numpy(), ref, x, form, "%s %s" % (name, form)))
    for name, form in FFN_RUNS:
        x = R.case_inputs(name, form, ffn=True)
        ref = R.case_reference(name, x, form, ffn=True)
        got = R.standin_relu_shift(x["h"], x["o"], V.STORAGE[form])
        worst[form] = max(worst[form], V.assert_within(got.double().numpy(), ref["out"], R.relu_shift_bound(ref, V.STORAGE[form]), name))
    print("stand-ins: largest |err| / bound bf16 %.3f, fp32 %.3f" % (worst["bf16"], worst["fp32"]))


def _applies(defect, name, form):
    null = R.CASES[name].get("null", ())
    if defect == "host_baked":
        return not any(s in null for s in ("scale", "offset", "scale2"))
    if defect == "xs_from_rounded":
        return form == "bf16" and "xs_out" not in null
    if defect == "scale2_dropped":
        return "scale2" not in null and "xs_out" not in null
    if defect == "scale_on_x":
        return "scale" not in null and "x" not in null
    if defect == "shift_before_residual":
        return "y" not in null and "xs_out" not in null
    return True


@pytest.mark.parametrize("defect", R.RES_DEFECTS)
def test_each_planted_residual_defect_is_outside_the_bound_somewhere(defect):
    caught = []
    for name, form in RUNS:
        if not _applies(defect, name, form):
            continue
        x = R.case_inputs(name, form)
        ref = R.case_reference(name, x, form)
        bad = R.case_reference(name, x, form, defect=defect)
        null = R.CASES[name].get("null", ())
        try:
            _check_residual(None if "x_out" in null else bad["x_out"], None if "xs_out" in null else bad["xs"], ref, x, form, defect)
        except AssertionError:
            caught.append((name, form))
    print("%s: outside the bound on %s" % (defect, caught))
    assert caught, defect


@pytest.mark.parametrize("defect", R.FFN_DEFECTS)
def test_each_planted_relu_shift_defect_is_outside_the_bound_somewhere(defect):
    caught = []
    for name, form in FFN_RUNS:
        if "offset" in R.FFN_CASES[name].get("null", ()):
            continue
        x = R.case_inputs(name, form, ffn=True)
        ref = R.case_reference(name, x, form, ffn=True)
        bad = R.case_reference(name, x, form, defect=defect, ffn=True)
        try:
            V.assert_within(bad["out"], ref["out"], R.relu_shift_bound(ref, V.STORAGE[form]), defect)
        except AssertionError:
            caught.append((name, form))
    print("%s: outside the bound on %s" % (defect, caught))
    assert caught, defect


def test_small_update_case_is_below_half_a_bf16_ulp_and_moves_the_fp32_stream():
    x = R.case_inputs("small_update", "bf16")
    ref = R.case_reference("small_update", x, "bf16")
    xo = torch.as_tensor(ref["x_out"]).float()
    assert (xo != x["x"]).all()                                                    # the fp32 stream moves everywhere ..
    assert (np.abs(ref["x_out"] - x["x"].double().numpy()) < 2.0 ** -9).all()      # .. by less than half a bf16 ulp of x >= 1
    assert (xo.bfloat16() == x["x"].bfloat16()).float().mean() > 0.5               # a bf16 stream would drop most updates


# ---------------------------------------------------------------------------------------------- the reference's two paths
def _tiny():
    hp = make_hp(MODEL, H=32, F=64, heads=2, layers=2, Vs=40, Vt=36, search_mode="cache")
    return hp, rt.to_torch(R.init_params(hp, 7), dtype=torch.float64)


def test_cached_steps_equal_the_full_sequence_decoder():
    hp, P = _tiny()
    rng = np.random.default_rng(3)
    B, Lt = 3, 6
    src = np.zeros((B, 7), dtype=np.int64)
    for b, n in enumerate((7, 3, 5)):
        src[b, :n - 1] = rng.integers(3, 40, n - 1)
        src[b, n - 1] = 2
    gold = torch.as_tensor(rng.integers(3, 36, (B, Lt)))
    hpc = rt.closing_dropout(copy.copy(hp))
    full = R.full_decoder(gold, R.encoder(torch.as_tensor(src), hpc, P), hpc, P)
    enc, dec = R.decoding_fns(hp, P)
    state = enc(torch.as_tensor(src))
    for t in range(Lt):
        tok = gold[:, t - 1:t] if t else torch.full((B, 1), hp.tgt_vocab.pad(), dtype=torch.long)
        logits, state = dec(tok, state, t)
        assert float((logits - full[:, t]).abs().max()) <= 1e-10 * float(full.abs().max()), t


def test_every_parameter_of_the_fixture_model_matters():
    """init_params leaves no matrix at zero and no scalar at its neutral value: each one moves the score."""
    hp, _ = _tiny()
    Pn = R.init_params(hp, 7)
    rng = np.random.default_rng(1)
    src = rng.integers(3, 40, (2, 5)); tgt = rng.integers(3, 36, (2, 4))
    base = R.score(hp, Pn, src, tgt)
    for name in Pn:
        if name in ("src_embedding", "tgt_embedding"):
            continue
        Q = dict(Pn)
        Q[name] = (Pn[name] + 0.05).astype(np.float32)
        assert np.abs(R.score(hp, Q, src, tgt) - base).max() > 1e-9, name


# ---------------------------------------------------------------------------------------------- the GPU tests' fixture
def test_fixture_of_the_gpu_model_tests():
    """make_fixture's assertions for the chosen seed; the reference under ref_torch's own bf16 storage model reproduces the
    fp32 reference's best hypotheses on the sharpened model (so the reference alone meets the bf16 test's condition); and the
    floor of the score test: the largest relative score error of the bf16 storage model against float64."""
    hp = make_hp(MODEL, search_mode="cache")
    src = V.ragged(R.FIXTURE_LENGTHS, hp.src_vocab.size(), R.SOURCE_SEED)
    f = R.make_fixture(hp, src, R.FIXTURE_SEED)
    print("seed %d: gap %.3e, err %.3e (x %.0f)" % (R.FIXTURE_SEED, f["gap"], f["err"], f["gap"] / f["err"]))
    assert f["gap"] > 4 * f["err"]
    Ps = V.sharpen(hp, f["Pn"])
    for K in (1, 4):
        a, _ = V.search(R.decoding_fns, hp, Ps, src, K, torch.float32)
        b, _ = V.search(R.decoding_fns, hp, Ps, src, K, torch.float32, store_bf16=True)
        assert rt.decode_hypothesis(a["seq"], hp) == rt.decode_hypothesis(b["seq"], hp), K
    tgt = V.ragged(R.TARGET_LENGTHS, hp.tgt_vocab.size(), R.TARGET_SEED)
    s64 = R.score(hp, f["Pn"], src, tgt)
    sbf = R.score(hp, f["Pn"], src, tgt, torch.float32, store_bf16=True)
    floor = float(np.abs(sbf / s64 - 1).max())
    print("score: bf16 storage model against float64, largest relative error %.3e" % floor)
    assert abs(floor - R.SCORE_FLOOR) <= 0.02 * R.SCORE_FLOOR, (floor, R.SCORE_FLOOR)
    assert 4 * R.SCORE_FLOOR <= 5e-3
