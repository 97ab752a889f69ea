"""transformer_rela on the CPU: the variable layout and the refusals, the two paths of the restated reference against
each other, and the check of tests/test_gpu_rela_kernels.py shown to pass a correct stand-in and to reject planted defects.

The stand-in (rela_ref.standin: torch float32, keys summed in the opposite order, one rounding to the storage type) lies
within rela_ref.bound on every kernel-test case.  Measured headroom, largest |err| / bound per form over all cases:
bf16 0.98 (the half ulp of the one rounding to bf16 IS the bound's leading term), fp32 0.03.

Planted defects (rela_ref.DEFECTS), each outside the bound on at least one case; measured, the cases that catch them:
    mask_added, rms_per_head, neighbour_keys     every case they apply to
    normalised, no_qscale                        every case but the bf16 form of "special" (one key per row: a common factor
                                                 of the weights cancels in the RMSNorm, gate = 0 there)
    gate_no_x                                    every case but "special" (gate = 0)
    extra_key                                    "self" at time 0, 1, 8 (the slot behind the last key holds data in the
                                                 reference's inputs and NaN on the device)
    eps_outside                                  "special" only: its rows have a mean square of 0 (0 * inf) or ~1e-5;
                                                 everywhere else ms >= 0.29 and eps = 1e-8 cannot be seen at all
"""
import copy

import numpy as np
import pytest
import torch

from oracle import ref_torch as rt
from tests import rela_ref as R
from tests import variant_ref as V
from tests.common import make_hp

RUNS = [(name, form, t) for name, cs in R.CASES.items() for form in cs["forms"] for (t,) in R.case_runs(name)]


def _applies(defect, name, t):
    cs = R.CASES[name]
    if defect == "extra_key":
        return t is not None and t + 1 < cs["Lk"]
    if defect == "neighbour_keys":
        return cs["B"] // cs["G"] >= 2
    return True


@pytest.fixture(scope="module")
def refs():
    """The float64 reference of every run, computed once."""
    out = {}
    for name, form, t in RUNS:
        x = R.case_inputs(name, form)
        out[(name, form, t)] = (x, R.case_reference(name, x, t))
    return out


def test_standin_is_within_the_bound_on_every_case(refs):
    worst = {"bf16": 0.0, "fp32": 0.0}
    for (name, form, t), (x, ref) in refs.items():
        cs = R.CASES[name]
        got = R.standin(x["q"], x["k"], x["v"], cs["nh"], x["scale"], x["gate"], V.STORAGE[form], x["kmask"], cs["G"],
                        None if t is None else t + 1)
        ratio = V.assert_within(got.double().numpy(), ref["out"], R.bound(ref, V.STORAGE[form]), "%s %s %s" % (name, form, t))
        worst[form] = max(worst[form], ratio)
        if not cs.get("special"):
            assert ref["ms"].min() > 0.1, (name, ref["ms"].min())          # far above eps = 1e-8
    print("stand-in: largest |err| / bound bf16 %.3f, fp32 %.3f" % (worst["bf16"], worst["fp32"]))


def test_special_rows(refs):
    """Rows 0, 1: no positive score -> exact zeros.  Rows 2 .. 5: one positive score per head of 0.05, 1, 20 and 3e-3 -> the
    value vector of that key over its RMS, whatever the score (up to eps / score^2 inside the rsqrt)."""
    x, ref = refs[("special", "fp32", None)]
    assert (ref["out"][:2] == 0).all() and (ref["ms"][:2] == 0).all()
    v, scale = x["v"].double().numpy(), x["scale"].double().numpy()
    nh, d, Lk = 2, 64, 9
    for b in range(2, 6):
        picked = np.concatenate([v[b, (b + h) % Lk, h * d:(h + 1) * d] for h in range(nh)])
        want = 0.5 * scale * picked / np.sqrt((picked ** 2).mean())
        tol = 1e-5 if b < 5 else 2e-3              # eps / ms = 1e-8 / (9e-6 mean v^2) for the score of 3e-3
        assert np.abs(ref["out"][b, 0] - want).max() <= tol * np.abs(want).max(), b


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_each_planted_defect_is_outside_the_bound_somewhere(refs, defect):
    caught = []
    for (name, form, t), (x, ref) in refs.items():
        if not _applies(defect, name, t):
            continue
        bad = R.case_reference(name, x, t, defect=defect)
        try:
            V.assert_within(bad["out"], ref["out"], R.bound(ref, V.STORAGE[form]), defect)
        except AssertionError:
            caught.append((name, form, t))
    print("%s: outside the bound on %s" % (defect, caught))
    assert caught, defect


def test_masked_keys_of_the_cross_case_score_high():
    """The inputs that make the mask matter: the masked keys of sentence 1 score far above the valid ones."""
    x = R.case_inputs("cross", "bf16")
    cs = R.CASES["cross"]
    q, k = x["q"].double().numpy(), x["k"].double().numpy()
    s = np.einsum("bihd,jhd->bhij", q[3:].reshape(3, 1, cs["nh"], cs["d"]), k[1].reshape(-1, cs["nh"], cs["d"])) * cs["d"] ** -0.5
    assert s[..., 6:].min() > 2.0 and s[..., 6:].min() > 2 * np.abs(s[..., :6]).mean()


# ---------------------------------------------------------------------------------------------- the reference's two paths
def _tiny():
    hp = make_hp("transformer_rela", H=32, F=64, heads=2, layers=2, Vs=40, Vt=36, search_mode="cache")
    return hp, rt.to_torch(R.init_params(hp, 7), dtype=torch.float64)


def test_cached_steps_equal_the_full_sequence_decoder_and_source_padding_changes_nothing():
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

    def cached(source):
        enc, dec = R.decoding_fns(hp, P)
        state = enc(torch.as_tensor(source))
        steps = []
        for t in range(Lt):
            tok = gold[:, t - 1:t] if t else torch.full((B, 1), hp.tgt_vocab.pad(), dtype=torch.long)
            logits, state = dec(tok, state, t)
            steps.append(logits)
        return torch.stack(steps, 1)
    inc = cached(src)
    assert float((inc - full).abs().max()) <= 1e-10 * float(full.abs().max())
    # extra masked source positions (garbage encoder rows behind every sentence, mask 0): the multiplied mask gives them the
    # weight 0 exactly, in the full-sequence decoder and in the cached steps
    m = (torch.as_tensor(src) != 0).double()
    st = R.encoder(torch.as_tensor(src), hpc, P)
    enc_pad = torch.cat([st["encodes"], torch.randn(B, 4, hp.hidden_size, dtype=torch.float64) * 5], 1)
    st_pad = {"encodes": enc_pad, "mask": torch.cat([m, torch.zeros(B, 4, dtype=torch.float64)], 1)}
    full_pad = R.full_decoder(gold, st_pad, hpc, P)
    assert float((full_pad - full).abs().max()) <= 1e-12 * float(full.abs().max())
    _, dec = R.decoding_fns(hp, P)
    state = dict(st_pad, decoder={"state": st["decoder_initializer"]})
    for t in range(Lt):
        tok = gold[:, t - 1:t] if t else torch.full((B, 1), hp.tgt_vocab.pad(), dtype=torch.long)
        logits, state = dec(tok, state, t)
        assert float((logits - inc[:, t]).abs().max()) <= 1e-12 * float(full.abs().max()), t


# ---------------------------------------------------------------------------------------------- layout and refusals
def _expected_names(hp, shared):
    """Written out from models/transformer_rela.py and modules/rela.py:34-84 (creation order)."""
    names = ["embedding" if shared else "src_embedding", "bias"]
    ln = lambda p: [p + "/layer_norm/scale", p + "/layer_norm/offset"]
    ffn = lambda p: [p + "/ffn_layer/enlarge/W_0_0", p + "/ffn_layer/enlarge/b_0", p + "/ffn_layer/output/W_0_0",
                     p + "/ffn_layer/output/b_0"] + ln(p)

    def att(p, maps):
        a = p + "/dot_attention/"
        out = []
        for m in maps:
            out += [a + m + "/W_0_0", a + m + "/b_0"]
        return out + [a + "post/scale", a + "post/gate", a + "o_map/W_0_0", a + "o_map/b_0"] + ln(p)
    for l in range(hp.num_encoder_layer):
        names += att("encoder/layer_%d/self_attention" % l, ["qkv_map"]) + ffn("encoder/layer_%d/feed_forward" % l)
    if not shared:
        names.append("tgt_embedding")
    for l in range(hp.num_decoder_layer):
        names += att("decoder/layer_%d/self_attention" % l, ["qkv_map"])
        names += att("decoder/layer_%d/cross_attention" % l, ["q_map", "k_map", "v_map"])
        names += ffn("decoder/layer_%d/feed_forward" % l)
    if not shared and not hp.shared_target_softmax_embedding:
        names.append("softmax_embedding")
    return names


@pytest.mark.parametrize("shared", [False, True])
def test_variable_specs(shared):
    from zero_amd.variables import variable_specs, initial_values
    hp = make_hp("transformer_rela", shared_source_target_embedding=shared)
    if shared:
        hp.tgt_vocab = hp.src_vocab
    specs = variable_specs(hp, "transformer_rela")
    names = [s[0] for s in specs]
    assert names == _expected_names(hp, shared)
    H = hp.hidden_size
    shapes = {s[0]: s[1] for s in specs}
    post = [n for n in names if "/post/" in n]
    assert len(post) == 2 * (hp.num_encoder_layer + 2 * hp.num_decoder_layer) and all(shapes[n] == (H,) for n in post)
    base = variable_specs(hp, "transformer")
    assert [s for s in specs if "/post/" not in s[0]] == base          # `transformer` is a subsequence, shapes and kinds too
    vals = initial_values(hp, "transformer_rela", 11)
    for n in post:
        if n.endswith("scale"):
            assert (vals[n] == 1).all()
        else:
            assert vals[n].std() > 0 and np.abs(vals[n]).max() < 1.0          # drawn, not constant


def test_decode_only_refusals_touch_no_device(monkeypatch):
    from zero_amd.models import model as registry, load_all, _factory
    load_all()
    monkeypatch.setattr(_factory, "get_core", lambda *a, **k: pytest.fail("a refusal built a core"))
    triple = registry.get_model("transformer_rela")
    hp = make_hp("transformer_rela")
    feats = {"source": np.ones((1, 2)), "target": np.ones((1, 2))}
    with pytest.raises(NotImplementedError, match="backward of the ReLU"):
        triple.train_fn(feats, hp)
    with pytest.raises(NotImplementedError, match="gated RMSNorm"):
        triple.score_fn(feats, hp)
    hp.search_mode = "dev"
    with pytest.raises(NotImplementedError, match="training-path decoder"):
        triple.infer_fn(hp)
    from zero_amd.models import _ensemble
    with pytest.raises(NotImplementedError, match="transformer_rela"):
        _ensemble.check_members([make_hp("transformer"), make_hp("transformer_rela")])
