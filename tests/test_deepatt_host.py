"""rnnsearch_deepatt on the host: registry and refusals, variable specs for both cells, and the references of
tests/deepatt_ref.py checked on their own (every planted GRU defect against the bound, the stand-in inside it, the cached step
against the teacher-forced decoder, the model fixture's measured margins)."""
import copy

import numpy as np
import pytest
import torch

from oracle import ref_torch as rt
from tests import deepatt_ref as D
from tests import variant_ref as V
from tests.common import make_hp

MODEL = "rnnsearch_deepatt"


def _tiny(cell="gru", NE=2, ND=2, **kw):
    hp = make_hp(MODEL, H=12, heads=1, Vs=11, Vt=9, cell=cell, layer_norm=False, search_mode="cache", num_encoder_layer=NE,
                 num_decoder_layer=ND, **kw)
    hp.embed_size = 8
    return hp


# ---------------------------------------------------------------------------------------------- registry and refusals
def test_registered_and_refusals_touch_no_device(monkeypatch):
    from zero_amd.models import model as registry, load_all, _factory
    load_all()
    monkeypatch.setattr(_factory, "get_core", lambda *a, **k: pytest.fail("a refusal built a core"))
    triple = registry.get_model(MODEL)
    assert callable(triple.train_fn) and callable(triple.score_fn) and callable(triple.infer_fn)
    hp = _tiny()
    feats = {"source": np.ones((1, 2)), "target": np.ones((1, 2))}
    with pytest.raises(NotImplementedError, match="rnnsearch_deepatt.*backward of the recurrent scans"):
        triple.train_fn(feats, hp)
    with pytest.raises(NotImplementedError, match="rnnsearch_deepatt.*teacher-forced decoder scan"):
        triple.score_fn(feats, hp)
    for key, value, what in (("cell", "lstm", "rnnsearch_deepatt.*cell=atr.*cell=gru.*lstm"),
                             ("cell", "sru", "rnnsearch_deepatt.*sru"),
                             ("layer_norm", True, "rnnsearch_deepatt.*layer_norm=True.*LayerNorm behind every product"),
                             ("num_heads", 2, "rnnsearch_deepatt.*num_heads=1.*num_heads=2"),
                             ("search_mode", "dev", "rnnsearch_deepatt.*search_mode=cache only")):
        bad = copy.copy(hp)
        setattr(bad, key, value)
        with pytest.raises(NotImplementedError, match=what):
            triple.infer_fn(bad)
    for cell in ("atr", "gru"):                       # the supported settings build the closures without a core
        enc, dec = triple.infer_fn(_tiny(cell))
        assert callable(enc) and callable(dec) and callable(dec.step_static)
    from zero_amd.models import _ensemble
    with pytest.raises(NotImplementedError, match="member 1 is a rnnsearch_deepatt"):
        _ensemble.check_members([make_hp("transformer"), _tiny()])


def test_rnnsearch_keeps_its_own_refusals():
    """The GRU cell arrives under the new name only."""
    from zero_amd.models import model as registry, load_all
    load_all()
    hp = _tiny("gru")
    hp.model_name = "rnnsearch"
    with pytest.raises(NotImplementedError, match="rnnsearch.*cell=atr only.*gru"):
        registry.get_model("rnnsearch").infer_fn(hp)


# ---------------------------------------------------------------------------------------------- variables
def _expected(cell, NE, ND, shared, soft_shared):
    H, E, Vs, Vt = 12, 8, 11, 11 if shared else 9
    c = cell

    def fetch(pre, s, width):
        p = pre + "fetch_state_%s/" % s
        return ([(p + "gate_x/W_0_0", (width, 2 * H))] if c == "gru" else []) + [(p + "hide_x/W_0_0", (width, H))]

    def rec(pre, s):
        p = pre + "cell_%s/" % s
        gate = [(p + "gate_h/W_0_0", (H, 2 * H)), (p + "gate_h/b_0", (2 * H,))] if c == "gru" else []
        return gate + [(p + "hide_h/W_0_0", (H, H)), (p + "hide_h/b_0", (H,))]
    v = [("embedding" if shared else "src_embedding", (Vs, E)), ("bias", (E,))]
    v += fetch("encoder/layer_0/", c, E) + rec("encoder/layer_0/", c)
    for l in range(1, NE + 1):
        p = "encoder/layer_%d/" % l
        # cond_rnn: both input projections in front of tf.scan, the recurrent maps inside it
        v += fetch(p, c + "_lower", E) + fetch(p, c + "_higher", H) + rec(p, c + "_lower") + rec(p, c + "_higher")
    v += [("decoder_initializer/dec_init_state_init/W_0_0", (H, H)), ("decoder_initializer/dec_init_state_init/b_0", (H,))]
    if not shared:
        v.append(("tgt_embedding", (Vt, E)))
    v += fetch("decoder/", c + "_lower", E) + [("decoder/context_att/W_0_0", (H, H))] + rec("decoder/", c + "_lower")
    for l in range(ND):
        a = "decoder/deep_attention_%d/" % l
        v += [(a + "feed_query/W_0_0", (H, H)), (a + "feed_query/b_0", (H,)),
              (a + "feed_logits/W_0_0", (H, 1)), (a + "feed_logits/b_0", (1,))]
        v += fetch("decoder/", "%s_higher_%d" % (c, l), H) + rec("decoder/", "%s_higher_%d" % (c, l))
    v += [("ff/W_0_0", (H + ND * H + E, E)), ("ff/b_0", (E,))]
    if not shared and not soft_shared:
        v.append(("softmax_embedding", (Vt, E)))
    return v


@pytest.mark.parametrize("cell", ["atr", "gru"])
@pytest.mark.parametrize("NE,ND", [(0, 1), (2, 2), (2, 1), (0, 2)])
@pytest.mark.parametrize("shared,soft_shared", [(False, True), (False, False), (True, True)])
def test_variable_specs(cell, NE, ND, shared, soft_shared):
    from zero_amd.variables import variable_specs, initial_values
    hp = _tiny(cell, NE, ND, shared_source_target_embedding=shared, shared_target_softmax_embedding=soft_shared)
    if shared:
        hp.tgt_vocab = hp.src_vocab
    specs = variable_specs(hp, MODEL)                 # hidden_size != embed_size: taken before the Transformer's H == E test
    assert [(n, s) for n, s, _, _ in specs] == _expected(cell, NE, ND, shared, soft_shared)
    assert len({n for n, _, _, _ in specs}) == len(specs)
    vals = initial_values(hp, MODEL, 5)
    for n, _, k, _ in specs:
        if n.endswith("/b_0"):
            assert k == "zeros" and not vals[n].any(), n
        elif "embedding" in n:
            assert k == "embed_w", n
        else:
            assert k == "w" and vals[n].std() > 0, n


def test_variable_names_spelled_out():
    """A few names written out by hand (the helper above shares its structure with the code under test)."""
    from zero_amd.variables import variable_specs
    names = [n for n, _, _, _ in variable_specs(_tiny("gru", 1, 1), MODEL)]
    assert names[2:8] == ["encoder/layer_0/fetch_state_gru/gate_x/W_0_0", "encoder/layer_0/fetch_state_gru/hide_x/W_0_0",
                          "encoder/layer_0/cell_gru/gate_h/W_0_0", "encoder/layer_0/cell_gru/gate_h/b_0",
                          "encoder/layer_0/cell_gru/hide_h/W_0_0", "encoder/layer_0/cell_gru/hide_h/b_0"]
    assert names[8] == "encoder/layer_1/fetch_state_gru_lower/gate_x/W_0_0"
    assert names[10] == "encoder/layer_1/fetch_state_gru_higher/gate_x/W_0_0"
    assert names[12] == "encoder/layer_1/cell_gru_lower/gate_h/W_0_0"
    i = names.index("decoder/context_att/W_0_0")
    assert names[i - 1] == "decoder/fetch_state_gru_lower/hide_x/W_0_0" and names[i + 1] == "decoder/cell_gru_lower/gate_h/W_0_0"
    j = names.index("decoder/deep_attention_0/feed_query/W_0_0")
    assert names[j + 4:j + 7] == ["decoder/fetch_state_gru_higher_0/gate_x/W_0_0", "decoder/fetch_state_gru_higher_0/hide_x/W_0_0",
                                  "decoder/cell_gru_higher_0/gate_h/W_0_0"]
    assert names[-3:] == ["ff/W_0_0", "ff/b_0", "softmax_embedding"] or names[-2:] == ["ff/W_0_0", "ff/b_0"]
    atr = [n for n, _, _, _ in variable_specs(_tiny("atr", 1, 1), MODEL)]
    assert "decoder/cell_atr_higher_0/hide_h/W_0_0" in atr and not any("gate_" in n for n in atr)


# ---------------------------------------------------------------------------------------------- the GRU reference
def _gru_inputs(R_, H, seed, n_prev=None):
    g = np.random.default_rng(seed)
    n_prev = R_ if n_prev is None else n_prev
    bf = lambda x: torch.as_tensor(x).float().to(torch.bfloat16).double().numpy()
    f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)
    return dict(h_prev=f32(g.normal(0, 1, (n_prev, H))), Ug=bf(g.normal(0, H ** -0.5, (H, 2 * H))), bg=f32(g.normal(0, 0.3, 2 * H)),
                Uh=bf(g.normal(0, H ** -0.5, (H, H))), bh=f32(g.normal(0, 0.3, H)), xg=bf(g.normal(0, 1, (R_, 2 * H))),
                xh=bf(g.normal(0, 1, (R_, H))), mask=(g.random(R_) < 0.6).astype(np.float64), idx=g.integers(0, n_prev, R_))


OUTPUTS = ("z", "rh", "out", "copy")


@pytest.mark.parametrize("form", ["bf16", "fp32"])
def test_gru_reference_standin_and_defects(form):
    x = _gru_inputs(9, 24, 0)
    x["mask"][:2] = (0.0, 1.0)
    x["idx"][:3] = (4, 4, 0)                          # repeats, and rows that differ from their own index
    ref = D.gru_step(**x)
    got = D.gru_standin(form=form, **x)
    for what in OUTPUTS:
        worst = V.assert_within(got[what], ref["out" if what == "copy" else what], D.gru_bound(ref, form, what),
                                "stand-in %s %s" % (form, what))
        assert worst <= 1.0
    carried = x["mask"] == 0
    assert (D.gru_bound(ref, form)[carried] == 0).all() and np.array_equal(ref["out"][carried], ref["h"][carried])
    assert np.array_equal(got["out"][carried], ref["h"][carried])
    for d in D.GRU_DEFECTS:
        bad = D.gru_step(defect=d, **x)["out"]
        assert V.exceeds(bad, ref["out"], D.gru_bound(ref, form)), d          # (the fp32 state: what the next step reads)
    # the zero state: no product, rh = 0, out = (1 - z) tanh(xh + bh)
    z0 = dict(x, h_prev=None, idx=None)
    ref0 = D.gru_step(**z0)
    assert not ref0["h"].any() and not ref0["rh"].any() and np.allclose(ref0["q"], x["bh"][None, :])
    got0 = D.gru_standin(form=form, **z0)
    for what in OUTPUTS:
        V.assert_within(got0[what], ref0["out" if what == "copy" else what], D.gru_bound(ref0, form, what), "zero state " + what)


def test_gru_bound_catches_a_bf16_state_with_u_zero():
    """Ug = Uh = 0: both products vanish, so the only place the state enters is z h and the carry -- in fp32.  A state that is
    not bf16-representable then shows a kernel that keeps (or reads) it in bf16, in BOTH forms."""
    x = _gru_inputs(5, 16, 1)
    x["Ug"], x["Uh"] = np.zeros_like(x["Ug"]), np.zeros_like(x["Uh"])
    x["h_prev"] = np.asarray(x["h_prev"] * (1 + 2.0 ** -12), np.float32).astype(np.float64)
    assert not np.array_equal(D._bf(x["h_prev"]), x["h_prev"])
    ref = D.gru_step(**x)
    for form in ("bf16", "fp32"):
        bound = D.gru_bound(ref, form)
        assert bound.max() < 2.0 ** -16
        V.assert_within(D.gru_standin(form=form, **x)["out"], ref["out"], bound, "stand-in, U = 0")
        assert V.exceeds(D.gru_step(defect="bf16_state", **x)["out"], ref["out"], bound)


# ---------------------------------------------------------------------------------------------- the model restated
@pytest.mark.parametrize("cell", ["atr", "gru"])
@pytest.mark.parametrize("NE,ND", [(2, 2), (0, 1), (1, 1)])
def test_full_decoder_equals_the_cached_steps(cell, NE, ND):
    """float64: the teacher-forced scan over a target and the cached step fed the same tokens one at a time give the same
    logits; the source's padding columns change nothing (the carry)."""
    hp = _tiny(cell, NE, ND)
    P = rt.to_torch(D.init_params(hp, 2), dtype=torch.float64)
    src = torch.as_tensor(V.ragged((6, 3, 5), hp.src_vocab.size(), 2))
    tgt = torch.as_tensor(np.random.default_rng(3).integers(3, hp.tgt_vocab.size(), (3, 5)))
    enc, dec = D.decoding_fns(hp, P)
    state = enc(src)
    full = D.full_decoder(tgt, state, hp, P)
    assert full.shape == (3, 5, hp.tgt_vocab.size())
    prev = torch.full((3, 1), hp.tgt_vocab.pad(), dtype=torch.long)
    for t in range(5):
        logits, state = dec(prev, state, t)
        assert torch.allclose(logits, full[:, t], rtol=0, atol=1e-12), t
        prev = tgt[:, t:t + 1]
    padded = torch.nn.functional.pad(src, (0, 3))
    assert torch.equal(enc(padded)["encodes"], enc(src)["encodes"])      # remove_invalid_seq drops the all-pad columns


@pytest.mark.parametrize("NE", [0, 1, 2])
def test_encoder_feature_is_the_last_scanned_state(NE):
    """The decoder's initial state comes from position 0 of the memory for odd NE and from the last position for even NE (the
    sources here are unpadded, so the last position is the last token)."""
    hp = _tiny("gru", NE, 1)
    P = rt.to_torch(D.init_params(hp, 4), dtype=torch.float64)
    src = torch.as_tensor(V.ragged((5, 5), hp.src_vocab.size(), 1))
    st = D.encoder(src, hp, P)
    i = "decoder_initializer/dec_init_state_init"
    pos = 0 if NE % 2 == 1 else src.shape[1] - 1
    want = st["encodes"][:, pos] @ P[i + "/W_0_0"] + P[i + "/b_0"]
    assert torch.allclose(st["decoder_initializer"], want, rtol=0, atol=1e-12)
    assert st["encodes"].shape == (2, 5, hp.hidden_size) and st["pm"].shape == (2, 5, hp.hidden_size)


@pytest.mark.parametrize("cell", ["atr", "gru"])
def test_model_fixture_margins(cell):
    """The measurements the GPU model tests rest on (recorded in tests/deepatt_ref.py), re-made on every CPU run."""
    hp = D.fixture_hp(cell)
    assert (hp.num_encoder_layer, hp.num_decoder_layer, hp.hidden_size, hp.embed_size) == (2, 2, 128, 64)
    f = D.make_fixture(hp, V.ragged(D.LENGTHS, hp.src_vocab.size(), 5), D.SEEDS[cell])
    print("cell=%s: gap %.3e err %.3e rel %.3f" % (cell, f["gap"], f["err"], f["rel"]))
    assert f["gap"] > 4 * f["err"]
    assert f["rel"] <= 0.25 and D.score_tol(f["rel"], f["err"]) == (D.RTOL, D.ATOL)
