"""deepnmt on the host: registry and refusals, variable specs over every switch, and the references of tests/deepnmt_ref.py
checked on their own (every planted ff + residual defect against the bound, the stand-in inside it, the cached step against the
teacher-forced decoder for each layer form, the feature position, the model fixtures' measured margins)."""
import copy

import numpy as np
import pytest
import torch

from oracle import ref_torch as rt
from tests import deepnmt_ref as D
from tests import variant_ref as V
from tests.common import make_hp

MODEL = "deepnmt"


def _tiny(cell="atr", NE=2, ND=2, E=8, **kw):
    hp = make_hp(MODEL, H=12, heads=1, Vs=11, Vt=9, cell=cell, layer_norm=False, search_mode="cache", num_encoder_layer=NE,
                 num_decoder_layer=ND, **kw)
    hp.embed_size = E
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
    with pytest.raises(NotImplementedError, match="deepnmt.*backward of the recurrent scans"):
        triple.train_fn(feats, hp)
    with pytest.raises(NotImplementedError, match="deepnmt.*teacher-forced decoder scan"):
        triple.score_fn(feats, hp)
    for key, value, what in (("cell", "lstm", "deepnmt.*cell=atr.*cell=gru.*lstm"),
                             ("cell", "sru", "deepnmt.*sru"),
                             ("layer_norm", True, "deepnmt.*layer_norm=True"),
                             ("num_heads", 2, "deepnmt.*num_heads=1.*num_heads=2"),
                             ("search_mode", "dev", "deepnmt.*search_mode=cache only")):
        bad = copy.copy(hp)
        setattr(bad, key, value)
        with pytest.raises(NotImplementedError, match=what):
            triple.infer_fn(bad)
    for key in ("num_encoder_layer", "num_decoder_layer"):
        bad = copy.copy(hp)
        setattr(bad, key, 0)
        with pytest.raises(ValueError, match="deepnmt.*%s >= 1" % key):
            triple.infer_fn(bad)
    for cell in ("atr", "gru"):                       # the supported settings build the closures without a core
        for ca, deep, redict in ((True, False, True), (False, True, False), (False, False, True)):
            enc, dec = triple.infer_fn(_tiny(cell, caencoder=ca, use_deep_att=deep, dl4mt_redict=redict))
            assert callable(enc) and callable(dec) and callable(dec.step_static)
    enc, dec = triple.infer_fn(_tiny(E=12))           # hidden_size == embed_size too
    assert callable(enc)
    from zero_amd.models import _ensemble
    with pytest.raises(NotImplementedError, match="member 1 is a deepnmt"):
        _ensemble.check_members([make_hp("transformer"), _tiny()])


def test_get_core_knows_the_name():
    from zero_amd.models import _factory
    from zero_amd.models._deepnmt import DeepNmtCore
    assert _factory._core_class(MODEL) is DeepNmtCore


# ---------------------------------------------------------------------------------------------- variables
def _expected(c, NE, ND, ca, deep, redict, shared, soft_shared, E):
    H, Vs, Vt = 12, 11, 11 if shared else 9

    def fetch(pre, s, width):
        p = pre + "fetch_state_%s/" % s
        return ([(p + "gate_x/W_0_0", (width, 2 * H))] if c == "gru" else []) + [(p + "hide_x/W_0_0", (width, H))]

    def rec(pre, s):
        p = pre + "cell_%s/" % s
        gate = [(p + "gate_h/W_0_0", (H, 2 * H)), (p + "gate_h/b_0", (2 * H,))] if c == "gru" else []
        return gate + [(p + "hide_h/W_0_0", (H, H)), (p + "hide_h/b_0", (H,))]
    lin = lambda p, a, b: [(p + "W_0_0", (a, b)), (p + "b_0", (b,))]
    v = [("embedding" if shared else "src_embedding", (Vs, E)), ("bias", (E,))]
    for l in range(NE):
        p = "encoder/layer_%d/" % l
        v += fetch(p + "forward/", c, E) + rec(p + "forward/", c)
        if l == 0 and ca:         # cond_rnn: both input projections in front of tf.scan, the recurrent maps inside it
            b = p + "backward/"
            v += fetch(b, c + "_lower", E) + fetch(b, c + "_higher", H) + rec(b, c + "_lower") + rec(b, c + "_higher")
        elif l == 0:
            v += fetch(p + "backward/", c, E) + rec(p + "backward/", c)
        v += lin(p + "ff/", 2 * H if (l == 0 and not ca) else H, E)
    if E != H:
        v += lin("x_map/", E, H) + [("layer_norm/scale", (H,)), ("layer_norm/offset", (H,))]
    for l in range(ND):
        v += lin("layer_%d_init/" % l, 2 * H if (NE == 1 and not ca) else H, H)
    if not shared:
        v.append(("tgt_embedding", (Vt, E)))
    for l in range(ND):
        p = "decoder/layer_%d/" % l
        if l == 0 or deep:
            v += fetch(p, c + "_lower", E) + [(p + "context_att/W_0_0", (H, H))] + rec(p, c + "_lower")
            v += lin(p + "attention/feed_query/", H, H) + lin(p + "attention/feed_logits/", H, 1)
            v += fetch(p, c + "_higher", H) + rec(p, c + "_higher")
        elif ca:
            v += fetch(p, c + "_lower", E) + fetch(p, c + "_higher", H) + rec(p, c + "_lower") + rec(p, c + "_higher")
        else:
            v += fetch(p, c, E + H) + rec(p, c)
        v += lin(p + "ff/", H, E)
    if redict:
        v += lin("ff/", E + H, E)
    if not shared and not soft_shared:
        v.append(("softmax_embedding", (Vt, E)))
    return v


@pytest.mark.parametrize("cell", ["atr", "gru"])
@pytest.mark.parametrize("NE,ND", [(1, 1), (2, 3), (1, 3), (2, 1)])
@pytest.mark.parametrize("ca,deep,redict", [(True, False, True), (False, False, False), (False, True, True), (True, True, False)])
@pytest.mark.parametrize("shared,soft_shared,E", [(False, True, 8), (False, False, 12), (True, True, 8)])
def test_variable_specs(cell, NE, ND, ca, deep, redict, shared, soft_shared, E):
    from zero_amd.variables import variable_specs, initial_values
    hp = _tiny(cell, NE, ND, E, caencoder=ca, use_deep_att=deep, dl4mt_redict=redict, shared_source_target_embedding=shared,
               shared_target_softmax_embedding=soft_shared)
    if shared:
        hp.tgt_vocab = hp.src_vocab
    specs = variable_specs(hp, MODEL)                 # hidden_size != embed_size: taken before the Transformer's H == E test
    assert [(n, s) for n, s, _, _ in specs] == _expected(cell, NE, ND, ca, deep, redict, shared, soft_shared, E)
    assert len({n for n, _, _, _ in specs}) == len(specs)
    vals = initial_values(hp, MODEL, 5)
    for n, _, k, _ in specs:
        if n.endswith("/b_0") or n.endswith("/offset"):
            assert k == "zeros" and not vals[n].any(), n
        elif n.endswith("/scale"):
            assert k == "ones" and (vals[n] == 1).all(), n
        elif "embedding" in n:
            assert k == "embed_w", n
        else:
            assert k == "w" and vals[n].std() > 0, n


def test_variable_names_spelled_out():
    """Names and shapes written out by hand (the helper above shares its structure with the code under test): the defaults'
    form with gru, H = 12, E = 8, NE = 2, ND = 2."""
    from zero_amd.variables import variable_specs
    specs = variable_specs(_tiny("gru", 2, 2, caencoder=True, use_deep_att=False, dl4mt_redict=True,
                                 shared_target_softmax_embedding=False), MODEL)
    names = [n for n, _, _, _ in specs]
    shape = {n: s for n, s, _, _ in specs}
    assert names[:4] == ["src_embedding", "bias", "encoder/layer_0/forward/fetch_state_gru/gate_x/W_0_0",
                         "encoder/layer_0/forward/fetch_state_gru/hide_x/W_0_0"]
    assert names[8:12] == ["encoder/layer_0/backward/fetch_state_gru_lower/gate_x/W_0_0",
                           "encoder/layer_0/backward/fetch_state_gru_lower/hide_x/W_0_0",
                           "encoder/layer_0/backward/fetch_state_gru_higher/gate_x/W_0_0",
                           "encoder/layer_0/backward/fetch_state_gru_higher/hide_x/W_0_0"]
    assert names[12] == "encoder/layer_0/backward/cell_gru_lower/gate_h/W_0_0"
    assert shape["encoder/layer_0/backward/fetch_state_gru_higher/gate_x/W_0_0"] == (12, 24)
    assert names[20:22] == ["encoder/layer_0/ff/W_0_0", "encoder/layer_0/ff/b_0"] and shape["encoder/layer_0/ff/W_0_0"] == (12, 8)
    assert "encoder/layer_1/backward/fetch_state_gru/hide_x/W_0_0" not in names
    i = names.index("x_map/W_0_0")
    assert names[i - 1] == "encoder/layer_1/ff/b_0"
    assert names[i:i + 6] == ["x_map/W_0_0", "x_map/b_0", "layer_norm/scale", "layer_norm/offset",
                              "layer_0_init/W_0_0", "layer_0_init/b_0"]
    assert shape["x_map/W_0_0"] == (8, 12) and shape["layer_1_init/W_0_0"] == (12, 12)
    # models/deepnmt.py:86-98: the `decoder_initializer` scope only builds the cell; get_init_state runs behind it, at model scope
    assert not any(n.startswith("decoder_initializer/") for n in names)
    assert names[i + 6:i + 9] == ["layer_1_init/W_0_0", "layer_1_init/b_0", "tgt_embedding"]
    j = names.index("decoder/layer_0/context_att/W_0_0")
    assert names[j - 1] == "decoder/layer_0/fetch_state_gru_lower/hide_x/W_0_0"
    assert names[j + 1] == "decoder/layer_0/cell_gru_lower/gate_h/W_0_0"
    k = names.index("decoder/layer_0/attention/feed_logits/b_0")
    assert names[k + 1] == "decoder/layer_0/fetch_state_gru_higher/gate_x/W_0_0" and shape[names[k]] == (1,)
    assert shape["decoder/layer_1/fetch_state_gru_higher/hide_x/W_0_0"] == (12, 12)
    assert "decoder/layer_1/context_att/W_0_0" not in names
    assert names[-4:] == ["decoder/layer_1/ff/b_0", "ff/W_0_0", "ff/b_0", "softmax_embedding"] and shape["ff/W_0_0"] == (20, 8)
    plain = {n: s for n, s, _, _ in variable_specs(_tiny("atr", 1, 2, caencoder=False, dl4mt_redict=False), MODEL)}
    assert plain["decoder/layer_1/fetch_state_atr/hide_x/W_0_0"] == (20, 12) and "ff/W_0_0" not in plain
    assert plain["encoder/layer_0/ff/W_0_0"] == (24, 8) and plain["layer_0_init/W_0_0"] == (24, 12)
    assert not any("gate_" in n for n in plain)


# ---------------------------------------------------------------------------------------------- ff + residual reference
@pytest.mark.parametrize("form", ["bf16", "fp32"])
def test_ff_reference_standin_and_defects(form):
    x = D.ff_inputs(9, 40, 40, form, 0)               # K = N (w_transposed), K % 32 = 8 (k_tail_dropped)
    ref = D.ff_residual(**x)
    for copy_ in (False, True):
        got = D.ff_residual_standin(form=form, copy=copy_, **x)
        assert V.assert_within(got, ref["out"], D.ff_residual_bound(ref, form, copy_), "stand-in %s copy=%s" % (form, copy_)) <= 1.0
    for d in D.FF_DEFECTS:
        bad = D.ff_residual(defect=d, **x)
        if d == "copy_of_product":                    # out is right, the copy is not
            assert not V.exceeds(bad["out"], ref["out"], D.ff_residual_bound(ref, form))
            assert V.exceeds(bad["copy_src"], ref["out"], D.ff_residual_bound(ref, form, True)), d
        else:
            assert V.exceeds(bad["out"], ref["out"], D.ff_residual_bound(ref, form)), d


def test_ff_bound_catches_a_bf16_stream_with_w_zero():
    """W = 0, b = 0: out is x.  With an x that is not bf16-representable the reference is x bit for bit, the bound is far below
    a bf16 ulp, and a stream kept in bf16 is outside it -- in BOTH forms."""
    for form in ("bf16", "fp32"):
        x = D.ff_inputs(5, 16, 24, form, 1, zero_w=True)
        ref = D.ff_residual(**x)
        assert np.array_equal(ref["out"], x["x"])
        bound = D.ff_residual_bound(ref, form)
        assert bound.max() < 2.0 ** -16
        assert np.array_equal(D.ff_residual_standin(form=form, **x), x["x"])
        assert V.exceeds(D.ff_residual(defect="bf16_stream", **x)["out"], ref["out"], bound)


# ---------------------------------------------------------------------------------------------- the model restated
FORMS = {"one2one": dict(caencoder=True, use_deep_att=False), "plain": dict(caencoder=False, use_deep_att=False),
         "att": dict(caencoder=True, use_deep_att=True)}


@pytest.mark.parametrize("cell", ["atr", "gru"])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("redict", [True, False])
def test_full_decoder_equals_the_cached_steps(cell, form, redict):
    """float64: the teacher-forced decoder (every layer one scan over the whole target) and the cached step fed the same
    tokens one at a time give the same logits, for each form of the layers >= 1; the source's padding columns change nothing."""
    hp = _tiny(cell, 2, 3, dl4mt_redict=redict, **FORMS[form])
    assert D.form_of(hp, 0) == "att" and D.form_of(hp, 2) == form
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
    ragged = D.encoder(src, hp, P)                                         # a padded position carries every scan's state
    alone = D.encoder(src[1:2, :3], hp, P)
    assert torch.allclose(ragged["encodes"][1, :3], alone["encodes"][0], rtol=0, atol=1e-12)
    for l in range(3):
        assert torch.allclose(ragged["decoder_initializer"]["layer_%d" % l][1], alone["decoder_initializer"]["layer_%d" % l][0],
                              rtol=0, atol=1e-12)


@pytest.mark.parametrize("NE", [1, 2])
@pytest.mark.parametrize("ca", [True, False])
def test_encoder_feature_is_the_last_scanned_state(NE, ca):
    """z: position Ls - 1 of a forward scan (NE = 2), position 0 of layer 0's backward scan with caencoder, [f_{Ls-1} | b_0]
    for NE = 1 without it -- recomputed here from the stream by hand for the last layer (unpadded sources)."""
    hp = _tiny("atr", NE, 2, caencoder=ca)
    H = hp.hidden_size
    P = rt.to_torch(D.init_params(hp, 4), dtype=torch.float64)
    src = torch.as_tensor(V.ragged((5, 5), hp.src_vocab.size(), 1))
    st = D.encoder(src, hp, P, return_z=True)
    z = st["z"]
    assert z.shape == (2, 2 * H if (NE == 1 and not ca) else H)
    assert st["encodes"].shape == (2, 5, H) and sorted(st["pm"]) == [0]
    for l in range(2):
        i = "layer_%d_init" % l
        assert torch.allclose(st["decoder_initializer"]["layer_%d" % l], z @ P[i + "/W_0_0"] + P[i + "/b_0"], rtol=0, atol=1e-12)
    x = P["src_embedding"][src] + P["bias"]
    ys = []
    for l in range(NE):                               # re-run the layers, keeping y of each
        pre = "encoder/layer_%d/" % l
        inp = D.cell_fetch(x, P, pre + "forward/", "atr", "atr")
        h = torch.zeros(2, H, dtype=torch.float64)
        fw = []
        for t in range(5):
            h = D.cell_call(h, (inp[0][:, t],), P, pre + "forward/", "atr", "atr")
            fw.append(h)
        fw = torch.stack(fw, 1)
        if l == 0 and ca:
            b = pre + "backward/"
            lo, hi = D.cell_fetch(x, P, b, "atr_lower", "atr"), D.cell_fetch(fw, P, b, "atr_higher", "atr")
            g = torch.zeros(2, H, dtype=torch.float64)
            gs = [None] * 5
            for t in range(4, -1, -1):
                s = D.cell_call(g, (lo[0][:, t],), P, b, "atr_lower", "atr")
                g = D.cell_call(s, (hi[0][:, t],), P, b, "atr_higher", "atr")
                gs[t] = g
            y = torch.stack(gs, 1)
        elif l == 0:
            inp = D.cell_fetch(x, P, pre + "backward/", "atr", "atr")
            h = torch.zeros(2, H, dtype=torch.float64)
            bw = [None] * 5
            for t in range(4, -1, -1):
                h = D.cell_call(h, (inp[0][:, t],), P, pre + "backward/", "atr", "atr")
                bw[t] = h
            y = torch.cat([fw, torch.stack(bw, 1)], -1)
        else:
            y = fw
        ys.append(y)
        x = x + (y @ P[pre + "ff/W_0_0"] + P[pre + "ff/b_0"])
    y = ys[-1]
    if NE == 2:
        want = y[:, 4]
    elif ca:
        want = y[:, 0]
    else:
        want = torch.cat([y[:, 4, :H], y[:, 0, H:]], -1)
    assert torch.allclose(z, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("config", sorted(D.CONFIGS))
def test_model_fixture_margins(config):
    """The measurements the GPU model tests rest on (recorded in tests/deepnmt_ref.py), re-made on every CPU run."""
    hp = D.fixture_hp(config)
    want = D.CONFIGS[config]
    assert (hp.num_encoder_layer, hp.num_decoder_layer, hp.hidden_size, hp.embed_size) == \
        (want["num_encoder_layer"], want["num_decoder_layer"], want["H"], want["E"])
    f = D.make_fixture(hp, V.ragged(D.LENGTHS, hp.src_vocab.size(), 5), D.SEEDS[config])
    print("config %s: gap %.3e err %.3e rel %.3f" % (config, f["gap"], f["err"], f["rel"]))
    assert f["gap"] > 4 * f["err"]
    rtol, atol = D.score_tol(f["rel"], f["err"])
    assert rtol == D.RTOL and (atol == D.ATOL if f["rel"] <= 0.25 else atol == 4 * f["err"])
