"""The lrn / olrn cells on the host: registry and refusals of both models, variable specs over the switches the existing host
tests use, and the references of tests/lrn_ref.py checked on their own (every planted defect against the propagated bound, the
stand-in inside it, a scan against its chained single steps, the cached step against the teacher-forced decoder, the model
fixtures' measured margins)."""
import copy

import numpy as np
import pytest
import torch

from oracle import ref_torch as rt
from tests import deepatt_ref as DA
from tests import deepnmt_ref as DN
from tests import lrn_ref as L
from tests import variant_ref as V
from tests.common import make_hp

CELLS = ("lrn", "olrn")
WIDTH = {"lrn": 3, "olrn": 4}


def _tiny(model, cell, NE=2, ND=2, E=8, **kw):
    hp = make_hp(model, H=12, heads=1, Vs=11, Vt=9, cell=cell, layer_norm=False, search_mode="cache", num_encoder_layer=NE,
                 num_decoder_layer=ND, **kw)
    hp.embed_size = E
    return hp


# ---------------------------------------------------------------------------------------------- registry and refusals
@pytest.mark.parametrize("model", ["rnnsearch_deepatt", "deepnmt"])
def test_cells_are_admitted_without_a_core(model, monkeypatch):
    from zero_amd.models import model as registry, load_all, _factory
    load_all()
    monkeypatch.setattr(_factory, "get_core", lambda *a, **k: pytest.fail("infer_fn built a core"))
    triple = registry.get_model(model)
    for cell in CELLS:
        enc, dec = triple.infer_fn(_tiny(model, cell))
        assert callable(enc) and callable(dec) and callable(dec.step_static)
    for cell, what in (("lstm", model + ".*cell=atr.*cell=gru.*lstm"), ("sru", model + ".*sru")):
        with pytest.raises(NotImplementedError, match=what):
            triple.infer_fn(_tiny(model, cell))
    with pytest.raises(NotImplementedError, match="cell=lrn.*cell=olrn"):       # the refusal names what IS built
        triple.infer_fn(_tiny(model, "lstm"))
    for key, value in (("layer_norm", True), ("num_heads", 2)):                  # the other refusals hold for the new cells
        bad = _tiny(model, "lrn")
        setattr(bad, key, value)
        with pytest.raises(NotImplementedError, match=model):
            triple.infer_fn(bad)


def test_rnnsearch_still_refuses_the_new_cells():
    from zero_amd.models import model as registry, load_all
    load_all()
    for cell in CELLS:
        hp = _tiny("rnnsearch_deepatt", cell)
        hp.model_name = "rnnsearch"
        with pytest.raises(NotImplementedError, match="rnnsearch.*cell=atr only.*%s" % cell):
            registry.get_model("rnnsearch").infer_fn(hp)


def test_the_gru_size_limit_does_not_apply():
    """check_shape reads the model's name, core.cell, H, E and M only: the 2048 limit of the additive attention holds for every
    cell, the GRU's LDS limit is the GRU's, and the recipe's 1000 / 620 is taken by the fp32 mode and refused by the bf16 mode as
    for atr."""
    from zero_amd.models import _rnn as mod
    for model in ("rnnsearch_deepatt", "deepnmt"):
        core = lambda cell, H, E: type("C", (), {"model": model, "cell": cell, "H": H, "E": E, "M": H})()
        for cell in CELLS:
            mod.check_shape(core(cell, 1000, 624), False)
            mod.check_shape(core(cell, 1000, 620), True)
            with pytest.raises(ValueError, match="multiples of 8.*1000 and 620.*decode_dtype=float32 takes these"):
                mod.check_shape(core(cell, 1000, 620), False)
            mod.check_shape(core(cell, 2048, 64), False)
            with pytest.raises(ValueError, match="multiples of 8"):
                mod.check_shape(core(cell, 12, 8), False)
            with pytest.raises(ValueError, match="multiples of 4"):
                mod.check_shape(core(cell, 10, 8), True)
            with pytest.raises(ValueError, match="at most 2048"):
                mod.check_shape(core(cell, 2056, 64), False)


def test_engine_binding_exists():
    from zero_amd.func import Engine
    from zero_amd import hip
    assert callable(Engine.rnn_lrn_scan)
    assert {"zk_rnn_lrn_scan", "zk_f32_rnn_lrn_scan"} <= set(hip.lib().protos)
    text = open(hip.HEADER_PATH).read()
    for needle in ("rnns/lrn.py:32-53", "rnns/olrn.py:32-58", "rnns/rnn.py:41-49", "rnns/rnn.py:119-146"):
        assert needle in text, needle


# ---------------------------------------------------------------------------------------------- variables
def _deepatt_expected(c, NE, ND, shared, soft_shared):
    H, E, Vs, Vt = 12, 8, 11, 11 if shared else 9
    fetch = lambda pre, s, width: [(pre + "fetch_state_%s/hide_x/W_0_0" % s, (width, WIDTH[c] * H))]
    v = [("embedding" if shared else "src_embedding", (Vs, E)), ("bias", (E,))]
    v += fetch("encoder/layer_0/", c, E)
    for l in range(1, NE + 1):
        p = "encoder/layer_%d/" % l
        v += fetch(p, c + "_lower", E) + fetch(p, c + "_higher", H)
    v += [("decoder_initializer/dec_init_state_init/W_0_0", (H, H)), ("decoder_initializer/dec_init_state_init/b_0", (H,))]
    if not shared:
        v.append(("tgt_embedding", (Vt, E)))
    v += fetch("decoder/", c + "_lower", E) + [("decoder/context_att/W_0_0", (H, H))]
    for l in range(ND):
        a = "decoder/deep_attention_%d/" % l
        v += [(a + "feed_query/W_0_0", (H, H)), (a + "feed_query/b_0", (H,)),
              (a + "feed_logits/W_0_0", (H, 1)), (a + "feed_logits/b_0", (1,))]
        v += fetch("decoder/", "%s_higher_%d" % (c, l), H)
    v += [("ff/W_0_0", (H + ND * H + E, E)), ("ff/b_0", (E,))]
    if not shared and not soft_shared:
        v.append(("softmax_embedding", (Vt, E)))
    return v


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("NE,ND", [(0, 1), (2, 2), (2, 1), (0, 2)])
@pytest.mark.parametrize("shared,soft_shared", [(False, True), (False, False), (True, True)])
def test_deepatt_variable_specs(cell, NE, ND, shared, soft_shared):
    from zero_amd.variables import variable_specs, initial_values
    hp = _tiny("rnnsearch_deepatt", cell, NE, ND, shared_source_target_embedding=shared,
               shared_target_softmax_embedding=soft_shared)
    if shared:
        hp.tgt_vocab = hp.src_vocab
    specs = variable_specs(hp, "rnnsearch_deepatt")
    assert [(n, s) for n, s, _, _ in specs] == _deepatt_expected(cell, NE, ND, shared, soft_shared)
    assert not any("/cell_" in n for n, _, _, _ in specs)          # the reference creates no variable under cell_<s>
    vals = initial_values(hp, "rnnsearch_deepatt", 5)
    for n, _, k, _ in specs:
        if n.endswith("/b_0"):
            assert k == "zeros" and not vals[n].any(), n
        elif "embedding" in n:
            assert k == "embed_w", n
        else:
            assert k == "w" and vals[n].std() > 0, n


def _deepnmt_expected(c, NE, ND, ca, deep, redict, shared, soft_shared, E):
    H, Vs, Vt = 12, 11, 11 if shared else 9
    fetch = lambda pre, s, width: [(pre + "fetch_state_%s/hide_x/W_0_0" % s, (width, WIDTH[c] * H))]
    lin = lambda p, a, b: [(p + "W_0_0", (a, b)), (p + "b_0", (b,))]
    v = [("embedding" if shared else "src_embedding", (Vs, E)), ("bias", (E,))]
    for l in range(NE):
        p = "encoder/layer_%d/" % l
        v += fetch(p + "forward/", c, E)
        if l == 0 and ca:
            v += fetch(p + "backward/", c + "_lower", E) + fetch(p + "backward/", c + "_higher", H)
        elif l == 0:
            v += fetch(p + "backward/", c, E)
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
            v += fetch(p, c + "_lower", E) + [(p + "context_att/W_0_0", (H, H))]
            v += lin(p + "attention/feed_query/", H, H) + lin(p + "attention/feed_logits/", H, 1)
            v += fetch(p, c + "_higher", H)
        elif ca:
            v += fetch(p, c + "_lower", E) + fetch(p, c + "_higher", H)
        else:
            v += fetch(p, c, E + H)
        v += lin(p + "ff/", H, E)
    if redict:
        v += lin("ff/", E + H, E)
    if not shared and not soft_shared:
        v.append(("softmax_embedding", (Vt, E)))
    return v


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("NE,ND", [(1, 1), (2, 3), (1, 3), (2, 1)])
@pytest.mark.parametrize("ca,deep,redict", [(True, False, True), (False, False, False), (False, True, True), (True, True, False)])
@pytest.mark.parametrize("shared,soft_shared,E", [(False, True, 8), (False, False, 12), (True, True, 8)])
def test_deepnmt_variable_specs(cell, NE, ND, ca, deep, redict, shared, soft_shared, E):
    from zero_amd.variables import variable_specs
    hp = _tiny("deepnmt", cell, NE, ND, E, caencoder=ca, use_deep_att=deep, dl4mt_redict=redict,
               shared_source_target_embedding=shared, shared_target_softmax_embedding=soft_shared)
    if shared:
        hp.tgt_vocab = hp.src_vocab
    specs = variable_specs(hp, "deepnmt")
    assert [(n, s) for n, s, _, _ in specs] == _deepnmt_expected(cell, NE, ND, ca, deep, redict, shared, soft_shared, E)
    assert len({n for n, _, _, _ in specs}) == len(specs) and not any("/cell_" in n for n, _, _, _ in specs)


def test_variable_names_spelled_out():
    """A few names and shapes written out by hand (the helpers above share their structure with the code under test)."""
    from zero_amd.variables import variable_specs
    specs = variable_specs(_tiny("rnnsearch_deepatt", "olrn", 1, 1), "rnnsearch_deepatt")
    names, shape = [n for n, _, _, _ in specs], {n: s for n, s, _, _ in specs}
    assert names[2:6] == ["encoder/layer_0/fetch_state_olrn/hide_x/W_0_0", "encoder/layer_1/fetch_state_olrn_lower/hide_x/W_0_0",
                          "encoder/layer_1/fetch_state_olrn_higher/hide_x/W_0_0", "decoder_initializer/dec_init_state_init/W_0_0"]
    assert shape[names[2]] == (8, 48) and shape[names[4]] == (12, 48)
    i = names.index("decoder/context_att/W_0_0")
    assert names[i - 1] == "decoder/fetch_state_olrn_lower/hide_x/W_0_0"
    assert names[i + 1] == "decoder/deep_attention_0/feed_query/W_0_0"
    assert names[i + 5] == "decoder/fetch_state_olrn_higher_0/hide_x/W_0_0" and shape[names[i + 5]] == (12, 48)
    specs = variable_specs(_tiny("deepnmt", "lrn", 1, 2, caencoder=False, use_deep_att=False, dl4mt_redict=False), "deepnmt")
    names, shape = [n for n, _, _, _ in specs], {n: s for n, s, _, _ in specs}
    assert names[2:6] == ["encoder/layer_0/forward/fetch_state_lrn/hide_x/W_0_0",
                          "encoder/layer_0/backward/fetch_state_lrn/hide_x/W_0_0", "encoder/layer_0/ff/W_0_0",
                          "encoder/layer_0/ff/b_0"]
    assert shape["decoder/layer_1/fetch_state_lrn/hide_x/W_0_0"] == (8 + 12, 36) and shape["layer_0_init/W_0_0"] == (24, 12)


# ---------------------------------------------------------------------------------------------- the scan reference
CASES = [(gated, paired, reverse) for gated in (False, True) for paired in (False, True) for reverse in (False, True)]


def _inputs(T, R, H, form, gated, paired, seed=0):
    x = L.scan_inputs(T, R, H, form, seed, gated, paired)
    x["mask"][1, 2] = 0.5               # one fractional value: what tells a carry per pair from a carry per cell
    return x


def _call(x, reverse, gated, **kw):
    return L.lrn_scan(x["lo"], x["hi"], x["h_prev"], x["idx"], x["mask"], reverse, gated, **kw)


@pytest.mark.parametrize("form", ["bf16", "fp32"])
@pytest.mark.parametrize("gated,paired,reverse", CASES)
def test_standin_is_inside_the_bound_and_every_defect_outside(form, gated, paired, reverse):
    T, R, H = 6, 7, 8
    x = _inputs(T, R, H, form, gated, paired, seed=3 * gated + paired)
    ref = _call(x, reverse, gated)
    got = L.lrn_standin(x["lo"], x["hi"], x["h_prev"], x["idx"], x["mask"], reverse, gated, form)
    for what in ("out", "seq"):
        worst = V.assert_within(got[what], ref[what], L.lrn_bound(ref, form, what), "stand-in %s %s" % (form, what))
        assert worst <= 1.0
    carried = x["mask"][:, 0] == 0                                # row 0 is masked everywhere: the gathered state, bit for bit
    assert carried.all() and np.array_equal(ref["out"][0], ref["h0"][0]) and np.array_equal(got["out"][0], ref["h0"][0])
    assert (L.lrn_bound(ref, form)[0] == 0).all()
    for d in L.LRN_DEFECTS:
        if d in ("gate_reads_old_state", "ungated_carried") and not gated:
            continue
        if d == "mask_once_per_pair" and not paired:
            continue
        if d in ("reverse_ignored", "seq_at_scan_index") and not reverse:
            continue
        bad = _call(x, reverse, gated, defect=d)
        broke = V.exceeds(bad["out"], ref["out"], L.lrn_bound(ref, form, "out")) or \
            V.exceeds(bad["seq"], ref["seq"], L.lrn_bound(ref, form, "seq"))
        assert broke, d


@pytest.mark.parametrize("gated,paired,reverse", CASES)
def test_a_scan_is_its_chained_single_steps(gated, paired, reverse):
    """lrn_scan over T positions = T calls of lrn_scan with T = 1 that hand the state on, exactly (float64, same order)."""
    T, R, H = 5, 4, 8
    x = _inputs(T, R, H, "fp32", gated, paired, seed=7)
    ref = _call(x, reverse, gated)
    h = ref["h0"]
    for n in range(T):
        t = T - 1 - n if reverse else n
        one = L.lrn_scan(x["lo"][t:t + 1], None if x["hi"] is None else x["hi"][t:t + 1], h, None, x["mask"][t:t + 1], False, gated)
        h = one["out"]
        assert np.array_equal(one["seq"][0], ref["seq"][t]), (n, t)
    assert np.array_equal(h, ref["out"])


def test_null_state_and_no_mask():
    x = L.scan_inputs(4, 3, 8, "bf16", 1, True, True, mask=None)
    ref = L.lrn_scan(x["lo"], x["hi"], None, None, None, True, True)
    assert not ref["h0"].any() and len(ref["steps"]) == 4 and ref["steps"][0]["t"] == 3
    assert all(len(s["cells"]) == 2 and set(s["cells"][0]) >= {"h_", "p", "q", "r", "s", "i", "f", "u", "g", "v", "out"}
               for s in ref["steps"])
    assert np.array_equal(ref["seq"][0], ref["out"])              # reversed: position 0 is scanned last
    got = L.lrn_standin(x["lo"], x["hi"], None, None, None, True, True, "bf16")
    V.assert_within(got["seq"], ref["seq"], L.lrn_bound(ref, "bf16", "seq"), "null state")


# ---------------------------------------------------------------------------------------------- the models restated
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("NE,ND", [(2, 2), (0, 1)])
def test_deepatt_full_decoder_equals_the_cached_steps(cell, NE, ND):
    hp = _tiny("rnnsearch_deepatt", cell, NE, ND)
    M = DA
    P = rt.to_torch(M.init_params(hp, 2), dtype=torch.float64)
    src = torch.as_tensor(V.ragged((6, 3, 5), hp.src_vocab.size(), 2))
    tgt = torch.as_tensor(np.random.default_rng(3).integers(3, hp.tgt_vocab.size(), (3, 5)))
    enc, dec = M.decoding_fns(hp, P)
    state = enc(src)
    full = M.full_decoder(tgt, state, hp, P)
    prev = torch.full((3, 1), hp.tgt_vocab.pad(), dtype=torch.long)
    for t in range(5):
        logits, state = dec(prev, state, t)
        assert torch.allclose(logits, full[:, t], rtol=0, atol=1e-12), t
        prev = tgt[:, t:t + 1]
    assert torch.equal(enc(torch.nn.functional.pad(src, (0, 3)))["encodes"], enc(src)["encodes"])


@pytest.mark.parametrize("cell,ca,deep,redict", [("olrn", True, False, True), ("lrn", False, False, False), ("lrn", True, True, False)])
def test_deepnmt_full_decoder_equals_the_cached_steps(cell, ca, deep, redict):
    hp = _tiny("deepnmt", cell, 2, 3, caencoder=ca, use_deep_att=deep, dl4mt_redict=redict)
    M = DN
    P = rt.to_torch(M.init_params(hp, 2), dtype=torch.float64)
    src = torch.as_tensor(V.ragged((6, 3, 5), hp.src_vocab.size(), 2))
    tgt = torch.as_tensor(np.random.default_rng(3).integers(3, hp.tgt_vocab.size(), (3, 5)))
    enc, dec = M.decoding_fns(hp, P)
    state = enc(src)
    full = M.full_decoder(tgt, state, hp, P)
    prev = torch.full((3, 1), hp.tgt_vocab.pad(), dtype=torch.long)
    for t in range(5):
        logits, state = dec(prev, state, t)
        assert torch.allclose(logits, full[:, t], rtol=0, atol=1e-12), t
        prev = tgt[:, t:t + 1]


def test_restated_encoder_is_the_scan_reference():
    """The torch restatement of a one-to-one encoder layer and lrn_scan (the kernel's statement) are the same function."""
    hp = _tiny("rnnsearch_deepatt", "olrn", 1, 1)
    P = rt.to_torch(DA.init_params(hp, 4), dtype=torch.float64)
    src = torch.as_tensor(V.ragged((5, 3), hp.src_vocab.size(), 1))
    st = DA.encoder(src, hp, P)
    x = P["src_embedding"][src] + P["bias"]
    mask = (src != 0).double().numpy().T
    tm = lambda a: a.numpy().transpose(1, 0, 2)
    h0 = L.lrn_scan(tm(x @ P["encoder/layer_0/fetch_state_olrn/hide_x/W_0_0"]), None, None, None, mask, False, True)
    lo = tm(x @ P["encoder/layer_1/fetch_state_olrn_lower/hide_x/W_0_0"])
    hi = torch.as_tensor(h0["seq"]) @ P["encoder/layer_1/fetch_state_olrn_higher/hide_x/W_0_0"]
    h1 = L.lrn_scan(lo, hi.numpy(), None, None, mask, True, True)
    assert np.allclose(st["encodes"].numpy().transpose(1, 0, 2), h1["seq"], rtol=0, atol=1e-12)


FIXTURES = ["deepatt_lrn", "deepatt_olrn", "deepnmt_olrn_ca", "deepnmt_lrn_plain"]


def fixture_of(name):
    """-> (hparams, the model's reference module)."""
    if name.startswith("deepatt_"):
        return L.deepatt_hp(name[len("deepatt_"):]), DA
    return L.deepnmt_hp(name[len("deepnmt_"):]), DN


@pytest.mark.parametrize("name", FIXTURES)
def test_model_fixture_margins(name):
    """The measurements the GPU model tests rest on (recorded in tests/lrn_ref.py), re-made on every CPU run."""
    hp, M = fixture_of(name)
    f = M.make_fixture(hp, V.ragged(L.LENGTHS, hp.src_vocab.size(), 5), L.SEEDS[name])
    print("%s: gap %.3e err %.3e rel %.3f" % (name, f["gap"], f["err"], f["rel"]))
    assert f["gap"] > 4 * f["err"]
    assert f["rel"] <= 0.25 and L.score_tol(f["rel"], f["err"]) == (L.RTOL, L.ATOL)
