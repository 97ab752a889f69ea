"""rnnsearch on the host: registry and refusals, variable specs, and the references of tests/rnnsearch_ref.py checked on
their own (the cached step against the teacher-forced decoder, every planted defect against the bound, the stand-ins
inside it, the model fixture's measured margins)."""
import copy

import numpy as np
import pytest
import torch

from oracle import ref_torch as rt
from tests import rnnsearch_ref as R
from tests import variant_ref as V
from tests.common import make_hp


def _tiny(**kw):
    hp = make_hp("rnnsearch", H=12, Vs=11, Vt=9, cell="atr", layer_norm=False, search_mode="cache", **kw)
    hp.embed_size = 8
    return hp


# ---------------------------------------------------------------------------------------------- registry and refusals
def test_registered_and_refusals_touch_no_device(monkeypatch):
    from zero_amd.models import model as registry, load_all, _factory
    load_all()
    monkeypatch.setattr(_factory, "get_core", lambda *a, **k: pytest.fail("a refusal built a core"))
    triple = registry.get_model("rnnsearch")
    assert callable(triple.train_fn) and callable(triple.score_fn) and callable(triple.infer_fn)
    hp = _tiny()
    feats = {"source": np.ones((1, 2)), "target": np.ones((1, 2))}
    with pytest.raises(NotImplementedError, match="rnnsearch.*backward of the ATR scans"):
        triple.train_fn(feats, hp)
    with pytest.raises(NotImplementedError, match="rnnsearch.*teacher-forced decoder scan"):
        triple.score_fn(feats, hp)
    for key, value, what in (("cell", "gru", "rnnsearch.*cell=atr only.*gru"), ("cell", "lstm", "rnnsearch.*lstm"),
                             ("layer_norm", True, "rnnsearch.*layer_norm=True"),
                             ("search_mode", "dev", "rnnsearch.*search_mode=cache only")):
        bad = copy.copy(hp)
        setattr(bad, key, value)
        with pytest.raises(NotImplementedError, match=what):
            triple.infer_fn(bad)
    enc, dec = triple.infer_fn(hp)                    # the supported settings build the closures without a core
    assert callable(enc) and callable(dec) and callable(dec.step_static)
    from zero_amd.models import _ensemble
    with pytest.raises(NotImplementedError, match="member 1 is a rnnsearch"):
        _ensemble.check_members([make_hp("transformer"), _tiny()])


def test_reference_defaults_name_the_model():
    from zero_amd.config import default_params
    from zero_amd.models import model as registry, load_all
    load_all()
    hp = default_params()                             # the reference's defaults (run.py:24-239)
    assert (hp.model_name, hp.cell, hp.caencoder, hp.layer_norm, hp.search_mode) == ("rnnsearch", "atr", True, False, "cache")
    triple = registry.get_model(hp.model_name)
    assert callable(triple.infer_fn(hp)[0])           # none of the refusals fires on them
    from zero_amd.config import SyntheticVocab
    from zero_amd.variables import variable_specs
    hp.src_vocab, hp.tgt_vocab = SyntheticVocab(30), SyntheticVocab(30)
    shapes = {n: s for n, s, _, _ in variable_specs(hp, hp.model_name)}
    assert shapes["pre_logits/W_0_0"] == (1000 + 1000 + 620, 620)


# ---------------------------------------------------------------------------------------------- variables
def _expected(ca, shared, soft_shared):
    H, E, Vs, Vt = 12, 8, 11, 11 if shared else 9
    M = H if ca else 2 * H
    v = [("embedding" if shared else "src_embedding", (Vs, E)), ("bias", (E,)),
         ("encoder/forward/fetch_state_atr/hide_x/W_0_0", (E, H)),
         ("encoder/forward/cell_atr/hide_h/W_0_0", (H, H)), ("encoder/forward/cell_atr/hide_h/b_0", (H,))]
    if ca:
        v += [("encoder/backward/fetch_state_atr_lower/hide_x/W_0_0", (E, H)),
              ("encoder/backward/fetch_state_atr_higher/hide_x/W_0_0", (H, H)),
              ("encoder/backward/cell_atr_lower/hide_h/W_0_0", (H, H)), ("encoder/backward/cell_atr_lower/hide_h/b_0", (H,)),
              ("encoder/backward/cell_atr_higher/hide_h/W_0_0", (H, H)), ("encoder/backward/cell_atr_higher/hide_h/b_0", (H,))]
    else:
        v += [("encoder/backward/fetch_state_atr/hide_x/W_0_0", (E, H)),
              ("encoder/backward/cell_atr/hide_h/W_0_0", (H, H)), ("encoder/backward/cell_atr/hide_h/b_0", (H,))]
    v += [("decoder_initializer/atr_init/W_0_0", (M, H)), ("decoder_initializer/atr_init/b_0", (H,))]
    if not shared:
        v.append(("tgt_embedding", (Vt, E)))
    v += [("decoder/fetch_state_atr_lower/hide_x/W_0_0", (E, H)), ("decoder/context_att/W_0_0", (M, M)),
          ("decoder/cell_atr_lower/hide_h/W_0_0", (H, H)), ("decoder/cell_atr_lower/hide_h/b_0", (H,)),
          ("decoder/attention/feed_query/W_0_0", (H, M)), ("decoder/attention/feed_query/b_0", (M,)),
          ("decoder/attention/feed_logits/W_0_0", (M, 1)), ("decoder/attention/feed_logits/b_0", (1,)),
          ("decoder/fetch_state_atr_higher/hide_x/W_0_0", (M, H)),
          ("decoder/cell_atr_higher/hide_h/W_0_0", (H, H)), ("decoder/cell_atr_higher/hide_h/b_0", (H,)),
          ("pre_logits/W_0_0", (H + M + E, E)), ("pre_logits/b_0", (E,))]
    if not shared and not soft_shared:
        v.append(("softmax_embedding", (Vt, E)))
    return v


@pytest.mark.parametrize("ca", [True, False])
@pytest.mark.parametrize("shared,soft_shared", [(False, True), (False, False), (True, True)])
def test_variable_specs(ca, shared, soft_shared):
    from zero_amd.variables import variable_specs, initial_values
    hp = _tiny(caencoder=ca, shared_source_target_embedding=shared, shared_target_softmax_embedding=soft_shared)
    if shared:
        hp.tgt_vocab = hp.src_vocab
    specs = variable_specs(hp, "rnnsearch")           # hidden_size != embed_size: taken before the Transformer's H == E test
    assert [(n, s) for n, s, _, _ in specs] == _expected(ca, shared, soft_shared)
    with pytest.raises(ValueError, match="hidden_size must equal embed_size"):
        variable_specs(hp, "transformer")
    kinds = {n: k for n, _, k, _ in specs}
    vals = initial_values(hp, "rnnsearch", 5)
    for n, k in kinds.items():
        if n.endswith("/b_0"):
            assert k == "zeros" and not vals[n].any(), n
        elif "embedding" in n:
            # the scope initialiser (uniform_unit_scaling: bounded by its limit), not N(0, H^-0.5)
            assert k == "embed_w", n
            lim = (3.0 / ((vals[n].shape[0] + vals[n].shape[1]) / 2.0)) ** 0.5
            assert 0 < np.abs(vals[n]).max() <= lim, n
        else:
            assert k == "w" and vals[n].std() > 0, n


# ---------------------------------------------------------------------------------------------- the references
def _atr_inputs(R_, H, seed, n_prev=None):
    g = np.random.default_rng(seed)
    n_prev = R_ if n_prev is None else n_prev
    bf = lambda x: torch.as_tensor(x).float().to(torch.bfloat16).double().numpy()
    return dict(h_prev=g.normal(0, 1, (n_prev, H)).astype(np.float32).astype(np.float64), U=bf(g.normal(0, H ** -0.5, (H, H))),
                b=g.normal(0, 0.3, H).astype(np.float32).astype(np.float64), p=bf(g.normal(0, 1, (R_, H))),
                mask=(g.random(R_) < 0.6).astype(np.float64), idx=g.integers(0, n_prev, R_))


@pytest.mark.parametrize("form", ["bf16", "fp32"])
def test_atr_reference_standin_and_defects(form):
    x = _atr_inputs(9, 24, 0)
    x["mask"][:2] = (0.0, 1.0)
    x["idx"][:3] = (4, 4, 0)                          # repeats, and rows that differ from their own index
    ref = R.atr_step(**x)
    for copy_ in (False, True):
        bound = R.atr_bound(ref, form, copy=copy_)
        worst = V.assert_within(R.atr_standin(form=form, copy=copy_, **x), ref["out"], bound, "stand-in %s" % form)
        assert worst <= 1.0
    carried = x["mask"] == 0
    assert (R.atr_bound(ref, form)[carried] == 0).all() and np.array_equal(ref["out"][carried], ref["h"][carried])
    for d in R.ATR_DEFECTS:
        bad = R.atr_step(defect=d, **x)["out"]
        assert V.exceeds(bad, ref["out"], R.atr_bound(ref, form)), d          # (the fp32 state: what the next step reads)
    # the zero state: q = b
    z = dict(x, h_prev=None, idx=None)
    ref0 = R.atr_step(**z)
    assert np.allclose(ref0["q"], x["b"][None, :]) and not ref0["h"].any()
    V.assert_within(R.atr_standin(form=form, **z), ref0["out"], R.atr_bound(ref0, form), "stand-in, zero state")


def test_atr_bound_catches_a_bf16_state_with_u_zero():
    """U = 0: q = b exactly, so the only place the state enters is f h and the carry -- in fp32.  A state that is not
    bf16-representable then shows a kernel that keeps (or reads) it in bf16, in BOTH forms."""
    x = _atr_inputs(5, 16, 1)
    x["U"] = np.zeros_like(x["U"])
    x["h_prev"] = x["h_prev"] * (1 + 2.0 ** -12)
    assert not np.array_equal(R._bf(x["h_prev"]), x["h_prev"])
    ref = R.atr_step(**x)
    for form in ("bf16", "fp32"):
        bound = R.atr_bound(ref, form)
        V.assert_within(R.atr_standin(form=form, **x), ref["out"], bound, "stand-in, U = 0")
        assert V.exceeds(R.atr_step(defect="bf16_state", **x)["out"], ref["out"], bound)


def _add_inputs(seed, R_=6, G=3, M=24, L=9, lengths=(9, 4), hot=True):
    g = torch.Generator().manual_seed(seed)
    bf = lambda t: t.to(torch.bfloat16).double().numpy()
    nB = R_ // G
    qa, pm, mem = torch.randn(R_, M, generator=g), torch.randn(nB, L, M, generator=g), torch.randn(nB, L, M, generator=g)
    v = torch.randn(M, generator=g) * 0.5
    mask = torch.zeros(nB, L)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
    if hot:      # the masked keys of the last sentence are the hottest: pm = 3 sign(v) - qa puts every tanh at +-1 with v's sign
        b = nB - 1
        pm[b, lengths[b]:] = 3.0 * torch.sign(v)[None, :] - qa[b * G:(b + 1) * G].mean(0)[None, :]
    return dict(qa=bf(qa), pm=bf(pm), mem=bf(mem), v=v.double().numpy(), mask=mask.double().numpy(), kv_group=G)


@pytest.mark.parametrize("form", ["bf16", "fp32"])
def test_add_attention_reference_standin_and_defects(form):
    x = _add_inputs(3)
    ref = R.add_attention(**x)
    assert (ref["a"][3:, 4:] == 0).all()              # masked keys: exactly zero weights
    for copy_ in (False, True):
        bound = R.add_bound(ref, form, copy=copy_)
        got = R.add_standin(x["qa"], x["pm"], x["mem"], x["v"], x["mask"], x["kv_group"], 9, form, copy=copy_)
        assert V.assert_within(got, ref["out"], bound, "stand-in %s" % form) <= 1.0
    bound = R.add_bound(ref, form, copy=True)
    for d in R.ADD_DEFECTS:
        y = dict(x)
        if d == "extra_key":                          # keys 0 .. 7 exist, the ninth is there to be read by mistake
            y["mask"] = np.ones_like(x["mask"])
            good = R.add_attention(Ls=8, **y)
            assert V.exceeds(R.add_attention(Ls=8, defect=d, **y)["out"], good["out"], R.add_bound(good, form, copy=True)), d
            continue
        assert V.exceeds(R.add_attention(defect=d, **x)["out"], ref["out"], bound), d
    # tanh saturates: huge arguments of both signs stay finite
    big = dict(x, qa=x["qa"] * 1e30)
    assert np.isfinite(R.add_attention(**big)["out"]).all()
    assert np.isfinite(R.add_standin(big["qa"], x["pm"], x["mem"], x["v"], x["mask"], 3, 9, form)).all()


@pytest.mark.parametrize("ca", [True, False])
def test_full_decoder_equals_the_cached_steps(ca):
    """float64: the teacher-forced scan over a target and the cached step fed the same tokens one at a time give the same
    logits; the source's padding columns change nothing (the carry)."""
    hp = _tiny(caencoder=ca)
    P = rt.to_torch(R.init_params(hp, 2), dtype=torch.float64)
    src = torch.as_tensor(V.ragged((6, 3, 5), hp.src_vocab.size(), 2))
    tgt = torch.as_tensor(np.random.default_rng(3).integers(3, hp.tgt_vocab.size(), (3, 5)))
    enc, dec = R.decoding_fns(hp, P)
    state = enc(src)
    full = R.full_decoder(tgt, state, hp, P)
    assert full.shape == (3, 5, hp.tgt_vocab.size())
    prev = torch.full((3, 1), hp.tgt_vocab.pad(), dtype=torch.long)
    for t in range(5):
        logits, state = dec(prev, state, t)
        assert torch.allclose(logits, full[:, t], rtol=0, atol=1e-12), t
        prev = tgt[:, t:t + 1]
    padded = torch.nn.functional.pad(src, (0, 3))
    state2 = enc(padded)                              # remove_invalid_seq drops the all-pad columns
    assert torch.equal(state2["encodes"], enc(src)["encodes"])


@pytest.mark.parametrize("ca", [True, False])
def test_model_fixture_margins(ca):
    """The measurements the GPU model tests rest on (recorded in tests/rnnsearch_ref.py), re-made on every CPU run."""
    hp = R.fixture_hp(ca)
    f = R.make_fixture(hp, V.ragged(R.LENGTHS, hp.src_vocab.size(), 5), R.SEEDS[ca])
    print("caencoder=%s: gap %.3e err %.3e rel %.3f" % (ca, f["gap"], f["err"], f["rel"]))
    assert f["gap"] > 4 * f["err"]
    assert f["rel"] <= 0.25 and R.score_tol(f["rel"], f["err"]) == (R.RTOL, R.ATOL)
