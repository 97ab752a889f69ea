"""References of deepnmt at inference (a plain module, no pytest in it), in the manner of tests/deepatt_ref.py on
tests/variant_ref.py.

Reference arithmetic (models/deepnmt.py, rnns/rnn.py, rnns/{atr,gru}.py, func.py:14-65, 107-161, 289-303): every layer is a
recurrent scan followed by x = x + (outputs W_ff + b_ff) on a residual stream that nothing re-normalises.  The cells and the
attention are those of tests/rnnsearch_ref.py / tests/deepatt_ref.py, unchanged; what is this model's own:

``ff_residual``            out = x + (a W + b) in float64 numpy with everything the bound needs; ``defect=`` plants ONE defect.
``ff_residual_bound``      the element-wise bound zk_rnn_ff_residual / zk_f32_rnn_ff_residual are held to (derivation there).
``ff_residual_standin``    what a correct kernel computes, in torch float32 with another summation order.
``encoder`` / ``decoder_step`` / ``decoding_fns`` / ``full_decoder``   the model restated for oracle.ref_torch.beam_search.
``init_params`` / ``make_fixture`` / ``fixture_hp``   the tiny models of the GPU model tests and what the REFERENCE ALONE shows.

make_fixture on the fixtures of tests/test_gpu_deepnmt_model.py (vocabularies 120 / 104, sources of 14, 5, 9 and 11 tokens,
beams 1 and 4), measured on the CPU (tests/test_deepnmt_host.py re-measures and asserts; the figures move by an ulp of a score
with the CPU's matrix-product order, the tests assert gap > 4 err and the score_tol rule, not the figures):

    (A) atr, caencoder, dl4mt_redict, NE 2, ND 3, H 128, E 64,  seed %(A)s
    (B) atr, neither switch,          NE 1, ND 2, H 64,  E 64,  seed %(B)s
    (C) gru, caencoder, use_deep_att, dl4mt_redict, NE 2, ND 2, H 128, E 128,  seed %(C)s

%(FIGURES)s

gap, err, rel as in tests/rnnsearch_ref.py.  The bf16-storage restatement keeps the fp32 best hypotheses of the x 6 sharpened
model on all three.
"""
import copy

import numpy as np
import torch

from oracle import ref_torch as rt
from tests import deepatt_ref as DA
from tests import rnnsearch_ref as RS
from tests import variant_ref as V

FF_DEFECTS = ("bf16_stream", "no_bias", "no_residual", "w_transposed", "k_tail_dropped", "col_neighbour", "copy_of_product")
# config -> the seed of its model fixture (the widest gap / err among the seeds 1 .. 39, picked as deepatt_ref.SEEDS were)
SEEDS = {"A": 36, "B": 11, "C": 23}
FIGURES = """    (A)  gap 1.74e-04   err 3.8e-06 (gap = 46 x err)   rel 0.029
    (B)  gap 1.79e-04   err 3.8e-06 (gap = 47 x err)   rel 0.021
    (C)  gap 2.34e-04   err 7.6e-06 (gap = 31 x err)   rel 0.025"""
__doc__ = __doc__ % dict(SEEDS, FIGURES=FIGURES)
RTOL, ATOL = RS.RTOL, RS.ATOL
score_tol = RS.score_tol
_bf = RS._bf


# ---------------------------------------------------------------------------------------------- numpy, float64
def ff_residual(a, W, b, x, defect=None):
    """a [R, K]; W [K, N]; b [N]; x [R, N].  -> dict of float64 arrays: out = x + (a W + b), copy_src (what the copy in the
    storage type is a rounding of: out) and, for ff_residual_bound: y = a W + b, mag = |a| |W| + |b|, x, K.

    defect (one at a time; each is something a kernel could do):
      bf16_stream      x rounded to bf16 before the add (a stream kept in the storage type)
      no_bias          b dropped
      no_residual      out = a W + b
      w_transposed     a W^T (needs K == N)
      k_tail_dropped   the last K % 32 terms of the product dropped (needs K % 32 != 0)
      col_neighbour    column j of the product taken from column j + 1 of W (the last from column 0)
      copy_of_product  the copy taken before the add: copy = a W + b while out is right"""
    a, W, b, x = (np.asarray(t, np.float64) for t in (a, W, b, x))
    K = a.shape[1]
    Wm = W
    if defect == "w_transposed":
        assert W.shape[0] == W.shape[1]
        Wm = W.T
    if defect == "col_neighbour":
        Wm = np.roll(W, -1, axis=1)
    am = a
    if defect == "k_tail_dropped":
        assert K % 32 != 0
        am = a.copy()
        am[:, K - K % 32:] = 0.0
    bias = np.zeros_like(b) if defect == "no_bias" else b
    y = am @ Wm + bias
    xm = _bf(x) if defect == "bf16_stream" else x
    out = y if defect == "no_residual" else xm + y
    return {"out": out, "copy_src": y if defect == "copy_of_product" else out, "y": y, "x": x, "K": K,
            "mag": np.abs(a) @ np.abs(W) + np.abs(b)}


def ff_residual_bound(ref, form, copy=False):
    """Element-wise bound of zk_rnn_ff_residual (form "bf16") / zk_f32_rnn_ff_residual ("fp32") against ff_residual(...) = ref,
    for inputs that are exactly representable where the kernel reads them (a and W in the storage type, b and x in fp32).
    Derived term by term as rnnsearch_ref.atr_bound is, PER_TERM = 2^-23 (twice the unit roundoff) per accumulated term:

      y     fp32 accumulation of K products and the bias:  |dy| <= (K + 8) 2^-23 mag,  mag = |a| |W| + |b|  (the bf16 form's
            MFMA operands are bf16 ALREADY: their products are exact in fp32, no 2^-8 term);
      out   = x + y, one fp32 add:  |dout| <= |dy| + 2^-23 (|x| + |y|);
      + u |out|, u = 2^-8, for the copy in the bf16 storage type only; the fp32 stream has no further rounding.
    x enters the add in fp32 in BOTH forms: no u |x| term -- that is what catches a bf16 stream."""
    from tests import parity as PR
    bound = (ref["K"] + 8) * PR.PER_TERM * ref["mag"] + PR.PER_TERM * (np.abs(ref["x"]) + np.abs(ref["y"]))
    if copy and form == "bf16":
        bound = bound + 2.0 ** -8 * np.abs(ref["out"])
    return bound


def ff_residual_standin(a, W, b, x, form, copy=False):
    """What a correct kernel computes, on the CPU in torch float32: the product summed over k in DESCENDING order (the
    reference sums ascending in float64), the add in fp32; the copy rounded once in the bf16 form."""
    f = lambda t: torch.as_tensor(np.asarray(t, np.float64)).float()
    a, W, b, x = f(a), f(W), f(b), f(x)
    rev = torch.arange(a.shape[1] - 1, -1, -1)
    out = x + (a[:, rev] @ W[rev] + b)
    if copy and form == "bf16":
        out = out.to(torch.bfloat16).float()
    return out.double().numpy()


def ff_inputs(R, K, N, form, seed, zero_w=False):
    """float64 arrays exactly representable where the kernels read them.  zero_w: W = 0, b = 0 and an x that is NOT
    bf16-representable -- out must be x bit for bit."""
    g = np.random.default_rng(300 + seed)
    st = lambda t: torch.as_tensor(np.asarray(t, np.float64)).float().to(V.STORAGE[form]).double().numpy()
    f32 = lambda t: np.asarray(t, np.float32).astype(np.float64)
    x = dict(a=st(g.normal(0, 1, (R, K))), W=st(g.normal(0, K ** -0.5, (K, N))), b=f32(g.normal(0, 0.3, N)),
             x=f32(g.normal(0, 1, (R, N))))
    if zero_w:
        x["W"], x["b"] = np.zeros((K, N)), np.zeros(N)
        x["x"] = f32(x["x"] * (1 + 2.0 ** -12))
        assert not np.array_equal(_bf(x["x"]), x["x"])
    return x


# ---------------------------------------------------------------------------------------------- ref_torch model
_w, _carry, _names = RS._w, RS._carry, RS._names
cell_fetch, cell_call = DA.cell_fetch, DA.cell_call


def _ff(x, a, P, pre):
    """x + linear(a, embed_size, scope=pre + "ff") on the fp32 stream: a is the stored state, the sum is not stored."""
    return x + (torch.matmul(rt._st(a, "rnn_state"), _w(P, pre + "ff/W_0_0")) + P[pre + "ff/b_0"])


def form_of(hp, l):
    if l == 0 or hp.use_deep_att:
        return "att"
    return "one2one" if hp.caencoder else "plain"


def encoder(source, hp, P, return_z=False):
    """models/deepnmt.py:16-100 (positions un-reversed).  The stream x is fp32; every product reads its stored copy."""
    dt = P["bias"].dtype
    H, E, c, NE, ND, ca = hp.hidden_size, hp.embed_size, str(hp.cell).lower(), hp.num_encoder_layer, hp.num_decoder_layer, \
        bool(hp.caencoder)
    mask = (source != 0).to(dt)
    source, mask = rt.remove_invalid_seq(source, mask)
    B, L = source.shape
    x = _w(P, _names(hp)[0])[source] + P["bias"]
    m = lambda t: mask[:, t:t + 1]
    at = lambda inp, t: tuple(v[:, t] for v in inp)

    def scan(pre, s, xin, order):
        inp = cell_fetch(xin, P, pre, s, c)
        h = torch.zeros(B, H, dtype=dt)
        seq = [None] * L
        for t in order:
            h = _carry(m(t), cell_call(h, at(inp, t), P, pre, s, c), h)
            seq[t] = h
        return torch.stack(seq, 1), h
    for l in range(NE):
        pre = "encoder/layer_%d/" % l
        xc = rt._st(x, "embed")
        fw, sf = scan(pre + "forward/", c, xc, range(L))
        if l == 0 and ca:
            b = pre + "backward/"
            lo = cell_fetch(xc, P, b, c + "_lower", c)
            hi = cell_fetch(rt._st(fw, "rnn_state"), P, b, c + "_higher", c)
            g = torch.zeros(B, H, dtype=dt)
            gs = [None] * L
            for t in range(L - 1, -1, -1):
                s = _carry(m(t), cell_call(g, at(lo, t), P, b, c + "_lower", c), g)
                g = _carry(m(t), cell_call(s, at(hi, t), P, b, c + "_higher", c), s)
                gs[t] = g
            y, z = torch.stack(gs, 1), g
        elif l == 0:
            bw, sb = scan(pre + "backward/", c, xc, range(L - 1, -1, -1))
            y, z = torch.cat([fw, bw], -1), torch.cat([sf, sb], -1)
        else:
            y, z = fw, sf
        x = _ff(x, y, P, pre)
    xc = rt._st(x, "embed")
    if E != H:        # layer_norm(linear(x, hidden_size, scope="x_map")): the product stays fp32, the normalised rows are stored
        xm = torch.matmul(xc, _w(P, "x_map/W_0_0")) + P["x_map/b_0"]
        mean = xm.mean(-1, keepdim=True)
        var = ((xm - mean) ** 2).mean(-1, keepdim=True)
        enc = rt._st(P["layer_norm/scale"] * (xm - mean) * torch.rsqrt(var + rt.Cfg.eps) + P["layer_norm/offset"], "ln")
    else:
        enc = xc
    zs = rt._st(z, "rnn_state")
    init = {"layer_%d" % l: torch.matmul(zs, _w(P, "layer_%d_init/W_0_0" % l)) +
            P["layer_%d_init/b_0" % l] for l in range(ND)}                       # (no tanh)
    pm = {l: rt.linear(enc, P, "decoder/layer_%d/context_att" % l, bias=False) for l in range(ND) if form_of(hp, l) == "att"}
    out = {"encodes": enc, "pm": pm, "decoder_initializer": init, "mask": mask}
    if return_z:
        out["z"] = z
    return out


def decoder_step(y, hs, state, hp, P):
    """One position of the decoder stack (models/deepnmt.py:133-194): y [N, E] the fp32 input embedding, hs {layer_l: [N, H]}
    -> (logits [N, V], hs')."""
    c = str(hp.cell).lower()
    enc, mask = state["encodes"], state["mask"]
    x, ctx, new = y, None, {}
    for l in range(hp.num_decoder_layer):
        pre = "decoder/layer_%d/" % l
        h = hs["layer_%d" % l]
        xc = rt._st(x, "embed")
        form = form_of(hp, l)
        if form == "plain":
            hn = cell_call(h, cell_fetch(torch.cat([xc, ctx], -1), P, pre, c, c), P, pre, c, c)
        else:
            s = cell_call(h, cell_fetch(xc, P, pre, c + "_lower", c), P, pre, c + "_lower", c)
            if form == "att":
                a = pre + "attention/"
                qa = rt.linear(rt._st(s, "rnn_state"), P, a + "feed_query")
                v = P[a + "feed_logits/W_0_0"][:, 0]
                logit = torch.matmul(torch.tanh(qa[:, None, :] + state["pm"][l]), v) + P[a + "feed_logits/b_0"]
                logit = logit + (1.0 - mask) * (-rt.Cfg.inf)
                w = torch.softmax(logit, -1)
                ctx = rt._st((w[:, :, None] * enc).sum(1), "attn_out")
            hn = cell_call(s, cell_fetch(ctx, P, pre, c + "_higher", c), P, pre, c + "_higher", c)
        new["layer_%d" % l] = hn
        x = _ff(x, hn, P, pre)
    xc = rt._st(x, "embed")
    if hp.dl4mt_redict:
        feat = rt._st(torch.tanh(torch.matmul(torch.cat([xc, ctx], -1), _w(P, "ff/W_0_0")) + P["ff/b_0"]))
    else:
        feat = xc
    return torch.matmul(feat, _w(P, _names(hp)[2]).t()), new


def decoding_fns(hp, P):
    """(encoding_fn, decoding_fn) of models/deepnmt.py:252-283 (search_mode = cache) for rt.beam_search."""
    hp = rt.closing_dropout(copy.copy(hp))

    def encoding_fn(source):
        return V.cached_state(encoder(source, hp, P))

    def decoding_fn(target, state, time):
        tok = target[:, -1]
        y = _w(P, _names(hp)[1])[tok] + P["bias"]
        if bool((target == hp.tgt_vocab.pad()).all()):          # deepnmt.py:126-128
            y = torch.zeros_like(y)
        logits, hn = decoder_step(y, state["decoder"]["state"], state, hp, P)
        state["decoder"]["state"] = hn
        return logits, state

    return encoding_fn, decoding_fn


def full_decoder(target, state, hp, P):
    """The training-path decoder (models/deepnmt.py:103-194 with is_training): inputs shifted right by one zero row, every
    layer ONE scan over the whole target before the next layer starts.  target [B, Lt] without padding -> logits [B, Lt, V]."""
    c = str(hp.cell).lower()
    enc, mask = state["encodes"], state["mask"]
    y = _w(P, _names(hp)[1])[target] + P["bias"]
    x = torch.nn.functional.pad(y, (0, 0, 1, 0))[:, :-1, :]
    Lt = target.shape[1]
    ctx = None
    for l in range(hp.num_decoder_layer):
        pre = "decoder/layer_%d/" % l
        h = state["decoder_initializer"]["layer_%d" % l]
        xc = rt._st(x, "embed")
        form = form_of(hp, l)
        outs, cs = [], []
        lo = cell_fetch(torch.cat([xc, ctx], -1) if form == "plain" else xc, P, pre, c if form == "plain" else c + "_lower", c)
        hi = cell_fetch(ctx, P, pre, c + "_higher", c) if form == "one2one" else None
        for t in range(Lt):
            inp = tuple(v[:, t] for v in lo)
            if form == "plain":
                h = cell_call(h, inp, P, pre, c, c)
            else:
                s = cell_call(h, inp, P, pre, c + "_lower", c)
                if form == "att":
                    a = pre + "attention/"
                    qa = rt.linear(rt._st(s, "rnn_state"), P, a + "feed_query")
                    v = P[a + "feed_logits/W_0_0"][:, 0]
                    logit = torch.matmul(torch.tanh(qa[:, None, :] + state["pm"][l]), v) + P[a + "feed_logits/b_0"]
                    w = torch.softmax(logit + (1.0 - mask) * (-rt.Cfg.inf), -1)
                    ct = rt._st((w[:, :, None] * enc).sum(1), "attn_out")
                    cs.append(ct)
                    hin = cell_fetch(ct, P, pre, c + "_higher", c)
                else:
                    hin = tuple(v[:, t] for v in hi)
                h = cell_call(s, hin, P, pre, c + "_higher", c)
            outs.append(h)
        if form == "att":
            ctx = torch.stack(cs, 1)
        x = _ff(x, torch.stack(outs, 1), P, pre)
    xc = rt._st(x, "embed")
    if hp.dl4mt_redict:
        feat = rt._st(torch.tanh(torch.matmul(torch.cat([xc, ctx], -1), _w(P, "ff/W_0_0")) + P["ff/b_0"]))
    else:
        feat = xc
    return torch.matmul(feat, _w(P, _names(hp)[2]).t())


def init_params(hp, seed):
    return V.init_params(hp, "deepnmt", seed)


def make_fixture(hp, src, seed, factor=4.0):
    """variant_ref.make_fixture on this model -> dict Pn, gap, err, rel (the worst over beam 1 and 4)."""
    return V.make_fixture("deepnmt", decoding_fns, (ATOL, RTOL), hp, src, seed, factor)


LENGTHS = (14, 5, 9, 11)
CONFIGS = {
    "A": dict(cell="atr", caencoder=True, use_deep_att=False, dl4mt_redict=True, num_encoder_layer=2, num_decoder_layer=3, H=128,
              E=64),
    "B": dict(cell="atr", caencoder=False, use_deep_att=False, dl4mt_redict=False, num_encoder_layer=1, num_decoder_layer=2, H=64,
              E=64),
    "C": dict(cell="gru", caencoder=True, use_deep_att=True, dl4mt_redict=True, num_encoder_layer=2, num_decoder_layer=2, H=128,
              E=128),
}


def fixture_hp(config="A", **kw):
    """The hparams of configuration (A), (B) or (C); kw overrides."""
    from tests.common import make_hp
    cfg = dict(CONFIGS[config], **kw)
    H, E = cfg.pop("H"), cfg.pop("E")
    cfg.setdefault("scope_name", "t_deepnmt_%s" % config)
    hp = make_hp("deepnmt", H=H, heads=1, search_mode="cache", layer_norm=False, **cfg)
    hp.embed_size = E
    return hp
