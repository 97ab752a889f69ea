"""References of rnnsearch_deepatt at inference (a plain module, no pytest in it), in the manner of tests/rnnsearch_ref.py and
on tests/variant_ref.py.

Reference arithmetic (models/rnnsearch_deepatt.py, rnns/rnn.py, rnns/gru.py, rnns/atr.py, func.py:107-161), carry(m, a, b) =
m a + (1 - m) b:

    GRU cell    [z | r] = sigmoid(xg + h Ug + bg);  c = tanh(xh + (r h) Uh + bh);  o = z h + (1 - z) c;  out = carry(m, o, h)
    ATR cell, attention    tests/rnnsearch_ref.py (atr_step, add_attention and their bounds serve this model unchanged)

``gru_step``                       the float64 numpy statement with everything the bound needs; ``defect=`` plants ONE defect.
``gru_bound``                      the element-wise bounds zk_rnn_gru_gates + zk_rnn_gru_out are held to (derivation in its docstring).
``gru_standin``                    what correct kernels compute, in torch float32 with another summation order.
``encoder`` / ``decoder_step`` / ``decoding_fns`` / ``full_decoder``   the model restated for oracle.ref_torch.beam_search.
``init_params`` / ``make_fixture`` / ``fixture_hp``   the tiny model of the GPU model tests and what the REFERENCE ALONE shows.

make_fixture on the fixture of tests/test_gpu_deepatt_model.py (H = 128, E = 64, vocabularies 120 / 104, sources of 14, 5, 9 and
11 tokens, NE = 2, D = 2, beams 1 and 4), measured on the CPU (tests/test_deepatt_host.py re-measures and asserts; the figures
move by an ulp of a score with the CPU's matrix-product order, the tests assert gap > 4 err and the score_tol rule, not the
figures):

    cell=atr, seed 11:  gap 7.44e-04   err 3.8e-06 (gap = 195 x err)   rel 0.012
    cell=gru, seed 40:  gap 1.46e-04   err 1.9e-06 (gap =  77 x err)   rel 0.024

gap, err, rel as in tests/rnnsearch_ref.py (another machine measured err 3.8e-06 / 7.6e-06, i.e. 195 x / 19 x, with the same
gaps).  The bf16-storage restatement keeps the fp32 best hypotheses of the x 6 sharpened
model on both.
"""
import copy

import numpy as np
import torch

from oracle import ref_torch as rt
from tests import rnnsearch_ref as RS
from tests import variant_ref as V

GRU_DEFECTS = ("zr_swapped", "r_after_product", "blend_swapped", "no_carry", "bf16_state", "no_gather", "no_bg", "ug_neighbour")
SEEDS = {"atr": 11, "gru": 40}     # cell -> the seed of the model fixture (the widest gap / err among the seeds 1 .. 79)
RTOL, ATOL = RS.RTOL, RS.ATOL
score_tol = RS.score_tol
_bf, _sig = RS._bf, RS._sig


# ---------------------------------------------------------------------------------------------- numpy, float64
def gru_step(h_prev, Ug, bg, Uh, bh, xg, xh, mask=None, idx=None, defect=None):
    """h_prev [n_prev, H] or None (zero state); Ug [H, 2 H] (the z columns first); bg [2 H]; Uh [H, H]; bh [H]; xg [R, 2 H] and
    xh [R, H] the input projections; mask [R] of 0 / 1 or None; idx [R] int or None.
    -> dict of float64 arrays: out, z, r, rh, c [R, H] and, for gru_bound: h (the gathered state), q = rh Uh + bh, xh,
    mag_g = |h| |Ug| + |bg| and mag_ug = |h| |Ug| [R, 2 H], mag_h = |rh| |Uh| + |bh|, absUh, m.

    defect (one at a time; each is something a kernel could do):
      zr_swapped       the first H columns taken as r, the second as z
      r_after_product  r (.) (h Uh) in place of (r (.) h) Uh
      blend_swapped    (1 - z) h + z c
      no_carry         the mask ignored
      bf16_state       h rounded to bf16 everywhere, not only in the products
      no_gather        idx ignored
      no_bg            bg dropped
      ug_neighbour     r_j from column j + 1 of Ug in place of column H + j"""
    Ug, bg, Uh, bh, xg, xh = (np.asarray(t, np.float64) for t in (Ug, bg, Uh, bh, xg, xh))
    R, H = xh.shape
    if h_prev is None:
        h = np.zeros((R, H))
    else:
        h_prev = np.asarray(h_prev, np.float64)
        rows = np.arange(R) if (idx is None or defect == "no_gather") else np.asarray(idx)
        h = h_prev[rows]
    if defect == "bf16_state":
        h = _bf(h)
    Ugm = np.concatenate([Ug[:, :H], Ug[:, 1:H + 1]], 1) if defect == "ug_neighbour" else Ug
    bias_g = np.zeros_like(bg) if defect == "no_bg" else bg
    g = xg + h @ Ugm + bias_g
    mag_ug = np.abs(h) @ np.abs(Ugm)
    mag_g = mag_ug + np.abs(bias_g)
    z, r = _sig(g[:, :H]), _sig(g[:, H:])
    if defect == "zr_swapped":
        z, r = r, z
    rh = r * h
    q = (r * (h @ Uh) if defect == "r_after_product" else rh @ Uh) + bh
    mag_h = np.abs(rh) @ np.abs(Uh) + np.abs(bh)
    c = np.tanh(xh + q)
    o = (1.0 - z) * h + z * c if defect == "blend_swapped" else z * h + (1.0 - z) * c
    m = np.ones(R) if (mask is None or defect == "no_carry") else np.asarray(mask, np.float64)
    out = m[:, None] * o + (1.0 - m[:, None]) * h
    return {"out": out, "h": h, "z": z, "r": r, "rh": rh, "c": c, "q": q, "xh": xh, "mag_g": mag_g, "mag_ug": mag_ug,
            "mag_h": mag_h, "absUh": np.abs(Uh), "m": m}


def gru_bound(ref, form, what="out"):
    """Element-wise bounds of zk_rnn_gru_gates + zk_rnn_gru_out (form "bf16") / their zk_f32_ forms ("fp32") against
    gru_step(...) = ref, for inputs that are exactly representable where the kernels read them.  what: "z" (the fp32 update
    gate), "rh" (the second product's operand in the storage type), "out" (the fp32 state), "copy" (the state in the storage
    type).  Derived term by term as rnnsearch_ref.atr_bound is, PER_TERM = 2^-23 per accumulated term, u = 2^-8 (bf16) or 0:

      g     fp32 accumulation of H products, the bias and xg:  |dg| <= (H + 8) 2^-23 mag_g,  mag_g = |h| |Ug| + |bg|;
            bf16 form: the MFMA operand is h rounded to bf16 (Ug is bf16 already):  + 2^-8 |h| |Ug|;
      z, r  sigmoid has slope <= 1/4:  |dz| <= |dg_z| / 4 + 4 2^-23 z,  |dr| <= |dg_r| / 4 + 4 2^-23 r  (the sum, exp, 1 + e,
            the division);
      rh    = r h from the fp32 h:  |d rh| <= |h| |dr| + 2^-23 |rh|;  stored in the storage type, ONE rounding:  + u |rh|;
      q     = rh Uh + bh:  (H + 8) 2^-23 mag_h,  mag_h = |rh| |Uh| + |bh|,  + |d rh| |Uh|  -- that is 2^-8 |r h| |Uh| for the
            rounded operand plus the propagated error of r;
      c     tanh has slope <= 1:  |dc| <= |dq| + 2^-23 (|xh| + |q|) + 4 2^-23 |c|  (the sum, tanhf);
      o     = z h + (1 - z) c:  |do| <= |h - c| |dz| + (1 - z) |dc| + 8 2^-23 (|z h| + |(1 - z) c|);
      out   = m o + (1 - m) h with m in {0, 1}: the bound times m -- a carried row (m = 0) is h EXACTLY, bound 0;
      + u |out| for the copy in the storage type; the fp32 state has no further rounding.
    h itself enters z h and the carry in fp32 in BOTH forms: no 2^-8 |h| term -- that is what catches a bf16 state."""
    from tests import parity as PR
    H = ref["out"].shape[1]
    PT = PR.PER_TERM
    u = 2.0 ** -8 if form == "bf16" else 0.0
    dg = (H + 8) * PT * ref["mag_g"] + u * ref["mag_ug"]
    z, r, h, c, rh = ref["z"], ref["r"], ref["h"], ref["c"], ref["rh"]
    dz = dg[:, :H] / 4 + 4 * PT * z
    if what == "z":
        return dz
    dr = dg[:, H:] / 4 + 4 * PT * r
    drh = np.abs(h) * dr + PT * np.abs(rh) + u * np.abs(rh)
    if what == "rh":
        return drh
    dq = (H + 8) * PT * ref["mag_h"] + drh @ ref["absUh"]
    dc = dq + PT * (np.abs(ref["xh"]) + np.abs(ref["q"])) + 4 * PT * np.abs(c)
    do = np.abs(h - c) * dz + (1 - z) * dc + 8 * PT * (np.abs(z * h) + np.abs((1 - z) * c))
    bound = ref["m"][:, None] * do
    if what == "copy":
        bound = bound + u * np.abs(ref["out"])
    return bound


def gru_standin(h_prev, Ug, bg, Uh, bh, xg, xh, mask, idx, form):
    """What correct kernels compute, on the CPU in torch float32: both products summed over k in DESCENDING order (the
    reference sums ascending in float64); the bf16 form with the gate product's operand rounded and rh rounded once; the copy
    rounded once.  -> dict z, rh, out, copy (float64 arrays)."""
    f = lambda t: torch.as_tensor(np.asarray(t, np.float64)).float()
    Ug, bg, Uh, bh, xg, xh = f(Ug), f(bg), f(Uh), f(bh), f(xg), f(xh)
    R, H = xh.shape
    h = torch.zeros(R, H) if h_prev is None else f(h_prev)[torch.arange(R) if idx is None else torch.as_tensor(np.asarray(idx))]
    rnd = (lambda t: t.to(torch.bfloat16).float()) if form == "bf16" else (lambda t: t)
    rev = torch.arange(H - 1, -1, -1)
    g = xg + (rnd(h)[:, rev] @ Ug[rev] + bg)
    z, r = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:])
    rh = rnd(r * h)
    c = torch.tanh(xh + (rh[:, rev] @ Uh[rev] + bh))
    o = z * h + (1 - z) * c
    m = torch.ones(R) if mask is None else f(mask)
    out = m[:, None] * o + (1 - m[:, None]) * h
    return {k: v.double().numpy() for k, v in dict(z=z, rh=rh, out=out, copy=rnd(out)).items()}


# ---------------------------------------------------------------------------------------------- ref_torch model
_w, _carry, _names = RS._w, RS._carry, RS._names


def cell_fetch(x, P, pre, s, c):
    """rnns/{atr,gru,lrn,olrn}.py fetch_states under pre + "fetch_state_<s>": the input projections (no bias), stored; lrn /
    olrn have ONE, 3 H or 4 H wide."""
    p = pre + "fetch_state_%s/" % s
    if c in ("atr", "lrn", "olrn"):
        return (rt.linear(x, P, p + "hide_x", bias=False),)
    return (rt.linear(x, P, p + "gate_x", bias=False), rt.linear(x, P, p + "hide_x", bias=False))


def cell_call(h, inp, P, pre, s, c):
    """rnns/atr.py:32-60 / rnns/gru.py:32-57 under pre + "cell_<s>".  Storage sites of the kernels: the operands of the
    recurrent products are the stored (rounded) state and the stored r h; z, the blend and the carry use the fp32 state.
    rnns/lrn.py:32-53 / rnns/olrn.py:32-58: no variable, no product; the state is fp32, the projection is the stored one."""
    p = pre + "cell_%s" % s
    if c == "atr":
        return RS.atr_cell(h, inp[0], P, p)
    H = h.shape[-1]
    if c in ("lrn", "olrn"):
        x = inp[0]
        u = torch.sigmoid(x[..., :H] + h) * x[..., 2 * H:3 * H] + torch.sigmoid(x[..., H:2 * H] - h) * h
        return u * torch.sigmoid(x[..., 3 * H:] - u) if c == "olrn" else u
    g = inp[0] + (torch.matmul(rt._st(h, "rnn_state"), _w(P, p + "/gate_h/W_0_0")) + P[p + "/gate_h/b_0"])
    z, r = torch.sigmoid(g[..., :H]), torch.sigmoid(g[..., H:])
    q = torch.matmul(rt._st(r * h, "rnn_state"), _w(P, p + "/hide_h/W_0_0")) + P[p + "/hide_h/b_0"]
    return z * h + (1.0 - z) * torch.tanh(inp[1] + q)


def encoder(source, hp, P):
    """models/rnnsearch_deepatt.py:68-128 (positions un-reversed)."""
    dt = P["bias"].dtype
    H, c, NE = hp.hidden_size, str(hp.cell).lower(), hp.num_encoder_layer
    mask = (source != 0).to(dt)
    source, mask = rt.remove_invalid_seq(source, mask)
    B, L = source.shape
    x = rt._st(_w(P, _names(hp)[0])[source] + P["bias"], "embed")
    m = lambda t: mask[:, t:t + 1]
    at = lambda inp, t: tuple(v[:, t] for v in inp)
    pre = "encoder/layer_0/"
    inp = cell_fetch(x, P, pre, c, c)
    h = torch.zeros(B, H, dtype=dt)
    seq = []
    for t in range(L):
        h = _carry(m(t), cell_call(h, at(inp, t), P, pre, c, c), h)
        seq.append(h)
    hseq, last = torch.stack(seq, 1), h
    for l in range(1, NE + 1):
        pre = "encoder/layer_%d/" % l
        lo = cell_fetch(x, P, pre, c + "_lower", c)
        hi = cell_fetch(rt._st(hseq, "rnn_state"), P, pre, c + "_higher", c)
        g = torch.zeros(B, H, dtype=dt)
        gs = [None] * L
        for t in (range(L - 1, -1, -1) if l % 2 == 1 else range(L)):
            s = _carry(m(t), cell_call(g, at(lo, t), P, pre, c + "_lower", c), g)
            g = _carry(m(t), cell_call(s, at(hi, t), P, pre, c + "_higher", c), s)
            gs[t] = g
        hseq, last = torch.stack(gs, 1), g
    enc = rt._st(hseq, "rnn_state")
    i = "decoder_initializer/dec_init_state_init"
    init = torch.matmul(rt._st(last, "rnn_state"), _w(P, i + "/W_0_0")) + P[i + "/b_0"]          # (no tanh)
    pm = rt.linear(enc, P, "decoder/context_att", bias=False)        # once; shared by every deep_attention_l
    return {"encodes": enc, "pm": pm, "decoder_initializer": init, "mask": mask}


def decoder_step(y, h, state, hp, P):
    """One position of deep_att_dec_rnn + ff (models/rnnsearch_deepatt.py:180-211, 284-303): y [N, E] the (stored) input
    embedding, h [N, H] -> (logits [N, V], h')."""
    d, c = "decoder/", str(hp.cell).lower()
    enc, pm, mask = state["encodes"], state["pm"], state["mask"]
    s = cell_call(h, cell_fetch(y, P, d, c + "_lower", c), P, d, c + "_lower", c)
    ctx = []
    for l in range(hp.num_decoder_layer):
        a = d + "deep_attention_%d/" % l
        qa = rt.linear(rt._st(s, "rnn_state"), P, a + "feed_query")
        v = P[a + "feed_logits/W_0_0"][:, 0]
        logit = torch.matmul(torch.tanh(qa[:, None, :] + pm), v) + P[a + "feed_logits/b_0"]
        logit = logit + (1.0 - mask) * (-rt.Cfg.inf)
        w = torch.softmax(logit, -1)
        cs = rt._st((w[:, :, None] * enc).sum(1), "attn_out")
        ctx.append(cs)
        name = "%s_higher_%d" % (c, l)
        s = cell_call(s, cell_fetch(cs, P, d, name, c), P, d, name, c)
    cat = torch.cat([rt._st(s, "rnn_state")] + ctx + [y], -1)
    feat = rt._st(torch.tanh(torch.matmul(cat, _w(P, "ff/W_0_0")) + P["ff/b_0"]))
    return torch.matmul(feat, _w(P, _names(hp)[2]).t()), s


def decoding_fns(hp, P):
    """(encoding_fn, decoding_fn) of models/rnnsearch_deepatt.py:361-392 (search_mode = cache) for rt.beam_search."""
    hp = rt.closing_dropout(copy.copy(hp))

    def encoding_fn(source):
        return V.cached_state(encoder(source, hp, P))

    def decoding_fn(target, state, time):
        tok = target[:, -1]
        y = _w(P, _names(hp)[1])[tok] + P["bias"]
        if bool((target == hp.tgt_vocab.pad()).all()):          # rnnsearch_deepatt.py:261-263
            y = torch.zeros_like(y)
        logits, hn = decoder_step(rt._st(y, "embed"), state["decoder"]["state"], state, hp, P)
        state["decoder"]["state"] = hn
        return logits, state

    return encoding_fn, decoding_fn


def full_decoder(target, state, hp, P):
    """The training-path decoder (models/rnnsearch_deepatt.py:240-303 with is_training): inputs shifted right by one zero
    row, one scan over the whole target.  target [B, Lt] without padding -> logits [B, Lt, V]."""
    y = _w(P, _names(hp)[1])[target] + P["bias"]
    y = rt._st(torch.nn.functional.pad(y, (0, 0, 1, 0))[:, :-1, :], "embed")
    h = state["decoder_initializer"]
    out = []
    for t in range(target.shape[1]):
        logits, h = decoder_step(y[:, t], h, state, hp, P)
        out.append(logits)
    return torch.stack(out, 1)


def init_params(hp, seed):
    return V.init_params(hp, "rnnsearch_deepatt", seed)


def make_fixture(hp, src, seed, factor=4.0):
    """variant_ref.make_fixture on this model -> dict Pn, gap, err, rel (the worst over beam 1 and 4)."""
    return V.make_fixture("rnnsearch_deepatt", decoding_fns, (ATOL, RTOL), hp, src, seed, factor)


LENGTHS = (14, 5, 9, 11)


def fixture_hp(cell="gru", **kw):
    from tests.common import make_hp
    kw.setdefault("num_encoder_layer", 2)
    kw.setdefault("num_decoder_layer", 2)
    hp = make_hp("rnnsearch_deepatt", H=128, heads=1, search_mode="cache", cell=cell, layer_norm=False,
                 scope_name="t_deepatt_%s" % cell, **kw)
    hp.embed_size = 64
    return hp
