"""References of rnnsearch at inference (a plain module, no pytest in it).

Reference arithmetic (models/rnnsearch.py, rnns/rnn.py, rnns/atr.py, func.py:107-161), carry(m, a, b) = m a + (1 - m) b:

    ATR cell    q = h U + b;  i = sigmoid(p + q);  f = sigmoid(p - q);  o = i p + f h;  out = carry(m, o, h)
    attention   logit_j = v . tanh(qa + pm_j) + (1 - mask_j) * -inf;  a = softmax_j;  c = sum_j a_j mem_j

``atr_step`` / ``add_attention``   the float64 numpy statements with everything the bounds need; ``defect=`` plants ONE defect.
``atr_bound`` / ``add_bound``      the element-wise bounds the kernels are held to (derivations in their docstrings).
``atr_standin`` / ``add_standin``  what a correct kernel computes, in torch float32 with another summation order.
``decoding_fns``                   encoding_fn / decoding_fn for oracle.ref_torch.beam_search: rt.linear, rt.remove_invalid_seq
                                   and rt's storage sites (Cfg.store_bf16) around the restated scans and attention.
``full_decoder``                   the teacher-forced decoder (cond_rnn over the whole target): the dual of the cached step.
``init_params`` / ``make_fixture`` the tiny model of the GPU model tests and what the REFERENCE ALONE shows on it.

make_fixture on the fixture of tests/test_gpu_rnnsearch_model.py (H = 128, E = 64, vocabularies 120 / 104, sources of 14, 5,
9 and 11 tokens, beams 1 and 4), measured on the CPU (tests/test_rnnsearch_host.py re-measures and asserts them):

    caencoder=True,  seed 37:  gap 1.96e-04   err 5.7e-06 (gap = 34 x err)   rel 0.023
    caencoder=False, seed  9:  gap 2.92e-04   err 5.7e-06 (gap = 51 x err)   rel 0.028

gap: the smallest difference between a kept candidate and its runner-up; err: the largest |score_fp32 - score_float64| over
the kept candidates (scores of magnitude 20 .. 30: a few fp32 ulps of the score itself); rel: err as a share of the project's
fp32 score tolerance atol 1e-6 + rtol 1e-5 |score|.  (err is one to three ulps of a score and moves by an ulp with the CPU's
matrix-product order: another machine measured 3.8e-06 / 5.7e-06; the tests assert gap > 4 err and rel <= 1/4, not the
figures.)  rel <= 1/4 in both forms, so the GPU tests hold the scores to that standard (score_tol).  The bf16-storage
restatement keeps the fp32 best hypotheses of the x 6 sharpened model on both.
"""
import copy
import functools

import numpy as np
import torch

from oracle import ref_torch as rt
from tests import variant_ref as V

ATR_DEFECTS = ("no_twin", "gates_swapped", "no_carry", "bf16_state", "no_bias", "no_gather", "u_transposed")
ADD_DEFECTS = ("mask_ignored", "neighbour_memory", "ctx_from_pm", "no_tanh", "extra_key", "no_v")
INF = 1e8                       # utils/dtype.py inf() of float32
SEEDS = {True: 37, False: 9}    # caencoder -> the seed of the model fixture (the widest gap / err among the seeds 1 .. 79)
RTOL, ATOL = 1e-5, 1e-6         # the project's fp32 standard for scores (tests/test_gpu_decode_f32.py)


def score_tol(rel, err):
    """(rtol, atol) of the fp32 GPU score check.  rel: the largest |score_fp32 - score_float64| / (ATOL + RTOL |score|) that
    make_fixture measures.  The project's fp32 standard where the fp32 reference itself is within a quarter of it, else
    4 x the measured distance err as the absolute part."""
    return (RTOL, ATOL) if rel <= 0.25 else (RTOL, 4.0 * err)


def _bf(x):
    return torch.as_tensor(np.asarray(x, np.float64)).float().to(torch.bfloat16).double().numpy()


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


# ---------------------------------------------------------------------------------------------- numpy, float64
def atr_step(h_prev, U, b, p, mask=None, idx=None, defect=None):
    """h_prev [n_prev, H] or None (zero state); U [H, H]; b [H]; p [R, H]; mask [R] of 0 / 1 or None; idx [R] int or None.
    -> dict of float64 arrays: out [R, H] and, for atr_bound: h (the gathered state), q, mag_u = |h| |U|, mag = mag_u + |b|, i, f, m.

    defect (one at a time; each is something a kernel could do):
      no_twin        the input gate as 1 - f (rnns/atr.py:55-56, the twin=False form)
      gates_swapped  i = sigmoid(p - q), f = sigmoid(p + q)
      no_carry       the mask ignored
      bf16_state     h rounded to bf16 everywhere, not only in the product
      no_bias        b dropped
      no_gather      idx ignored
      u_transposed   h U^T"""
    U, b, p = (np.asarray(t, np.float64) for t in (U, b, p))
    R, H = p.shape
    if h_prev is None:
        h = np.zeros((R, H))
    else:
        h_prev = np.asarray(h_prev, np.float64)
        rows = np.arange(R) if (idx is None or defect == "no_gather") else np.asarray(idx)
        h = h_prev[rows]
    if defect == "bf16_state":
        h = _bf(h)
    Um = U.T if defect == "u_transposed" else U
    bias = np.zeros_like(b) if defect == "no_bias" else b
    q = h @ Um + bias
    mag_u = np.abs(h) @ np.abs(Um)
    mag = mag_u + np.abs(bias)
    i, f = _sig(p + q), _sig(p - q)
    if defect == "gates_swapped":
        i, f = f, i
    if defect == "no_twin":
        i = 1.0 - f
    o = i * p + f * h
    m = np.ones(R) if (mask is None or defect == "no_carry") else np.asarray(mask, np.float64)
    out = m[:, None] * o + (1.0 - m[:, None]) * h
    return {"out": out, "h": h, "q": q, "mag": mag, "mag_u": mag_u, "i": i, "f": f, "p": p, "m": m}


def atr_bound(ref, form, copy=False):
    """Element-wise bound of zk_rnn_atr_step (form "bf16") / zk_f32_rnn_atr_step ("fp32") against atr_step(...) = ref, for
    inputs that are exactly representable where the kernel reads them.  Derived as tests/parity.py:gemm_bound is, with
    PER_TERM = 2^-23 (twice the unit roundoff) per accumulated term:

      q     fp32 accumulation of H products and the bias: |dq| <= (H + 8) 2^-23 mag,  mag = |h| |U| + |b|;
            bf16 form: the MFMA operand is h rounded to bf16 (unit roundoff 2^-8, U is bf16 already):  + 2^-8 |h| |U|;
      i, f  sigmoid has slope i (1 - i) <= 1/4: |di| <= i (1 - i) |dq| + 4 2^-23 i  (the sum p + q, exp, 1 + e, the division);
      o     = i p + f h:  |do| <= (|p| i (1 - i) + |h| f (1 - f)) |dq| + 8 2^-23 (|i p| + |f h|)
      out   = m o + (1 - m) h with m in {0, 1}: the bound times m -- a carried row (m = 0) is h EXACTLY, bound 0;
      + u_out |out| for the copy in the storage type (2^-8 bf16); the fp32 state has no further rounding.
    h itself enters f h and the carry in fp32 in BOTH forms: no 2^-8 |h| term -- that is what catches a bf16 state."""
    from tests import parity as PR
    H = ref["out"].shape[1]
    dq = (H + 8) * PR.PER_TERM * ref["mag"] + (2.0 ** -8 * ref["mag_u"] if form == "bf16" else 0.0)
    i, f, p, h = ref["i"], ref["f"], ref["p"], ref["h"]
    do = (np.abs(p) * i * (1 - i) + np.abs(h) * f * (1 - f)) * dq + 8 * PR.PER_TERM * (np.abs(i * p) + np.abs(f * h))
    bound = ref["m"][:, None] * do
    if copy:
        bound = bound + (2.0 ** -8 if form == "bf16" else 0.0) * np.abs(ref["out"])
    return bound


def atr_standin(h_prev, U, b, p, mask, idx, form, copy=False):
    """What a correct kernel computes, on the CPU in torch float32: the product summed over k in DESCENDING order (the
    reference sums ascending in float64), the bf16 form with the operand rounded; the copy rounded once."""
    f = lambda t: torch.as_tensor(np.asarray(t, np.float64)).float()
    U, b, p = f(U), f(b), f(p)
    R, H = p.shape
    h = torch.zeros(R, H) if h_prev is None else f(h_prev)[torch.arange(R) if idx is None else torch.as_tensor(np.asarray(idx))]
    ho = h.to(torch.bfloat16).float() if form == "bf16" else h
    rev = torch.arange(H - 1, -1, -1)
    q = ho[:, rev] @ U[rev] + b
    o = torch.sigmoid(p + q) * p + torch.sigmoid(p - q) * h
    m = torch.ones(R) if mask is None else f(mask)
    out = m[:, None] * o + (1 - m[:, None]) * h
    if copy and form == "bf16":
        out = out.to(torch.bfloat16).float()
    return out.double().numpy()


def add_attention(qa, pm, mem, v, mask=None, kv_group=1, Ls=None, inf=INF, defect=None):
    """qa [R, M]; pm, mem [R / kv_group, L, M] (L >= Ls: keys 0 .. Ls - 1 exist); v [M]; mask [R / kv_group, L] or None.
    -> dict: out [R, M] (the context), a [R, Ls], x = logit - max, absmem = sum_j a_j |mem_j|, vsum = sum |v|.

    defect:  mask_ignored;  neighbour_memory (the next sentence's pm / mem / mask under kv_group);  ctx_from_pm (the context
    summed over the PROJECTED memory);  no_tanh;  extra_key (one key past Ls; needs L > Ls);  no_v (the logit is the plain
    sum of the tanh)."""
    qa, pm, mem, v = (np.asarray(t, np.float64) for t in (qa, pm, mem, v))
    R, M = qa.shape
    nB, L, _ = pm.shape
    assert nB * kv_group == R
    n = L if Ls is None else int(Ls)
    if defect == "extra_key":
        assert n < L
        n += 1
    owner = np.arange(R) // kv_group
    if defect == "neighbour_memory":
        owner = (owner + 1) % nB
    mk = np.ones((nB, L)) if (mask is None or defect == "mask_ignored") else np.asarray(mask, np.float64)
    z = qa[:, None, :] + pm[owner, :n]
    t = z if defect == "no_tanh" else np.tanh(z)
    logit = t.sum(-1) if defect == "no_v" else t @ v
    logit = logit + (1.0 - mk[owner, :n]) * -inf
    x = logit - logit.max(-1, keepdims=True)
    e = np.exp(x)
    a = e / e.sum(-1, keepdims=True)
    src = pm if defect == "ctx_from_pm" else mem
    out = np.einsum("rj,rjm->rm", a, src[owner, :n])
    absmem = np.einsum("rj,rjm->rm", a * 1.0, np.abs(src[owner, :n]))
    xmem = np.einsum("rj,rjm->rm", a * np.abs(x), np.abs(src[owner, :n]))
    return {"out": out, "a": a, "x": x, "absmem": absmem, "xmem": xmem, "vsum": float(np.abs(v).sum()), "M": M, "Ls": n}


def add_bound(ref, form, copy=False):
    """Element-wise bound of zk_add_attn ("bf16") / zk_f32_add_attn ("fp32") against add_attention(...) = ref; all arithmetic
    is fp32 in both forms (the inputs are exactly representable in the storage type), PER_TERM = 2^-23 per term:

      logit   a term v_c tanh(z_c): the rounding of z_c = qa_c + pm_c moves tanh by <= 2^-24 |z| (1 - tanh^2) <= 2^-24 / 2,
              tanhf and the product a few units more, each against |tanh| <= 1; M accumulated terms:
              |dlogit| <= (M + 8) 2^-23 sum_c |v_c|   (=: dl; a masked key's added -inf swallows all of it, its weight is 0);
      a_j     = exp(x_j) / sum exp(x), x_j = logit_j - max: relative error <= 2 dl (numerator and denominator) + 2^-23 |x_j|
              (the rounding of x_j; a key far below the maximum has a tiny weight) + (Ls + 8) 2^-23 (exp, the sum -- in tiles,
              with a rescale per tile --, the division);
      c       = sum_j a_j mem_j:  |dc| <= (2 dl + (2 Ls + 10) 2^-23) sum_j a_j |mem_j| + 2^-23 sum_j a_j |x_j| |mem_j|
      + u_out |c| for the copy in the storage type.
    A key with weight 0 in the reference (masked: exp(-1e8) = 0) contributes 0 to the bound: it must contribute exactly 0."""
    from tests import parity as PR
    dl = (ref["M"] + 8) * PR.PER_TERM * ref["vsum"]
    bound = (2 * dl + (2 * ref["Ls"] + 10) * PR.PER_TERM) * ref["absmem"] + PR.PER_TERM * ref["xmem"]
    if copy:
        bound = bound + (2.0 ** -8 if form == "bf16" else 0.0) * np.abs(ref["out"])
    return bound


def add_standin(qa, pm, mem, v, mask, kv_group, Ls, form, copy=False, inf=INF):
    """torch float32, the keys in DESCENDING order and the channels summed by a matrix product; one rounding of the copy."""
    f = lambda t: torch.as_tensor(np.asarray(t, np.float64)).float()
    qa, pm, mem, v = f(qa), f(pm), f(mem), f(v)
    R = qa.shape[0]
    owner = torch.arange(R) // kv_group
    order = torch.arange(Ls - 1, -1, -1)
    mk = torch.ones(pm.shape[0], pm.shape[1]) if mask is None else f(mask)
    logit = torch.tanh(qa[:, None, :] + pm[owner][:, order]) @ v + (1 - mk[owner][:, order]) * torch.tensor(-inf)
    a = torch.softmax(logit, -1)
    out = torch.einsum("rj,rjm->rm", a, mem[owner][:, order])
    if copy and form == "bf16":
        out = out.to(torch.bfloat16).float()
    return out.double().numpy()


# ---------------------------------------------------------------------------------------------- ref_torch model
def _w(P, name):
    return rt._st_fwd(P[name])


def atr_cell(h, p, P, scope):
    """rnns/atr.py:32-60.  Storage sites of the kernel: the operand of the recurrent product is the stored (rounded) state,
    q stays in the accumulators, i p + f h uses the fp32 state."""
    q = torch.matmul(rt._st(h, "rnn_state"), _w(P, scope + "/hide_h/W_0_0")) + P[scope + "/hide_h/b_0"]
    return torch.sigmoid(p + q) * p + torch.sigmoid(p - q) * h


def _carry(m, a, b):
    return m * a + (1.0 - m) * b


def _names(hp):
    return rt._emb_name(hp, "src"), rt._emb_name(hp, "tgt"), rt._emb_name(hp, "softmax")


def encoder(source, hp, P):
    """models/rnnsearch.py:16-75 (positions un-reversed)."""
    dt = P["bias"].dtype
    H = hp.hidden_size
    mask = (source != 0).to(dt)
    source, mask = rt.remove_invalid_seq(source, mask)
    B, L = source.shape
    x = rt._st(_w(P, _names(hp)[0])[source] + P["bias"], "embed")
    f, b = "encoder/forward/", "encoder/backward/"
    m = lambda t: mask[:, t:t + 1]
    pf = rt.linear(x, P, f + "fetch_state_atr/hide_x", bias=False)
    h = torch.zeros(B, H, dtype=dt)
    hf = []
    for t in range(L):
        h = _carry(m(t), atr_cell(h, pf[:, t], P, f + "cell_atr"), h)
        hf.append(h)
    hf = torch.stack(hf, 1)
    if hp.caencoder:
        plo = rt.linear(x, P, b + "fetch_state_atr_lower/hide_x", bias=False)
        phi = rt.linear(rt._st(hf, "rnn_state"), P, b + "fetch_state_atr_higher/hide_x", bias=False)
        g = torch.zeros(B, H, dtype=dt)
        gs = [None] * L
        for t in range(L - 1, -1, -1):
            s = _carry(m(t), atr_cell(g, plo[:, t], P, b + "cell_atr_lower"), g)
            g = _carry(m(t), atr_cell(s, phi[:, t], P, b + "cell_atr_higher"), s)
            gs[t] = g
        enc = rt._st(torch.stack(gs, 1), "rnn_state")
        feature = enc[:, 0]
    else:
        pb = rt.linear(x, P, b + "fetch_state_atr/hide_x", bias=False)
        h = torch.zeros(B, H, dtype=dt)
        hb = [None] * L
        for t in range(L - 1, -1, -1):
            h = _carry(m(t), atr_cell(h, pb[:, t], P, b + "cell_atr"), h)
            hb[t] = h
        enc = rt._st(torch.cat([hf, torch.stack(hb, 1)], -1), "rnn_state")
        feature = torch.cat([enc[:, L - 1, :H], enc[:, 0, H:]], -1)
    i = "decoder_initializer/atr_init"
    init = torch.tanh(torch.matmul(feature, _w(P, i + "/W_0_0")) + P[i + "/b_0"])
    # (the projected memory is computed once; the reference recomputes the same values in every step)
    pm = rt.linear(enc, P, "decoder/context_att", bias=False)
    return {"encodes": enc, "pm": pm, "decoder_initializer": init, "mask": mask}


def decoder_step(y, h, state, hp, P):
    """One position of cond_rnn(one2one=False) + pre_logits (rnns/rnn.py:119-146; models/rnnsearch.py:118-133):
    y [N, E] the (stored) input embedding, h [N, H] -> (logits [N, V], h')."""
    d = "decoder/"
    enc, pm, mask = state["encodes"], state["pm"], state["mask"]
    plo = rt.linear(y, P, d + "fetch_state_atr_lower/hide_x", bias=False)
    s = atr_cell(h, plo, P, d + "cell_atr_lower")
    ss = rt._st(s, "rnn_state")
    qa = rt.linear(ss, P, d + "attention/feed_query")
    v = P[d + "attention/feed_logits/W_0_0"][:, 0]
    logit = torch.matmul(torch.tanh(qa[:, None, :] + pm), v) + P[d + "attention/feed_logits/b_0"]
    logit = logit + (1.0 - mask) * (-rt.Cfg.inf)
    a = torch.softmax(logit, -1)
    c = (a[:, :, None] * enc).sum(1)
    cs = rt._st(c, "attn_out")
    phi = rt.linear(cs, P, d + "fetch_state_atr_higher/hide_x", bias=False)
    hn = atr_cell(s, phi, P, d + "cell_atr_higher")
    cat = torch.cat([rt._st(hn, "rnn_state"), cs, y], -1)
    feat = rt._st(torch.tanh(torch.matmul(cat, _w(P, "pre_logits/W_0_0")) + P["pre_logits/b_0"]))
    return torch.matmul(feat, _w(P, _names(hp)[2]).t()), hn


def decoding_fns(hp, P):
    """(encoding_fn, decoding_fn) of models/rnnsearch.py:194-225 (search_mode = cache) for rt.beam_search."""
    hp = rt.closing_dropout(copy.copy(hp))

    def encoding_fn(source):
        return V.cached_state(encoder(source, hp, P))

    def decoding_fn(target, state, time):
        tok = target[:, -1]
        y = _w(P, _names(hp)[1])[tok] + P["bias"]
        if bool((target == hp.tgt_vocab.pad()).all()):          # rnnsearch.py:101-103
            y = torch.zeros_like(y)
        logits, hn = decoder_step(rt._st(y, "embed"), state["decoder"]["state"], state, hp, P)
        state["decoder"]["state"] = hn
        return logits, state

    return encoding_fn, decoding_fn


def full_decoder(target, state, hp, P):
    """The training-path decoder (models/rnnsearch.py:78-133 with is_training): inputs shifted right by one zero row, one
    scan over the whole target.  target [B, Lt] without padding -> logits [B, Lt, V]."""
    y = _w(P, _names(hp)[1])[target] + P["bias"]
    y = rt._st(torch.nn.functional.pad(y, (0, 0, 1, 0))[:, :-1, :], "embed")
    h = state["decoder_initializer"]
    out = []
    for t in range(target.shape[1]):
        logits, h = decoder_step(y[:, t], h, state, hp, P)
        out.append(logits)
    return torch.stack(out, 1)


def init_params(hp, seed):
    return V.init_params(hp, "rnnsearch", seed)


def make_fixture(hp, src, seed, factor=4.0):
    """variant_ref.make_fixture on this model -> dict Pn, gap, err, rel (the worst over beam 1 and 4)."""
    return V.make_fixture("rnnsearch", decoding_fns, (ATOL, RTOL), hp, src, seed, factor)


LENGTHS = (14, 5, 9, 11)


def fixture_hp(caencoder=True, **kw):
    from tests.common import make_hp
    hp = make_hp("rnnsearch", H=128, search_mode="cache", cell="atr", caencoder=caencoder, layer_norm=False,
                 scope_name="t_rnnsearch_%s" % ("ca" if caencoder else "bi"), **kw)
    hp.embed_size = 64
    return hp
