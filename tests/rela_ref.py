"""References of transformer_rela at inference (a plain module, no pytest in it).

Reference arithmetic (modules/rela.py:13-109; models/transformer_rela.py is models/transformer.py with every
func.dot_attention replaced by it).  For one query row i, head h of nh, d = H / nh, keys j < nkeys:

    s_ijh = (q_ih d^-0.5) . k_jh
    w_ijh = relu(s_ijh) m_j             m_j = 1 where the reference's additive bias is 0, else 0: MULTIPLIED (rela.py:66-72)
    c_i   = concat_h sum_j w_ijh v_jh                       no normalisation of the weights
    ms_i  = mean over ALL H channels of c_i^2               after combine_heads: across the heads
    o_i   = scale c_i rsqrt(ms_i + eps) sigmoid(gate c_i)   eps = 1e-8

``rela_attention``   the float64 numpy statement of the above with everything ``bound`` needs; ``defect=`` plants ONE defect.
``bound``            the element-wise bound the bf16 and the fp32 kernel are held to (derivation in its docstring).
``standin``          what a correct kernel computes, in torch float32 with another summation order, rounded to the storage type.
``CASES`` / ``case_inputs``   the operands of the kernel tests (tests/test_gpu_rela_kernels.py), built on the CPU.
``decoding_fns``     encoding_fn / decoding_fn for oracle.ref_torch.beam_search: ref_torch's own linear, split_heads,
                     combine_heads, layer_norm, residual_fn, ffn_layer, embedding and timing with its storage sites; only
                     dot_attention + gated_rms_norm restated (encoder and both decoder attentions).
``full_decoder``     the training-path decoder restated (causal mask multiplied in): the dual of the cached step.
``init_params`` / ``make_fixture``   the tiny model of the GPU model tests and its measured distance from the discontinuity.
"""
import copy
import functools

import numpy as np
import torch

from oracle import ref_torch as rt
from tests import variant_ref as V

EPS = 1e-8
DEFECTS = ("mask_added", "rms_per_head", "normalised", "gate_no_x", "no_qscale", "extra_key", "neighbour_keys",
           "eps_outside")


# ---------------------------------------------------------------------------------------------- numpy, float64
def rela_attention(q, k, v, nh, scale, gate, kmask=None, kv_group=1, nkeys=None, eps=EPS, defect=None):
    """q [B, Lq, H]; k, v [B / kv_group, Lk, H]; kmask [B / kv_group, Lk] (non-zero = the key takes part) or None;
    nkeys: the keys 0 .. nkeys - 1 exist (None: Lk); scale, gate [H].  -> dict of float64 arrays: out [B, Lq, H], c, ms
    [B, Lq], and for ``bound``: dc (bound of the error of c in fp32 arithmetic), r = rsqrt(ms + eps), z = gate c.

    defect (one at a time; each is something a kernel could do):
      mask_added      the mask added the way func.dot_attention adds it to a softmax, with a true infinity:
                      (1 - m) * -inf is NaN on every VALID key (0 * inf).  (With the finite 1e8 of utils/dtype.py the added
                      form equals the product after the ReLU, so the product is the only form there is to state.)
      rms_per_head    the mean square per head instead of over the H channels
      normalised      the weights divided by their sum
      gate_no_x       sigmoid(gate) instead of sigmoid(gate c)
      no_qscale       d^-0.5 dropped
      extra_key       one key beyond nkeys read (needs nkeys < Lk)
      neighbour_keys  the next sentence's keys / values / mask under kv_group
      eps_outside     rsqrt(ms) + eps"""
    q, k, v, scale, gate = (np.asarray(t, np.float64) for t in (q, k, v, scale, gate))
    B, Lq, H = q.shape
    nB, Lk, _ = k.shape
    d = H // nh
    assert nB * kv_group == B
    nk = Lk if nkeys is None else int(nkeys)
    if defect == "extra_key":
        assert nk < Lk
        nk += 1
    owner = np.arange(B) // kv_group
    if defect == "neighbour_keys":
        owner = (owner + 1) % nB
    m = np.ones((nB, Lk)) if kmask is None else (np.asarray(kmask, np.float64) != 0).astype(np.float64)
    qs = d ** -0.5 if defect != "no_qscale" else 1.0
    qh = (q * qs).reshape(B, Lq, nh, d)
    kh, vh = k[owner, :nk].reshape(B, nk, nh, d), v[owner, :nk].reshape(B, nk, nh, d)
    mm = m[owner, :nk]
    s = np.einsum("bihd,bjhd->bhij", qh, kh)
    s_abs = np.einsum("bihd,bjhd->bhij", np.abs(qh), np.abs(kh))
    if defect == "mask_added":
        with np.errstate(invalid="ignore"):
            w = np.maximum(s + ((1.0 - mm) * -np.inf)[:, None, None, :], 0.0)
    else:
        w = np.maximum(s, 0.0) * mm[:, None, None, :]
    if defect == "normalised":
        w = w / np.maximum(w.sum(-1, keepdims=True), 1e-300)
    c = np.einsum("bhij,bjhd->bihd", w, vh).reshape(B, Lq, H)
    # fp32 arithmetic (see bound): a score is off by at most (d + 2) 2^-23 sum |q_c k_c| (the rounding of q d^-0.5 and d
    # fused multiply-adds); a key whose score could not reach 0 from below by that much has the weight 0 exactly
    from tests import parity as PR
    ds = (d + 2) * PR.PER_TERM * s_abs
    dw = np.where(s > -ds, ds, 0.0) * mm[:, None, None, :]
    dc = (np.einsum("bhij,bjhd->bihd", dw, np.abs(vh)) +
          (nk + 2) * PR.PER_TERM * np.einsum("bhij,bjhd->bihd", w, np.abs(vh))).reshape(B, Lq, H)
    if defect == "rms_per_head":
        ms_el = np.repeat((c.reshape(B, Lq, nh, d) ** 2).mean(-1), d, axis=-1)
    else:
        ms_el = np.repeat((c ** 2).mean(-1, keepdims=True), H, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = 1.0 / np.sqrt(ms_el) + eps if defect == "eps_outside" else 1.0 / np.sqrt(ms_el + eps)
        z = gate * c
        sig = 1.0 / (1.0 + np.exp(-(gate if defect == "gate_no_x" else z)))
        out = scale * c * r * sig
    return {"out": out, "c": c, "ms": (c ** 2).mean(-1), "dc": dc, "r": r, "z": z, "sig": sig, "scale": scale, "eps": eps}


def bound(ref, out_dtype):
    """Element-wise bound of a kernel that forms everything in fp32 (in any summation order) from exactly representable
    inputs and rounds ONLY the output to its storage type, against rela_attention(...) = ref.  Derived as
    tests/parity.py:gemm_bound is, with PER_TERM = 2^-23 (twice the unit roundoff) per accumulated term:

      c      |dc| <= sum_j |dw_j| |v_j| + (nkeys + 2) 2^-23 sum_j w_j |v_j|,  |dw_j| <= (d + 2) 2^-23 sum_c |q_c k_c| for the
             keys whose score can be positive at all (ref["dc"], computed with the reference);
      ms     the mean of H squares: |dms| <= (2 / H) sum_c |c_c| |dc_c| + (H + 8) 2^-23 ms   (every term is positive);
      r      = rsqrt(ms + eps): |dr| / r <= |dms| / (2 (ms + eps))      -- the relative error of ms through rsqrt, halved;
      o      = scale c r sigmoid(gate c):  |do| <= |scale| r (sig + |z| sig (1 - sig)) |dc|   (the slope of c sigmoid(gate c))
                                                   + |o| |dr| / r + 8 2^-23 |o|              (rsqrt, exp, the products)
      + u_out |o|   one rounding to the storage type (2^-8 bf16, 2^-23 fp32).
    An element whose row has c = 0 everywhere has the bound 0: it must be exactly 0."""
    from tests import parity as PR
    c, dc, r, z, sig, o = ref["c"], ref["dc"], ref["r"], ref["z"], ref["sig"], ref["out"]
    H = c.shape[-1]
    ms = ref["ms"][..., None]
    dms = (2.0 / H) * (np.abs(c) * dc).sum(-1, keepdims=True) + (H + 8) * PR.PER_TERM * ms
    rel_r = dms / (2.0 * (ms + ref["eps"]))
    slope = np.abs(ref["scale"]) * r * (sig + np.abs(z) * sig * (1.0 - sig))
    return slope * dc + np.abs(o) * rel_r + (8 * PR.PER_TERM + PR.U_OUT[out_dtype]) * np.abs(o)


def standin(q, k, v, nh, scale, gate, out_dtype, kmask=None, kv_group=1, nkeys=None, eps=EPS):
    """What a correct kernel computes, on the CPU: torch float32, the keys summed in DESCENDING order by matrix products
    (the reference sums them ascending by einsum in float64), the mean square by torch.mean, one rounding to out_dtype."""
    f = lambda t: torch.as_tensor(np.asarray(t, np.float64)).float()
    q, k, v, scale, gate = f(q), f(k), f(v), f(scale), f(gate)
    B, Lq, H = q.shape
    d = H // nh
    nk = k.shape[1] if nkeys is None else int(nkeys)
    owner = torch.arange(B) // kv_group
    m = torch.ones(k.shape[0], k.shape[1]) if kmask is None else (f(kmask) != 0).float()
    idx = torch.arange(nk - 1, -1, -1)
    kh = k[owner][:, idx].reshape(B, nk, nh, d).permute(0, 2, 3, 1)          # [B, nh, d, nk]
    vh = v[owner][:, idx].reshape(B, nk, nh, d).permute(0, 2, 1, 3)          # [B, nh, nk, d]
    qh = (q * torch.tensor(d ** -0.5, dtype=torch.float32)).reshape(B, Lq, nh, d).permute(0, 2, 1, 3)
    w = torch.relu(qh @ kh) * m[owner][:, idx][:, None, None, :]
    c = (w @ vh).permute(0, 2, 1, 3).reshape(B, Lq, H)
    r = torch.rsqrt((c * c).mean(-1, keepdim=True) + torch.tensor(eps, dtype=torch.float32))
    return (scale * c * r * torch.sigmoid(gate * c)).to(out_dtype)


# ---------------------------------------------------------------------------------------------- kernel-test cases
# name -> shape of one direct call.  B: query sentences (rows of a decode step), G: kv_group, times: the values of the
# device-resident position of a cached step (keys 0 .. time exist), lengths: valid keys per memory (mask), forms: the
# storage types the case runs in.
CASES = {
    # decode cross-attention: 2 sentences x 3 beam rows; sentence 1 has 6 valid keys, its 11 masked keys score large
    "cross": dict(B=6, G=3, nh=2, d=64, Lq=1, Lk=17, lengths=(17, 6), hot_masked=True, layout="kv", forms=("bf16", "fp32")),
    # cached self-attention: 5 rows with a cache of 24 slots each, H = 192
    "self": dict(B=5, G=1, nh=3, d=64, Lq=1, Lk=24, times=(0, 1, 8, 23), layout="cache", forms=("bf16", "fp32")),
    # encoder: q / k / v slices of one [T, 3H] matrix, lengths 19, 1, 7
    "encoder": dict(B=3, G=1, nh=2, d=64, Lq=19, Lk=19, lengths=(19, 1, 7), layout="qkv", forms=("bf16", "fp32")),
    # rows without a positive score (exact zeros) and rows with exactly ONE positive score of very different sizes
    "special": dict(B=6, G=1, nh=2, d=64, Lq=1, Lk=9, layout="kv", special=True, forms=("bf16", "fp32")),
    "bf16_d32": dict(B=4, G=2, nh=2, d=32, Lq=1, Lk=11, lengths=(11, 4), layout="kv", forms=("bf16",)),
    "bf16_H2048": dict(B=2, G=2, nh=32, d=64, Lq=1, Lk=9, lengths=(7,), layout="kv", forms=("bf16",)),
    "fp32_d8": dict(B=4, G=2, nh=2, d=8, Lq=1, Lk=11, lengths=(11, 4), layout="kv", forms=("fp32",)),
}
SPECIAL_SCORES = (0.05, 1.0, 20.0, 3e-3)       # the single positive score of the rows 2 .. 5 of "special" (rows 0, 1: none)


def case_inputs(name, form, seed=0):
    """-> dict q [B, Lq, H], k, v [B / G, Lk, H], kmask [B / G, Lk] or None, scale, gate [H] (torch float32 tensors whose
    values are exactly representable in the storage type of `form`; scale and gate stay fp32: the kernels read masters).

    Queries lean towards the mean of their valid keys (q = noise + mean k), so that every row has positive scores and a
    mean square far above eps even with ONE key; masked keys are twice the mean query of their sentence: large positive
    scores, which only a mask that MULTIPLIES removes."""
    cs = CASES[name]
    st = V.STORAGE[form]
    B, G, nh, d, Lq, Lk = (cs[x] for x in ("B", "G", "nh", "d", "Lq", "Lk"))
    H, nB = nh * d, B // G
    g = torch.Generator().manual_seed(4200 + seed + sum(map(ord, name)))
    rnd = lambda *s: torch.randn(*s, generator=g)
    k, v = rnd(nB, Lk, H), rnd(nB, Lk, H)
    lengths = cs.get("lengths")
    kmask = None
    if lengths is not None:
        kmask = torch.zeros(nB, Lk)
        for b, n in enumerate(lengths):
            kmask[b, :n] = 1
    valid = torch.ones(nB, Lk) if kmask is None else kmask
    owner = torch.arange(B) // G
    scale = 1.0 + 0.2 * rnd(H)
    gate = 0.5 * rnd(H)
    if cs.get("special"):
        # orthogonal keys per head: key j of head h is e_j (x 4); q = sum_j t_j e_j gives the scores t_j / 2 exactly
        k = torch.zeros(nB, Lk, H)
        for h in range(nh):
            for j in range(Lk):
                k[:, j, h * d + j] = 4.0
        q = torch.zeros(B, Lq, H)
        for b in range(B):
            for h in range(nh):
                t = -(0.5 + torch.rand(Lk, generator=g))                       # every score negative ..
                if b >= 2:
                    t[(b + h) % Lk] = SPECIAL_SCORES[b - 2] * d ** 0.5 / 4.0   # .. but one: s = SPECIAL_SCORES[b - 2]
                q[b, 0, h * d:h * d + Lk] = t
        gate = torch.zeros(H)                       # sigmoid(0) = 1/2: the output is the normalised value vector / 2
    else:
        mean_k = (k * valid[..., None]).sum(1) / valid.sum(1, keepdim=True)          # [nB, H]
        q = rnd(B, Lq, H) + mean_k[owner][:, None, :]
        if cs.get("hot_masked"):
            for b in range(nB):
                mq = q[b * G:(b + 1) * G].mean((0, 1))
                k[b, valid[b] == 0] = 2.0 * mq
    rt_ = lambda t: t.to(st).float()
    return {"q": rt_(q), "k": rt_(k), "v": rt_(v), "kmask": kmask, "scale": scale, "gate": gate}


def case_reference(name, x, time=None, defect=None):
    cs = CASES[name]
    return rela_attention(x["q"].numpy(), x["k"].numpy(), x["v"].numpy(), cs["nh"], x["scale"].numpy(), x["gate"].numpy(),
                          kmask=None if x["kmask"] is None else x["kmask"].numpy(), kv_group=cs["G"],
                          nkeys=None if time is None else time + 1, defect=defect)


def case_runs(name):
    """The (time,) variants of a case: cached steps run once per device-resident position, the others once."""
    return [(t,) for t in CASES[name].get("times", (None,))]


# ---------------------------------------------------------------------------------------------- ref_torch model
def gated_rms_norm(x, P, scope, eps=EPS):
    """modules/rela.py:95-109; the fp32 masters of scale / gate whatever the storage model."""
    ms = (x ** 2).mean(-1, keepdim=True)
    return P[scope + "/scale"] * x * torch.rsqrt(ms + eps) * torch.sigmoid(P[scope + "/gate"] * x)


def dot_attention(query, memory, mem_mask, H, P, scope, nh, cache=None):
    """modules/rela.py:13-92 with ref_torch's storage sites: the projections (rt.linear) and the normalised output are
    stored, the weights and the context are not (the kernel keeps them in fp32)."""
    scope = scope + "/dot_attention"
    if memory is None:
        h = rt.linear(query, P, scope + "/qkv_map")
        q, k, v = torch.split(h, H, dim=-1)
        if cache is not None:                                   # rela.py:37-43
            k = torch.cat([cache["k"], k], dim=1)
            v = torch.cat([cache["v"], v], dim=1)
            cache = {"k": k, "v": v}
    else:
        q = rt.linear(query, P, scope + "/q_map")
        if cache is not None and ("mk" in cache and "mv" in cache):       # rela.py:46-54
            k, v = cache["mk"], cache["mv"]
        else:
            k = rt.linear(memory, P, scope + "/k_map")
            v = rt.linear(memory, P, scope + "/v_map")
        if cache is not None:
            cache["mk"], cache["mv"] = k, v
    q, k, v = rt.split_heads(q, nh), rt.split_heads(k, nh), rt.split_heads(v, nh)
    q = q * (H // nh) ** (-0.5)
    logits = torch.matmul(q, k.transpose(-1, -2))
    if mem_mask is not None:
        logits = logits * (mem_mask == 0).to(logits.dtype)      # rela.py:66-68
    weights = torch.relu(logits)
    o = rt.combine_heads(torch.matmul(weights, v))
    o = rt._st(gated_rms_norm(o, P, scope + "/post"), "attn_out")
    return {"weights": weights, "output": rt.linear(o, P, scope + "/o_map"), "cache": cache}


def encoder(source, hp, P):
    """models/transformer_rela.py:16-85 (ref_torch.encoder with the attention replaced)."""
    dt = P["bias"].dtype
    H = hp.hidden_size
    mask = (source != 0).to(dt)
    source, mask = rt.remove_invalid_seq(source, mask)
    x = rt._st_fwd(P[rt._emb_name(hp, "src")])[source] * (H ** 0.5) + P["bias"]
    x = rt._st(x + rt.timing_signal(x.shape[1], x.shape[2], dt), "embed")
    for l in range(hp.num_encoder_layer):
        pre = "encoder/layer_%d" % l
        y = dot_attention(x, None, rt.attention_bias(mask, "masking"), H, P, pre + "/self_attention", hp.num_heads)["output"]
        x = rt.layer_norm(rt.residual_fn(x, y), P, pre + "/self_attention")
        y = rt.ffn_layer(x, P, pre + "/feed_forward", None, False)
        x = rt.layer_norm(rt.residual_fn(x, y), P, pre + "/feed_forward")
    return {"encodes": x, "decoder_initializer": V.empty_caches(x.shape[0], H, hp.num_decoder_layer, dt), "mask": mask}


def _decoder_layers(x, state, hp, P, self_bias, caches):
    H, nh = hp.hidden_size, hp.num_heads
    for l in range(hp.num_decoder_layer):
        pre = "decoder/layer_%d" % l
        lc = None if caches is None else caches["layer_%d" % l]
        r = dot_attention(x, None, self_bias, H, P, pre + "/self_attention", nh, cache=lc)
        if lc is not None:
            lc.update(r["cache"])
        x = rt.layer_norm(rt.residual_fn(x, r["output"]), P, pre + "/self_attention")
        r = dot_attention(x, state["encodes"], rt.attention_bias(state["mask"], "masking"), H, P, pre + "/cross_attention",
                          nh, cache=lc)
        if lc is not None:
            lc.update(r["cache"])
        x = rt.layer_norm(rt.residual_fn(x, r["output"]), P, pre + "/cross_attention")
        y = rt.ffn_layer(x, P, pre + "/feed_forward", None, False)
        x = rt.layer_norm(rt.residual_fn(x, y), P, pre + "/feed_forward")
    return torch.matmul(x.reshape(-1, hp.embed_size), rt._st_fwd(P[rt._emb_name(hp, "softmax")]).t())


def decoding_fns(hp, P):
    """(encoding_fn, decoding_fn) of models/transformer_rela.py:252-285 (search_mode = cache) for rt.beam_search."""
    hp = rt.closing_dropout(copy.copy(hp))

    def encoding_fn(source):
        return V.cached_state(encoder(source, hp, P))

    def decoding_fn(target, state, time):
        x = V.embed_step(target, time, hp, P)
        # transformer_rela.py:131-140: the causal bias of ONE query position, [1, 1, 1, 1] of zeros -> every cached key counts
        logits = _decoder_layers(x, state, hp, P, rt.attention_bias(1, "causal").to(P["bias"].dtype), state["decoder"]["state"])
        return logits, state

    return encoding_fn, decoding_fn


def full_decoder(target, state, hp, P):
    """The training-path decoder (models/transformer_rela.py:88-181): shifted inputs, the [L, L] causal bias MULTIPLIED into
    the scores as a 0/1 mask.  target [B, Lt] without padding -> logits [B, Lt, V]."""
    x = V.embed_shifted(target, hp, P)
    logits = _decoder_layers(x, state, hp, P, rt.attention_bias(target.shape[1], "causal").to(P["bias"].dtype), None)
    return logits.reshape(target.shape[0], target.shape[1], -1)


POST = ("encoder/layer_%d/self_attention", "decoder/layer_%d/self_attention", "decoder/layer_%d/cross_attention")


def init_params(hp, seed):
    """rt.init_params(hp, "transformer") + perturbed biases and LayerNorm parameters + the post vectors of every attention
    scope: scale perturbed around 1, gate drawn from the scope initialiser (modules/rela.py:103-104; the layer initialiser
    under deep_transformer_init), as zero_amd.variables.initial_values draws it."""
    from tests.common import perturb
    rng = np.random.default_rng(seed)
    Pn = perturb(rt.init_params(hp, "transformer", seed=seed + 1), rng)
    H = hp.hidden_size
    for pat in POST:
        n = hp.num_encoder_layer if pat.startswith("encoder") else hp.num_decoder_layer
        for l in range(n):
            p = pat % l + "/dot_attention/post/"
            Pn[p + "scale"] = (1 + rng.normal(0, 0.1, H)).astype(np.float32)
            if hp.deep_transformer_init:
                g = rt._scope_init(rng, (H,), "uniform_unit_scaling", hp.initializer_gain * (l + 1) ** -0.5)
            else:
                g = rt._scope_init(rng, (H,), hp.initializer, hp.initializer_gain)
            Pn[p + "gate"] = np.asarray(g, np.float32)
    return Pn


def make_fixture(hp, src, seed, factor=4.0):
    """The tiny model of the GPU model tests, with the proof that the REFERENCE ALONE is far from its discontinuity on it.
    ReLA has one softmax lacks: a row whose only positive score is barely positive is normalised up to O(1) by the
    RMSNorm, so a rounding that flips that score's sign changes the row by O(1).  Measured on the CPU, for beam 1 and 4
    (variant_ref.candidate_margin): the float64 and the fp32 run of the restated reference give identical hypotheses and
    candidate orders, and the smallest gap between a kept candidate and its runner-up exceeds factor x the largest fp32 -
    float64 score difference.
    -> dict Pn, gap, err (the worst over both beams)."""
    Pn = init_params(hp, seed)
    return dict(V.candidate_margin(functools.partial(V.search, decoding_fns), hp, Pn, src, factor=factor, seed=seed), Pn=Pn)
