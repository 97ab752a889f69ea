"""References of the word-alignment option (hp.alignment_file): the kernel zk_align_probs / zk_f32_align_probs
(zero_amd/csrc/zk_align.hip) and the teacher-forced pass of zero_amd/models/_align.py (a plain module, no pytest in it).

THE RULE (stated here once).  For a sentence b, a decoder row t and a source position j

    P[b, t, j] = (1 / nh) * sum_h softmax_j(scale * q[b, t, h] . k[b, j, h] + (1 - kmask[b, j]) * -inf_const)

with the heads summed in ascending order.  Row t is the decoder row that PREDICTS target token t: its input is token t - 1,
the shifted target of the training path (transformer.py:108-112).  q and k are the chosen layer's q_map and k_map products
of the storage type, exactly as the model's own cross-attention consumes them; scale (d^-0.5) and inf_const (dtype_inf,
1e8) are the layer's.  A masked key has probability exactly 0 (exp(-1e8 - ..) underflows in float64 as it does in float32,
whenever the row has a valid key).  The hard alignment is a[b, t] = argmax_j P[b, t, j] over the ELIGIBLE positions, those
with amask[b, j] != 0; amask defaults to kmask; the lowest j wins on equal values; a row without an eligible position gives
-1.  The host clears the source's EOS position in amask (source lines carry an EOS, vocab.to_id), cuts the rows at the
hypothesis length and drops the hypothesis' own EOS row (zero_amd/align.py).

``align_probs`` / ``hard_align``   the rule in numpy float64.
``align_terms``     the rule with the pieces ``align_bound`` needs; ``defect=`` plants ONE defect (``DEFECTS``).
``align_bound``     the element-wise bound of a kernel whose softmax arithmetic is fp32 (derivation in its docstring).
``align_standin``   what a correct kernel computes: torch float32, another summation order.
``accept_best``     the arg-max acceptance rule of the kernel tests.
``CASES``           the case table of tests/test_gpu_align_kernels.py; ``DEFECTS`` maps a defect to the case named for it.
``model_*``         the model restated on oracle.ref_torch: teacher-forced, shifted input, weights of the chosen layer.

Measured on the CPU by tests/test_align_checker.py (python -m pytest tests/test_align_checker.py -s prints them) and asserted
there not to exceed these figures:
    F32_MODEL_FLOOR    the largest |P32 - P64| of the float32 restatement of the model pass over the MODEL_CASES and both
                       layers: 6.47e-07 measured; the fp32 pass on the GPU is held to 4 x F32_MODEL_FLOOR = 2.6e-06
    BF16_MODEL_FLOOR   the largest |Pbf - P64| of the bf16-storage restatement (oracle.ref_torch Cfg.store_bf16):
                       8.82e-03 measured; a row is DECISIVE when its best-to-second gap exceeds 4 x BF16_MODEL_FLOOR = 0.036,
                       and at most 18 % of the reference's rows are not (cap: 25 %)
"""
import numpy as np
import torch

from tests import parity as PR

U = PR.PER_TERM                  # 2^-23 per accumulated term
MASK_INF = 1e8                   # utils/dtype.py:12-15
BLOCK_ROWS = 16                  # decoder rows per workgroup (ALN_BR)
KEY_TILE = {"bf16": 16, "fp32": 64}      # keys per tile of the wave-strided score loop
MAX_LK = 1024                    # zk_align_max_lk()
EXP_ULP = 2.0                    # expf: the larger of the documented figures (CUDA 2 ulp, HIP 1 ulp); counted TWICE below
FORMS = ("bf16", "fp32")

F32_MODEL_FLOOR = 6.6e-07       # measured 6.47e-07 (transformer, layer -1)
BF16_MODEL_FLOOR = 9.0e-03      # measured 8.82e-03


# ---------------------------------------------------------------------------------------------- the rule
def _heads(x, nh):
    B, L, H = x.shape
    return x.reshape(B, L, nh, H // nh).transpose(0, 2, 1, 3)


def align_terms(q, k, kmask, nh, scale=None, inf_const=MASK_INF, defect=None, amask=None):
    """q [B, Lq, H], k [B, Lk, H], kmask [B, Lk] or None (float64-convertible) -> dict P [B, Lq, Lk], p [B, nh, Lq, Lk],
    s (scores with the mask term), S (their magnitude sum_c |q_c| |k_c| scale + |mask term|), best [B, Lq].

    defect (one at a time, each something a kernel could do):
      neighbour_keys     the keys of sentence b + 1              neighbour_mask    the mask row of sentence b + 1
      mask_ignored       no mask term                            amask_ignored     eligibility from kmask
      mask_stride_lk     the mask row of sentence b read at b * Lk of the [B, ldmask] buffer (ldmask = Lk + 3 in the tests)
      scale_after_mask   scale * (q . k + mask term)             head_dropped      the last head missing from the sum
      div_nh_minus_1     the sum divided by nh - 1               tie_later         equal values: the LATER index
      key_tile_skipped   the row sum misses the last tile of 16 keys (rows keep their maximum)
      row16_next         decoder row 16 of a sentence reads the query of sentence b + 1
      argmax_per_head    the arg-max of max_h p_h instead of the head average"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    B, Lq, H = q.shape
    Lk = k.shape[1]
    d = H // nh
    scale = d ** -0.5 if scale is None else scale
    km = np.ones((B, Lk)) if kmask is None else np.asarray(kmask, np.float64)
    am = km if amask is None or defect == "amask_ignored" else np.asarray(amask, np.float64)
    nxt = (np.arange(B) + 1) % B
    if defect == "neighbour_keys":
        k = k[nxt]
    if defect == "neighbour_mask":
        km = km[nxt]
    if defect == "mask_stride_lk":
        flat = np.zeros((B, Lk + 3))
        flat[:, :Lk] = km
        flat = flat.reshape(-1)
        km = np.stack([flat[b * Lk:b * Lk + Lk] for b in range(B)])
    if defect == "mask_ignored":
        km = np.ones((B, Lk))
    if defect == "row16_next" and Lq > 16:
        q = q.copy()
        q[:, 16] = q[nxt, 16]
    qh, kh = _heads(q, nh), _heads(k, nh)
    dot = qh @ kh.transpose(0, 1, 3, 2)
    mterm = ((1.0 - km) * -inf_const)[:, None, None, :]
    s = (dot + mterm) * scale if defect == "scale_after_mask" else dot * scale + mterm
    S = (np.abs(qh) @ np.abs(kh).transpose(0, 1, 3, 2)) * scale + np.abs(mterm)
    mx = s.max(-1, keepdims=True)
    e = np.exp(s - mx)
    el = e
    if defect == "key_tile_skipped" and Lk > 16:
        el = e[..., :(Lk - 1) // 16 * 16]
    p = e / el.sum(-1, keepdims=True)
    P = np.zeros((B, Lq, Lk))
    for h in range(nh - 1 if defect == "head_dropped" else nh):     # heads ascending
        P = P + p[:, h]
    P = P / ((nh - 1) if defect == "div_nh_minus_1" else nh)
    score = p.max(1) if defect == "argmax_per_head" else P
    return {"P": P, "p": p, "s": s, "S": S, "mx": mx, "best": hard_align(score, am, later=defect == "tie_later"),
            "nh": nh, "d": d, "amask": am}


def align_probs(q, k, kmask, nh, scale=None, inf_const=MASK_INF):
    return align_terms(q, k, kmask, nh, scale, inf_const)["P"]


def hard_align(P, amask, later=False):
    """argmax over the eligible positions, the lowest index on equal values (later: the highest), -1 without any."""
    P = np.asarray(P, np.float64)
    el = np.broadcast_to((np.asarray(amask) != 0)[:, None, :], P.shape)
    v = np.where(el, P, -np.inf)
    if later:
        best = P.shape[-1] - 1 - np.argmax(v[..., ::-1], -1)
    else:
        best = np.argmax(v, -1)
    return np.where(el.any(-1), best, -1).astype(np.int32)


def align_bound(ref, form):
    """Element-wise bound [B, Lq, Lk] of zk_align_probs (form "bf16") / zk_f32_align_probs ("fp32") against align_terms(...)
    = ref, for operands that are exact in the storage type.  PER_TERM u = 2^-23 per accumulated term (tests/parity.py), first
    order, term by term:

      score    s_j = scale (q . k_j) + mask term: d accumulated products (bf16 operands: exact products, fp32 accumulation in
               the matrix core; fp32: d fused multiply-adds), the product with scale and the mask addition -- d + 2 terms:
                                                   |ds_j| <= (d + 2) u S_j,   S_j = scale sum_c |q_c| |k_jc| + |mask term_j|
      max      the subtraction s_j - max rounds once: u |s_j - max|; the maximum itself is off by at most max_k |ds_k|
      expf     counted at TWICE its documented ulp error (2 ulp): 2 EXP_ULP u; the argument's error passes through:
                                                   rel(e_j) <= eps_j = |ds_j| + max_k |ds_k| + (|s_j - max| + 2 EXP_ULP) u
      sum      l = sum_k e_k over Lk keys in any order, Lk + 2 terms:    rel(l) <= sum_k p_k eps_k + (Lk + 2) u
      divide   p_j = e_j / l, one rounding:        rel(p_j) <= rho_j = eps_j + sum_k p_k eps_k + (Lk + 3) u
      average  P_j = (sum_h p_hj) / nh: nh - 1 additions and the division, nh + 1 terms:
                                                   |dP_j| <= (1 / nh) sum_h p_hj rho_hj + (nh + 1) u P_j
    The operands are exact in the storage type and every product is formed from them: there is NO 2^-8 term, in either form
    (a kernel that rounds a score, an exponential or a probability to bf16 misses this bound by orders of magnitude).  A key
    with p = 0 (masked under inf_const = 1e8) has the bound 0: it must be exactly 0.  No constant is fitted to the kernel."""
    assert form in FORMS, form
    p, s, S, mx, nh, d = ref["p"], ref["s"], ref["S"], ref["mx"], ref["nh"], ref["d"]
    Lk = p.shape[-1]
    live = p > 0
    ds = (d + 2) * U * S
    ds_max = np.max(np.where(live, ds, 0.0), -1, keepdims=True)
    eps = np.where(live, ds + ds_max + (np.abs(s - mx) + 2 * EXP_ULP) * U, 0.0)
    rho = eps + (p * eps).sum(-1, keepdims=True) + (Lk + 3) * U
    return (p * rho).sum(1) / nh + (nh + 1) * U * ref["P"]


def align_standin(q, k, kmask, nh, form, scale=None, inf_const=MASK_INF, amask=None, defect=None):
    """What a correct kernel computes, on the CPU: torch float32 through matrix products with the channels and the keys in
    DESCENDING order and the heads summed in DESCENDING order (the reference sums ascending in float64), torch.softmax.
    defect: the stand-in of a defective kernel -- the float64 statement of the defect rounded to float32.
    -> (P float64 [B, Lq, Lk], best int32 [B, Lq])."""
    assert form in FORMS, form
    if defect is not None:
        r = align_terms(q, k, kmask, nh, scale, inf_const, defect=defect, amask=amask)
        return r["P"].astype(np.float32).astype(np.float64), r["best"]
    f = lambda t: torch.as_tensor(np.asarray(t, np.float64)).float()
    q, k = f(q), f(k)
    B, Lq, H = q.shape
    Lk = k.shape[1]
    d = H // nh
    scale = d ** -0.5 if scale is None else scale
    km = torch.ones(B, Lk) if kmask is None else f(kmask)
    rc, rk = torch.arange(d - 1, -1, -1), torch.arange(Lk - 1, -1, -1)
    qh = q.view(B, Lq, nh, d).permute(0, 2, 1, 3)[..., rc]
    kh = k.view(B, Lk, nh, d).permute(0, 2, 1, 3)[..., rc][:, :, rk]
    s = (qh @ kh.transpose(-1, -2)) * torch.tensor(scale, dtype=torch.float32)
    s = s + ((1.0 - km[:, rk]) * torch.tensor(-inf_const, dtype=torch.float32))[:, None, None, :]
    p = torch.softmax(s, -1)
    P = torch.zeros(B, Lq, Lk)
    for h in range(nh - 1, -1, -1):
        P = P + p[:, h]
    P = (P / float(nh))[..., rk].double().numpy()          # (rk is its own inverse)
    am = km.numpy() if amask is None else np.asarray(amask)
    return P, hard_align(P, am)


def accept_best(best, P_ref, bound, amask):
    """The arg-max acceptance rule: every returned index is eligible and P_ref[j] + bound[j] >= max_eligible (P_ref - bound)
    -- it can be the arg-max of SOME result inside the bound; a row without eligible positions must return -1.  No row is
    skipped.  -> list of (b, t, got, why) violations."""
    bad = []
    el = np.asarray(amask) != 0
    B, Lq, _ = P_ref.shape
    for b in range(B):
        for t in range(Lq):
            j = int(best[b, t])
            if not el[b].any():
                if j != -1:
                    bad.append((b, t, j, "no eligible position: -1 expected"))
                continue
            if j < 0 or j >= el.shape[1] or not el[b, j]:
                bad.append((b, t, j, "not eligible"))
                continue
            low = np.max(np.where(el[b], P_ref[b, t] - bound[b, t], -np.inf))
            if P_ref[b, t, j] + bound[b, t, j] < low:
                bad.append((b, t, j, "P_ref %.9g + bound %.3g < %.9g" % (P_ref[b, t, j], bound[b, t, j], low)))
    return bad


# ---------------------------------------------------------------------------------------------- kernel cases
# d = (bf16 form, fp32 form).  lengths: valid keys per sentence (kmask; None = no mask); hole: (sentence, position) masked
# inside the valid part; amask: None | "last" (the last valid position cleared -- the host's EOS) | "zero" (nothing eligible);
# tie: (sentence, j1, j2) two bit-identical maximal key rows; inf: the mask_inf argument.
# Lq in {1, 15, 16, 17, 33}; Lk in {1, 15, 16, 17, 63, 64, 65, 130} (65 / 130: second / third trip of the wave-strided key
# loop of the bf16 form, 4 tiles of 16 per trip) and MAX_LK; nh in {1, 2, 8}; B in {1, 3}.
CASES = {
    "q1_k1": dict(B=1, nh=1, Lq=1, Lk=1, d=(32, 4)),
    "q15_k15_ragged": dict(B=3, nh=2, Lq=15, Lk=15, d=(64, 20), lengths=(15, 7, 1), amask="last"),
    "q16_k16_h8": dict(B=1, nh=8, Lq=16, Lk=16, d=(32, 4), lengths=(13,)),
    "q17_k17_hole": dict(B=3, nh=2, Lq=17, Lk=17, d=(128, 128), lengths=(17, 9, 12), hole=(0, 5)),
    "q33_k63": dict(B=1, nh=2, Lq=33, Lk=63, d=(64, 64)),
    "q16_k64_last": dict(B=3, nh=1, Lq=16, Lk=64, d=(32, 20), lengths=(64, 33, 2), amask="last"),
    "q17_k65": dict(B=3, nh=2, Lq=17, Lk=65, d=(64, 64), lengths=(65, 40, 64), amask="last"),
    "q33_k130_h8": dict(B=3, nh=8, Lq=33, Lk=130, d=(32, 4), lengths=(130, 70, 129), hole=(2, 64)),
    "q1_k130_zero": dict(B=1, nh=2, Lq=1, Lk=130, d=(96, 64), lengths=(101,), amask="zero"),
    "limit": dict(B=1, nh=1, Lq=1, Lk=MAX_LK, d=(32, 4), lengths=(MAX_LK - 5,)),
    "ties": dict(B=3, nh=2, Lq=17, Lk=33, d=(32, 20), lengths=(33, 33, 20), tie=(4, 19)),
    "small_inf": dict(B=3, nh=2, Lq=5, Lk=17, d=(32, 20), lengths=(17, 9, 12), inf=3.0),
}
LD_EXTRA_MASK, LD_EXTRA_PROBS = 3, 5          # ldmask = Lk + 3, ldp = Lk + 5

DEFECTS = {          # defect -> the case named for it
    "neighbour_keys": "q17_k65",
    "neighbour_mask": "q15_k15_ragged",
    "mask_ignored": "q17_k17_hole",
    "amask_ignored": "q16_k64_last",
    "mask_stride_lk": "q33_k130_h8",
    "scale_after_mask": "small_inf",
    "head_dropped": "q16_k16_h8",
    "div_nh_minus_1": "q16_k16_h8",
    "tie_later": "ties",
    "key_tile_skipped": "q33_k63",
    "row16_next": "q17_k65",
    "argmax_per_head": "q33_k130_h8",
}


def bf16_exact(x):
    return torch.as_tensor(x).to(torch.bfloat16).to(torch.float32)


def case_inputs(name, form, seed=0):
    """-> dict q [B, Lq, H], k [B, Lk, H] float32 CPU tensors exact in the form's storage type, kmask / amask [B, Lk] float32
    or None, nh, d, inf.  Queries and keys have unit scale times 1.5: the rows are peaked enough for decisive maxima."""
    cs = CASES[name]
    B, nh, Lq, Lk = cs["B"], cs["nh"], cs["Lq"], cs["Lk"]
    d = cs["d"][FORMS.index(form)]
    H = nh * d
    g = torch.Generator().manual_seed(9100 + seed + sum(map(ord, name)))
    q, k = 1.5 * torch.randn(B, Lq, H, generator=g), 1.5 * torch.randn(B, Lk, H, generator=g)
    if cs.get("tie"):
        j1, j2 = cs["tie"]
        v = torch.sign(torch.randn(H, generator=g))
        q = q.abs() * v                           # q . v = sum |q| for every row: the key 2 v scores highest
        k[:, j1] = 2.0 * v
        k[:, j2] = 2.0 * v
    if form == "bf16":
        q, k = bf16_exact(q), bf16_exact(k)
    km = am = None
    if cs.get("lengths") is not None:
        km = torch.zeros(B, Lk)
        for b, n in enumerate(cs["lengths"]):
            km[b, :n] = 1
        if cs.get("hole"):
            km[cs["hole"][0], cs["hole"][1]] = 0
    if cs.get("amask") == "last":
        am = km.clone()
        for b, n in enumerate(cs["lengths"]):
            am[b, n - 1] = 0
    elif cs.get("amask") == "zero":
        am = torch.zeros(B, Lk)
    return {"q": q, "k": k, "kmask": km, "amask": am, "nh": nh, "d": d, "inf": cs.get("inf", MASK_INF)}


def case_reference(x, defect=None):
    return align_terms(x["q"].numpy(), x["k"].numpy(), None if x["kmask"] is None else x["kmask"].numpy(), x["nh"],
                       inf_const=x["inf"], defect=defect, amask=None if x["amask"] is None else x["amask"].numpy())


def worst_ratio(got, ref, bound):
    """largest |got - ref| / bound (0 / 0 counts as 0, a non-finite element or an excess over a zero bound as inf)."""
    got, ref, bound = (np.asarray(t, np.float64) for t in (got, ref, bound))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    return float(np.where(np.isfinite(got), ratio, np.inf).max())


# ---------------------------------------------------------------------------------------------- the model pass
MODEL_CASES = ("transformer", "transformer_aan", "transformer_fuse")
MODEL_LAYERS = (-1, 0)
SOURCE_LENGTHS = (14, 5, 9, 11)          # tokens including the EOS
TARGET_LENGTHS = (12, 4, 7, 9)
MODEL_SEED = 24          # chosen among 21 .. 24 x Q_FACTOR 1, 3, 6, 10 on the CPU: the fewest non-decisive reference rows (18 %)
# random tiny weights attend almost uniformly: the decoder layers' q_map (weights and bias) times this factor makes the rows
# peaked enough that the float64 reference alone has at most DECISIVE_CAP non-decisive rows (tests/test_align_checker.py)
Q_FACTOR = 3.0
DECISIVE_CAP = 0.25


def model_fixture(model, seed=MODEL_SEED):
    """-> (hp, Pn, src, tgt): the tiny model of tests.common.make_hp (H = 128, 2 heads, vocabularies 120 / 104) with
    perturbed biases / LayerNorm parameters and sharpened cross-attention queries; padded sources and targets."""
    from oracle import ref_torch as rt
    from tests import variant_ref as V
    from tests.common import make_hp, perturb
    hp = make_hp(model, scope_name="t_align_" + model)
    Pn = perturb(rt.init_params(hp, model, seed=seed + 1), np.random.default_rng(seed))
    cross = "fuse_attention" if model == "transformer_fuse" else "cross_attention"
    for l in range(hp.num_decoder_layer):
        for v in ("W_0_0", "b_0"):
            name = "decoder/layer_%d/%s/dot_attention/q_map/%s" % (l, cross, v)
            Pn[name] = (Pn[name] * Q_FACTOR).astype(np.float32)
    src = V.ragged(SOURCE_LENGTHS, hp.src_vocab.size(), 5)
    tgt = V.ragged(TARGET_LENGTHS, hp.tgt_vocab.size(), 6)
    return hp, Pn, src, tgt


def model_probs(hp, Pn, model, src, tgt, layer, dtype=torch.float64, store_bf16=False):
    """The model restated on oracle.ref_torch: the teacher-forced training-path forward (rt.score_fn: shifted input, row t
    predicts target token t), the weights of the chosen decoder layer's cross-attention captured from rt.dot_attention from
    outside, averaged over the heads -> float64 [B, Lt, Ls]."""
    from oracle import ref_torch as rt
    cross = "fuse_attention" if model == "transformer_fuse" else "cross_attention"
    want = "decoder/layer_%d/%s" % (layer % hp.num_decoder_layer, cross)
    seen = []
    inner = rt.dot_attention

    def spy(query, memory, mem_mask, H, P, scope, *a, **kw):
        r = inner(query, memory, mem_mask, H, P, scope, *a, **kw)
        if scope == want:
            seen.append(r["weights"].detach().double())
        return r
    old = rt.Cfg.store_bf16
    rt.dot_attention, rt.Cfg.store_bf16 = spy, bool(store_bf16)
    try:
        rt.score_fn({"source": torch.as_tensor(src), "target": torch.as_tensor(tgt)}, hp, rt.to_torch(Pn, dtype=dtype), model)
    finally:
        rt.dot_attention, rt.Cfg.store_bf16 = inner, old
    assert len(seen) == 1, (want, len(seen))
    w = seen[0].numpy()
    P = np.zeros(w[:, 0].shape)
    for h in range(w.shape[1]):
        P = P + w[:, h]
    return P / w.shape[1]


def eligible(src, eos=2):
    """the host's amask: the source's tokens without its EOS (zero_amd.models._align.eligible_mask restated)"""
    src = np.asarray(src)
    am = (src != 0).astype(np.float64)
    for b in range(src.shape[0]):
        n = int((src[b] != 0).sum())
        if n and src[b, n - 1] == eos:
            am[b, n - 1] = 0
    return am


def row_gaps(P, amask):
    """best-to-second gap among the eligible positions of every row [B, Lt] (inf with a single eligible position)"""
    v = np.where((np.asarray(amask) != 0)[:, None, :], P, -np.inf)
    top = -np.sort(-v, -1)
    return top[..., 0] - (top[..., 1] if v.shape[-1] > 1 else -np.inf)


def live_rows(tgt):
    """[B, Lt] bool: the rows the host keeps -- the hypothesis' words, without its EOS row and the padding"""
    tgt = np.asarray(tgt)
    n = (tgt != 0).sum(1)
    return np.arange(tgt.shape[1])[None, :] < (n - 1)[:, None]
