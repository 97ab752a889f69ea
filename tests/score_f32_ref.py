"""References of the fp32 scorer's full-sequence kernels (a plain module, no pytest in it): zk_f32_attn_seq, zk_f32_cumavg,
zk_f32_embed_shift (zero_amd/csrc/zk_f32_seq.hip) and the fixtures / floors of tests/test_gpu_score_f32_model.py.

``attn_reference``   float64 reference of the attention: ``parity.attn_math`` (func.py:218-256 with causal, kmask, relative
                     positions and clipping) fed so that it also covers q_pos0 and the fp32 behaviour of a fully masked row.
``attn_f64``         the same arithmetic restated in numpy with everything ``attn_bound`` needs; ``defect=`` plants ONE defect.
``attn_bound``       the element-wise bound of an all-fp32 kernel (derivation in its docstring).
``attn_standin``     what a correct kernel computes, in torch float32 with the keys in DESCENDING order.
``cumavg_*`` / ``embed_*``   the same four for the cumulative average (on oracle.ref_torch) and the shifted embedding.
``ATTN_CASES`` ...   the case tables of tests/test_gpu_score_f32_kernels.py.
``model_fixture`` / ``identity_fixture``, ``ORACLE_FLOOR`` / ``IDENTITY_FLOOR``   the model tests' inputs and the measured
                     floors of the oracle itself (tests/test_score_f32_checker.py re-measures them).
"""
import copy
import types

import numpy as np
import torch

from oracle import ref_torch as rt
from tests import parity as PR
from tests import variant_ref as V

U = PR.PER_TERM                  # 2^-23: twice the unit roundoff of fp32, per accumulated term
TILE_ROWS, TILE_KEYS = 32, 64    # zk_f32_attn_seq: query rows per workgroup (SEQ_BR), keys per staged tile (SEQ_TK)
MASK_INF = 1e8                   # utils/dtype.py:12-15

ATTN_DEFECTS = ("causal_plus_one", "causal_minus_one", "neighbour_sentence", "rpr_sign", "clip_m_minus_1", "q_pos0_ignored",
                "dropped_key_tile", "mask_multiplied")
EMBED_DEFECTS = ("shift_missing", "shift_two")
CUMAVG_DEFECTS = ("divided_by_L",)

# name -> one direct call.  lengths: valid keys per sentence (kmask), None = no mask.  slices: q / k / v are column slices of
# one [T, 3H] matrix.  The row block is 32 and the key tile 64 (TILE_ROWS, TILE_KEYS), so besides the issue's shapes there is
# one length on each side of 32 and of 64, causal (Lq = Lk) and not.
ATTN_CASES = {
    "causal_L1": dict(B=2, nh=2, d=64, Lq=1, Lk=1, causal=True),
    "causal_L65": dict(B=2, nh=2, d=64, Lq=65, Lk=65, causal=True, slices=True),
    "causal_L130": dict(B=1, nh=2, d=64, Lq=130, Lk=130, causal=True),
    "causal_L31": dict(B=1, nh=2, d=64, Lq=31, Lk=31, causal=True),
    "causal_L33": dict(B=1, nh=2, d=64, Lq=33, Lk=33, causal=True),
    "causal_L63": dict(B=1, nh=2, d=64, Lq=63, Lk=63, causal=True),
    "ragged": dict(B=3, nh=2, d=64, Lq=37, Lk=53, lengths=(53, 1, 20)),
    "keys_63": dict(B=1, nh=2, d=64, Lq=33, Lk=63),
    "keys_65": dict(B=1, nh=2, d=64, Lq=31, Lk=65, lengths=(65,)),
    "keys_130": dict(B=2, nh=2, d=64, Lq=5, Lk=130, lengths=(130, 70)),
    "fully_masked": dict(B=2, nh=2, d=64, Lq=5, Lk=7, lengths=(7, 0)),
    "rpr_causal": dict(B=2, nh=2, d=64, Lq=20, Lk=20, causal=True, rpr=4),
    "rpr_cross": dict(B=2, nh=2, d=64, Lq=9, Lk=13, rpr=4, q_pos0=3, lengths=(13, 6)),
    "d8": dict(B=2, nh=2, d=8, Lq=9, Lk=9, causal=True),
    # the other forms of the kernel: a head size that is no multiple of 8 (key rows unpadded in LDS), and two channels per
    # lane (64 < d <= 128) without and with relative positions
    "d12": dict(B=2, nh=2, d=12, Lq=9, Lk=13, lengths=(13, 5)),
    "d128": dict(B=1, nh=2, d=128, Lq=33, Lk=70, lengths=(66,)),
    "d128_rpr": dict(B=2, nh=2, d=128, Lq=40, Lk=40, causal=True, rpr=4),
}
HOT_VALUE = 50.0


def attn_inputs(name, seed=0):
    """-> dict of float32 CPU tensors q [B*Lq, H], k, v [B*Lk, H], kmask [B, Lk] or None, rk, rv [2m+1, d] or None.
    Causal cases: the LAST key of every sentence is twice the mean query of that sentence (the highest score for every
    query, as rela_ref's hot_masked keys) and its value row is HOT_VALUE everywhere: a query that sees it by an off-by-one
    is wrong by O(HOT_VALUE), not by a rounding."""
    cs = ATTN_CASES[name]
    B, nh, d, Lq, Lk = (cs[x] for x in ("B", "nh", "d", "Lq", "Lk"))
    H = nh * d
    g = torch.Generator().manual_seed(7100 + seed + sum(map(ord, name)))
    rnd = lambda *s: torch.randn(*s, generator=g)
    q, k, v = rnd(B, Lq, H), rnd(B, Lk, H), rnd(B, Lk, H)
    if cs.get("causal"):
        mq = q.mean(1)
        k[:, -1] = 2.0 * mq + 0.5 * torch.sign(mq)          # (+ a margin: the score is positive and the largest)
        v[:, -1] = HOT_VALUE
    x = {"q": q.reshape(B * Lq, H), "k": k.reshape(B * Lk, H), "v": v.reshape(B * Lk, H), "kmask": None, "rk": None, "rv": None}
    if cs.get("lengths") is not None:
        km = torch.zeros(B, Lk)
        for b, n in enumerate(cs["lengths"]):
            km[b, :n] = 1
        x["kmask"] = km
    if cs.get("rpr"):
        x["rk"], x["rv"] = 0.3 * rnd(2 * cs["rpr"] + 1, d), 0.3 * rnd(2 * cs["rpr"] + 1, d)
    return x


def _full_rows(cs, x):
    """Sentences whose keys are ALL masked."""
    if x["kmask"] is None:
        return np.zeros(cs["B"], bool)
    return (x["kmask"].numpy() == 0).all(1)


def attn_reference(name, x):
    """float64 [B*Lq, H] through parity.attn_math.  Two things attn_math does not state are brought to it:
      q_pos0   the query rows sit at positions q_pos0 + i: q_pos0 zero rows are put in front of every sentence's queries and
               cut off the result (attn_math indexes the relative-position tables by row number);
      a fully masked sentence   in fp32, s + (1 - m) * -1e8 is -1e8 for EVERY key (|s| < 4 = half an ulp of 1e8; asserted),
               so the softmax is uniform (func.py:372-387 in the reference's float32); in float64 the scores would
               survive.  The queries of such a sentence are zeroed: all scores equal, softmax uniform."""
    cs = ATTN_CASES[name]
    B, nh, d, Lq, Lk = (cs[x_] for x_ in ("B", "nh", "d", "Lq", "Lk"))
    H, p0 = nh * d, cs.get("q_pos0", 0)
    q = x["q"].double().view(B, Lq, H).clone()
    full = _full_rows(cs, x)
    if full.any():
        assert float(attn_f64(name, x)["s"][full].__abs__().max()) < 4.0
        q[torch.as_tensor(full)] = 0
    q = torch.cat([torch.zeros(B, p0, H, dtype=torch.float64), q], 1).reshape(B * (p0 + Lq), H)
    r = PR.attn_math(q, x["k"], x["v"], torch.zeros(B * (p0 + Lq), H), B, nh, p0 + Lq, Lk, d, kmask=x["kmask"],
                     causal=bool(cs.get("causal")), rk=x["rk"], rv=x["rv"], max_rel=cs.get("rpr", 0))
    return r["out"].view(B, p0 + Lq, H)[:, p0:].reshape(B * Lq, H)


def attn_f64(name, x, defect=None):
    """The arithmetic of zk_f32_attn_seq in numpy float64 -> dict out [B*Lq, H] and, for attn_bound: s (scores without the
    mask term) and s_abs [B, nh, Lq, Lk], p, v_h, and the relative-position pieces.

    defect (one at a time; each is something a kernel could do):
      causal_plus_one      keys j <= i + 1 take part           causal_minus_one   keys j < i (row 0 sees nothing: zeros)
      neighbour_sentence   keys, values and mask of sentence b + 1
      rpr_sign             tables indexed by clip(j - i)       clip_m_minus_1     clipped at max_rel - 1
      q_pos0_ignored       query positions start at 0
      dropped_key_tile     the last tile of TILE_KEYS keys is never visited (cases with more than one tile)
      mask_multiplied      the probabilities are multiplied by the mask instead of the bias being added to the scores: a
                           fully masked row has nothing left (zeros) instead of the uniform average"""
    cs = ATTN_CASES[name]
    B, nh, d, Lq, Lk = (cs[x_] for x_ in ("B", "nh", "d", "Lq", "Lk"))
    H, m, p0 = nh * d, cs.get("rpr", 0), cs.get("q_pos0", 0)
    f = lambda t: t.double().numpy()
    own = np.arange(B)
    if defect == "neighbour_sentence":
        own = (own + 1) % B
    qh = f(x["q"]).reshape(B, Lq, nh, d).transpose(0, 2, 1, 3) * d ** -0.5
    kh = f(x["k"]).reshape(B, Lk, nh, d).transpose(0, 2, 1, 3)[own]
    vh = f(x["v"]).reshape(B, Lk, nh, d).transpose(0, 2, 1, 3)[own]
    s = qh @ kh.transpose(0, 1, 3, 2)
    s_abs = np.abs(qh) @ np.abs(kh).transpose(0, 1, 3, 2)
    i = np.arange(Lq)[:, None] + (0 if defect == "q_pos0_ignored" else p0)
    j = np.arange(Lk)[None, :]
    idx = None
    if m:
        mm = m - 1 if defect == "clip_m_minus_1" else m
        rel = (j - i) if defect == "rpr_sign" else (i - j)
        idx = np.clip(rel, -mm, mm) + m
        rk, rv = f(x["rk"]), f(x["rv"])
        s = s + np.einsum("bhqd,qkd->bhqk", qh, rk[idx])
        s_abs = s_abs + np.einsum("bhqd,qkd->bhqk", np.abs(qh), np.abs(rk[idx]))
    live = np.ones((B, 1, Lq, Lk), bool)
    if cs.get("causal"):
        off = {"causal_plus_one": 1, "causal_minus_one": -1}.get(defect, 0)
        live = live & (np.arange(Lk)[None, :] <= np.arange(Lq)[:, None] + off)[None, None]
    if defect == "dropped_key_tile" and Lk > TILE_KEYS:
        live = live & (np.arange(Lk) < (Lk - 1) // TILE_KEYS * TILE_KEYS)[None, None, None, :]
    km = np.ones((B, Lk)) if x["kmask"] is None else f(x["kmask"])[own]
    full = (km == 0).all(1)
    lg = s.copy()
    if defect != "mask_multiplied":
        # float32 semantics of the additive mask: a masked key of a row that has valid keys gets probability 0, a fully
        # masked row has all scores rounded to -1e8 (uniform)
        lg = np.where(km[:, None, None, :] != 0, lg, -np.inf)
        lg[full] = 0.0
    lg = np.where(live, lg, -np.inf)
    with np.errstate(invalid="ignore"):
        e = np.exp(lg - np.max(lg, -1, keepdims=True))
    e = np.where(np.isfinite(e), e, 0.0)
    if defect == "mask_multiplied":
        e = e * km[:, None, None, :]
    p = e / np.maximum(e.sum(-1, keepdims=True), 1e-300)
    o = p @ vh
    ov_abs = p @ np.abs(vh)
    if m:
        o = o + np.einsum("bhqk,qkd->bhqd", p, rv[idx])
        ov_abs = ov_abs + np.einsum("bhqk,qkd->bhqd", p, np.abs(rv[idx]))
    out = o.transpose(0, 2, 1, 3).reshape(B * Lq, H)
    return {"out": out, "s": s, "s_abs": s_abs, "p": p, "vh": vh, "ov_abs": ov_abs, "full": full, "lg": lg, "idx": idx,
            "rv": rv if m else None}


def attn_bound(name, x):
    """Element-wise bound [B*Lq, H] of a kernel that forms everything in fp32, in any summation order and with an online
    (rescaling) softmax, from exactly representable inputs, against attn_reference.  PER_TERM u = 2^-23 per accumulated term
    (twice the unit roundoff), first order, as parity.gemm_bound and rela_ref.bound are derived:

      score    s_j = sum_c (q_c d^-0.5) k_jc, d fused multiply-adds and the rounding of q d^-0.5; with relative positions a
               second d-long chain and one addition:        |ds_j| <= (d + 2) u S_j + u |s_j|,  S_j = sum_c |q_c| |k_jc| d^-0.5
               (+ sum_c |q_c| |r_c| d^-0.5).  The mask adds exactly 0 to a valid key; a fully masked row's scores all round
               to -1e8: ds = 0 there.
      exp      e_j = exp(s_j - max): the subtraction rounds to u |s_j - max|, expf is good to 2 ulp:
                                                             rel(e_j) <= eps_j = |ds_j| + |ds_max| + (|s_j - max| + 4) u
      softmax  p_j = e_j / sum_k e_k, the sum over n live keys in any order and, online, at most one rescaling product per
               key on the way:       rel(p_j) <= eps_j + sum_k p_k eps_k + (2 n + 8) u =: rho_j
      values   o_c = sum_j p_j v_jc (+ sum_j p_j r_jc), n fused multiply-adds (+ n rescalings):
                                     |do_c| <= sum_j p_j rho_j |v_jc| + (2 n + 4) u sum_j p_j |v_jc|      (both sums)
      output   one division by the running sum and one rounding: + 2 u |o_c|.
    A row without a live key (there is none in a correct run) would have the bound 0."""
    cs = ATTN_CASES[name]
    return attn_bound_from(attn_f64(name, x), cs["B"], cs["nh"], cs["Lq"], cs["d"])


def attn_bound_from(r, B, nh, Lq, d):
    """attn_bound on the pieces of a float64 statement (the dict attn_f64 returns); tests/f32_ref.py states zk_f32_attn in the
    same terms (kv_group, a cached key count, a key bias) and is held to the same bound."""
    p, lg = r["p"], r["lg"]
    ds = (d + 2) * U * r["s_abs"] + U * np.abs(r["s"])
    ds[r["full"]] = 0.0
    finite = np.isfinite(lg)
    mx = np.max(lg, -1, keepdims=True)
    ds_max = np.max(np.where(finite, ds, 0.0), -1, keepdims=True)          # (whichever key the kernel took as the maximum)
    eps = np.where(finite, ds + ds_max + (np.abs(np.where(finite, lg - mx, 0.0)) + 4) * U, 0.0)
    n = finite.sum(-1, keepdims=True)
    rho = eps + (p * eps).sum(-1, keepdims=True) + (2 * n + 8) * U
    av = np.abs(r["vh"])
    do = (p * rho) @ av
    if r["idx"] is not None:
        do = do + np.einsum("bhqk,qkd->bhqd", p * rho, np.abs(r["rv"][r["idx"]]))
    do = do + (2 * n + 4) * U * r["ov_abs"]
    do = do.transpose(0, 2, 1, 3).reshape(B * Lq, nh * d)
    return do + 2 * U * np.abs(r["out"])


def attn_standin(name, x, seq_call=True):
    """What a correct kernel computes, on the CPU: torch float32, the keys in DESCENDING order through matrix products (the
    reference sums ascending in float64), the additive finite mask in float32, torch.softmax, then the values."""
    cs = ATTN_CASES[name]
    B, nh, d, Lq, Lk = (cs[x_] for x_ in ("B", "nh", "d", "Lq", "Lk"))
    m, p0 = cs.get("rpr", 0), cs.get("q_pos0", 0)
    rev = torch.arange(Lk - 1, -1, -1)
    qh = (x["q"].float() * torch.tensor(d ** -0.5, dtype=torch.float32)).view(B, Lq, nh, d).permute(0, 2, 1, 3)
    kh = x["k"].float().view(B, Lk, nh, d).permute(0, 2, 1, 3)[:, :, rev]
    vh = x["v"].float().view(B, Lk, nh, d).permute(0, 2, 1, 3)[:, :, rev]
    lg = qh @ kh.transpose(-1, -2)
    if m:
        idx = ((torch.arange(Lq)[:, None] + p0 - rev[None, :]).clamp(-m, m) + m)
        lg = lg + torch.einsum("bhqd,qkd->bhqk", qh, x["rk"].float()[idx])
    if x["kmask"] is not None:
        lg = lg + ((1.0 - x["kmask"].float()[:, rev]) * torch.tensor(-MASK_INF, dtype=torch.float32))[:, None, None, :]
    if cs.get("causal"):
        lg = lg.masked_fill((rev[None, :] > torch.arange(Lq)[:, None])[None, None], float("-inf"))
    w = torch.softmax(lg, -1)
    o = w @ vh
    if m:
        o = o + torch.einsum("bhqk,qkd->bhqd", w, x["rv"].float()[idx])
    return o.permute(0, 2, 1, 3).reshape(B * Lq, nh * d)


def worst_ratio(got, ref, bound):
    """largest |got - ref| / bound over the elements (0 / 0 counts as 0, a non-finite element as inf)."""
    got, ref, bound = (np.asarray(t, np.float64) for t in (got, ref, bound))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    return float(np.where(np.isfinite(got), ratio, np.inf).max())


# ---------------------------------------------------------------------------------------------- cumulative average
CUMAVG_SHAPE = dict(B=3, L=9, H=64, lengths=(9, 1, 6))


def cumavg_inputs(seed=0):
    cs = CUMAVG_SHAPE
    g = torch.Generator().manual_seed(7300 + seed)
    x = torch.randn(cs["B"] * cs["L"], cs["H"], generator=g)
    add = torch.randn(cs["B"] * cs["L"], cs["H"], generator=g)
    mask = torch.zeros(cs["B"], cs["L"])
    for b, n in enumerate(cs["lengths"]):
        mask[b, :n] = 1
    return {"x": x, "add": add, "mask": mask}


def cumavg_reference(x, mask, use_mask, add=None, defect=None):
    """transformer_aan.py:92-108 through oracle.ref_torch.average_attention (training branch) in float64; add: the merged
    attention's o + aan_o (func.py:258-275).  -> (out, bound) float64 [B*L, H].

    Bound of an fp32 kernel that sums in position order: avg_t = (sum of n_t <= t + 1 terms) / count -- n_t additions, the
    mask product and the division: |d avg_t| <= (n_t + 3) u mean_abs_t, mean_abs_t = the same average of |x|; the addend's
    sum and the output rounding: + 2 u (|add| + |avg|).  Padded rows under use_mask are exact zeros (bound 0 without add)."""
    B, L = mask.shape
    H = x.shape[1]
    hp = types.SimpleNamespace(aan_mask=bool(use_mask))
    xd, md = x.double().view(B, L, H), mask.double()
    avg = rt.average_attention(xd, md, None, 0, hp, True)
    mean_abs = rt.average_attention(xd.abs(), md, None, 0, hp, True)
    if defect == "divided_by_L":
        run = torch.cumsum(xd * (md[:, :, None] if use_mask else 1.0), 1) / float(L)
        avg = run * (md[:, :, None] if use_mask else 1.0)
    nt = torch.arange(1, L + 1, dtype=torch.float64)[None, :, None]
    bound = (nt + 3) * U * mean_abs
    out = avg
    if add is not None:
        out = add.double().view(B, L, H) + avg
        bound = bound + 2 * U * (add.double().view(B, L, H).abs() + avg.abs())
    else:
        bound = bound + 2 * U * avg.abs()
    return out.reshape(B * L, H).numpy(), bound.reshape(B * L, H).numpy()


def cumavg_standin(x, mask, use_mask, add=None):
    """float32, by the matrix product with the averaging weights (another summation order and 1 / n multiplied)."""
    B, L = mask.shape
    H = x.shape[1]
    xf, mf = x.float().view(B, L, H), mask.float()
    tri = torch.tril(torch.ones(L, L))
    if use_mask:
        w = tri[None] * mf[:, None, :] * mf[:, :, None]
        w = w / w.sum(-1, keepdim=True).clamp_min(1.0)
    else:
        cnt = torch.cumsum(mf, 1)
        w = tri[None] / torch.where(cnt <= 0, torch.ones_like(cnt), cnt)[:, :, None]
    out = w @ xf
    if add is not None:
        out = add.float().view(B, L, H) + out
    return out.reshape(B * L, H)


# ---------------------------------------------------------------------------------------------- shifted embedding
EMBED_SHAPE = dict(B=2, L=5, H=64, V=23)


def embed_inputs(seed=0):
    cs = EMBED_SHAPE
    g = torch.Generator().manual_seed(7400 + seed)
    ids = torch.randint(0, cs["V"], (cs["B"], cs["L"]), generator=g, dtype=torch.int32)
    return {"ids": ids, "table": torch.randn(cs["V"], cs["H"], generator=g), "bias": 0.1 * torch.randn(cs["H"], generator=g)}


def embed_reference(ids, table, bias, timing, defect=None):
    """transformer.py:88-112 in float64: pad(table[ids] sqrt(H) + bias, one row in front)[:-1] + timing[:L] -> (out, bound).
    Bound: the fp32 value of sqrt(H) (half a unit), the product, two additions: 4 u (|e| sqrt(H) + |bias| + |timing|)."""
    B, L = ids.shape
    H = table.shape[1]
    e = table.double()[ids.long()] * (H ** 0.5) + bias.double()
    mag = table.double().abs()[ids.long()] * (H ** 0.5) + bias.double().abs()
    sh = {None: 1, "shift_missing": 0, "shift_two": 2}[defect]
    pad = lambda t: torch.nn.functional.pad(t, (0, 0, sh, 0))[:, :L]
    tim = timing.double()[:L][None]
    out, mag = pad(e) + tim, pad(mag) + tim.abs()
    return out.reshape(B * L, H).numpy(), (4 * U * mag).reshape(B * L, H).numpy()


def embed_standin(ids, table, bias, timing):
    B, L = ids.shape
    H = table.shape[1]
    e = torch.addcmul(bias.float(), table.float()[ids.long()], torch.tensor(H ** 0.5, dtype=torch.float32))
    e = torch.cat([torch.zeros(B, 1, H), e[:, :-1]], 1)
    return (timing.float()[:L][None] + e).reshape(B * L, H)


# ---------------------------------------------------------------------------------------------- the model tests
MODEL_CASES = {          # name -> (model, hparams on top of tests.common.make_hp)
    "transformer": ("transformer", {}),
    "transformer_aan": ("transformer_aan", {}),
    "transformer_aan-use_ffn": ("transformer_aan", {"use_ffn": True}),
    "transformer_aan-aan_mask0": ("transformer_aan", {"aan_mask": False}),
    "transformer_rpr": ("transformer_rpr", {}),
    "transformer_fuse": ("transformer_fuse", {}),
}
SOURCE_LENGTHS = (14, 5, 9, 11)
TARGET_LENGTHS = (10, 4, 7, 6)
# The oracle's own floor: the largest relative difference, over the six MODEL_CASES and their four sentences, between
# oracle.ref_torch.score_fn run in float32 and in float64 on model_fixture().  Reproduce (CPU, prints every case):
#     python -m pytest tests/test_score_f32_checker.py -k oracle_floor -s
ORACLE_FLOOR = 1.259e-07
# The same for the forced-decoding identity  -score n / ((5 + n) / 6)^alpha == beam score  evaluated with the float32
# oracle alone (rt.beam_search against rt.score_fn, K = 1 and 4) on identity_fixture(); relative.  Reproduce:
#     python -m pytest tests/test_score_f32_checker.py -k identity_floor -s
IDENTITY_FLOOR = 2.636e-07
IDENTITY_MODEL = "transformer"
IDENTITY_SEED = 33            # chosen among 31 .. 37 (x EOS strengths 1 .. 3): every top hypothesis ends in EOS, one is 18 tokens long
IDENTITY_EOS = 2.0            # sharpening: the EOS logit gains this constant, the pad logit loses IDENTITY_PAD
IDENTITY_PAD = 6.0
IDENTITY_DIR = 4.0            # length of the direction added to the last LayerNorm offset that carries both


def model_fixture(case, seed=11):
    """-> (hp, Pn, src, tgt): the tiny model of tests.common.make_hp with perturbed biases / LayerNorm parameters, padded
    sources (14, 5, 9, 11 tokens) and targets (10, 4, 7, 6 tokens)."""
    from tests.common import make_hp, perturb
    model, kw = MODEL_CASES[case]
    hp = make_hp(model, scope_name="t_sf32_" + case.replace("-", "_"), **kw)
    Pn = perturb(rt.init_params(hp, model, seed=seed + 1), np.random.default_rng(seed))
    src = V.ragged(SOURCE_LENGTHS, hp.src_vocab.size(), 5)
    tgt = V.ragged(TARGET_LENGTHS, hp.tgt_vocab.size(), 6)
    return hp, Pn, src, tgt


def oracle_scores(hp, Pn, model, src, tgt, dtype):
    out = rt.score_fn({"source": torch.as_tensor(src), "target": torch.as_tensor(tgt)}, hp, rt.to_torch(Pn, dtype=dtype), model)
    return out["score"].double().numpy()


def identity_fixture():
    """-> (hp, Pn, src): a sharpened tiny model on which, under the oracle, the top hypothesis of EVERY sentence ends in EOS
    and holds no pad for beam 1 and beam 4 (checked in tests/test_score_f32_checker.py; no sentence is left out).
    Sharpening (in the spirit of tests/fullsize.py beam_params, which shapes the softmax rows): an untrained tiny model
    never prefers EOS, so the last LayerNorm's offset gains a fixed direction e (|e| = 1, times IDENTITY_DIR) that every
    decoder output then carries, the EOS row of the softmax embedding gains IDENTITY_EOS / IDENTITY_DIR e and the pad row
    loses IDENTITY_PAD / IDENTITY_DIR e: a constant on the two logits (a hypothesis that holds the pad id cannot be scored:
    the loss masks it, transformer.py:208-216)."""
    from tests.common import make_hp, perturb
    hp = make_hp(IDENTITY_MODEL, scope_name="t_sf32_identity", search_mode="cache", decode_length=12)
    Pn = perturb(rt.init_params(hp, IDENTITY_MODEL, seed=IDENTITY_SEED + 1), np.random.default_rng(IDENTITY_SEED))
    H = hp.hidden_size
    e = np.random.default_rng(IDENTITY_SEED + 77).choice([-1.0, 1.0], H) / np.sqrt(H)
    on = "decoder/layer_%d/feed_forward/layer_norm/offset" % (hp.num_decoder_layer - 1)
    Pn[on] = (Pn[on] + IDENTITY_DIR * e).astype(np.float32)
    name = rt._emb_name(hp, "softmax")
    E = Pn[name].astype(np.float64)
    E[hp.tgt_vocab.eos()] += IDENTITY_EOS / IDENTITY_DIR * e
    E[hp.tgt_vocab.pad()] -= IDENTITY_PAD / IDENTITY_DIR * e
    Pn[name] = E.astype(np.float32)
    src = V.ragged(SOURCE_LENGTHS, hp.src_vocab.size(), 5)
    return hp, Pn, src


def top_hypotheses(seqs, scores, eos):
    """-> [(tokens including the EOS, beam score)] of beam 0 of every sentence; asserts that each ends in EOS."""
    out = []
    for b in range(seqs.shape[0]):
        row = [int(t) for t in seqs[b, 0]]
        assert eos in row, ("the top hypothesis of sentence %d does not end in EOS" % b, row)
        assert 0 not in row[:row.index(eos)], ("the top hypothesis of sentence %d holds the pad id" % b, row)
        out.append((row[:row.index(eos) + 1], float(scores[b, 0])))
    return out


def identity_sides(hyps, score_of, alpha):
    """hyps from top_hypotheses; score_of(list of token lists) -> per-sentence scores (mean cross entropy).
    -> (lhs = -score n / ((5 + n) / 6)^alpha, rhs = beam score), float64 arrays."""
    sc = np.asarray(score_of([h for h, _ in hyps]), np.float64)
    n = np.array([len(h) for h, _ in hyps], np.float64)
    return -sc * n / ((5.0 + n) / 6.0) ** alpha, np.array([s for _, s in hyps], np.float64)


def pad_targets(hyps):
    L = max(len(h) for h, _ in hyps)
    tgt = np.zeros((len(hyps), L), dtype=np.int64)
    for b, (h, _) in enumerate(hyps):
        tgt[b, :len(h)] = h
    return tgt


def oracle_identity(hp, Pn, src, K, dtype=torch.float32):
    """The identity with the oracle alone: -> (lhs, rhs, hyps)."""
    hp = copy.copy(hp)
    hp.beam_size = K
    P = rt.to_torch(Pn, dtype=dtype)
    enc, dec = rt.infer_fn(hp, P, IDENTITY_MODEL)
    out = rt.beam_search({"source": torch.as_tensor(src)}, enc, dec, hp)
    hyps = top_hypotheses(out["seq"], out["score"], hp.tgt_vocab.eos())
    score_of = lambda toks: oracle_scores(hp, Pn, IDENTITY_MODEL, src, pad_targets([(t, 0) for t in toks]), dtype)
    lhs, rhs = identity_sides(hyps, score_of, hp.decode_alpha)
    return lhs, rhs, hyps
