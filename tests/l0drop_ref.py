"""References of transformer_l0drop at inference (a plain module, no pytest in it).

Reference model (models/transformer_l0drop.py:16-135, 244-273; modules/l0norm.py:75-96, 166-177, GAMMA = -0.1,
ZETA = 1.1), per sentence with encoder outputs x_j, source mask m_j:

    log_alpha_j = x_j . W + b0                      gate_j = clip(sigmoid(log_alpha_j) * 1.2 - 0.1, 0, 1)
    keep_j = (gate_j != 0) m_j                      n_kept = sum keep,  n_dropped = sum m - n_kept
    memory = [0 | x_j gate_j for the kept j, ascending | fillers up to k = max over the batch of n_kept]
    mask   = [n_dropped > 0 | 1 .. | 0 ..]          count = [max(n_dropped, 1) | 1 ..]
    weights = exp(l - max l) count / sum(exp(l - max l) count),  l = scaled scores + (1 - mask) (-inf value)

``gate`` / ``compact`` / ``count_attention``   the float64 numpy statement of the above (the kernels' reference).
``dense_attention``    the same attention WITHOUT compaction: every source position stays where it is, the dropped and
                       the padded ones are masked, and one extra zero key with weight n_dropped is appended.
``decoding_fns``       encoding_fn / decoding_fn for oracle.ref_torch.beam_search: ref_torch's own encoder, linear,
                       layer_norm, ffn_layer and dot_attention (self-attention), only the cross-attention restated.
``make_fixture``       the tiny model and batch of the GPU model tests with the measured keep margins.
Every ``defect`` argument plants ONE defect of the kind the kernels could have; None = correct.
"""
import copy
import math

import numpy as np
import torch

from oracle import ref_torch as rt
from tests import variant_ref as V

LOG_ALPHA_0 = math.log(1.0 / 11.0)          # sigmoid(a) * 1.2 - 0.1 = 0  <=>  a = log(1 / 11)
MASK_INF = 1e9                              # as tests/decode_parity.py


# ---------------------------------------------------------------------------------------------- numpy, float64
def gate(enc, W, b0):
    """enc [B, Ls, H], W [H], b0 scalar -> (log_alpha, gate) float64 [B, Ls]."""
    la = np.asarray(enc, np.float64) @ np.asarray(W, np.float64).reshape(-1) + float(b0)
    return la, np.clip(1.0 / (1.0 + np.exp(-la)) * 1.2 - 0.1, 0.0, 1.0)


def compact(enc, g, smask, Lm=None, defect=None):
    """-> dict mem [B, Lm, H], gmask, count, kbias [B, Lm], pos (list of arrays), nkeep, ndrop [B], kmax.
    Lm None: 1 + kmax."""
    enc, g, smask = (np.asarray(v, np.float64) for v in (enc, g, smask))
    B, Ls, H = enc.shape
    keep = (g != 0) & (smask != 0)
    pos = [np.nonzero(keep[b])[0] for b in range(B)]
    if defect == "descending":
        pos = [p[::-1] for p in pos]
    nkeep = np.array([len(p) for p in pos])
    nvalid = (smask != 0).sum(1) if defect != "count_padding" else np.full(B, Ls)
    ndrop = nvalid - nkeep
    kmax = int(nkeep.max()) if B else 0
    Lm = 1 + kmax if Lm is None else Lm
    assert Lm >= 1 + kmax
    mem = np.zeros((B, Lm, H))
    gmask = np.zeros((B, Lm))
    count = np.ones((B, Lm))
    for b in range(B):
        mem[b, 1:1 + nkeep[b]] = enc[b, pos[b]] * g[b, pos[b], None]
        gmask[b, 1:1 + nkeep[b]] = 1
        gmask[b, 0] = 1.0 if (ndrop[b] > 0 or defect == "zero_slot_open") else 0.0
        count[b, 0] = max(ndrop[b], 1)
        if defect == "filler_valid" and 1 + nkeep[b] < Lm:
            gmask[b, 1 + nkeep[b]] = 1
    return {"mem": mem, "gmask": gmask, "count": count, "kbias": np.log(count), "pos": pos, "nkeep": nkeep,
            "ndrop": ndrop, "kmax": kmax}


def count_attention(q, k, v, mask, count, scale, mask_inf=MASK_INF):
    """q [B, R, d], k / v [B, L, d], mask / count [B, L] -> [B, R, d]: the reference's softmax with counts."""
    q, k, v, mask, count = (np.asarray(t, np.float64) for t in (q, k, v, mask, count))
    l = np.einsum("brd,bjd->brj", q, k) * scale + ((1 - mask) * -mask_inf)[:, None, :]
    e = np.exp(l - l.max(-1, keepdims=True)) * count[:, None, :]
    return np.einsum("brj,bjd->brd", e / e.sum(-1, keepdims=True), v)


def dense_attention(q, keys, vals, g, smask, scale):
    """No compaction: keys / vals [B, Ls + 1, d] are the projections of x_j gate_j for EVERY source position j and, last,
    of one zero memory row.  Dropped and padded positions are masked, the last key weighs n_dropped."""
    q, keys, vals, g, smask = (np.asarray(t, np.float64) for t in (q, keys, vals, g, smask))
    keep = (g != 0) & (smask != 0)
    ndrop = (smask != 0).sum(1) - keep.sum(1)
    assert keys.shape[1] == keep.shape[1] + 1
    w = np.concatenate([keep.astype(np.float64), ndrop[:, None].astype(np.float64)], 1)     # weight per key
    l = np.einsum("brd,bjd->brj", q, keys) * scale
    l = np.where(w[:, None, :] > 0, l, -np.inf)
    e = np.exp(l - l.max(-1, keepdims=True)) * w[:, None, :]
    return np.einsum("brj,bjd->brd", e / e.sum(-1, keepdims=True), vals)


# ---------------------------------------------------------------------------------------------- kernel-level checks
def gate_bound(enc, W, b0):
    """Bound of the fp32 gate against the float64 one.  log_alpha is a K = H term dot product of fp32 accumulation: the
    GEMM bound of tests/parity.py, (K + 8) 2^-23 (|x| . |W| + |b0|) (operand products are exact for bf16 rows; for fp32
    rows each product rounds once more, which the factor two in 2^-23 per term covers).  The gate's slope in log_alpha is
    at most 1.2 / 4; sigmoid, the multiply-add and the clip add a few units of 2^-23 of a value <= 1.2: eight of them.
    This term is an ADDITION to the one rounding of the storage type that the memory rows are checked with
    (assert_compact): the device forms the gate in fp32 and the reference in float64, so the two products differ by
    |x| times the gate's error before any rounding of the product; the term is ~1e-5 of a row element."""
    from tests import parity as PR
    enc, W = np.asarray(enc, np.float64), np.asarray(W, np.float64).reshape(-1)
    mag = np.abs(enc) @ np.abs(W) + abs(float(b0))
    la_bound = (enc.shape[-1] + 8) * PR.PER_TERM * mag
    return la_bound, 0.3 * la_bound + 8 * PR.PER_TERM * 1.2


def assert_compact(got, ref, enc, g_bound, out_dtype, what):
    """got: dict pos [B, Ls] (-1 behind the kept ones), nkeep, ndrop [B], kmax, gmask, kbias [B, Lm], mem [B, Lm, H] as the
    kernels wrote them; ref: compact(...) on the float64 gate with the same Lm.  pos, counts, kmax and gmask exact, kbias
    within 1e-6, mem within one rounding of its storage type of the float64 product (tests/parity.py U_OUT) plus what the
    bound of the gate (gate_bound) moves the product by."""
    from tests import parity as PR
    B = len(ref["pos"])
    assert int(got["kmax"]) == ref["kmax"], (what, got["kmax"], ref["kmax"])
    assert np.array_equal(np.asarray(got["nkeep"]), ref["nkeep"]), (what, "nkeep", got["nkeep"], ref["nkeep"])
    assert np.array_equal(np.asarray(got["ndrop"]), ref["ndrop"]), (what, "ndrop", got["ndrop"], ref["ndrop"])
    for b in range(B):
        n = int(ref["nkeep"][b])
        assert np.array_equal(np.asarray(got["pos"])[b, :n], ref["pos"][b]), (what, "pos", b)
        assert (np.asarray(got["pos"])[b, n:] == -1).all(), (what, "pos tail", b)
    assert np.array_equal(np.asarray(got["gmask"], np.float64), ref["gmask"]), (what, "gmask")
    err = np.abs(np.asarray(got["kbias"], np.float64) - ref["kbias"]).max()
    assert err <= 1e-6, (what, "kbias", err)
    # the bound of a kept row: the gate's bound times |x|, and one rounding of the storage type
    enc = np.asarray(enc, np.float64)
    bound = np.zeros_like(ref["mem"])
    for b in range(B):
        p = ref["pos"][b]
        bound[b, 1:1 + len(p)] = np.abs(enc[b, p]) * g_bound[b, p, None]
    bound = bound + PR.U_OUT[out_dtype] * np.abs(ref["mem"])
    PR.assert_elementwise(torch.as_tensor(np.asarray(got["mem"], np.float64)).reshape(-1, enc.shape[-1]),
                          torch.as_tensor(ref["mem"]).reshape(-1, enc.shape[-1]),
                          torch.as_tensor(bound).reshape(-1, enc.shape[-1]), what + ": mem")


def standin_compact(ref, Ls, out_dtype):
    """What correct kernels write for compact(...)'s result, on the CPU (the checker's stand-in for the device)."""
    B = len(ref["pos"])
    pos = -np.ones((B, Ls), np.int64)
    for b in range(B):
        pos[b, :len(ref["pos"][b])] = ref["pos"][b]
    mem = torch.as_tensor(ref["mem"]).to(out_dtype).double().numpy()
    return {"pos": pos, "nkeep": ref["nkeep"], "ndrop": ref["ndrop"], "kmax": ref["kmax"], "gmask": ref["gmask"],
            "kbias": ref["kbias"].astype(np.float32), "mem": mem}


def gate_inputs(Ls, storage, H=128, seed=0):
    """B = 4 sentences for zk_l0_gate / zk_l0_compact: 0 keeps all, 1 keeps none, 2 keeps an interleaved subset, 3 has a
    padded tail whose gates are positive.  Rows are built so that log_alpha is +-2 (+ noise of 0.2) around log(1/11):
    x = noise orthogonal part + t W / |W|^2.  -> enc (of `storage`), W, b0 (fp32), smask."""
    g = torch.Generator().manual_seed(900 + Ls + seed)
    W = torch.randn(H, generator=g) * 0.3
    b0 = torch.tensor(0.25)
    sign = torch.ones(4, Ls)
    sign[1] = -1
    sign[2, 1::2] = -1
    sign[2, 5] = -1
    sign[3, ::3] = -1
    target = LOG_ALPHA_0 + sign * (2.0 + 0.2 * torch.rand(4, Ls, generator=g)) - b0
    x = torch.randn(4, Ls, H, generator=g)
    x = x + ((target - x @ W) / (W @ W))[..., None] * W
    smask = torch.ones(4, Ls)
    smask[3, Ls - max(3, Ls // 4):] = 0            # the padded tail: its rows keep the pattern, some gates are positive
    smask[1, Ls - 2:] = 0
    return x.to(storage), W, b0, smask


def kb_case(Lk):
    """The smallest cross case of tests/decode_parity.py with Lk memory slots laid out as zk_l0_compact leaves them:
    sentence 0 dropped nothing (slot 0 masked, count 1), sentence 1 dropped 5 (count 5), sentence 2 dropped 2 and has
    three fillers.  -> (case, gmask [B, Lk], kbias [B, Lk])."""
    case = dict(H=128, BR=(3, 4), group=3, Lk=Lk, mask="l0drop", layout="halves", rel=None)
    gmask = torch.ones(3, Lk)
    gmask[0, 0] = 0
    gmask[2, Lk - 3:] = 0
    count = torch.ones(3, Lk)
    count[1, 0], count[2, 0] = 5, 2
    return case, gmask, torch.log(count)


def kb_inputs(case, gmask):
    """cross_inputs of tests/decode_parity.py with the memory's mask; slot 0 and the fillers hold the key / value of a
    ZERO memory row (the projections' biases: one vector for all of them), as the projections of zk_l0_compact's output do."""
    from tests import decode_parity as DP
    x = DP.cross_inputs(dict(case, mask=None))
    x["kmask"] = gmask.clone()
    g = DP._gen(77)
    kb0, vb0 = DP._randn(g, case["H"], scale=0.3), DP._randn(g, case["H"], scale=0.3)
    zero = gmask == 0
    zero[:, 0] = True
    x["keys"][zero], x["vals"][zero] = kb0, vb0
    return x


def kb_math(case, x, kbias, emulate=False, defect=None):
    """decode_parity.dec_attn_math's cross form with the log counts added to the scaled scores.  defect "no_kbias": the
    counts are ignored."""
    from tests import decode_parity as DP
    dt = DP.F32 if emulate else DP.F64
    rnd = DP._bf if emulate else (lambda v: v)
    c = lambda v: v.detach().to("cpu").to(dt)
    (B, R), H = case["BR"], case["H"]
    nh, rows = H // DP.D, B * R
    q = rnd(c(x["x"]) @ c(x["wqt"]).t() + c(x["bq"]))
    sent = torch.arange(rows) // R
    Kr, Vr, m = c(x["keys"])[sent], c(x["vals"])[sent], c(x["kmask"])[sent]
    n = Kr.shape[1]
    sc = torch.einsum("rhd,rjhd->rhj", q.view(rows, nh, DP.D), Kr.reshape(rows, n, nh, DP.D)) * DP.SCALE
    smax = float(sc.abs().max())
    sc = sc + ((1 - m) * -DP.MASK_INF)[:, None, :]
    if defect != "no_kbias":
        sc = sc + c(kbias)[sent][:, None, :]
    p = rnd(torch.softmax(sc, -1))
    ctx = rnd(torch.einsum("rhj,rjhd->rhd", p, Vr.reshape(rows, n, nh, DP.D)))
    parts = torch.einsum("rhd,hdo->hro", ctx, c(x["wot"]).t().reshape(nh, DP.D, H))
    return {"parts": parts.double(), "sum": parts.sum(0).double(), "smax": smax}


# ---------------------------------------------------------------------------------------------- ref_torch decoder step
def _prune_torch(enc, mask, P):
    """-> (memory [B, 1 + k, H], mask, count [B, 1 + k], log_alpha [B, Ls]).  The gate reads the fp32 MASTERS of
    source_pruning whatever the storage model (the keep decision is discrete); the product is stored like any activation."""
    la = (enc.reshape(-1, enc.shape[-1]) @ P["source_pruning/W_0_0"]).reshape(enc.shape[:2]) + P["source_pruning/b_0"]
    g = torch.clamp(torch.sigmoid(la) * 1.2 - 0.1, 0.0, 1.0)
    memory = rt._st(enc * g[..., None])
    keep = (g != 0) & (mask != 0)
    nkeep = keep.sum(1)
    ndrop = (mask != 0).sum(1) - nkeep
    k = int(nkeep.max())
    B, _, H = enc.shape
    mem = torch.zeros(B, 1 + k, H, dtype=enc.dtype)
    gm = torch.zeros(B, 1 + k, dtype=enc.dtype)
    cnt = torch.ones(B, 1 + k, dtype=enc.dtype)
    for b in range(B):
        idx = torch.nonzero(keep[b]).reshape(-1)
        mem[b, 1:1 + len(idx)] = memory[b, idx]
        gm[b, 1:1 + len(idx)] = 1
        gm[b, 0] = 1.0 if int(ndrop[b]) > 0 else 0.0
        cnt[b, 0] = max(int(ndrop[b]), 1)
    return mem, gm, cnt, la


def _cross_attention(x, memory, mem_mask, count, H, P, scope, nh, cache):
    """models/transformer_l0drop.py:16-100 with ref_torch's storage sites (dot_attention of oracle/ref_torch.py)."""
    scope = scope + "/dot_attention"
    q = rt.linear(x, P, scope + "/q_map")
    if "mk" in cache and "mv" in cache:
        k, v = cache["mk"], cache["mv"]
    else:
        k = rt.linear(memory, P, scope + "/k_map")
        v = rt.linear(memory, P, scope + "/v_map")
    cache["mk"], cache["mv"] = k, v
    q = rt.split_heads(q, nh) * (H // nh) ** (-0.5)
    k, v = rt.split_heads(k, nh), rt.split_heads(v, nh)
    logits = torch.matmul(q, k.transpose(-1, -2)) + rt.attention_bias(mem_mask, "masking")
    logits = logits - logits.max(-1, keepdim=True).values
    e = torch.exp(logits) * count[:, None, None, :]
    w = rt._st_fwd(e / e.sum(-1, keepdim=True), "probs")
    o = rt._st(rt.combine_heads(torch.matmul(w, v)), "attn_out")
    return rt.linear(o, P, scope + "/o_map")


def decoding_fns(hp, P, trace=None):
    """(encoding_fn, decoding_fn) of models/transformer_l0drop.py:418-451 (search_mode = cache) for rt.beam_search.
    trace: a dict that receives log_alpha [B, Ls] and the source mask of the encoded batch."""
    hp = rt.closing_dropout(copy.copy(hp))
    H, nh = hp.hidden_size, hp.num_heads

    def encoding_fn(source):
        state = V.cached_state(rt.encoder(source, hp, P, "transformer", False))
        if trace is not None:
            _, _, _, la = _prune_torch(state["encodes"], state["mask"], P)
            trace["log_alpha"], trace["mask"] = la.detach().double().numpy(), state["mask"].numpy()
        return state

    def decoding_fn(target, state, time):
        dt = P["bias"].dtype
        x = V.embed_step(target, time, hp, P)
        memory, mem_mask, count, _ = _prune_torch(state["encodes"], state["mask"], P)
        for l in range(hp.num_decoder_layer):
            pre = "decoder/layer_%d" % l
            lc = state["decoder"]["state"]["layer_%d" % l]
            r = rt.dot_attention(x, None, rt.attention_bias(1, "causal").to(dt), H, P, pre + "/self_attention", nh, cache=lc,
                                 training=False)
            lc.update(r["cache"])
            x = rt.layer_norm(rt.residual_fn(x, r["output"]), P, pre + "/self_attention")
            y = _cross_attention(x, memory, mem_mask, count, H, P, pre + "/cross_attention", nh, lc)
            x = rt.layer_norm(rt.residual_fn(x, y), P, pre + "/cross_attention")
            y = rt.ffn_layer(x, P, pre + "/feed_forward", None, False)
            x = rt.layer_norm(rt.residual_fn(x, y), P, pre + "/feed_forward")
        feature = x.reshape(-1, hp.embed_size)
        logits = torch.matmul(feature, rt._st_fwd(P[rt._emb_name(hp, "softmax")]).t())
        return logits, state

    return encoding_fn, decoding_fn


def with_pruning(Pn, W, b0):
    """Pn (numpy parameters of the `transformer` layout) plus the source_pruning pair, as float32."""
    out = dict(Pn)
    out["source_pruning/W_0_0"] = np.asarray(W, np.float32).reshape(-1, 1)
    out["source_pruning/b_0"] = np.asarray([b0], np.float32).reshape(1)
    return out


def log_alpha_of(hp, Pn, src, store_bf16=False, dtype=torch.float32):
    """log_alpha [B, Ls] (float64 numpy) and the source mask of ref_torch's encoder on `src`."""
    with V.storage_model(store_bf16):
        P = rt.to_torch(Pn, dtype=dtype)
        st = rt.encoder(torch.as_tensor(src), rt.closing_dropout(copy.copy(hp)), P, "transformer", False)
        _, _, _, la = _prune_torch(st["encodes"], st["mask"], P)
        return la.detach().double().numpy(), st["mask"].double().numpy()


def make_fixture(hp, src, seed, lo=0.25, hi=0.75):
    """The tiny model of the GPU model tests: rt.init_params + perturbed biases + a source_pruning pair scaled and shifted
    until between `lo` and `hi` of the valid positions of `src` are kept.  Measures, on the CPU with the reference:
      margin      min |log_alpha - log(1/11)| over the valid positions (fp32 run)
      err_f32     max |log_alpha_fp32 - log_alpha_float64|
      err_bf16    max |log_alpha(bf16 storage) - log_alpha(fp32)|
    and asserts margin >= 4 err_f32 and margin >= 4 err_bf16, and that the bf16-storage run keeps the same set.
    -> dict Pn, margin, err_f32, err_bf16, kept (bool [B, Ls]), frac."""
    from tests.common import perturb
    rng = np.random.default_rng(seed)
    Pn = perturb(rt.init_params(hp, "transformer", seed=seed + 1), rng)
    H = hp.hidden_size
    w = rng.normal(0.0, 1.0, H)
    la0, mask = log_alpha_of(hp, with_pruning(Pn, w, 0.0), src)
    valid = mask != 0
    v = la0[valid]
    # scale: a spread of ~3 around the threshold; shift: the median position sits ON the threshold, then the pair is nudged
    # until the nearest position is as far from it as it can be between its two neighbours
    scale = 3.0 / v.std()
    s = np.sort(v * scale)
    best = None
    for i in range(len(s) - 1):
        frac = 1.0 - (i + 1) / len(s)
        if lo <= frac <= hi and (best is None or s[i + 1] - s[i] > best[0]):
            best = (s[i + 1] - s[i], 0.5 * (s[i] + s[i + 1]))
    assert best is not None
    b0 = LOG_ALPHA_0 - best[1]
    Pn = with_pruning(Pn, w * scale, b0)
    la32, _ = log_alpha_of(hp, Pn, src)
    la64, _ = log_alpha_of(hp, Pn, src, dtype=torch.float64)
    labf, _ = log_alpha_of(hp, Pn, src, store_bf16=True)
    margin = float(np.abs(la32[valid] - LOG_ALPHA_0).min())
    err_f32 = float(np.abs(la32 - la64)[valid].max())
    err_bf16 = float(np.abs(labf - la32)[valid].max())
    kept = (la32 > LOG_ALPHA_0) & valid
    frac = kept.sum() / valid.sum()
    assert lo <= frac <= hi, frac
    assert margin >= 4 * err_f32, (margin, err_f32)
    assert margin >= 4 * err_bf16, (margin, err_bf16)
    assert np.array_equal((labf > LOG_ALPHA_0) & valid, kept)
    return {"Pn": Pn, "margin": margin, "err_f32": err_f32, "err_bf16": err_bf16, "kept": kept, "frac": float(frac)}
