"""References, bounds, checker, case tables and CPU stand-ins of the beam-search tail kernels of
zero_amd/csrc/zk_decode.hip (a plain module, no pytest in it): zk_beam_topk, zk_beam_topk_advance, zk_beam_dev_prepare,
zk_beam_dev_advance, zk_gather_rows_ex, zk_add_gumbel.  tests/test_beam_checker.py (CPU) shows that the clean stand-ins
pass every case and that each planted defect fails; tests/test_gpu_beam_elementwise.py runs the kernels on the same
cases.

``topk_ref``         float64 scores of all K*V candidates of every sentence from the fp32 inputs, and the COUNTED bound.
``assert_topk``      the checker of a [B, k2] result: it does not depend on how near-ties fall.
``topk_exact_case``  cases whose order is exact by construction (small integer logits, equal maxima planted so that they
                     straddle every level of the selection).
``book_stop`` / ``book_ref``   the numpy bookkeeping of zero_amd/search.py:85-113,168-228; ``dev_prepare_expected`` /
                     ``dev_advance_expected`` apply it to the device-resident state (``BOOK_FIELDS``, ``Arena``).
``rand_u32_ref`` / ``gumbel_ref``   the counter-based generator of zk_common.h in uint32 arithmetic and the noise.
``topk_standin`` / ``book_standin``   what correct kernels compute, in fp32 numpy and in the kernels' own structure;
                     every ``defect`` plants ONE defect of the kind the kernels could have, None = correct.
``GuardedWords``     a flat int32 / fp32 buffer between two guard bands (workspace, indices, the search state).

Units as in tests/parity.py: one fp32 operation is off by at most 2^-24 of its result, every count is charged
PER_TERM = 2^-23, twice that.  The only measured constant is the project's C_EXP (__expf, __logf and the fp32 sum of
the exponentials: the cross-entropy kernels use the same intrinsics and the same kind of sum).
"""
import functools

import numpy as np
import torch

from tests.parity import PER_TERM, C_EXP, LEAD

f32, f64, i32 = np.float32, np.float64, np.int32
F32_MIN = np.finfo(np.float32).min
TOPK_MAX = 16                    # zk_decode.hip
TOPK_CHUNK_MAX = 8192
NONE_IDX = 0x7fffffff
GUARD_WORD = 0x4ACE4ACE          # the fp32 guard pattern of parity.Guarded
SENTINEL = 0x7BADBEEF            # prefill of integer outputs nobody wrote yet (as fp32: 1.8e36, finite)
NAN_WORD = 0x7FC00000


# ---------------------------------------------------------------------------------------------- the host's dispatch
def topk_chunks(K, V, k2):
    """zk_decode.hip topk_chunks: the number of column chunks, 0 = the one-block-per-row fallback."""
    nc = min(256 // (K * k2), 8)
    if nc < 1 or (V + nc - 1) // nc + 3 > TOPK_CHUNK_MAX:
        return 0
    return nc


def topk_chunk(V, nc):
    return ((V + nc - 1) // nc + 3) & ~3


def topk_path(K, V, k2):
    """"rows", "nv4" or "nv8": the kernel zk_beam_topk launches for the shape."""
    nc = topk_chunks(K, V, k2)
    if nc == 0:
        return "rows"
    return "nv4" if topk_chunk(V, nc) <= 4096 else "nv8"


def topk_workspace(B, K, k2):
    return B * K * (8 * k2 * 8 + 8 * 8)


def inv_temp_of(temperature):
    """1.f / temperature as the host forms it: the argument is a C float."""
    return f32(1.0) / f32(temperature)


def scal_words(penalty, forbid_id):
    """scal_dev: {fp32 bits of the length penalty, banned symbol or -1}."""
    return np.array([int(f32(penalty).view(i32)), int(forbid_id)], dtype=i32)


# ---------------------------------------------------------------------------------------------- top-k reference
def topk_ref(logits, prev, K, V, inv_temp_f32, penalty, forbid_id, forbid_value, terms=False):
    """logits fp32 [B*K, >= V], prev fp32 [B*K] -> (ref, bound), float64 [B, K*V] (flat candidate = beam * V + symbol).
        key = z * inv_temp;  m = max key;  lse = m + log sum exp(key - m);  lp = key - lse, the banned symbol's lp minus
        forbid_value AFTER the log-softmax;  score = (prev + lp) / penalty.
    The bound counts, in units of PER_TERM, before the division:
        |key|                     the product z * inv_temp (one rounding);
        C_EXP (|m| + |lse - m|)   __expf, the fp32 sum and __logf; the two parts separately: lse can be 0 while both are large;
        |lp|                      the subtraction key - lse, on its result;
        |lp_banned|               the subtraction of forbid_value, on its result (the banned candidate only);
        |prev + lp|               the addition of prev, on its result;
    all divided by the penalty, and after it
        |score|                   the division.  The library is built with hipcc -O3 and no fast-math or
                                  -fno-hip-fp32-correctly-rounded-divide-sqrt flag, so the fp32 division is correctly
                                  rounded: half an ulp, charged one PER_TERM like every other operation.
    terms = True: (ref, bound, fixed, shape) with bound = fixed + C_EXP PER_TERM shape (for topk_c_exp_needed)."""
    z = np.asarray(logits, dtype=f32)[:, :V].astype(f64)
    rows = z.shape[0]
    it, pen, fv = float(f32(inv_temp_f32)), float(f32(penalty)), float(f32(forbid_value))
    key = z * it
    m = key.max(1)
    lse_m = np.log(np.exp(key - m[:, None]).sum(1))
    lp = key - (m + lse_m)[:, None]
    mag = np.abs(key) + np.abs(lp)
    if forbid_id >= 0:
        lp[:, forbid_id] -= fv
        mag[:, forbid_id] += np.abs(lp[:, forbid_id])
    t = np.asarray(prev, dtype=f32).astype(f64).reshape(rows, 1) + lp
    ref = t / pen
    fixed = PER_TERM * ((mag + np.abs(t)) / abs(pen) + np.abs(ref))
    shape = np.broadcast_to(((np.abs(m) + np.abs(lse_m)) / abs(pen))[:, None], ref.shape)
    B = rows // K
    out = (ref.reshape(B, K * V), (fixed + C_EXP * PER_TERM * shape).reshape(B, K * V))
    if terms:
        out = out + (fixed.reshape(B, K * V), shape.reshape(B, K * V))
    return out


def topk_c_exp_needed(got_s, got_i, ref, fixed, shape):
    """The smallest c_exp with which the returned scores are inside the bound: for the measurement."""
    gi = np.asarray(got_i).astype(np.int64)
    take = lambda a: np.take_along_axis(a, gi, axis=1)
    err = np.abs(np.asarray(got_s).astype(f64) - take(ref))
    need = (err - take(fixed)) / np.maximum(PER_TERM * take(shape), 1e-300)
    return float(np.maximum(need, 0.0).max())


def topk_ratio(got_s, got_i, ref, bound):
    """The largest |err| / bound over the returned candidates."""
    gi = np.asarray(got_i).astype(np.int64)
    err = np.abs(np.asarray(got_s).astype(f64) - np.take_along_axis(ref, gi, 1))
    return float((err / np.maximum(np.take_along_axis(bound, gi, 1), 1e-300)).max())


def topk_order(ref, k):
    """argsort(-ref, stable)[:k] per sentence: descending, ties -> lower flat index."""
    return np.argsort(-ref, axis=1, kind="stable")[:, :k]


def topk_decisive(ref, bound, k2):
    """Per sentence: every pairwise gap among the reference's top k2 + 1 exceeds the sum of the two bounds (and so does
    the gap between the k2-th and everything below it, whose bounds can be larger: the banned candidates)."""
    B, n = ref.shape
    top = topk_order(ref, min(k2 + 1, n))
    r, b = np.take_along_axis(ref, top, 1), np.take_along_axis(bound, top, 1)
    gap = r[:, :, None] - r[:, None, :]
    need = b[:, :, None] + b[:, None, :]
    upper = np.triu(np.ones((top.shape[1],) * 2, dtype=bool), 1)[None]
    ok = np.where(upper, gap > need, True).all(axis=(1, 2))
    if n > k2:
        rest = (ref + bound).copy()
        np.put_along_axis(rest, top[:, :k2], -np.inf, 1)
        ok &= rest.max(1) < r[:, k2 - 1] - b[:, k2 - 1]
    return ok


def assert_topk(got_s, got_i, ref, bound, K, V, what):
    """got_s fp32 / got_i int [B, k2] against topk_ref's (ref, bound).  Per sentence:
      1. the indices lie in [0, K*V) and are pairwise distinct;
      2. |got_s[j] - ref[got_i[j]]| <= bound[got_i[j]];
      3. got_s is non-increasing and equal neighbours have ascending indices (on the kernel's own fp32 values);
      4. completeness: no candidate that was not returned has ref - bound > ref[last] + bound[last];
      5. a DECISIVE sentence (topk_decisive) returns exactly argsort(-ref, stable)[:k2].
    Returns the share of decisive sentences."""
    gs = np.asarray(got_s, dtype=f32)
    gi = np.asarray(got_i).astype(np.int64)
    B, k2 = gs.shape
    n = K * V
    fail = lambda b, msg: AssertionError("%s: sentence %d: %s; scores %r indices %r" % (what, b, msg, gs[b], gi[b]))
    for b in range(B):
        if not np.isfinite(gs[b]).all():
            raise fail(b, "non-finite score (check 2)")
        if (gi[b] < 0).any() or (gi[b] >= n).any():
            raise fail(b, "index outside [0, %d) (check 1)" % n)
        if len(set(gi[b].tolist())) != k2:
            raise fail(b, "an index returned twice (check 1)")
    err = np.abs(gs.astype(f64) - np.take_along_axis(ref, gi, 1))
    bnd = np.take_along_axis(bound, gi, 1)
    if (err > bnd).any():
        b, j = (int(v) for v in np.argwhere(err > bnd)[0])
        raise fail(b, "score %d (candidate %d = beam %d, symbol %d) is %r, reference %r, bound %.3e, |err| / bound = %.3g "
                   "(check 2)" % (j, gi[b, j], gi[b, j] // V, gi[b, j] % V, gs[b, j], ref[b, gi[b, j]], bnd[b, j],
                                  err[b, j] / max(bnd[b, j], 1e-300)))
    for b in range(B):
        for j in range(k2 - 1):
            if gs[b, j] < gs[b, j + 1]:
                raise fail(b, "scores %d, %d ascend (check 3)" % (j, j + 1))
            if gs[b, j] == gs[b, j + 1] and gi[b, j] > gi[b, j + 1]:
                raise fail(b, "equal scores %d, %d with descending indices (check 3)" % (j, j + 1))
    lower = ref - bound
    np.put_along_axis(lower, gi, -np.inf, 1)
    last = gi[:, -1:]
    limit = (np.take_along_axis(ref, last, 1) + np.take_along_axis(bound, last, 1))[:, 0]
    if (lower.max(1) > limit).any():
        b = int(np.argmax(lower.max(1) > limit))
        c = int(lower[b].argmax())
        raise fail(b, "candidate %d (beam %d, symbol %d, reference %r) is missing although the last one returned has %r "
                   "(check 4)" % (c, c // V, c % V, ref[b, c], ref[b, gi[b, -1]]))
    dec = topk_decisive(ref, bound, k2)
    want = topk_order(ref, k2)
    for b in np.nonzero(dec)[0]:
        if not np.array_equal(gi[b], want[b]):
            raise fail(int(b), "a decisive sentence must return %r (check 5)" % (want[b],))
    return float(dec.mean())


# ---------------------------------------------------------------------------------------------- top-k cases
FORBID_VALUE = 1e8               # zdtype.inf()
DECISIVE_FLOOR = 0.9             # every random case: at least this share of its sentences is decisive (check 5 is not vacuous)
PENALTY = 1.2345
_P = lambda B, K, V, ld, k2=None, off=0, kind="rand", note="": dict(B=B, K=K, V=V, ld=ld, k2=2 * K if k2 is None else k2,
                                                                   off=off, kind=kind, note=note)
# the shapes: every path of zk_beam_topk and the edges; kind "rand": randn * 2, prev randn; "sharp": the logits scaled by
# 6 and prev in -3 .. -30 (the regime of tests/fullsize.py); "step0": prev = [0, F32_MIN, ..] per sentence, the EOS ban on
TOPK_SHAPES = [
    _P(3, 4, 1000, 1000, note="chunked NV=4"), _P(2, 8, 517, 520, note="chunked NV=4, ld > V"),
    _P(2, 8, 9001, 9008, note="chunked NV=8"), _P(2, 1, 33000, 33000, note="chunked NV=8, K=1"),
    _P(2, 16, 8189, 8192, k2=16, note="boundary nc=1, chunked side: the largest chunk, 8192"),
    _P(2, 16, 8190, 8190, k2=16, note="boundary nc=1, row-fallback side"),
    _P(2, 8, 16378, 16380, k2=16, note="boundary nc=2, chunked side"),
    _P(2, 8, 16379, 16379, k2=16, note="boundary nc=2, row-fallback side"),
    _P(2, 4, 1001, 1001, note="scalar loads: odd rows are not 16-byte aligned"),
    _P(2, 4, 1000, 1004, off=1, note="scalar loads: the base pointer is one float off"),
    _P(2, 2, 4, 4, k2=4, note="V = k2"), _P(2, 1, 2, 2, k2=2, note="V = k2, K = 1"),
    _P(2, 3, 9, 16, note="most chunks are empty"), _P(1, 4, 1000, 1000, note="B = 1"),
    _P(3, 4, 1000, 1000, kind="step0", note="the real step-0 state"),
    _P(2, 8, 9001, 9008, kind="step0", note="the real step-0 state, NV=8"),
    _P(2, 8, 16379, 16379, k2=16, kind="step0", note="the real step-0 state, row fallback"),
    _P(3, 4, 1000, 1000, kind="sharp", note="sharpened logits"),
    _P(2, 8, 9001, 9008, kind="sharp", note="sharpened logits, NV=8"),
    _P(2, 16, 8190, 8190, k2=16, kind="sharp", note="sharpened logits, row fallback"),
]
EOS_ID = 2


def topk_variants(shape):
    """(temperature, penalty, forbid_id, through scal_dev) of one shape: forbid in {-1, an id} x the scalars through the
    arguments and through scal_dev x temperature 1.0 and 0.7; the step-0 state has its own penalty ((5 + 1) / 6)^alpha = 1
    and always bans EOS."""
    if shape["kind"] == "step0":
        return [(t, 1.0, min(EOS_ID, shape["V"] - 1), dev) for t in (1.0, 0.7) for dev in (False, True)]
    fid = min(EOS_ID, shape["V"] - 1)
    return [(t, PENALTY, f, dev) for t in (1.0, 0.7) for f in (-1, fid) for dev in (False, True)]


def topk_inputs(shape, seed=0):
    """-> logits fp32 [B*K, V], prev fp32 [B*K] (numpy)."""
    B, K, V = shape["B"], shape["K"], shape["V"]
    rng = np.random.default_rng(7000 + seed + 31 * V + K)
    z = (rng.standard_normal((B * K, V)) * 2).astype(f32)
    if shape["kind"] == "step0":
        prev = np.tile(np.array([0.0] + [F32_MIN] * (K - 1), dtype=f32), B)
    elif shape["kind"] == "sharp":
        z = (z * f32(6)).astype(f32)
        prev = rng.uniform(-30, -3, B * K).astype(f32)
    else:
        prev = rng.standard_normal(B * K).astype(f32)
    return z, prev


def exact_pairs(V, chunk):
    """Column pairs for two equal maxima: two slots of one thread (e, e + 1 and e, e + 1024), two threads of one wave, the
    wave boundaries (thread 63 | 64 and thread 255 | 0: elements 1023, 1024 of a chunk), a chunk boundary (v0 - 1, v0),
    column 0 and column V - 1.  The same column in two beams comes with every pair: all K rows carry the same logits."""
    pairs = [(8, 9), (16, 24), (255, 256), (0, V - 1)]
    if chunk > 1032 and V > 1032:
        pairs += [(8, 1032), (1023, 1024)]
    if chunk < V:
        pairs += [(chunk - 1, chunk), (2 * chunk - 1, 2 * chunk) if 2 * chunk < V else (chunk - 2, chunk + 1)]
    return [p for p in pairs if p[1] < V]


# (K, V, ld, k2): chunked NV=4 with chunk 1128 > 1032, chunked NV=8, the row fallback, and the scalar-load form of the first
EXACT_SHAPES = [(4, 9000, 9000, 8), (8, 9001, 9008, 16), (8, 16379, 16379, 16), (4, 9000, 9001, 8)]
EXACT_FAMILIES = ["equal_prev", "beam_major", "ban_low", "ban_max"]


def topk_exact_case(K, V, k2, family, seed=0):
    """A case whose order is exact BY CONSTRUCTION.  All K rows of a sentence carry the same logits (integers in -8 .. 3 with
    many duplicates, and two equal maxima, 6, at one of exact_pairs per sentence: one sentence per pair), the temperature is
    1.  "equal_prev": all beams have prev = -1.5, so every beam's block does identical arithmetic and equal keys give
    bit-equal scores: the order is "key descending, flat index ascending".  "beam_major": prev = -1000 k, which puts all of
    beam 0 first with a wide margin.  "ban_low": equal_prev with the ban on a non-winning id (the row minimum); "ban_max":
    the banned id is the row maximum (7) and lies in a chunk c > 0 where the shape has one.
    -> dict(logits [B*K, V], prev [B*K], forbid, expect [B, k2] int64, penalty)."""
    nc = topk_chunks(K, V, k2)
    chunk = topk_chunk(V, nc) if nc else V
    pairs = exact_pairs(V, chunk)
    B = len(pairs)
    rng = np.random.default_rng(9000 + seed + V + K)
    z = np.empty((B, V), dtype=f64)
    forbid = -1
    for b, (c1, c2) in enumerate(pairs):
        z[b] = rng.integers(-8, 4, V)
        z[b, c1] = z[b, c2] = 6
    if family == "ban_low":
        forbid = 5
        z[:, forbid] = -9
    elif family == "ban_max":
        forbid = chunk + 5 if chunk + 5 < V else V - 2
        z[:, forbid] = 7
    prev = np.tile((-1000.0 * np.arange(K)) if family == "beam_major" else np.full(K, -1.5), B)
    eff = np.repeat(z[:, None, :], K, 1) + prev.reshape(B, K, 1)           # exact in float64: the order of the scores
    if forbid >= 0:
        eff[:, :, forbid] -= FORBID_VALUE
    return {"logits": np.repeat(z, K, 0).astype(f32), "prev": prev.astype(f32), "forbid": forbid, "penalty": PENALTY,
            "expect": topk_order(eff.reshape(B, K * V), k2), "B": B}


# ---------------------------------------------------------------------------------------------- top-k stand-ins
TOPK_DEFECTS = ["rescan_ge", "reduce_noindex", "tail_dropped", "lse_chunk_missing", "ban_before", "ban_no_v0", "flat_ld",
                "penalty_mul", "scal_ignored", "prev_beam0", "temp_after_lse"]


def _chunk_select(key, n, k2, NV, defect):
    """k2 arg-max rounds of k_beam_topk_chunks<NV> over a chunk's keys: element e belongs to thread (e / 4) % 256, slot
    (e / 1024) * 4 + e % 4; every thread offers its best (the FIRST of equal keys: its slots are in element order), the
    block takes the best offer (ties -> lower element), the owner retires it.  -> [(key, element or NONE_IDX)] * k2."""
    E = NV * 1024
    full = np.full(E, -np.inf, dtype=f32)
    full[:n] = key[:n]
    e = np.arange(E)
    tab = np.empty((256, NV * 4), dtype=f32)
    el = np.empty((256, NV * 4), dtype=np.int64)
    tab[(e // 4) % 256, (e // 1024) * 4 + e % 4] = full
    el[(e // 4) % 256, (e // 1024) * 4 + e % 4] = e
    ar, out = np.arange(256), []
    for _ in range(k2):
        s = (NV * 4 - 1 - np.argmax(tab[:, ::-1], axis=1)) if defect == "rescan_ge" else np.argmax(tab, axis=1)
        bs = tab[ar, s]
        bi = np.where(bs > -np.inf, el[ar, s], NONE_IDX)
        cand = np.nonzero(bs == bs.max())[0]
        t = cand[-1] if defect == "reduce_noindex" else cand[np.argmin(bi[cand])]
        if bi[t] < n:
            out.append((bs[t], int(bi[t])))
            tab[t, s[t]] = -np.inf
        else:
            out.append((f32(-np.inf), NONE_IDX))
    return out


def _pick(score, flat, k2, tie_high=False):
    order = np.lexsort((-flat if tie_high else flat, -score))[:k2]
    short = k2 - order.size                  # (a defect can lose candidates: the selection then returns -inf, NONE_IDX)
    return (np.concatenate([score[order], np.full(short, -np.inf, dtype=f32)]),
            np.concatenate([flat[order], np.full(short, NONE_IDX, dtype=np.int64)]))


def topk_standin(logits, prev, B, K, V, ld, k2, temperature, penalty, forbid_id, forbid_value, scal=None, defect=None):
    """zk_beam_topk in fp32 numpy, in the form the host picks for the shape (topk_chunks): the chunked kernels with their
    per-chunk {m, s} partials, per-chunk k2 rounds and the merge by (score, flat index), or the one-block-per-row
    fallback.  logits [B*K, V]; scal = scal_words(..) or None.  -> (scores fp32 [B, k2], indices int64 [B, k2]).
    defect: "rescan_ge" (the per-thread rescan takes the LATER of equal keys), "reduce_noindex" (the wave / block reduction
    ignores the index), "tail_dropped" (the n % 4 tail of the last chunk is lost), "lse_chunk_missing" (chunk 1's partial
    is missing from lse), "ban_before" (the ban enters the log-softmax), "ban_no_v0" (the ban compares the chunk-local
    element with forbid_id), "flat_ld" (flat index k * ld + v), "penalty_mul", "scal_ignored", "prev_beam0" (every beam
    adds beam 0's prev), "temp_after_lse" (the log-softmax of z, then the temperature)."""
    z = np.asarray(logits, dtype=f32)[:, :V]
    prev = np.asarray(prev, dtype=f32)
    it, pen, fv = inv_temp_of(temperature), f32(penalty), f32(forbid_value)
    if scal is not None and defect != "scal_ignored":
        pen, forbid_id = np.asarray(scal, dtype=i32)[:1].view(f32)[0], int(scal[1])
    nc = topk_chunks(K, V, k2)
    stride = ld if defect == "flat_ld" else V
    late = defect == "temp_after_lse"
    out_s, out_i = np.empty((B, k2), dtype=f32), np.empty((B, k2), dtype=np.int64)
    for b in range(B):
        cs, ci = [], []
        for k in range(K):
            row = b * K + k
            pv = prev[b * K] if defect == "prev_beam0" else prev[row]
            key = z[row].copy() if late else (z[row] * it).astype(f32)
            fin = (lambda kk, lse: ((pv + (kk - lse) * it) if late else (pv + (kk - lse))))
            div = (lambda t: (t * pen) if defect == "penalty_mul" else (t / pen))
            if nc == 0:                                   # k_beam_topk_rows
                if forbid_id >= 0 and defect == "ban_before":
                    key[forbid_id] -= fv
                m = key.max()
                lse = m + np.log(np.exp(key - m, dtype=f32).sum(dtype=f32), dtype=f32)
                lp = key - lse
                if late:
                    lp = (lp * it).astype(f32)
                if forbid_id >= 0 and defect != "ban_before":
                    lp[forbid_id] += -fv
                sc = div((pv + lp).astype(f32)).astype(f32)
                s_, i_ = _pick(sc, k * stride + np.arange(V), k2, defect in ("rescan_ge", "reduce_noindex"))
                cs.append(s_); ci.append(i_)
                continue
            chunk = topk_chunk(V, nc)
            NV = 4 if chunk <= 4096 else 8
            pm, cand = [], []
            for c in range(nc):
                v0 = c * chunk
                n = max(0, min(chunk, V - v0))
                if defect == "tail_dropped" and v0 + n == V:
                    n -= n % 4
                kc = key[v0:v0 + n].copy()
                ban_at = (forbid_id if defect == "ban_no_v0" else forbid_id - v0) if forbid_id >= 0 else -1
                if defect == "ban_before" and 0 <= ban_at < n:
                    kc[ban_at] -= fv
                if n > 0:
                    m = kc.max()
                    pm.append((m, np.exp(kc - m, dtype=f32).sum(dtype=f32)))
                else:
                    pm.append((f32(-np.inf), f32(0)))
                if defect != "ban_before" and 0 <= ban_at < n:
                    kc[ban_at] -= fv
                cand += [(kk, v0 + e) for kk, e in _chunk_select(kc, n, k2, NV, defect) if e != NONE_IDX]
            if defect == "lse_chunk_missing" and nc > 1 and pm[1][0] > -np.inf:
                pm[1] = (f32(-np.inf), f32(0))
            m = max(p[0] for p in pm)
            s = f32(0)
            for pm_m, pm_s in pm:
                if pm_m > -np.inf:
                    s = f32(s + pm_s * np.exp(f32(pm_m - m), dtype=f32))
            with np.errstate(divide="ignore", invalid="ignore"):
                lse = f32(m + np.log(s, dtype=f32))
            kk =np.array([c_[0] for c_ in cand], dtype=f32)
            vv = np.array([c_[1] for c_ in cand], dtype=np.int64)
            cs.append(div(fin(kk, lse).astype(f32)).astype(f32)); ci.append(k * stride + vv)
        tie_high = nc == 0 and defect in ("rescan_ge", "reduce_noindex")
        out_s[b], out_i[b] = _pick(np.concatenate(cs), np.concatenate(ci), k2, tie_high)
    return out_s, out_i


# ---------------------------------------------------------------------------------------------- bookkeeping reference
def _top_k(x, k):
    idx = np.argsort(-x, axis=-1, kind="stable")[..., :k]
    return np.take_along_axis(x, idx, axis=-1), idx


def book_init(B, K, pad):
    """The state search.py starts from: seq [B, K, 1] = pad, fin_seq zeros, log_probs [0, F32_MIN, ..], .."""
    seq = np.full((B, K, 1), pad, dtype=np.int64)
    log_probs = np.tile(np.array([[0.] + [F32_MIN] * (K - 1)], dtype=f32), (B, 1))
    return {"seq": seq, "fin_seq": np.zeros_like(seq), "log_probs": log_probs, "scores": np.zeros_like(log_probs),
            "fin_scores": np.full((B, K), F32_MIN, dtype=f32), "fin_flags": np.zeros((B, K), dtype=bool)}


def book_stop(st, max_lp, mtl_i, time):
    """search.py:85-113: stop when every sentence's worst finished score beats its best alive bound, or when no sentence
    may grow.  -> (stop, every sentence bounded, some sentence may grow)."""
    with np.errstate(over="ignore"):
        worst = (st["fin_scores"] * st["fin_flags"].astype(f32)).min(axis=1) + \
            (f32(1.) - st["fin_flags"].any(axis=1).astype(f32)) * F32_MIN
        bound = bool((worst > st["log_probs"][:, 0] / max_lp).all())
    length = bool((time < mtl_i).any())
    return bound or not length, bound, length


def book_ref(st, ts, ti, time, V, mtl_i, eos, pad, penalty):
    """search.py:168-228 as in zero_amd/search.py: one step from the [B, 2K] survivors.  Returns the new state with the
    next step's inputs: flat_idx (b * K + source beam), next_tok, prev (= log_probs).  fp32, bit for bit."""
    seq, fin_seq, fin_scores, fin_flags = st["seq"], st["fin_seq"], st["fin_scores"], st["fin_flags"]
    B, K = fin_scores.shape
    penalty = f32(penalty)
    beam_idx = ti.astype(np.int64) // V; sym = ti.astype(np.int64) % V
    bpos = np.arange(B)[:, None]
    curr_seq = np.concatenate([seq[bpos, beam_idx], sym[:, :, None]], axis=2)
    curr_fin = (sym == eos) | (time >= mtl_i)[:, None]
    with np.errstate(over="ignore"):
        alive_scores, alive_idx = _top_k(ts + curr_fin.astype(f32) * F32_MIN, K)
        alive_lp = (alive_scores * penalty).astype(f32)
        cfs = ts + (f32(1.) - curr_fin.astype(f32)) * F32_MIN
    all_flags = np.concatenate([fin_flags, curr_fin], axis=1); all_scores = np.concatenate([fin_scores, cfs], axis=1)
    fin_scores, fin_idx = _top_k(all_scores, K)
    fin_flags = all_flags[bpos, fin_idx]
    all_seq = np.concatenate([np.concatenate([fin_seq, np.full((B, K, 1), pad, dtype=seq.dtype)], axis=2), curr_seq], axis=1)
    fin_seq = all_seq[bpos, fin_idx]
    flat = (np.arange(B)[:, None] * K + beam_idx[bpos, alive_idx]).reshape(-1)
    seq = curr_seq[bpos, alive_idx]
    return {"seq": seq, "fin_seq": fin_seq, "log_probs": alive_lp, "scores": alive_scores, "fin_scores": fin_scores,
            "fin_flags": fin_flags, "flat_idx": flat, "next_tok": seq[:, :, -1].reshape(-1), "prev": alive_lp.reshape(-1)}


# ---- the device-resident state (zk_decode.hip BeamDev), one numpy array per field
BOOK_FIELDS = ["ctrl", "stepbuf", "pen_table", "max_lp", "mtl_i", "topk_scores", "topk_idx", "seq", "fin_seq", "log_probs",
               "scores", "fin_scores", "fin_flags", "flat_idx", "next_tok", "prev"]          # the order of the C arguments
BOOK_F32 = {"pen_table", "max_lp", "topk_scores", "log_probs", "scores", "fin_scores", "prev"}
BOOK_SCRATCH = {"topk_scores", "topk_idx"}


def book_cfg(B, K, V, Tmax, mtl, eos=EOS_ID, pad=0, alpha=0.6):
    return {"B": B, "K": K, "V": V, "Tmax": Tmax, "Tcap": Tmax + 2, "eos": eos, "pad": pad, "alpha": alpha,
            "mtl": np.asarray(mtl, dtype=f32)}


def dev_init(cfg):
    """The arena as _beam_search_device lays it out (Tcap = Tmax + 2), with the sentinel in the columns of seq / fin_seq
    beyond the one written so far and in the outputs nobody wrote yet."""
    B, K, Tcap, mtl = cfg["B"], cfg["K"], cfg["Tcap"], cfg["mtl"]
    alpha = f32(cfg["alpha"])
    sent_i = lambda *s: np.full(s, SENTINEL, dtype=i32)
    sent_f = lambda *s: np.full(s, SENTINEL, dtype=i32).view(f32)
    d = {"ctrl": np.zeros(4, dtype=i32), "stepbuf": sent_i(4),
         "pen_table": np.array([f32(np.power(f32((f32(5.) + f32(t + 1)) / f32(6.)), alpha)) for t in range(Tcap)], dtype=f32),
         "max_lp": np.array([f32(np.power(f32((f32(5.) + m) / f32(6.)), alpha)) for m in mtl], dtype=f32),
         "mtl_i": mtl.astype(i32), "topk_scores": sent_f(B, 2 * K), "topk_idx": sent_i(B, 2 * K),
         "seq": sent_i(B, K, Tcap), "fin_seq": sent_i(B, K, Tcap),
         "log_probs": np.tile(np.array([0.] + [F32_MIN] * (K - 1), dtype=f32), (B, 1)), "scores": np.zeros((B, K), dtype=f32),
         "fin_scores": np.full((B, K), F32_MIN, dtype=f32), "fin_flags": np.zeros((B, K), dtype=i32),
         "flat_idx": sent_i(B * K), "next_tok": sent_i(B * K)}
    d["prev"] = d["log_probs"].reshape(-1).copy()
    d["seq"][:, :, 0] = cfg["pad"]
    d["fin_seq"][:, :, 0] = 0
    return d


def _ref_state(d, time):
    n = time + 1
    return {"seq": d["seq"][:, :, :n].astype(np.int64), "fin_seq": d["fin_seq"][:, :, :n].astype(np.int64),
            "log_probs": d["log_probs"], "scores": d["scores"], "fin_scores": d["fin_scores"],
            "fin_flags": d["fin_flags"] != 0}


def dev_prepare_expected(d, cfg):
    """zk_beam_dev_prepare through book_stop: -> the expected arrays (copies) and the cause ("frozen", "bound", "length",
    "overflow" or None = the step goes ahead)."""
    d = {k: v.copy() for k, v in d.items()}
    if d["ctrl"][1]:
        return d, "frozen"
    time = int(d["ctrl"][0])
    stop, bound, length = book_stop(_ref_state(d, 0), d["max_lp"], d["mtl_i"], time)
    if stop:
        d["ctrl"][1] = 1
        return d, "bound" if bound else "length"
    if time >= cfg["Tmax"]:
        d["ctrl"][1] = d["ctrl"][2] = 1
        return d, "overflow"
    d["stepbuf"][:3] = [time, int(d["pen_table"][time:time + 1].view(i32)[0]), cfg["eos"] if time < 1 else -1]
    d["ctrl"][0] = time + 1
    return d, None


def dev_advance_expected(d, cfg, ts=None, ti=None):
    """zk_beam_dev_advance through book_ref on the survivors ts / ti (default: the arena's topk_scores / topk_idx)."""
    d = {k: v.copy() for k, v in d.items()}
    if d["ctrl"][1]:
        return d
    ts = d["topk_scores"] if ts is None else np.asarray(ts, dtype=f32)
    ti = d["topk_idx"] if ti is None else ti
    time = int(d["stepbuf"][0])
    new = book_ref(_ref_state(d, time), ts, ti, time, cfg["V"], d["mtl_i"], cfg["eos"], cfg["pad"], d["stepbuf"][1:2].view(f32)[0])
    n = time + 2
    d["seq"][:, :, :n], d["fin_seq"][:, :, :n] = new["seq"], new["fin_seq"]
    for key in ("log_probs", "scores", "fin_scores", "flat_idx", "next_tok", "prev"):
        d[key][...] = new[key].reshape(d[key].shape)
    d["fin_flags"][...] = new["fin_flags"].astype(i32)
    return d


def book_survivors(cfg, time, seed, finish_at=None):
    """Synthetic survivors of one step: sorted scores with exact ties (one at the head, one across the alive cut K - 1 | K),
    random candidates, some EOS symbols.  finish_at == time: the first K candidates of every sentence end in EOS with high
    scores and the others fall far behind, so that the next stop test finds every sentence bounded."""
    B, K, V, eos = cfg["B"], cfg["K"], cfg["V"], cfg["eos"]
    rng = np.random.default_rng(100 * seed + time)
    ts = np.sort(rng.standard_normal((B, 2 * K)).astype(f32) * 3 - f32(time), axis=1)[:, ::-1].copy()
    ti = rng.integers(0, K * V, (B, 2 * K)).astype(i32)
    ti[ti % V == eos] += 1
    for b in range(B):
        if b % 3 == 0:
            ts[b, 1] = ts[b, 0]
        if b % 3 == 1:
            ts[b, K] = ts[b, K - 1]
        if b % 2 == 1:
            ts[b, 2 * K - 1] = ts[b, 2 * K - 2]
            j = int(rng.integers(0, 2 * K))
            ti[b, j] = (ti[b, j] // V) * V + eos
    if finish_at is not None and time == finish_at:
        ti[:, :K] = (ti[:, :K] // V) * V + eos
        ts[:, K:] -= f32(200)
    return ts, ti


BOOK_K = [1, 2, 3, 5, 8, 16]
BOOK_B = [1, 5, 300]
BOOK_SCENARIOS = {                      # name -> (Tmax, the length caps cycled over the sentences, finish_at)
    "length": (6, [3, 0, 1, 5, 2], None),           # runs until no sentence may grow (mtl_i = 0 and 1 are in it)
    "bound": (10, [9, 8, 9, 7, 9], 2),              # every sentence is bounded after step 2
}
BOOK_V = 50


def book_scenario(name, B, K):
    Tmax, caps, finish_at = BOOK_SCENARIOS[name]
    return book_cfg(B, K, BOOK_V, Tmax, [caps[b % len(caps)] for b in range(B)]), finish_at


# zk_beam_topk_advance against the two calls, (K, V, ld, off, temperature): NV = 4 at K = 1, 4, 8; NV = 8; the scalar-load
# path (odd ld; the base one float off); the chunked side of the nc = 2 boundary (one column more and it returns -2)
FUSED_CASES = [(1, 1000, 1000, 0, 1.0), (4, 1000, 1000, 0, 1.0), (8, 1000, 1000, 0, 0.7), (8, 9001, 9008, 0, 0.7),
               (4, 1001, 1001, 0, 1.0), (4, 1000, 1004, 1, 0.7), (8, 16378, 16380, 0, 1.0)]


def book_standin(d, cfg, phase, defect=None):
    """k_beam_prepare (phase "prepare") / k_beam_advance (phase "advance") on the arrays of the arena, in fp32 and with
    the kernels' own loops (zk_decode.hip:618-740).  defect: "tie_high" (a tie goes to the higher index), "fin_no_time" (the
    finished flag lacks time >= mtl_i), "no_pad_col" (the pad column of a carried finished row is not written),
    "no_parent" (seq is copied from row k instead of the parent beam), "not_frozen" (the state moves on after the stop),
    "prev_unscaled" (prev is not multiplied by the penalty)."""
    d = {k: v.copy() for k, v in d.items()}
    B, K, V, Tmax, eos, pad = cfg["B"], cfg["K"], cfg["V"], cfg["Tmax"], cfg["eos"], cfg["pad"]
    if d["ctrl"][1] and defect != "not_frozen":
        return d
    if phase == "prepare":
        time = int(d["ctrl"][0])
        bound_fail = length = False
        with np.errstate(over="ignore"):
            for b in range(B):
                best_alive = f32(d["log_probs"][b, 0] / d["max_lp"][b])
                fl = d["fin_flags"][b] != 0
                worst = f32(np.inf)
                for k in range(K):
                    worst = min(worst, f32(d["fin_scores"][b, k] * f32(1. if fl[k] else 0.)))
                worst = f32(worst + f32(1. - (1. if fl.any() else 0.)) * F32_MIN)
                bound_fail |= not (worst > best_alive)
                length |= time < d["mtl_i"][b]
        if not bound_fail or not length:
            d["ctrl"][1] = 1
            return d
        if time >= Tmax:
            d["ctrl"][1] = d["ctrl"][2] = 1
            return d
        d["stepbuf"][:3] = [time, int(d["pen_table"][time:time + 1].view(i32)[0]), eos if time < 1 else -1]
        d["ctrl"][0] = time + 1
        return d

    def top_k(x, k):
        used, idx = set(), []
        for _ in range(k):
            best = -1
            for i in range(len(x)):
                if i in used:
                    continue
                if best < 0 or (x[i] >= x[best] if defect == "tie_high" else x[i] > x[best]):
                    best = i
            idx.append(best); used.add(best)
        return idx
    time = int(d["stepbuf"][0])
    ln = time + 1
    penalty = d["stepbuf"][1:2].view(f32)[0]
    with np.errstate(over="ignore"):
        for b in range(B):
            ts, ti = d["topk_scores"][b], d["topk_idx"][b]
            l_seq, l_fin = d["seq"][b].copy(), d["fin_seq"][b].copy()
            beam, cur = ti // V, ti % V
            fin = (cur == eos) | (False if defect == "fin_no_time" else bool(time >= d["mtl_i"][b]))
            masked = (ts + fin.astype(f32) * F32_MIN).astype(f32)
            allsc = np.concatenate([d["fin_scores"][b], (ts + (f32(1.) - fin.astype(f32)) * F32_MIN).astype(f32)])
            allfl = np.concatenate([d["fin_flags"][b], fin.astype(i32)])
            aidx, fidx = top_k(masked, K), top_k(allsc, K)
            for k in range(K):
                c, j = aidx[k], fidx[k]
                lp = f32(masked[c] * penalty)
                d["scores"][b, k], d["log_probs"][b, k] = masked[c], lp
                d["prev"][b * K + k] = masked[c] if defect == "prev_unscaled" else lp
                d["flat_idx"][b * K + k], d["next_tok"][b * K + k] = b * K + beam[c], cur[c]
                d["fin_scores"][b, k], d["fin_flags"][b, k] = allsc[j], allfl[j]
                d["seq"][b, k, :ln] = l_seq[k if defect == "no_parent" else beam[c], :ln]
                d["seq"][b, k, ln] = cur[c]
                if j < K:
                    d["fin_seq"][b, k, :ln] = l_fin[j, :ln]
                    if defect != "no_pad_col":
                        d["fin_seq"][b, k, ln] = pad
                else:
                    d["fin_seq"][b, k, :ln] = l_seq[beam[j - K], :ln]
                    d["fin_seq"][b, k, ln] = cur[j - K]
    return d


BOOK_DEFECTS = ["tie_high", "fin_no_time", "no_pad_col", "no_parent", "not_frozen", "prev_unscaled"]


def assert_book_equal(got, want, what, skip=()):
    """Every array of the state bit for bit (the float arrays through their int32 views)."""
    for name in BOOK_FIELDS:
        if name in skip:
            continue
        g, w = np.ascontiguousarray(got[name]).view(i32), np.ascontiguousarray(want[name]).view(i32)
        if not np.array_equal(g, w):
            at = tuple(int(v) for v in np.argwhere(g != w)[0])
            raise AssertionError("%s: %s differs in %d word(s); the first at %r: got %#x (%r), expected %#x (%r)" %
                                 (what, name, int((g != w).sum()), at, int(g[at]) & 0xffffffff, got[name][at],
                                  int(w[at]) & 0xffffffff, want[name][at]))


# ---------------------------------------------------------------------------------------------- guarded flat buffers
class GuardedWords(object):
    """n 32-bit words between two guard bands of LEAD words (GUARD_WORD); the interior starts as ``fill`` (one word, or
    an int32 / fp32 numpy array of n words).  ``ptr`` is 256-byte aligned plus LEAD words, so 16-byte aligned."""

    def __init__(self, n, fill=SENTINEL, device="cpu"):
        self.n = int(n)
        host = np.full(self.n + 2 * LEAD, GUARD_WORD, dtype=i32)
        host[LEAD:LEAD + self.n] = np.ascontiguousarray(fill).view(i32).reshape(-1) if isinstance(fill, np.ndarray) else fill
        self.before = host.copy()
        self.t = torch.from_numpy(host.copy()).to(device)

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * LEAD

    def words(self):
        return self.t.detach().cpu().numpy()[LEAD:LEAD + self.n].copy()

    def check_guard(self, what):
        now = self.t.detach().cpu().numpy()
        bad = np.nonzero(np.concatenate([now[:LEAD] != GUARD_WORD, now[LEAD + self.n:] != GUARD_WORD]))[0]
        if bad.size:
            at = int(bad[0]) - LEAD if bad[0] < LEAD else int(bad[0]) - LEAD + self.n
            raise AssertionError("%s: %d word(s) outside the %d-word buffer were written; the first at word %d" %
                                 (what, bad.size, self.n, at))

    def check_intact(self, what):
        now = self.t.detach().cpu().numpy()
        bad = np.nonzero(now != self.before)[0]
        if bad.size:
            raise AssertionError("%s: %d word(s) changed; the first at word %d of %d" %
                                 (what, bad.size, int(bad[0]) - LEAD, self.n))


class Arena(object):
    """The search state on the device: every field of BOOK_FIELDS in its own GuardedWords."""

    def __init__(self, d, device):
        self.shapes = {k: d[k].shape for k in BOOK_FIELDS}
        self.buf = {k: GuardedWords(d[k].size, np.ascontiguousarray(d[k]), device) for k in BOOK_FIELDS}

    def args(self, cfg):
        return [self.buf[k].ptr for k in BOOK_FIELDS] + [cfg["B"], cfg["K"], cfg["V"], cfg["Tcap"], cfg["Tmax"], cfg["eos"],
                                                         cfg["pad"]]

    def write(self, name, arr):
        arr = np.ascontiguousarray(arr).view(i32).reshape(-1)
        self.buf[name].t[LEAD:LEAD + arr.size] = torch.from_numpy(arr.copy()).to(self.buf[name].t.device)

    def read(self, what="arena"):
        out = {}
        for k in BOOK_FIELDS:
            self.buf[k].check_guard("%s [%s]" % (what, k))
            w = self.buf[k].words().reshape(self.shapes[k])
            out[k] = w.view(f32) if k in BOOK_F32 else w
        return out


# ---------------------------------------------------------------------------------------------- Gumbel noise
def _mix32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def rand_u32_ref(seed, sid, idx):
    """zk_mix32 / zk_rand_u32 of zk_common.h in uint32 arithmetic (wrapping): seed a 64-bit integer, sid 32 bits, idx an
    array of 64-bit element indices; an element with a non-zero high index word takes the extra round."""
    u32 = np.uint32
    seed, sid = int(seed) & (2 ** 64 - 1), int(sid) & 0xffffffff
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        a = _mix32(np.array([(seed & 0xffffffff) ^ ((sid * 0x9E3779B1) & 0xffffffff)], dtype=u32))
        hi = u32(seed >> 32)
        b = np.broadcast_to(_mix32(hi + a), idx.shape).copy()
        ih = (idx >> np.uint64(32)).astype(u32)
        high = ih != 0
        if high.any():
            b[high] = _mix32(hi + ih[high] * u32(0x85EBCA77) + a)
        return _mix32(idx.astype(u32) * u32(0xC2B2AE3D) + b)


GUMBEL_CAP_BOUND = 1e-3          # the condition of the issue: at most GUMBEL_CAP_SHARE of the elements may have a bound
GUMBEL_CAP_SHARE = 0.005         # above GUMBEL_CAP_BOUND (the function's conditioning where u is close to 1)


def gumbel_ref(u32_words, eps):
    """The noise -log(-log(u + eps) + eps) of k_add_gumbel from the generator's words -> (ref, bound), float64.
    u = fp32(word) * 2^-32 and x = u + eps are formed in fp32, which numpy reproduces bit for bit; a = -log x and
    out = -log(a + eps) in float64.  The kernel's two __logf cost c PER_TERM each, c = C_EXP: the outer one on |out|; the
    inner one on |a| + 1 (near x = 1 the intrinsic's error is absolute, not relative to a), and the rounding of a + eps on
    a + eps itself, both amplified by d out / d a = 1 / (a + eps):
        bound = C_EXP PER_TERM (|out| + (|a| + 1) / (a + eps))
    The bound is wide where u is close to 1 (a + eps small): the function's conditioning, not slack."""
    e = f32(eps)
    u = (np.asarray(u32_words).astype(f32) * f32(2.0 ** -32)).astype(f32)
    x = (u + e).astype(f32).astype(f64)
    a = -np.log(x)
    out = -np.log(a + float(e))
    return out, C_EXP * PER_TERM * (np.abs(out) + (np.abs(a) + 1.0) / (a + float(e)))


def gumbel_wide_share(bound):
    return float((bound > GUMBEL_CAP_BOUND).mean())


# (rows, V, ld, seed, sid): the small case; rows * V > 2 097 152 = 8192 blocks x 256 with V no multiple of 256, so the
# grid-stride loop wraps in the middle of a row; a seed above 2^32
GUMBEL_EPS = 1e-8
GUMBEL_CASES = [(3, 37, 40, 5, 1), (66, 32003, 32008, 11, 7001), (3, 37, 40, (9 << 32) + 12345, 7001)]


@functools.lru_cache(maxsize=None)
def gumbel_case_ref(case):
    rows, V, ld, seed, sid = case
    return gumbel_ref(rand_u32_ref(seed, sid, np.arange(rows * V, dtype=np.uint64)).reshape(rows, V), GUMBEL_EPS)
