"""The bf16 attention launch (zk_attn_fwd) in its decode forms: cases, inputs, the float64 reference, the CPU stand-in and
the planted defects (a plain module, no pytest in it; CPU only).

What the decode callers set and the training layout never does (zero_amd/models/_decode.py, zero_amd/models/_ops.py):
``kv_group`` > 1 (beam-tiled query rows share one sentence's keys, values and mask row), sentence strides of q / k / v
that are given, not derived, a position that lives in device memory (``pos_flags`` bit 0: it is the query's absolute
position; bit 1: only the keys 0 .. position exist, the slots behind hold whatever the last batch left), a single query
row, and the silent fall-back to the reference kernel for d != 64 or more than 256 keys.

Arithmetic of one query row b, position i, head h of nh (d = H / nh), written from the definition (func.py:218-256 of the
reference project with modules/rpr.py:10-75):

    rel(i, j) = clip(q_pos0 + i - j, -max_rel, max_rel) + max_rel
    s_j  = q_bih . (k_sjh + rk[rel(i, j)]) d^-0.5  - 1e8 [mask_sj == 0]  - 1e8 [causal and j > q_pos0 + i]     s = b // kv_group
    p    = softmax of s over the keys 0 .. nkeys - 1
    o    = sum_j p_j (v_sjh + rv[rel(i, j)])

``reference``   float64 numpy, one (row, head, position) at a time.
``standin``     what a correct kernel computes: float32, batched, the keys summed in descending order, bf16 rounding of the
                probabilities ahead of P.V and of the output (the sites parity._RoundFwd models); ``defect=`` plants ONE defect.
``check``       the row check of tests/parity.py on d-vectors under ``C_OUT``; nothing is excused.
"""
import numpy as np
import torch

from tests import parity as PR

MASK_INF = 1e8
MAX_REL = 4
WRONG_BY = 7        # a call that passes the position on the device passes position + WRONG_BY by value: the device's must win

# Twice the stand-in's worst row ratio over every run below is 7.1e-3 (measured on the CPU: 3.53e-3, block_offset
# with the causal mask; tests/test_attn_decode_checker.py re-measures it on every run).  That
# is not larger than the constant of the training layout (tests/test_gpu_attention_elementwise.py C_X["out"]): the
# existing constant is used.
STANDIN_WORST = 3.53e-3
C_OUT = 7.9e-3

DEFECTS = ("neighbour_keys", "mask_row_of_b", "mask_ignored", "one_key_more", "one_key_less", "position_by_value", "rpr_sign",
           "batch_stride_default", "dead_row_leak", "stale_chunk")


def run(time=None, rpr=False, pos=None, causal=False):
    """One call of a case.  time: the position (None: the case's own q_pos0); pos: "dev" = the position is read from
    device memory (and a wrong one passed by value), "value" = passed by value only, None = the case has none."""
    return dict(time=time, rpr=rpr, pos=pos, causal=causal)


def run_id(r):
    return "%s%s%s%s" % ("" if r["time"] is None else "t%d" % r["time"], "-rpr" if r["rpr"] else "",
                         "" if r["pos"] is None else "-" + r["pos"], "-causal" if r["causal"] else "")


def _cross(Ls, **kw):
    cs = dict(B=6, G=3, nh=2, d=64, Lq=1, Lk=Ls, lengths=(Ls, 70 if Ls > 70 else Ls // 2), layout="kv", pos_flags=0,
              runs=[run()])
    cs.update(kw)
    return cs


def _cached(Tmax, times):
    # per-row caches [B, Tmax, H], q the first H columns of the step's [B, 3H] projection; with the position on the device
    # the call names all Tmax slots and the kernel shrinks the key count; by value the call names time + 1 keys
    return dict(B=5, G=1, nh=3, d=64, Lq=1, Lk=Tmax, lengths=None, layout="cache", pos_flags=3,
                runs=[run(t, rpr, pos) for rpr in (False, True) for pos in ("dev", "value") for t in times])


# name -> shape of the direct calls.  B: query rows, G: kv_group, Lk: the allocated keys per sentence, lengths: valid keys
# per sentence (the mask; the masked keys of every sentence but the first score highest), layout: "kv" = k / v column
# slices of one [B / G * Lk, 2H + 16] matrix and q its own [B * Lq, H + 8] matrix, "cache" as above.
CASES = {
    "cross": _cross(17, lengths=(17, 6)),
    "cross_tiles_64": _cross(64), "cross_tiles_65": _cross(65), "cross_tiles_130": _cross(130), "cross_tiles_256": _cross(256),
    "cross_long": _cross(300),
    "cross_one_sentence": _cross(5, G=6, lengths=(4,)),
    "cross_flat": _cross(17, G=1, lengths=(17, 6, 11, 17, 3, 9)),
    "cross_rpr": _cross(17, lengths=(17, 6), pos_flags=1,
                        runs=[run(t, True, "dev") for t in (0, 3, 16, 40)] + [run(3, True, "value")]),
    "self_cached_24": _cached(24, (0, 1, 8, 23)),
    "self_cached_130": _cached(130, (0, 63, 64, 129)),
    "small_head": _cross(17, nh=4, d=16, lengths=(17, 6)),
    # the only form with more than one live query row; the sentence strides are the derived ones
    "block_offset": dict(B=2, G=1, nh=2, d=64, Lq=3, Lk=9, lengths=(9, 7), layout="kv", pos_flags=0, q_pos0=5,
                         default_strides=True, runs=[run(None, True, None, False), run(None, True, None, True)]),
}
# what only the reference kernel takes: impl = 2 must refuse these (tests/test_gpu_attn_decode_elementwise.py)
REFERENCE_KERNEL_ONLY = ("cross_long", "small_head")
RUNS = [(name, r) for name, cs in CASES.items() for r in cs["runs"]]


def bf16_round(a):
    """float32 array -> the nearest bf16 value (ties to even), as float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    u = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return u.view(np.float32)


def case_inputs(name, seed=0):
    """-> dict q [B, Lq, H], k, v [B / G, Lk, H], kmask [B / G, Lk] or None, rk, rv [2 MAX_REL + 1, d]: float32 torch
    tensors of bf16 values.  Queries lean towards the mean of their sentence's valid keys; a masked key is twice the mean
    query of its sentence, so the masked keys carry the largest raw scores; every sentence's values have an offset of
    their own, so another sentence's values show."""
    cs = CASES[name]
    B, G, nh, d, Lq, Lk = (cs[x] for x in ("B", "G", "nh", "d", "Lq", "Lk"))
    H, nB = nh * d, B // G
    g = torch.Generator().manual_seed(7100 + seed + sum(map(ord, name)))
    rnd = lambda *s: torch.randn(*s, generator=g)
    k, v = rnd(nB, Lk, H), rnd(nB, Lk, H) + rnd(nB, 1, H)
    kmask = None
    if cs["lengths"] is not None:
        kmask = torch.zeros(nB, Lk)
        for s, n in enumerate(cs["lengths"]):
            kmask[s, :n] = 1
    valid = torch.ones(nB, Lk) if kmask is None else kmask
    owner = torch.arange(B) // G
    mean_k = (k * valid[..., None]).sum(1) / valid.sum(1, keepdim=True)
    q = rnd(B, Lq, H) + mean_k[owner][:, None, :]
    for s in range(nB):
        k[s, valid[s] == 0] = 2.0 * q[s * G:(s + 1) * G].mean((0, 1))
    bf = lambda t: t.to(torch.bfloat16).float()
    return {"q": bf(q), "k": bf(k), "v": bf(v), "kmask": kmask, "rk": bf(0.3 * rnd(2 * MAX_REL + 1, d)),
            "rv": bf(0.3 * rnd(2 * MAX_REL + 1, d))}


def positions(name, r):
    """-> (q_pos0, nkeys) of a run: the query's absolute position and the number of keys that exist."""
    cs = CASES[name]
    pos = cs.get("q_pos0", 0) if r["time"] is None else r["time"]
    nkeys = min(cs["Lk"], pos + 1) if cs["layout"] == "cache" else cs["Lk"]
    return pos, nkeys


# ---------------------------------------------------------------------------------------------- float64, from the definition
def reference(name, x, time=None, rpr=False, causal=False):
    """-> {"out": [B, Lq, H], "lse": [B, nh, Lq]} float64."""
    cs = CASES[name]
    B, G, nh, d, Lq = (cs[n] for n in ("B", "G", "nh", "d", "Lq"))
    pos, nkeys = positions(name, run(time))
    q, k, v, rk, rv = (x[n].double().numpy() for n in ("q", "k", "v", "rk", "rv"))
    kmask = None if x["kmask"] is None else x["kmask"].double().numpy()
    out = np.zeros((B, Lq, nh * d))
    lse = np.zeros((B, nh, Lq))
    j = np.arange(nkeys)
    for b in range(B):
        s = b // G
        for h in range(nh):
            hs = slice(h * d, (h + 1) * d)
            for i in range(Lq):
                keys, vals = k[s, :nkeys, hs], v[s, :nkeys, hs]
                if rpr:
                    rel = np.clip(pos + i - j, -MAX_REL, MAX_REL) + MAX_REL
                    keys, vals = keys + rk[rel], vals + rv[rel]
                sc = keys @ q[b, i, hs] * d ** -0.5
                if kmask is not None:
                    sc = sc + np.where(kmask[s, :nkeys] == 0, -MASK_INF, 0.0)
                if causal:
                    sc = sc + np.where(j > pos + i, -MASK_INF, 0.0)
                e = np.exp(sc - sc.max())
                out[b, i, hs] = (e / e.sum()) @ vals
                lse[b, h, i] = sc.max() + np.log(e.sum())
    return {"out": out, "lse": lse}


def case_reference(name, x, r):
    return reference(name, x, r["time"], r["rpr"], r["causal"])


# ---------------------------------------------------------------------------------------------- float32 stand-in, defects
def applies(defect, name, r):
    """Can the defect change anything in this run at all?"""
    cs = CASES[name]
    nB = cs["B"] // cs["G"]
    pos, nkeys = positions(name, r)
    if defect == "neighbour_keys":
        return nB >= 2 and cs["G"] > 1
    if defect == "mask_row_of_b":
        return nB >= 2 and cs["G"] > 1 and cs["lengths"] is not None
    if defect == "mask_ignored":
        return cs["lengths"] is not None
    if defect == "one_key_more":
        return cs["layout"] == "cache" and nkeys < cs["Lk"]
    if defect == "one_key_less":
        return nkeys >= 2
    if defect == "position_by_value":
        return r["rpr"] and r["pos"] == "dev"
    if defect == "rpr_sign":
        return r["rpr"]
    if defect == "batch_stride_default":      # the given stride differs from keys * ld only where a cache is named in part
        return cs["layout"] == "cache" and r["pos"] == "value" and nkeys < cs["Lk"]
    return True


def standin(name, x, time=None, rpr=False, causal=False, pos=None, defect=None):
    """-> out [B, Lq, H] float64 (bf16 values; NaN where a defect leaves the prefill).

    defect (one at a time; each is something a kernel could do):
      neighbour_keys        k / v / mask of sentence b instead of b // kv_group
      mask_row_of_b         only the mask indexed by b
      mask_ignored          no key masked
      one_key_more          the key behind the position taken in (on the device that slot holds NaN; here the inputs' data)
      one_key_less          the last key left out
      position_by_value     the (wrong) by-value q_pos0 in the relative index where the device's holds the position
      rpr_sign              clip(j - i)
      batch_stride_default  sentence s's keys / values at s * keys * ld instead of the given stride
      dead_row_leak         the tile's rows >= Lq (zero queries: uniform weights) added into the live rows
      stale_chunk           one 8-element chunk of the output left at its prefill"""
    cs = CASES[name]
    B, G, nh, d, Lq, Lk = (cs[n] for n in ("B", "G", "nh", "d", "Lq", "Lk"))
    H, nB = nh * d, B // G
    r = run(time, rpr, pos, causal)
    assert defect is None or (defect in DEFECTS and applies(defect, name, r)), defect
    p0, nkeys = positions(name, r)
    f = np.float32
    q, k, v, rk, rv = (x[n].numpy().astype(f) for n in ("q", "k", "v", "rk", "rv"))
    owner = np.arange(B) // G
    mowner = owner
    if defect == "neighbour_keys":
        owner = mowner = np.arange(B) % nB
    if defect == "mask_row_of_b":
        mowner = np.arange(B) % nB
    nk = nkeys + (defect == "one_key_more") - (defect == "one_key_less")
    stride = nk if defect == "batch_stride_default" else Lk
    jd = np.arange(nk - 1, -1, -1)                                        # descending: another summation order
    rows = owner[:, None] * stride + jd[None, :]
    kh = k.reshape(nB * Lk, H)[rows].reshape(B, nk, nh, d).transpose(0, 2, 1, 3)      # [B, nh, nk, d]
    vh = v.reshape(nB * Lk, H)[rows].reshape(B, nk, nh, d).transpose(0, 2, 1, 3)
    qh = q.reshape(B, Lq, nh, d).transpose(0, 2, 1, 3)
    sc = np.matmul(qh, kh.transpose(0, 1, 3, 2))                           # [B, nh, Lq, nk]
    ia = p0 + np.arange(Lq)[:, None]
    if rpr:
        ir = ia + WRONG_BY if defect == "position_by_value" else ia
        dlt = jd[None, :] - ir if defect == "rpr_sign" else ir - jd[None, :]
        rel = np.clip(dlt, -MAX_REL, MAX_REL) + MAX_REL                  # [Lq, nk]
        sc = sc + np.einsum("bhid,ijd->bhij", qh, rk[rel]).astype(f)
    sc = sc * f(d ** -0.5)
    if x["kmask"] is not None and defect != "mask_ignored":
        m = x["kmask"].numpy()[mowner][:, jd]
        sc = sc + np.where(m == 0, f(-MASK_INF), f(0))[:, None, None, :]
    if causal:
        sc = sc + np.where(jd[None, :] > ia, f(-MASK_INF), f(0))[None, None]
    e = np.exp(sc - sc.max(-1, keepdims=True))
    p = bf16_round(e / e.sum(-1, keepdims=True))
    if defect == "dead_row_leak":
        p = p + bf16_round(np.full_like(p, 1.0 / nk))
    o = np.matmul(p, vh)
    if rpr:
        o = o + np.einsum("bhij,ijd->bhid", p, rv[rel]).astype(f)
    out = bf16_round(o.transpose(0, 2, 1, 3).reshape(B, Lq, H)).astype(np.float64)
    if defect == "stale_chunk":
        out[B - 1, Lq - 1, d + 8:d + 16] = np.nan
    return out


def case_standin(name, x, r, defect=None):
    return standin(name, x, r["time"], r["rpr"], r["causal"], r["pos"], defect)


# ---------------------------------------------------------------------------------------------- the check
def _rows(a, H):
    return torch.as_tensor(np.asarray(a, np.float64)).reshape(-1, H)


def row_ratio(name, got, ref_out):
    """The worst ||got - ref|| / max(||ref||, rms row norm) over the (row, position, head) d-vectors of a run."""
    cs = CASES[name]
    H = cs["nh"] * cs["d"]
    return float(PR.attn_row_ratio(_rows(got, H), _rows(ref_out, H), cs["d"]).max())


def check(name, got, ref_out, what):
    """parity.assert_attn_rows under C_OUT: every d-vector, none excused.  -> the worst ratio."""
    cs = CASES[name]
    H = cs["nh"] * cs["d"]
    return PR.assert_attn_rows(_rows(got, H), _rows(ref_out, H), cs["d"], C_OUT, what, heads=cs["nh"])


def single_key_rows(name, x, r):
    """The runs at position 0 of a cache: one visible key, so the row IS that key's value vector (+ the value table's row of
    distance 0).  -> want [B, Lq, H] float64, or None where the run has more than one visible key."""
    cs = CASES[name]
    pos, nkeys = positions(name, r)
    if cs["layout"] != "cache" or nkeys != 1:
        return None
    want = x["v"].double().numpy()[:, :1]
    if r["rpr"]:
        want = want + np.tile(x["rv"].double().numpy()[MAX_REL], cs["nh"])
    return want


def check_single_key(got, want, what):
    """One rounding to bf16 (2^-8 relative: half an ulp) of a sum of at most two bf16 values formed in fp32 (2^-23)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    tol = (2.0 ** -8 + 2.0 ** -20) * np.abs(want)
    assert np.isfinite(np.asarray(got, np.float64)).all() and (err <= tol).all(), (what, float((err - tol).max()))
