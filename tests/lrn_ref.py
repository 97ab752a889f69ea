"""References of the lrn / olrn cells at inference (a plain module, no pytest in it), in the manner of tests/deepatt_ref.py.

Reference arithmetic (rnns/lrn.py:32-53, rnns/olrn.py:32-58, rnns/rnn.py:41-49, 119-146), carry(m, a, b) = m a + (1 - m) b:

    cell(h_, [p|q|r])   = sigmoid(p + h_) r + sigmoid(q - h_) h_                          (lrn)
    cell(h_, [p|q|r|s]) = u sigmoid(s - u),  u = sigmoid(p + h_) r + sigmoid(q - h_) h_   (olrn: the gated value is carried)
    single:  h = carry(m_t, cell(h, lo_t), h)
    paired:  s = carry(m_t, cell(h, lo_t), h);   h = carry(m_t, cell(s, hi_t), s)

``lrn_scan``      the float64 numpy statement of zk_rnn_lrn_scan with every intermediate; ``defect=`` plants ONE defect.
``lrn_bound``     the element-wise bound propagated along the scan (derivation in its docstring).
``lrn_standin``   what a correct kernel computes, in torch float32 with another evaluation order.
``deepatt_hp`` / ``deepnmt_hp``   the model fixtures; the models themselves are restated in tests/deepatt_ref.py and
                  tests/deepnmt_ref.py, whose cell_fetch / cell_call run all four cells.

make_fixture on the fixtures of tests/test_gpu_lrn_model.py (vocabularies 120 / 104, sources of 14, 5, 9 and 11 tokens, beams 1
and 4), measured on the CPU (tests/test_lrn_host.py re-measures and asserts gap > 4 err and the score_tol rule, not the figures;
they move by an ulp of a score with the CPU's matrix-product order).  The seeds are the widest gap / err among the seeds 1 .. 39,
picked as deepatt_ref.SEEDS were:

%(FIGURES)s

gap, err, rel as in tests/rnnsearch_ref.py.  The bf16-storage restatement keeps the fp32 best hypotheses of the x 6 sharpened
model on all four.
"""
import numpy as np
import torch

from oracle import ref_torch as rt
from tests import deepatt_ref as DA
from tests import deepnmt_ref as DN
from tests import rnnsearch_ref as RS
from tests import variant_ref as V

LRN_DEFECTS = ("pq_swapped", "q_plus_h", "gate_reads_old_state", "ungated_carried", "mask_ignored", "mask_once_per_pair",
               "reverse_ignored", "seq_at_scan_index", "idx_ignored", "bf16_state", "last_dropped", "r_neighbour")
# fixture -> the seed of its model fixture
SEEDS = {"deepatt_lrn": 25, "deepatt_olrn": 20, "deepnmt_olrn_ca": 20, "deepnmt_lrn_plain": 35}
FIGURES = """    rnnsearch_deepatt  lrn,  NE 2, D 2, H 128, E 64                  seed 25:  gap 1.78e-04   err 5.7e-06 (gap =  31 x err)   rel 0.026
    rnnsearch_deepatt  olrn, NE 2, D 2, H 128, E 64                  seed 20:  gap 2.94e-04   err 1.9e-06 (gap = 154 x err)   rel 0.012
    deepnmt  olrn, caencoder, dl4mt_redict, NE 2, ND 3, H 128, E 64  seed 20:  gap 5.89e-04   err 5.7e-06 (gap = 103 x err)   rel 0.021
    deepnmt  lrn,  neither switch,          NE 1, ND 2, H 64,  E 64  seed 35:  gap 1.93e-04   err 5.7e-06 (gap =  34 x err)   rel 0.032

(about half of the seeds 1 .. 39 fail make_fixture's own assertions on these models -- a tie closer than 4 err, or a bf16-storage
run that flips a near-tie of the sharpened model: the element-wise cells leave a random model closer to ties than atr / gru do.)"""
__doc__ = __doc__ % dict(FIGURES=FIGURES)
RTOL, ATOL = RS.RTOL, RS.ATOL
score_tol = RS.score_tol
_bf, _sig = RS._bf, RS._sig
LENGTHS = DA.LENGTHS


# ---------------------------------------------------------------------------------------------- numpy, float64
def _cell(h_, x, H, gated, defect):
    """One cell on h_ [R, H] with x [R, 3 H | 4 H] -> dict of every intermediate; "v" is what the cell returns."""
    p, q, r = x[:, :H], x[:, H:2 * H], x[:, 2 * H:3 * H]
    if defect == "pq_swapped":
        p, q = q, p
    if defect == "r_neighbour":
        r = np.roll(r, -1, axis=1)
    i = _sig(p + h_)
    f = _sig(q + h_) if defect == "q_plus_h" else _sig(q - h_)
    u = i * r + f * h_
    c = {"h_": h_, "p": p, "q": q, "r": r, "i": i, "f": f, "u": u, "v": u}
    if gated:
        s = x[:, 3 * H:4 * H]
        g = _sig(s - (h_ if defect == "gate_reads_old_state" else u))
        c.update(s=s, g=g, v=u * g)
    return c


def lrn_scan(lo, hi=None, h_prev=None, idx=None, mask=None, reverse=False, gated=False, defect=None):
    """lo, hi [T, R, 3 H | 4 H] (hi None: the single form); h_prev [n_prev, H] or None (zero state); idx [R] int or None;
    mask [T, R] in [0, 1] or None.  -> dict: out [R, H] (the state after the last scanned position), seq [T, R, H] (the carried
    state AT every position), h0 (the gathered initial state), steps (per scanned position n: dict t, m [R], cells -- one
    _cell dict per cell with its "out", the carried value).

    defect (one at a time; each is something a kernel could do):
      pq_swapped            p and q swapped
      q_plus_h              f = sigmoid(q + h_)
      gate_reads_old_state  olrn: the output gate sigmoid(s - h_) from the un-updated state
      ungated_carried       olrn: u carried into the next step (the gated value only written out)
      mask_ignored          m = 1 everywhere
      mask_once_per_pair    paired: h = carry(m, higher(lower(h)), h) -- one carry per pair, not one per cell
      reverse_ignored       t ascending whatever `reverse`
      seq_at_scan_index     seq written at the scan index n, not at the position t
      idx_ignored           row r starts from h_prev[r]
      bf16_state            the state rounded to bf16 after every position
      last_dropped          the last scanned position left out
      r_neighbour           r_j taken from channel j + 1 (the last from channel 0)"""
    lo = np.asarray(lo, np.float64)
    T, R, W = lo.shape
    H = W // (4 if gated else 3)
    assert W == (4 if gated else 3) * H
    hi = None if hi is None else np.asarray(hi, np.float64)
    if h_prev is None:
        h = np.zeros((R, H))
    else:
        rows = np.arange(R) if (idx is None or defect == "idx_ignored") else np.asarray(idx)
        h = np.asarray(h_prev, np.float64)[rows]
    h0 = h
    mk = np.ones((T, R)) if (mask is None or defect == "mask_ignored") else np.asarray(mask, np.float64)
    carry = lambda m, a, b: m[:, None] * a + (1.0 - m[:, None]) * b
    seq = np.zeros((T, R, H))
    steps = []
    for n in range(T - 1 if defect == "last_dropped" else T):
        t = T - 1 - n if (reverse and defect != "reverse_ignored") else n
        m = mk[t]
        cells = []
        start, shown = h, None
        for x in ([lo[t]] if hi is None else [lo[t], hi[t]]):
            c = _cell(h, x, H, gated, defect)
            if defect == "mask_once_per_pair" and hi is not None:
                c["out"] = c["v"]
            else:
                c["out"] = carry(m, c["u"] if defect == "ungated_carried" else c["v"], h)
            shown = carry(m, c["v"], h)
            h = c["out"]
            cells.append(c)
        if defect == "mask_once_per_pair" and hi is not None:
            h = shown = carry(m, h, start)
        if defect == "bf16_state":
            h = _bf(h)
        seq[n if defect == "seq_at_scan_index" else t] = shown if defect == "ungated_carried" else h
        steps.append({"t": t, "m": m, "cells": cells})
    if defect == "last_dropped":
        seq[T - 1 if not reverse else 0] = h
    return {"out": h, "seq": seq, "h0": h0, "steps": steps, "H": H, "T": T, "gated": gated}


def lrn_bound(ref, form, what="out"):
    """Element-wise bound of zk_rnn_lrn_scan (form "bf16") / zk_f32_rnn_lrn_scan ("fp32") against lrn_scan(...) = ref, for
    inputs exactly representable where the kernel reads them (lo / hi in the storage type, h_prev and the mask in fp32).
    what: "out" (the fp32 state, [R, H]) or "seq" (every position in the storage type, [T, R, H]).  The state is fp32 in both
    forms and every product and sum is rounded on its own, so the bound is propagated cell by cell, PT = PER_TERM = 2^-23 (twice
    the unit roundoff) per operation, e_ the bound of the state h_ the cell reads (0 for the initial state):

      i = sigmoid(p + h_)   |di| <= S(i, PT |p + h_| + e_) + 4 PT i            (the sum; the slope; exp, 1 + e, the division)
      f = sigmoid(q - h_)   |df| <= S(f, PT |q - h_| + e_) + 4 PT f
      u = i r + f h_        |du| <= |r| di + |h_| df + f e_ + df e_ + 3 PT (|i r| + |f h_|)
                            -- the previous bound enters as at most e_ (|r| / 4 + |h_| / 4 + f), the rest is local
      olrn  g = sigmoid(s - u)   |dg| <= S(g, PT |s - u| + du) + 4 PT g
      S(y, d) = min(1/4, y (1 - y) + d / 10) d:  a sigmoid's slope is at most 1/4 everywhere, and within d of the point where
                            it is y (1 - y) at most y (1 - y) + d max|sigmoid''| with max|sigmoid''| = 0.0963 < 1/10.  The
                            second form is what keeps the bound of a saturated gate from compounding: with 1/4 alone the
                            factor |r| / 4 + |h_| / 4 + f passes 2 where |h_| > 3, and 34 cells of a 17-position pair would
                            carry bounds of the size of the values themselves (never wider than the 1/4 form)
            v = u g              |dv| <= |u| dg + g du + du dg + PT |u g|
      carry, m in {0, 1}    m = 1: the cell's value, no further rounding (1 v + 0 h_ is exact);  m = 0: h_ EXACTLY -- a carried
                            position adds nothing, its bound is e_
      carry, 0 < m < 1      m dv + (1 - m) e_ + 4 PT (|m v| + |(1 - m) h_|)      (1 - m, two products, the sum)
      + 2^-8 |value| for the bf16 copy in seq only (one rounding of the fp32 state); the fp32 form's copy is the state itself.
    No 2^-8 |h| term anywhere: that is what catches a state kept in bf16."""
    from tests import parity as PR
    PT = PR.PER_TERM
    R, H = ref["out"].shape
    e = np.zeros((R, H))
    seq_b = np.zeros((ref["T"], R, H))
    slope = lambda y, d: np.minimum(0.25, y * (1 - y) + 0.1 * d) * d
    for st in ref["steps"]:
        m = st["m"][:, None]
        frac = (m > 0) & (m < 1)
        for c in st["cells"]:
            h_, i, f, u = c["h_"], c["i"], c["f"], c["u"]
            di = slope(i, PT * np.abs(c["p"] + h_) + e) + 4 * PT * i
            df = slope(f, PT * np.abs(c["q"] - h_) + e) + 4 * PT * f
            dv = np.abs(c["r"]) * di + np.abs(h_) * df + f * e + df * e + 3 * PT * (np.abs(i * c["r"]) + np.abs(f * h_))
            if ref["gated"]:
                g = c["g"]
                dg = slope(g, PT * np.abs(c["s"] - u) + dv) + 4 * PT * g
                dv = np.abs(u) * dg + g * dv + dv * dg + PT * np.abs(u * g)
            e = m * dv + (1 - m) * e + frac * 4 * PT * (np.abs(m * c["v"]) + np.abs((1 - m) * h_))
        seq_b[st["t"]] = e
    if what == "out":
        return e
    return seq_b + (2.0 ** -8 * np.abs(ref["seq"]) if form == "bf16" else 0.0)


def lrn_standin(lo, hi, h_prev, idx, mask, reverse, gated, form):
    """What a correct kernel computes, on the CPU in torch float32 with another evaluation order: torch.sigmoid, u = f h_ + i r
    and the carry (1 - m) h_ + m v with the sums commuted; the copy rounded once in the bf16 form.  -> dict out, seq (float64)."""
    f32 = lambda t: torch.as_tensor(np.asarray(t, np.float64)).float()
    lo = f32(lo)
    T, R, W = lo.shape
    H = W // (4 if gated else 3)
    hi = None if hi is None else f32(hi)
    h = torch.zeros(R, H) if h_prev is None else f32(h_prev)[torch.arange(R) if idx is None else torch.as_tensor(np.asarray(idx))]
    mk = torch.ones(T, R) if mask is None else f32(mask)
    seq = torch.zeros(T, R, H)
    for n in range(T):
        t = T - 1 - n if reverse else n
        m = mk[t][:, None]
        for x in ([lo[t]] if hi is None else [lo[t], hi[t]]):
            p, q, r = x[:, :H], x[:, H:2 * H], x[:, 2 * H:3 * H]
            v = torch.sigmoid(q - h) * h + torch.sigmoid(h + p) * r
            if gated:
                v = torch.sigmoid(x[:, 3 * H:] - v) * v
            h = (1 - m) * h + m * v
        seq[t] = h.to(torch.bfloat16).float() if form == "bf16" else h
    return {"out": h.double().numpy(), "seq": seq.double().numpy()}


def scan_inputs(T, R, H, form, seed, gated, paired, n_prev=None, mask="mixed"):
    """float64 arrays exactly representable where the kernels read them: lo / hi in the storage type, the state in fp32.
    mask: "ones", "mixed" (an all-zero row, a hole in the middle of row 1, trailing padding elsewhere -- which a reversed scan
    meets first) or None.  idx repeats rows.  The projections are N(0, 0.7): the bound grows along a scan by up to
    |r| / 4 + f + |h_| / 4 per cell, which stays near 1 at this scale (17 positions of a pair: median bound 1e-6, largest 4e-4);
    at N(0, 1.5) the worst elements' bounds reach the size of the values and check nothing."""
    g = np.random.default_rng(500 + seed)
    st = lambda t: torch.as_tensor(np.asarray(t, np.float64)).float().to(V.STORAGE[form]).double().numpy()
    W = (4 if gated else 3) * H
    n_prev = R + 2 if n_prev is None else n_prev
    x = dict(lo=st(g.normal(0, 0.7, (T, R, W))), hi=st(g.normal(0, 0.7, (T, R, W))) if paired else None,
             h_prev=np.asarray(g.normal(0, 1, (n_prev, H)), np.float32).astype(np.float64), idx=g.integers(0, n_prev, R))
    x["idx"][:min(3, R)] = (n_prev - 1, n_prev - 1, 0)[:min(3, R)]
    if mask is None:
        x["mask"] = None
    elif mask == "ones":
        x["mask"] = np.ones((T, R))
    else:
        m = np.ones((T, R))
        for r in range(R):
            m[T - (r % max(T, 1)):, r] = 0.0          # trailing padding of r % T positions
        m[:, 0] = 0.0                                  # an all-zero row
        if T >= 3 and R >= 2:
            m[:, 1] = 1.0
            m[T // 2, 1] = 0.0                         # a hole in the middle
        x["mask"] = m
    return x


# ---------------------------------------------------------------------------------------------- the model fixtures
def deepatt_hp(cell, **kw):
    """The fixture of tests/test_gpu_deepatt_model.py (H 128, E 64, NE = D = 2) with an lrn / olrn cell."""
    return DA.fixture_hp(cell, **kw)                  # (scope t_deepatt_<cell>: no other fixture uses these cells)


DEEPNMT = {"olrn_ca": ("A", "olrn"), "lrn_plain": ("B", "lrn")}


def deepnmt_hp(which, **kw):
    """"olrn_ca": configuration (A) of tests/deepnmt_ref.py (the defaults' caencoder form, whose one-to-one decoder layers run)
    with olrn; "lrn_plain": configuration (B) (the plain [x | c] form) with lrn."""
    config, cell = DEEPNMT[which]
    kw.setdefault("scope_name", "t_lrn_deepnmt_%s" % which)
    return DN.fixture_hp(config, cell=cell, **kw)
