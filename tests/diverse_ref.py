"""Diverse beam search (diverse_beam_groups = G, diverse_beam_strength = lambda; Vijayakumar et al. 2016, the Hamming
penalty, fairseq --diverse-beam-groups / --diverse-beam-strength): the rule, stated once, a reference search with groups, a
stand-in with planted defects and the fixtures of the model tests (a plain module, no pytest in it).

THE RULE.  With Kg = K / G the K rows of sentence b are G groups of Kg consecutive rows: row b K + g Kg + j is beam j of group
g.  Every group is a beam search of its own of width Kg -- its own alive and finished lists, log-probs that start at
[0, F32_MIN, ..], the same stop test -- so the search sees B G pseudo-sentences s = b G + g.  The groups are coupled inside one
step only.  S[r, v] is the score the search tail gives candidate (row r, token v) today: temperature, log-softmax over the row,
the EOS ban at step 0, (prev + logp) / length_penalty.  For g = 0 .. G-1 in order:
  * every candidate of the group's rows scores S[r, v] - lambda cnt(v) / length_penalty, cnt(v) = how often the groups
    0 .. g-1 counted v in this step;
  * the group keeps its 2 Kg best candidates, ties to the lower beam_in_group * V + v (zk_beam_topk's tie rule);
  * the group counts the tokens of its Kg best kept candidates whose token is not EOS.
The penalty is on log-probabilities, after the normalisation; it becomes part of the accumulated log-prob (the bookkeeping
multiplies the kept score by the length penalty) and of the reported score.  At the end the G Kg hypotheses of a sentence -- per
group the finished ones where it has any, else its alive ones -- are sorted by score, descending and stable in group order.

``select_full``    the rule on a full [K, V] score matrix (float64 unless the scores come as fp32: then every operation is fp32,
                   in the kernel's order -- the reference search's arithmetic);
``row_lists`` / ``select_lists``   the same from per-row candidate lists of depth K + Kg, which is exact (DEPTH below);
``step``           lists + selection, with ONE planted defect (DEFECTS) or none;  ``merge``: the end of the search;
``search``         the reference search with groups on oracle.ref_torch's decoding functions and tests/beam_ref.book_ref;
``margin``         what the reference alone shows on a fixture: float64 and fp32 token- and order-identical, gap > 4 x err.

DEPTH.  A kept candidate whose token is unpenalised has fewer than 2 Kg unpenalised entries of its row above it and at most
(G - 1) Kg penalised ones (that many tokens are counted at most): it is among the row's K + Kg best.  A penalised candidate
outside the row's K + Kg best has at least K + Kg entries above it, at most (G - 1) Kg - 1 of them penalised, so 2 Kg + 1
unpenalised ones that still beat it after the penalty: it is not kept.  tests/test_diverse_host.py runs the comparison.
"""
import copy

import numpy as np
import torch

from oracle import ref_torch as rt
from tests import beam_ref as BR

f32, f64 = np.float32, np.float64
F32_MIN = BR.F32_MIN
DEPTH_MAX = BR.TOPK_MAX          # K + K / G <= 16: the depth of zk_beam_topk's lists
DEFECTS = ("no_carry", "own_group", "eos_counted", "count_all", "shallow", "tie_high", "undivided", "interleaved",
           "merge_unsorted")
KG_SETTINGS = ((2, 2), (4, 2), (4, 4), (6, 3), (8, 2), (8, 4), (12, 3))      # (K, G) of the kernel tests
RTOL, ATOL = 1e-5, 1e-6          # the project's fp32 standard for scores (tests/test_gpu_decode_f32.py)


def depth(K, G):
    return K + K // G


# ---------------------------------------------------------------------------------------------- the rule
def _pick(score, flat, n, tie_high=False):
    """The n best of (score, flat): descending, ties to the lower flat index (tie_high: the planted defect)."""
    order = np.lexsort((-flat if tie_high else flat, -score))[:n]
    return order


def _penalised(raw, tok, counted, lam, pen):
    """raw - lam * cnt(tok) / pen in raw's dtype, operation by operation (the kernel's order: product, quotient, difference;
    an uncounted token keeps its score bit for bit)."""
    dt = raw.dtype.type
    cnt = np.zeros(raw.shape, dtype=np.int64)
    for t in counted:
        cnt += (tok == t)
    sub = (dt(lam) * cnt.astype(raw.dtype)) / dt(pen)
    return np.where(cnt > 0, raw - sub, raw).astype(raw.dtype)


def select_lists(cs, ci, V, G, lam, pen, eos, defect=None, rows_of=None, extra=0):
    """One sentence.  cs / ci [K, d]: every row's d best (score, token), best first.  -> (ts [G, 2 Kg (+ extra)], ti) with
    ti = beam_in_group * V + token.  rows_of(g) -> the group's rows (default: g Kg .. g Kg + Kg - 1)."""
    cs = np.asarray(cs)
    cs = cs.astype(f64) if cs.dtype != f32 else cs
    ci = np.asarray(ci).astype(np.int64)
    K = cs.shape[0]
    Kg = K // G
    keep = 2 * Kg
    counted, last = [], []
    ts = np.zeros((G, keep + extra), dtype=cs.dtype)
    ti = np.zeros((G, keep + extra), dtype=np.int64)
    for g in range(G):
        if defect == "no_carry":
            counted = list(last)                           # only what the group just before counted
        rows = np.arange(g * Kg, (g + 1) * Kg) if rows_of is None else np.asarray(rows_of(g))
        raw, tok = cs[rows].reshape(-1), ci[rows].reshape(-1)
        flat = (np.repeat(np.arange(Kg), cs.shape[1]) * V + tok).astype(np.int64)
        sc = _penalised(raw, tok, counted, lam, 1.0 if defect == "undivided" else pen)
        if defect == "own_group":
            # every pick is counted at once, so the group's own later picks are penalised too
            own, taken, order = list(counted), np.zeros(len(raw), dtype=bool), []
            for r in range(keep + extra):
                sc = _penalised(raw, tok, own, lam, pen)
                o = [i for i in _pick(sc, flat, len(sc)) if not taken[i]][0]
                taken[o] = True
                order.append(o)
                if r < Kg and tok[o] != eos:
                    own.append(int(tok[o]))
            order = np.array(order)
        else:
            order = _pick(sc, flat, keep + extra, tie_high=(defect == "tie_high"))
        ts[g], ti[g] = sc[order], flat[order]
        n_count = keep if defect == "count_all" else Kg
        last = [int(tok[o]) for o in order[:n_count] if defect == "eos_counted" or tok[o] != eos]
        counted = counted + last
    return ts, ti


def row_lists(S, d):
    """S [K, V] -> every row's d best (score, token), best first, ties to the lower token (zk_beam_topk with beam 1)."""
    S = np.asarray(S)
    idx = np.argsort(-S.astype(f64), axis=1, kind="stable")[:, :d]
    return np.take_along_axis(S, idx, 1), idx


def select_full(S, G, lam, pen, eos, extra=0):
    """The rule on the full score matrix S [K, V] of one sentence -> (ts [G, 2 Kg + extra], ti).  extra: that many runner-ups
    behind the kept ones (for ``margin``)."""
    S = np.asarray(S)
    return select_lists(*row_lists(S, S.shape[1]), S.shape[1], G, lam, pen, eos, extra=extra)


def step(S, G, lam, pen, eos, defect=None):
    """What the device step computes for one sentence: per-row lists of depth K + Kg, then the selection.  defect: one of
    DEFECTS (merge_unsorted belongs to ``merge``), None = correct."""
    S = np.asarray(S)
    K, V = S.shape
    Kg = K // G
    cs, ci = row_lists(S, 2 * Kg if defect == "shallow" else depth(K, G))
    rows_of = (lambda g: g + np.arange(Kg) * G) if defect == "interleaved" else None
    return select_lists(cs, ci, V, G, lam, pen, eos, defect=defect, rows_of=rows_of)


def merge(seqs, scores, G, defect=None):
    """[B G, Kg, T] / [B G, Kg] -> [B, K, T] / [B, K]: by score, descending, stable in group order."""
    B, n = scores.shape[0] // G, G * scores.shape[1]
    s, q = scores.reshape(B, n), seqs.reshape(B, n, -1)
    if defect == "merge_unsorted":
        return q, s
    order = np.argsort(-s.astype(f64), axis=1, kind="stable")
    return np.take_along_axis(q, order[:, :, None], 1), np.take_along_axis(s, order, 1)


# ---------------------------------------------------------------------------------------------- cases
def dyadic_scores(seed, K, V, levels=9):
    """[K, V] float64 multiples of 1/4 in (-levels/4 - K, 0]: many equal scores within and across rows."""
    rng = np.random.default_rng(seed)
    return -(rng.integers(0, levels, (K, V)) / 4.0 + rng.integers(0, 3, (K, 1)) / 2.0)


def dyadic_lists(seed, rows, d, V, levels=24):
    """Candidate lists as zk_beam_topk returns them: [rows, d] scores (multiples of 1/4, descending, equal neighbours with
    ascending tokens) and distinct tokens per row drawn from a small pool plus 0, V - 1, so that groups collide."""
    rng = np.random.default_rng(seed)
    pool = np.unique(np.concatenate([[0, EOS, V - 1], rng.choice(V, d, replace=False)]))      # d .. d + 3 tokens
    cs, ci = np.zeros((rows, d)), np.zeros((rows, d), dtype=np.int64)
    for r in range(rows):
        if r == 0:      # the first row holds the largest id and EOS whatever the draw
            tok = np.concatenate([[V - 1, EOS], rng.choice(pool[(pool != V - 1) & (pool != EOS)], d - 2, replace=False)])
        else:
            tok = rng.choice(pool, d, replace=False)
        sc = -rng.integers(0, levels, d) / 4.0 - (r % 3) / 2.0
        order = np.lexsort((tok, -sc))
        cs[r], ci[r] = sc[order], tok[order]
    return cs, ci


# the case named for every step defect: (seed, K, G, V, lambda, length penalty) of dyadic_scores, found by a scan over seeds
# (the first seed on which the defect's output differs from the rule's; tests/test_diverse_host.py asserts that it does)
DEFECT_CASES = {
    "no_carry": (0, 6, 3, 9, 0.5, 1.0),
    "own_group": (0, 4, 2, 9, 0.5, 1.0),
    "eos_counted": (2, 4, 2, 5, 0.5, 1.0),
    "count_all": (0, 4, 2, 9, 0.5, 1.0),
    "shallow": (0, 6, 3, 12, 0.5, 1.0),
    "tie_high": (0, 4, 2, 9, 0.5, 1.0),
    "undivided": (0, 4, 2, 9, 0.5, 2.0),
    "interleaved": (0, 4, 2, 9, 0.5, 1.0),
}
EOS = 2


# ---------------------------------------------------------------------------------------------- the reference search
def grouped_search(source, encoding_fn, decoding_fn, hp, G, lam, trace=None, runner_ups=1):
    """rt.beam_search (search_mode = cache) with beam groups: the model runs on [B K] rows as ever, the bookkeeping
    (beam_ref.book_init / book_stop / book_ref, fp32 numpy as zero_amd/search.py) on B G pseudo-sentences of Kg beams, the
    step's selection is ``select_full`` on the fp32 scores.  trace: a list that receives per step (ts, ti) [B G, 2 Kg +
    runner_ups] of the rule."""
    K = hp.beam_size
    Kg = K // G
    alpha, eos, pad = hp.decode_alpha, hp.tgt_vocab.eos(), hp.tgt_vocab.pad()
    B = source.shape[0]
    state = encoding_fn(source)

    def tile(x):
        x = x.unsqueeze(1)
        reps = [1] * x.dim()
        reps[1] = K
        return x.repeat(*reps)
    state = rt._map_structure(tile, state)
    st = BR.book_init(B * G, Kg, pad)
    # search.py:56-77 cache_init: a dummy step, then the original entries restored (as rt.beam_search)
    snapshot = rt._copy_nest(state)
    _, s0 = decoding_fn(torch.as_tensor(st["seq"].reshape(B * K, 1)), rt._map_structure(lambda x: rt._merge(x, 0), state), 0)
    state = rt._dict_update(rt._map_structure(lambda x: rt._unmerge(x, B, 0), s0), snapshot)
    mtl = np.repeat((source != 0).sum(-1).numpy().astype(f32) + f32(hp.decode_length), G)
    mtl_i = mtl.astype(np.int32)
    max_lp = np.power((f32(5.) + mtl) / f32(6.), f32(alpha)).astype(f32)
    time = 0
    while not BR.book_stop(st, max_lp, mtl_i, time)[0]:
        flat_state = rt._map_structure(lambda x: rt._merge(x, 0), state)
        last = torch.as_tensor(st["seq"].reshape(B * K, -1)[:, -1:])
        logits, step_state = decoding_fn(last, flat_state, time)
        logits = logits.to(torch.float32) / hp.beam_search_temperature
        lp = logits - torch.logsumexp(logits, dim=-1, keepdim=True)
        V = lp.shape[-1]
        if time < 1:
            lp = lp + (torch.arange(V) == eos).to(torch.float32)[None, :] * -rt.Cfg.inf
        penalty = f32(np.power(f32((f32(5.) + f32(time + 1)) / f32(6.)), f32(alpha)))
        S = ((torch.as_tensor(st["log_probs"].reshape(B * K, 1)) + lp) / torch.tensor(float(penalty), dtype=torch.float32))
        S = S.numpy().reshape(B, K, V)
        sel = [select_full(S[b], G, lam, penalty, eos, extra=runner_ups if trace is not None else 0) for b in range(B)]
        ts = np.concatenate([s[0] for s in sel]).astype(f32)
        ti = np.concatenate([s[1] for s in sel])
        if trace is not None:
            trace.append((ts.copy(), ti.copy()))
        st = BR.book_ref(st, ts[:, :2 * Kg], ti[:, :2 * Kg], time, V, mtl_i, eos, pad, penalty)
        parent = torch.as_tensor(st["flat_idx"].reshape(B, K) - np.arange(B)[:, None] * K)
        step_state = rt._map_structure(lambda x: rt._unmerge(x, B, 0), step_state)
        state = rt._map_structure(lambda x: rt._gather_beams(x, parent), step_state)
        time += 1
    any_fin = st["fin_flags"].any(axis=1)
    seqs = np.where(any_fin[:, None, None], st["fin_seq"], st["seq"])
    scores = np.where(any_fin[:, None], st["fin_scores"], st["scores"])
    groups = {"seq": seqs[:, :, 1:].copy(), "score": scores.copy()}
    seqs, scores = merge(seqs, scores, G)
    return {"seq": seqs[:, :, 1:], "score": scores, "steps": time, "groups": groups}


def search(decoding_fns, hp, Pn, src, K, G, lam, dtype, trace=None, store_bf16=False):
    """grouped_search over decoding_fns(hp, P) with the numpy parameters Pn in `dtype` (variant_ref.search with groups;
    store_bf16: under ref_torch's bf16 storage model)."""
    from tests.variant_ref import storage_model
    hp = copy.copy(hp)
    hp.beam_size, hp.search_mode = K, "cache"
    with storage_model(store_bf16), torch.no_grad():
        enc, dec = decoding_fns(hp, rt.to_torch(Pn, dtype=dtype))
        return grouped_search(torch.as_tensor(src), enc, dec, hp, G, lam, trace=trace)


def margin(decoding_fns, hp, Pn, src, K, G, lam, factor=4.0, what=""):
    """The proof that the REFERENCE ALONE is far from a tie (variant_ref.candidate_margin with groups): the float64 and the
    fp32 model give identical hypotheses and, at every step, the same kept candidates in the same order per group;
      gap   the smallest difference, over all steps and groups of the float64 run, between a kept candidate and the next one in
            the group's ranking (kept or the runner-up) -- every decision of the rule (kept or not, counted or not, the order
            the bookkeeping sees) is a comparison of such neighbours;
      err   the largest |score_fp32 - score_float64| over the kept candidates;
    and gap > factor * err.  -> dict gap, err, rel (err as a share of ATOL + RTOL |score|)."""
    Kg = K // G
    t64, t32 = [], []
    o64 = search(decoding_fns, hp, Pn, src, K, G, lam, torch.float64, trace=t64)
    o32 = search(decoding_fns, hp, Pn, src, K, G, lam, torch.float32, trace=t32)
    assert np.array_equal(o64["seq"], o32["seq"]), ("float64 and fp32 reference disagree", what)
    assert len(t64) == len(t32)
    gap, err, rel = np.inf, 0.0, 0.0
    for (s64, i64), (s32, i32) in zip(t64, t32):
        s64, s32 = np.maximum(s64.astype(f64), -1e35), np.maximum(s32.astype(f64), -1e35)
        live = s64[:, :2 * Kg] > -1e30
        gap = min(gap, float(np.where(live, s64[:, :2 * Kg] - s64[:, 1:2 * Kg + 1], np.inf).min()))
        assert np.array_equal(i64[:, :2 * Kg][live], i32[:, :2 * Kg][live]), ("candidate order differs", what)
        diff = np.abs(s64[:, :2 * Kg] - s32[:, :2 * Kg])
        err = max(err, float(diff[live].max()))
        rel = max(rel, float((diff / (ATOL + RTOL * np.abs(s64[:, :2 * Kg])))[live].max()))
    assert gap > factor * err, (gap, err, what)
    return {"gap": gap, "err": err, "rel": rel, "ref": o32}


# ---------------------------------------------------------------------------------------------- the model fixtures
MODELS = ("transformer", "rnnsearch")
SETTINGS = ((4, 2, 0.5), (4, 4, 0.5), (6, 3, 0.5), (4, 2, 8.0))      # (K, G, lambda); 8.0: the groups' first tokens differ
# The seeds with the widest smallest gap / err over SETTINGS among the seeds 1 .. 79 (margin() at factor 4): transformer 28
# gap / err >= 260; rnnsearch (bidirectional encoder, as tests/ngram_ref.py) 62, gap / err >= 13 -- the widest among the seeds
# whose x 6 sharpened model also keeps its best hypotheses under the bf16 storage model at every setting (75, the widest
# without that condition, does not).
SEEDS = {"transformer": 28, "rnnsearch": 62}
# one combination each, (K, G, lambda) = SETTINGS[0]: the model it runs on and gap / err of the wrapped reference there
# (transformer + no_repeat_ngram_size = 2: 71; rnnsearch + sampling_topk = 5: 57; rnnsearch under the n-gram ban has 7, so
# that combination runs on the transformer)
COMBOS = {"ngram": ("transformer", 2), "topk": ("rnnsearch", 5)}


def combo_fns(kind, fns, K):
    """The decoding functions of a combination: the n-gram ban (tests/ngram_ref.constrained) or the top-k truncation
    (tests/sampling_ref.truncated) around the model's."""
    from tests import ngram_ref as N
    from tests import sampling_ref as S
    return N.constrained(fns, COMBOS[kind][1]) if kind == "ngram" else S.truncated(fns, COMBOS[kind][1], 0.0, K)


def fixture(model, seed=None):
    """-> (hp, src, Pn, decoding_fns) of the model's tiny fixture (tests/ngram_ref.py's: H = 128, sources of 14, 5, 9, 11)."""
    from tests import ngram_ref as N
    hp, src = N.fixture(model)
    Pn = N.MODELS[model]["init"](hp, SEEDS[model] if seed is None else seed)
    return hp, src, Pn, N.MODELS[model]["fns"]


def first_tokens(groups_seq, G):
    """[B G, Kg, T] -> [B, G]: the first token of every group's best hypothesis."""
    return groups_seq[:, 0, 0].reshape(-1, G)
