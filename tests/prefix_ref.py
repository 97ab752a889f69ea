"""tgt_prefix_file: the rule, stated once (a plain module, no pytest in it; CPU only).  zk_prefix_force
(zero_amd/csrc/zk_prefix.hip), models/_decode.py search_tail and the eager routes of zero_amd/search.py follow this file.

The rule.  Sentence b has a prefix p_b[0 .. n_b - 1] of target ids in [1, V), EOS not among them; n_b = 0: none.  The table
prefix [B, P] holds it right-padded with 0.  At decode step t (the step that chooses y_{t+1}) every beam row r of sentence
b = r // K (K: the model's beam_size; the groups of a diverse beam share the sentence's prefix) with t < n_b gets

    logits[r, v]      = -INF       for v != p_b[t], v != eos      (INF = utils/dtype.py inf() = 1e8, the tail's forbid value)
    logits[r, eos]    = -2 INF
    logits[r, p_b[t]]              untouched, bit for bit

Rows with t >= n_b and the columns V .. ld - 1 are untouched, bit for bit.  The overwrite is the LAST thing ahead of the search
tail (temperature, log-softmax, the step-0 EOS ban, the length penalty, the top-2K): after the n-gram ban, the truncation and
the Gumbel noise, so whatever those wrote into the other entries is gone.  The log-softmax then gives the forced token exactly
0: exp(-1e8 - x) is 0 in fp32 and in float64, so the row's log-sum-exp IS the forced logit.  A hypothesis' score is therefore
log P(continuation | prefix) under the usual length penalty (fairseq keeps the model's probability of the prefix).

The one thing the force cannot undo: "untouched" means the forced entry keeps what the launches before it left there.  If the
n-gram ban took the forced token ITSELF, the entry holds -INF like the fillers, ties with them and loses to the lower indices
(`step`, test_prefix_checker.py).  During its prefix a row's history is the prefix, so that happens exactly when the prefix holds
an n-gram twice; zero_amd refuses such a prefix before the encoder pass (models/_decode.py check_prefix_ngram).  Every other
ban of a prefix step hits an entry the force overwrites anyway.  The truncation of sampling_topk / sampling_topp takes a forced
token outside its kept set in the same way, and which tokens those are is not known beforehand: a step with a truncation
therefore forces twice, ahead of the truncation and ahead of the tail (`step_truncated`).

Why EOS goes lower.  During its prefix a sentence has ONE real candidate per step; the other 2K - 1 slots of the top-2K fill
with candidates at about -1e8, which tie after fp32 rounding, and the lowest index wins a tie: EOS, id 2, would be one of the
first.  It would land on the finished list, change the stop test and could surface in an n-best list.  At -2e8 it loses to
every other filler, and V >= 2K + 2 leaves enough of those.  The fillers that stay alive carry -1e8 and are displaced at the
sentence's first free step, when the real row alone supplies 2K real candidates (test_prefix_checker.py shows both facts from
the reference search alone).  Which fillers stay alive until then depends on fp32 rounding of equal scores and is nobody's
business: no output depends on it.

``force`` / ``step``          the rule in numpy (DEFECTS: the ways to get it wrong; CASES: where each one shows)
``constrained``               a model's restated decoding_fns with the rule, for oracle.ref_torch.beam_search; composes with
                              ngram_ref.constrained (the ban inside, the force outside: the force comes last)
``starts_with`` / ``ends_inside``   the properties the option guarantees
``free_margin``               variant_ref.candidate_margin on the FREE steps of a constrained search
``fixture`` / ``make_fixture``     ngram_ref's tiny models with PREFIX_LENGTHS = (0, 1, 3, 2) and what the REFERENCE ALONE shows

make_fixture, measured on the CPU at beams 1 and 4 (tests/test_prefix_checker.py re-measures and asserts; the seed of each model
is the lowest of 1 .. 79 that passes every assertion of make_fixture):

%(FIGURES)s

gap: the smallest difference, on free steps, between a kept real candidate and its runner-up; err: the largest |score_fp32 -
score_float64| over the kept real candidates of every step (required: gap > 4 err); rel: err as a share of the project's fp32
score tolerance (required: <= 0.25, so that tolerance is the GPU tests'); forced: the largest |log-probability| a forced step
added to a hypothesis (required: exactly 0).
"""
import numpy as np
import torch

from oracle import ref_torch as rt
from tests import ngram_ref as N
from tests import variant_ref as V

INF = N.INF          # utils/dtype.py inf() of float32: a forced row holds -INF, -2 INF at EOS
REAL = -1e7          # a score above this belongs to a real candidate, one below to a filler (or to an empty slot)
DEFECTS = ("row_mod_k", "t_plus_1", "t_minus_1", "eos_kept", "forced_rewritten", "pad_columns", "next_sentence", "resumed",
           "before_ngram")
FIGURES = """    transformer                seed  1:  gap 6.50e-04  err 4.8e-06  rel 0.053  forced 0.0 over 12 forced steps
    transformer_aan            seed  1:  gap 5.10e-05  err 3.3e-06  rel 0.064  forced 0.0 over 12 forced steps
    rnnsearch (bidirectional)  seed  1:  gap 3.43e-05  err 7.6e-06  rel 0.024  forced 0.0 over 12 forced steps
    rnnsearch_deepatt (gru)    seed  5:  gap 3.62e-05  err 7.6e-06  rel 0.031  forced 0.0 over 12 forced steps

(rnnsearch_deepatt: the seeds 1 .. 4 fail gap > 4 err, seed 1 with 1.29e-05 against 3.8e-06.)"""
__doc__ = __doc__ % dict(FIGURES=FIGURES)


# ---------------------------------------------------------------------------------------------- the rule
def lengths(prefix):
    """n_b of a right-padded table [B, P]."""
    return (np.asarray(prefix) != 0).sum(1)


def token_at(prefix, b, t, defect=None):
    """The token sentence b is forced to at step t, or 0 (not forced)."""
    prefix = np.asarray(prefix)
    if defect == "t_plus_1":
        t = t + 1
    if defect == "t_minus_1":
        t = t - 1
    if not 0 <= t < prefix.shape[1]:
        return 0
    tok = int(prefix[b, t])
    if defect == "resumed" and tok == 0:          # the prefix starts over behind its padding
        n = int((prefix[b] != 0).sum())
        tok = int(prefix[b, t % n]) if n > 0 else 0
    return tok


def force(logits, V_, prefix, t, K, value, eos, defect=None):
    """A copy of logits [rows, ld] with the rule applied at step t: prefix int [rows / K, P], value = -INF, eos < 0: no entry
    is lowered.  A token <= 0 or >= V_ forces nothing."""
    out = np.array(logits, copy=True)
    rows = out.shape[0]
    assert rows % K == 0 and np.asarray(prefix).shape[0] == rows // K
    B = rows // K
    for r in range(rows):
        b = r // K
        if defect == "row_mod_k":
            b = (r % K) % B
        if defect == "next_sentence":             # the first row of a sentence still belongs to the one before
            b = max(r - 1, 0) // K
        tok = token_at(prefix, b, t, defect)
        if tok <= 0 or tok >= V_:
            continue
        keep = out[r, tok].copy()
        width = out.shape[1] if defect == "pad_columns" else V_
        out[r, :width] = value
        if eos >= 0 and defect != "eos_kept":
            out[r, eos] = 2.0 * value
        out[r, tok] = 0.0 if defect == "forced_rewritten" else keep
    return out


def step(logits, V_, prefix, t, K, eos, hist=None, n=0, defect=None):
    """The two overwrites of a step in their order: the n-gram ban (hist [rows, ldh], n > 0), then the force.  Defect
    "before_ngram": the other order -- a ban then rewrites entries of a forced row: a banned EOS is back at -INF, level with
    the fillers.  (In neither order does a forced token survive a ban of ITSELF, see the module docstring.)"""
    ban = (lambda x: N.apply(x, V_, hist, t, n, -INF)) if n > 0 else (lambda x: x)
    if defect == "before_ngram":
        return ban(force(logits, V_, prefix, t, K, -INF, eos))
    return force(ban(logits), V_, prefix, t, K, -INF, eos, defect)


def step_truncated(logits, V_, prefix, t, K, eos, topk, topp, min_keep, single=False):
    """A step with sampling_topk / sampling_topp (tests/sampling_ref.py): force, truncate, force.  The truncation alone would
    write -INF over a forced token outside its kept set, and "untouched" would then mean a tie with the fillers; ahead of it the
    force makes the forced entry the row's only real one, which every truncation keeps; the truncation drops EOS (the lowest
    entry) to -INF, and the last force puts it back to -2 INF.  single=True: the truncation and ONE force, to show the loss."""
    from tests import sampling_ref as S
    x = logits if single else force(logits, V_, prefix, t, K, -INF, eos)
    return force(S.apply(x, V_, topk, topp, min_keep), V_, prefix, t, K, -INF, eos)


def logprobs(x):
    """log-softmax over the last axis, in the dtype of x (the tail's)."""
    m = x.max(-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))


# where each defect shows at the level of the rule: name -> (prefix [B, P], t, K, V, ld).  B = 3 sentences of K = 2 rows,
# lengths 2, 0, 3.
_P = np.array([[7, 5, 0, 0], [0, 0, 0, 0], [3, 4, 6, 0]])
CASES = {
    "row_mod_k": (_P, 0, 2, 9, 9),            # row 1 is sentence 0, not sentence 1
    "t_plus_1": (_P, 1, 2, 9, 9),             # sentence 0 would be free already, sentence 2 forced to 6
    "t_minus_1": (_P, 2, 2, 9, 9),            # sentence 0 would still be forced
    "eos_kept": (_P, 0, 2, 9, 9),             # column 2 at -INF
    "forced_rewritten": (_P, 0, 2, 9, 9),
    "pad_columns": (_P, 0, 2, 9, 12),
    "next_sentence": (_P, 0, 2, 9, 9),        # row 2, the first of the free sentence 1, forced to 7
    "resumed": (_P, 2, 2, 9, 9),              # sentence 0 at t = 2: its prefix has ended
}


# ---------------------------------------------------------------------------------------------- the properties
def starts_with(row, prefix_row, hp):
    """Does the hypothesis in one row of a search's seq output start with the non-zero part of prefix_row."""
    want = [int(v) for v in prefix_row if int(v) != 0]
    return [int(v) for v in row[:len(want)]] == want


def ends_inside(row, prefix_row, hp):
    """Does the hypothesis end (EOS or padding) before its prefix is over."""
    n = int((np.asarray(prefix_row) != 0).sum())
    return len(N.hypothesis(row, hp)) < n


# ---------------------------------------------------------------------------------------------- the reference's search
def constrained(decoding_fns, prefix, K, defect=None):
    """decoding_fns(hp, P) -> (encoding_fn, decoding_fn) with the rule on the step's logits [B * K, V]; prefix int [B, P],
    K = the beam size the search will run with.  None or all-zero: decoding_fns itself."""
    if prefix is None or not np.asarray(prefix).any():
        return decoding_fns
    prefix = np.asarray(prefix)

    def fns(hp, P):
        enc, dec = decoding_fns(hp, P)
        eos = hp.tgt_vocab.eos()

        def decoding_fn(target, state, time):
            logits, step_state = dec(target, state, time)
            x = logits.detach().numpy()
            return torch.from_numpy(force(x, x.shape[-1], prefix, time, K, -INF, eos, defect)), step_state

        return enc, decoding_fn
    return fns


def with_ngram(decoding_fns, prefix, K, n, defect=None):
    """The rule together with no_repeat_ngram_size = n: the ban inside, the force outside (it runs last).  Defect
    "before_ngram": the other nesting."""
    if defect == "before_ngram":
        return N.constrained(constrained(decoding_fns, prefix, K), n)
    return constrained(N.constrained(decoding_fns, n), prefix, K, defect)


def free_margin(search_fn, hp, Pn, src, prefix, beams=(1, 4), factor=4.0, tol=None, seed=None):
    """variant_ref.candidate_margin for a constrained search.  search_fn(hp, Pn, src, K, dtype) -> (result, trace).  The
    float64 and the fp32 run give identical hypotheses on every beam; on every step and sentence the REAL candidates among
    the kept 2K (score > REAL) are the same in both, in the same order; on a forced step there is exactly one and it is the
    forced token of the sentence's live row.
      gap     the smallest difference, over the FREE steps of the float64 run, between a kept real candidate and its
              runner-up (a filler runner-up is 1e8 away)
      err     the largest |score_fp32 - score_float64| over the kept real candidates of every step
      rel     with tol = (ATOL, RTOL): the same as a share of ATOL + RTOL |score_float64|
    and gap > factor * err.  -> dict gap, err, rel, forced_steps."""
    n_b = lengths(prefix)
    gap, err, rel, forced_steps = np.inf, 0.0, 0.0, 0
    for K in beams:
        o64, t64 = search_fn(hp, Pn, src, K, torch.float64)
        o32, t32 = search_fn(hp, Pn, src, K, torch.float32)
        assert np.array_equal(o64["seq"], o32["seq"]), ("float64 and fp32 reference disagree", K, seed)
        assert len(t64) == len(t32)
        Vt = hp.tgt_vocab.size()
        for t, ((s64, i64), (s32, i32)) in enumerate(zip(t64, t32)):
            s64, s32 = np.maximum(s64.astype(np.float64), -1e35), np.maximum(s32.astype(np.float64), -1e35)
            for b in range(s64.shape[0]):
                live = s64[b, :2 * K] > REAL
                assert np.array_equal(live, s32[b, :2 * K] > REAL), ("real candidates differ", K, t, b, seed)
                assert np.array_equal(i64[b, :2 * K][live], i32[b, :2 * K][live]), ("candidate order differs", K, t, b, seed)
                if t < n_b[b]:
                    assert live.sum() == 1 and live[0] and i64[b, 0] % Vt == prefix[b, t], ("forced step", K, t, b, seed)
                    forced_steps += 1
                elif live.any():
                    g = np.where(live, s64[b, :2 * K] - s64[b, 1:2 * K + 1], np.inf)
                    gap = min(gap, float(g.min()))
                diff = np.abs(s64[b, :2 * K] - s32[b, :2 * K])
                if live.any():
                    err = max(err, float(diff[live].max()))
                    if tol is not None:
                        rel = max(rel, float((diff / (tol[0] + tol[1] * np.abs(s64[b, :2 * K])))[live].max()))
    assert gap > factor * err, (gap, err, seed)
    return {"gap": gap, "err": err, "rel": rel, "forced_steps": forced_steps}


MODELS = N.MODELS
SEEDS = {"transformer": 1, "transformer_aan": 1, "rnnsearch": 1, "rnnsearch_deepatt": 5}
LENGTHS = N.LENGTHS
PREFIX_LENGTHS = (0, 1, 3, 2)
RTOL, ATOL = N.RTOL, N.ATOL
score_tol = N.score_tol


def prefixes(vocab_size, lengths_=PREFIX_LENGTHS, seed=17):
    """The fixture's table [len(lengths_), max(lengths_)]: ids drawn from 3 .. vocab_size - 1, right-padded with 0.  (Whether
    the unconstrained best hypotheses start with them is make_fixture's to assert.)"""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(lengths_), max(1, max(lengths_))), dtype=np.int64)
    for b, n in enumerate(lengths_):
        out[b, :n] = rng.integers(3, vocab_size, n)
    return out


def fixture(model):
    """-> (hp, src, prefix) of the model's tiny fixture."""
    hp, src = N.fixture(model)
    return hp, src, prefixes(hp.tgt_vocab.size())


def forced_logprob(decoding_fns, hp, Pn, src, prefix, K):
    """The largest |accumulated log-probability| of a sentence's live hypothesis during its prefix, in the fp32 reference: a
    prefix starts at step 0 with log-probability 0, every forced step adds its token's log-probability, and the step's best
    score is that sum over the length penalty.  Exactly 0 under the rule."""
    _, trace = V.search(constrained(decoding_fns, prefix, K), hp, Pn, src, K, torch.float32)
    n_b = lengths(prefix)
    return max([abs(float(s[b, 0])) for t, (s, _) in enumerate(trace) for b in range(prefix.shape[0]) if t < n_b[b]] + [0.0])


def make_fixture(model, seed=None, factor=4.0):
    """The tiny model with what the REFERENCE ALONE shows on it under the rule, for beam 1 and 4: free_margin's assertions, the
    x 6 sharpened model keeps its best hypotheses under the bf16 storage model, every output hypothesis of every beam starts
    with its prefix and none ends inside it, no output score is below REAL, a forced step adds exactly 0, and no sentence's
    unconstrained best hypothesis (beam 4) starts with its prefix.
    -> dict hp, src, prefix, Pn, gap, err, rel, forced."""
    m = MODELS[model]
    hp, src, prefix = fixture(model)
    Pn = m["init"](hp, SEEDS[model] if seed is None else seed)
    runs = {K: (lambda *a, _f=constrained(m["fns"], prefix, K), **k: V.search(_f, *a, **k)) for K in (1, 4)}
    run = lambda hp_, Pn_, src_, K, dtype, **k: runs[K](hp_, Pn_, src_, K, dtype, **k)
    out = dict(hp=hp, src=src, prefix=prefix, Pn=Pn)
    out.update(free_margin(run, hp, Pn, src, prefix, factor=factor, tol=(ATOL, RTOL), seed=seed))
    Ps = V.sharpen(hp, Pn)
    for K in (1, 4):
        a, _ = run(hp, Ps, src, K, torch.float32)
        b, _ = run(hp, Ps, src, K, torch.float32, store_bf16=True)
        assert rt.decode_hypothesis(a["seq"], hp) == rt.decode_hypothesis(b["seq"], hp), ("bf16 storage model", K, seed)
        con, _ = run(hp, Pn, src, K, torch.float32)
        for s in range(src.shape[0]):
            for k in range(K):
                if con["score"][s, k] > -1e30:
                    assert con["score"][s, k] > REAL, (s, k, con["score"][s, k])
                    assert starts_with(con["seq"][s, k], prefix[s], hp), (s, k, seed)
                    assert not ends_inside(con["seq"][s, k], prefix[s], hp), (s, k, seed)
    plain, _ = V.search(m["fns"], hp, Pn, src, 4, torch.float32)
    for s in range(src.shape[0]):
        if prefix[s].any():
            assert not starts_with(plain["seq"][s, 0], prefix[s], hp), ("the unconstrained reference starts with the prefix", s, seed)
    out["forced"] = max(forced_logprob(m["fns"], hp, Pn, src, prefix, K) for K in (1, 4))
    assert out["forced"] == 0.0, out["forced"]
    return out
