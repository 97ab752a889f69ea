"""The numpy reference of lexical shortlist construction (a plain module, CPU only), its stand-ins with planted defects, and
the cases the kernel test runs (tests/test_gpu_shortlist_kernels.py) and the host test shows to have teeth
(tests/test_shortlist_host.py).

The definition (zero_amd/shortlist.py, include/zero_hip.h zk_shortlist_build):
  1. the ``first`` lowest target ids;
  2. for every source token s of the batch with 0 < s < Vsrc (0 = pad), the first min(best, len) entries of row s of the
     lexical table (entries outside [0, V) skipped);
  3. n = |S|, Vs = min(V, ceil(n / round) * round); the lowest ids not yet in S are added until |S| = Vs.
-> ids[0 .. Vs) = S ascending, ids[Vs .. cap) = -1, count = (n, Vs).
"""
import itertools

import numpy as np


def build(src, off, lex, first, best, V, round_to, cap, defect=None):
    """-> (ids int32 [cap], (n, Vs)).  defect: one of DEFECTS, a stand-in that is wrong in that one way."""
    src = np.asarray(src).reshape(-1)
    Vsrc = len(off) - 1
    member = np.zeros(V, dtype=bool)
    member[:min(first, V)] = True
    for s in src:
        if defect == "pad_counts":
            if not 0 <= s < Vsrc:
                continue
        elif not 0 < s < Vsrc:
            continue
        row = lex[off[s]:off[s + 1]]
        row = row if defect == "best_ignored" else row[:best]
        row = row[(row >= 0) & (row < V)]
        member[row] = True
    n = int(member.sum())
    Vs = -(-n // round_to) * round_to
    if defect == "not_rounded":
        Vs = n
    if defect != "not_capped":
        Vs = min(V, Vs)
    missing = np.flatnonzero(~member)
    need = max(0, min(Vs, V) - n)
    fill = missing[len(missing) - need:] if defect == "fill_from_top" else missing[:need]
    member[fill] = True
    S = np.flatnonzero(member)
    if defect == "unsorted" and len(S) > 4:
        S = np.concatenate([S[:3], S[3:][::-1]])
    ids = np.full(cap, 0 if defect == "tail_zero" else -1, dtype=np.int32)
    ids[:len(S)] = S
    return ids, (n, Vs)


DEFECTS = ("fill_from_top", "pad_counts", "best_ignored", "unsorted", "not_rounded", "not_capped", "tail_zero")


# ---------------------------------------------------------------------------------------------- the cases
VOCABS = (40, 64, 70, 4100, 33000)      # partial mask word, exact words, more words than a wave (4100 / 32 = 129), more than
#                                         a workgroup (33000 / 32 = 1032 words for 1024 threads)
BESTS = (0, 1, 3, 1000)
ROUNDS = (8, 64, 1024)
VSRC = 50


def firsts(V):
    return (3, 17, V)


def table(V, seed=0):
    """A lexical table over VSRC source ids: row 0 (pad) is NOT empty -- a kernel that does not skip pad shows; rows 7 and
    11 are empty; row 5 has a thousand entries; some entries lie outside [0, V)."""
    rng = np.random.default_rng(seed)
    rows = []
    for s in range(VSRC):
        if s in (7, 11):
            rows.append(np.zeros(0, dtype=np.int32))
            continue
        n = 1000 if s == 5 else int(rng.integers(1, 9))
        r = rng.integers(3, V, n).astype(np.int32)
        if s == 0:
            r = np.arange(V - 6, V, dtype=np.int32)          # pad's row: the six highest ids, nobody else's
        if s == 9:
            r[0] = V + 3                                      # outside the vocabulary
        if s == 13:
            r[-1] = -2
        rows.append(r)
    off = np.zeros(VSRC + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in rows])
    return off, np.concatenate(rows).astype(np.int32)


def sources():
    """name -> int32 [rows, Ls] (with a wider leading dimension in the kernel test)."""
    rng = np.random.default_rng(3)
    a = np.array([[4]], dtype=np.int32)
    b = np.array([[6, 9, 13, 0, 0], [0, 0, 0, 0, 0], [21, 5, 2, 0, 0]], dtype=np.int32)      # padding, an all-pad row
    c = rng.integers(1, VSRC, (8, 16)).astype(np.int32)
    c[:, 3] = c[:, 2]                       # repeated tokens
    c[0, :4] = (7, 11, VSRC + 5, -1)        # ids whose row is empty, and ids without a table row
    c[5, 10:] = 0
    return {"1x1": a, "3x5": b, "8x16": c}


def product():
    """The cases: (V, source name, best, first, round).  The full product of the five factors is 540; a third of the 36
    (best, first, round) triples runs per vocabulary -- a Latin slice: every (best, first) pair once, with the round that
    makes the three indices and the vocabulary's sum to a multiple of 3 -- so that every V meets every value of every
    factor and every triple runs at some V; the sources rotate along.  12 cases per V, plus the edge cases by
    construction.  tests/test_shortlist_host.py asserts the coverage."""
    out = []
    names = list(sources())
    for V in VOCABS:
        k = VOCABS.index(V)
        pick = [(b, fi, r) for b, fi, r in itertools.product(range(len(BESTS)), range(3), range(len(ROUNDS)))
                if (b + fi + r + k) % 3 == 0]
        for i, (b, fi, r) in enumerate(pick):
            out.append((V, names[(i + b + k) % len(names)], BESTS[b], firsts(V)[fi], ROUNDS[r]))
    # the edge cases by construction: n an exact multiple of round (nothing filled) and a roundup beyond V (Vs = V)
    out.append((64, "1x1", 0, 16, 8))          # n = first = 16 = 2 x 8: nothing filled
    out.append((70, "3x5", 3, 17, 64))         # a fill up to 64 < V
    out.append((70, "8x16", 1000, 17, 64))     # n > 64: the roundup, 128, lies beyond V = 70 -> Vs = V
    out.append((40, "8x16", 3, 3, 1024))       # roundup 1024 > V
    return out


def case_inputs(case):
    V, name, best, first, rnd = case
    off, lex = table(V)
    return sources()[name], off, lex
