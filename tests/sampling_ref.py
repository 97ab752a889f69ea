"""sampling_topk / sampling_topp: the rule, stated once (a plain module, no pytest in it; CPU only, float64).
zk_sample_truncate (zero_amd/csrc/zk_sample.hip) and the host code of zero_amd/models/_decode.py / search.py follow this file.

The rule.  For one beam row let x be its V finite logits, s = softmax(x), c(v) = #{u : x_u > x_v} and M(v) = the sum of s_u over
x_u > x_v.  Token v is KEPT iff

    c(v) < min_keep   or   ( (topk == 0 or c(v) < topk)  and  (topp == 0 or M(v) < topp) )

and every other entry of the row is overwritten with -inf(), the finite -1e8 of utils/dtype.py.  Whether a token is kept
depends on its value alone and the predicate only turns false as the value falls, so the kept set is {v : x_v >= tau} for one
threshold per row: tied tokens share their fate and nothing depends on how a tie falls.  M(v) < topp is the usual nucleus (the
smallest prefix of the descending order whose mass reaches p); topp = 1 keeps everything (M(v) < 1 for finite logits -- `kept`
says so outright instead of leaving it to an exp() that underflows).  The mass is measured on softmax(x) of the RAW logits, not
after beam_search_temperature: the reference divides by the temperature after the noise (search.py:143-146), so the temperature
does not change which token a beam-1 Gumbel draw selects, and softmax(x) is the distribution that draw samples from.
min_keep = 2 * beam_size + 1 comes from the host: the top-2K of a step never has to take an overwritten entry, with the step-0
EOS ban on top.

Order inside a step: n-gram ban (banned tokens sit at -1e8: mass 0, the lowest rank), truncation, Gumbel noise, fused tail
(temperature, log-softmax over what is left, EOS ban, length penalty, top-2K).

``kept`` / ``apply``            the rule in numpy (DEFECTS: the ways to get it wrong; CASES: where each one shows)
``step``                       a step's order: truncate, then noise (defects: the mass after the temperature, the noise first)
``mass_delta`` / ``classify``  the band: which tokens a device that sums fp32 expf() terms in fixed point must agree on
``check_mask`` / ``check``     a device result against the rule: decided tokens agree, the kept set is a threshold set, kept
                               entries are bit-identical, dropped entries equal the value, columns >= V untouched
``truncated``                  a model's restated decoding_fns with the truncation, for oracle.ref_torch.beam_search
``make_fixture``               the tiny models of the GPU model tests and what the REFERENCE ALONE shows on them

The band.  The kernel's mass of token i is q_i = rint(expf(fl(x_i - max)) * 2^S) with S = min(40, 62 - ceil(log2 V)), summed
in 64-bit integers (exactly), and it keeps v iff Mq(v) < topp * Tq with that product rounded once in double.  Against
e_i = exp(x_i - max) in exact arithmetic:
  * the fp32 subtraction errs by at most half an ulp of d_i = x_i - max: a relative error of |d_i| 2^-24 in e_i;
  * expf is taken as accurate to 2 ulp, a relative 2^-22 (the math library documents 1 ulp);
  * the rounding to a multiple of 2^-S adds at most 2^-(S+1) per term, V quanta halves for the row;
so the row's total T = sum e_i is off by at most E = sum e_i (|d_i| 2^-24 + 2^-22) + V 2^-(S+1), any partial sum by no more,
and |Mq / Tq - M / T| <= 2 E / (T - E).  One rounding of topp * Tq in double adds 2^-52 relative.  delta = 2 E / (T - E) +
2^-50: a token is decided-kept when M(v) < topp - delta, decided-dropped when M(v) >= topp + delta, undecided in between.  For
top-k the device compares integers: with exact inputs (the kernel's fp32 logits) nothing is undecided; with inputs known to
x_err only (a model's logits), a token is undecided when moving values by x_err could carry it across rank k.
"""
import numpy as np
import torch

from tests import ngram_ref as N
from tests import variant_ref as V

INF = 1e8            # utils/dtype.py inf() of float32: the truncation writes -INF


def f32(p):
    """p as the device gets it."""
    return float(np.float32(p))


EXPF_REL = 2.0 ** -22
DEFECTS = ("k_off_by_one", "tie_split", "mass_le", "no_min_keep")
STEP_DEFECTS = ("after_temperature", "after_noise")


def min_keep_of(K):
    return 2 * int(K) + 1


def fixed_point_bits(V_):
    """S of the kernel's fixed-point masses: V terms of at most 2^S stay below 2^63."""
    lg = 0
    while (1 << lg) < int(V_):
        lg += 1
    return min(40, 62 - lg)


# ---------------------------------------------------------------------------------------------- the rule
def rank_mass(x):
    """c(v), M(v) and softmax(x) in float64 along the last axis of x ([V] or [rows, V]); ties share c and M (strictly greater
    values only)."""
    x = np.asarray(x, np.float64)
    x2 = x.reshape(-1, x.shape[-1])
    n = x2.shape[1]
    order = np.argsort(-x2, axis=1, kind="stable")
    xs = np.take_along_axis(x2, order, 1)
    e = np.exp(xs - xs[:, :1])
    s = e / e.sum(1, keepdims=True)
    first = np.concatenate([np.ones((x2.shape[0], 1), bool), xs[:, 1:] != xs[:, :-1]], 1)     # the first entry of a run of ties
    start = np.maximum.accumulate(np.where(first, np.arange(n)[None, :], 0), axis=1)          # where an entry's run starts
    before = np.concatenate([np.zeros((x2.shape[0], 1)), np.cumsum(s, 1)[:, :-1]], 1)         # the mass ahead of a position
    c, M, sm = np.empty(x2.shape, np.int64), np.empty(x2.shape), np.empty(x2.shape)
    np.put_along_axis(c, order, start, 1)
    np.put_along_axis(M, order, np.take_along_axis(before, start, 1), 1)
    np.put_along_axis(sm, order, s, 1)
    return c.reshape(x.shape), M.reshape(x.shape), sm.reshape(x.shape)


def kept(x, topk, topp, min_keep, defect=None):
    """The kept tokens along the last axis of x ([V] or [rows, V]) -> bool, the shape of x."""
    x = np.asarray(x, np.float64)
    c, M, _ = rank_mass(x)
    if defect == "tie_split":          # ranks by position in a stable sort: tied tokens get different ranks
        c = np.argsort(np.argsort(-x, axis=-1, kind="stable"), axis=-1, kind="stable")
    k_ok = np.ones(x.shape, bool) if topk == 0 else (c < topk + (1 if defect == "k_off_by_one" else 0))
    if topp == 0 or topp >= 1.0:
        p_ok = np.ones(x.shape, bool)
    else:
        p_ok = (M <= topp) if defect == "mass_le" else (M < topp)
    floor = np.zeros(x.shape, bool) if defect == "no_min_keep" else (c < min_keep)
    return floor | (k_ok & p_ok)


def apply(logits, V_, topk, topp, min_keep, value=-INF, defect=None):
    """A copy of logits [rows, ld] with the dropped entries among the first V_ columns of every row set to `value`."""
    out = np.array(logits, copy=True)
    if topk == 0 and topp == 0:
        return out
    k = kept(out[:, :V_], topk, topp, min_keep, defect)
    out[:, :V_][~k] = value
    return out


def step(x, topk, topp, min_keep, temperature=1.0, noise=None, defect=None):
    """What a step hands to the tail for ONE row: truncate, then add the noise.  Defects: "after_temperature" measures the
    mass on softmax(x / temperature); "after_noise" truncates x + noise."""
    x = np.asarray(x, np.float64)
    g = np.zeros_like(x) if noise is None else np.asarray(noise, np.float64)
    if defect == "after_noise":
        y = x + g
        return np.where(kept(y, topk, topp, min_keep), y, -INF)
    k = kept(x / temperature if defect == "after_temperature" else x, topk, topp, min_keep)
    return np.where(k, x + g, -INF)


# ---------------------------------------------------------------------------------------------- the band
def mass_delta(x):
    """delta of the module docstring per row of (fp32) logits: [rows, 1] for [rows, V], a float for [V]."""
    x = np.asarray(x, np.float64)
    d = x - x.max(-1, keepdims=True)
    e = np.exp(d)
    S = fixed_point_bits(x.shape[-1])
    E = (e * (np.abs(d) * 2.0 ** -24 + EXPF_REL)).sum(-1, keepdims=True) + x.shape[-1] * 2.0 ** -(S + 1)
    T = e.sum(-1, keepdims=True)
    out = 2.0 * E / (T - E) + 2.0 ** -50
    return out if x.ndim > 1 else float(out[0])


class Band(object):
    """rank_mass and mass_delta of a block of rows, computed once and shared by every setting it is asked about."""

    def __init__(self, x, delta=None, x_err=0.0):
        self.x = np.asarray(x, np.float64)
        self.c, self.M, _ = rank_mass(self.x)
        self.delta = mass_delta(self.x) if delta is None else delta
        self.x_err = float(x_err)
        if self.x_err > 0.0:
            n = self.x.shape[-1]
            x2 = self.x.reshape(-1, n)
            lo, hi = np.empty(x2.shape, np.int64), np.empty(x2.shape, np.int64)
            for r in range(x2.shape[0]):
                xs = np.sort(x2[r])
                lo[r] = n - np.searchsorted(xs, x2[r] + 2 * self.x_err, side="right")        # the values surely above
                hi[r] = n - np.searchsorted(xs, x2[r] - 2 * self.x_err, side="right") - 1    # possibly above (not itself)
            self.c_lo, self.c_hi = lo.reshape(self.x.shape), hi.reshape(self.x.shape)
        else:
            self.c_lo = self.c_hi = self.c

    def classify(self, topk, topp, min_keep):
        """-> (decided_kept, decided_dropped) bool, the shape of x; what is in neither is undecided.  topp: the number the
        device is handed (a caller that passes an fp32 rounds it first: f32(topp))."""
        shape = self.x.shape
        if topk == 0:
            k_yes, k_no = np.ones(shape, bool), np.zeros(shape, bool)
        else:
            k_yes, k_no = self.c_hi < topk, self.c_lo >= topk
        if topp == 0 or topp >= 1.0:
            p_yes, p_no = np.ones(shape, bool), np.zeros(shape, bool)
        else:
            p_yes, p_no = self.M < topp - self.delta, self.M >= topp + self.delta
        return (self.c_hi < min_keep) | (k_yes & p_yes), (self.c_lo >= min_keep) & (k_no | p_no)

    def undecided(self, topk, topp, min_keep):
        """The undecided tokens per row."""
        a, b = self.classify(topk, topp, min_keep)
        return (~a & ~b).sum(-1)


def classify(x, topk, topp, min_keep, delta=None, x_err=0.0):
    return Band(x, delta, x_err).classify(topk, topp, min_keep)


def check_mask(x, kept_obs, topk, topp, min_keep, known=None, what="", band=None):
    """kept_obs (bool, [V] or [rows, V]) against the rule: every decided token agrees, and the kept set of a row is a threshold
    set (no dropped value >= a kept value: ties are together).  known: the tokens whose state could be observed (default
    all)."""
    band = Band(x) if band is None else band
    x = band.x.reshape(-1, band.x.shape[-1])
    kept_obs = np.asarray(kept_obs, bool).reshape(x.shape)
    known = np.ones(x.shape, bool) if known is None else np.asarray(known, bool).reshape(x.shape)
    yes, no = (m.reshape(x.shape) for m in band.classify(topk, topp, min_keep))
    for bad, text in ((known & yes & ~kept_obs, "kept by the rule and was dropped"),
                      (known & no & kept_obs, "dropped by the rule and was kept")):
        if bad.any():
            r, v = np.argwhere(bad)[0]
            raise AssertionError("%s: row %d token %d (value %r, c %d, M %.9g) is %s"
                                 % (what, r, v, x[r, v], band.c.reshape(x.shape)[r, v], band.M.reshape(x.shape)[r, v], text))
    k, d = known & kept_obs, known & ~kept_obs
    lowest_kept = np.where(k, x, np.inf).min(1)
    highest_dropped = np.where(d, x, -np.inf).max(1)
    bad = highest_dropped >= lowest_kept
    assert not bad.any(), "%s: row %d: not a threshold set: a dropped value %r >= a kept value %r" \
        % (what, np.argmax(bad), highest_dropped[np.argmax(bad)], lowest_kept[np.argmax(bad)])


def check(before, after, V_, topk, topp, min_keep, value=-INF, what="", band=None):
    """A device result against the rule.  before / after: fp32 [rows, ld].  Kept entries are bit-identical to the input,
    dropped ones equal `value`, the columns V_ .. ld-1 are untouched, and check_mask holds.  An entry that held `value`
    before the call looks the same kept or dropped: it must still hold it, and is left out of the set checks.  band: the
    Band of before[:, :V_], where the caller shares it between settings."""
    b = np.ascontiguousarray(before, np.float32)
    a = np.ascontiguousarray(after, np.float32)
    assert a.shape == b.shape
    bb, ab = b.view(np.int32), a.view(np.int32)
    assert np.array_equal(ab[:, V_:], bb[:, V_:]), "%s: a column >= V = %d was written" % (what, V_)
    vbits = np.float32(value).view(np.int32)
    same = ab[:, :V_] == bb[:, :V_]
    bad = ~same & (ab[:, :V_] != vbits)
    if bad.any():
        r, v = np.argwhere(bad)[0]
        raise AssertionError("%s: row %d column %d holds %r: neither its input %r nor the value" % (what, r, v, a[r, v], b[r, v]))
    if topk == 0 and topp == 0:
        assert same.all(), "%s: the option is off and an entry changed" % what
        return
    check_mask(b[:, :V_], same, topk, topp, min_keep, known=bb[:, :V_] != vbits, what=what, band=band)


# named cases where each defect of `kept` changes the kept set: name -> (x, topk, topp, min_keep); they are exact (checked
# with delta = 0).  "mass_le" puts topp ON the mass of the third token, as this module computes it
_GEO = -np.arange(12) * np.log(2.0)                      # s ~ 1/2, 1/4, ..: M ~ 0, 1/2, 3/4, 7/8, ..
CASES = {
    "k_off_by_one": (np.array([9., 8., 7., 6., 5., 4.]), 3, 0.0, 1),              # {9, 8, 7} -> {9, 8, 7, 6}
    "tie_split": (np.array([9., 7., 7., 7., 5., 4.]), 2, 0.0, 1),                 # {9, 7, 7, 7} -> {9, 7}
    "mass_le": (_GEO, 0, float(rank_mass(_GEO)[1][2]), 1),                       # M = 0, .5 -> plus the token with M = topp
    "no_min_keep": (_GEO, 0, 0.4, 3),                                            # three by min_keep -> one
}


# ---------------------------------------------------------------------------------------------- the kernel test's cases
LDS_MAX_V = 32768        # zk_sample.hip stages rows of up to this many logits on chip; longer ones are re-read per pass
SHAPES = ((1, 4), (37, 40), (255, 256), (257, 264), (1000, 1000), (32000, 32000), (LDS_MAX_V, LDS_MAX_V),
          (LDS_MAX_V + 1, LDS_MAX_V + 8),
          # a stride that is no multiple of 4 words: the kernel then reads word by word, staged and not
          (37, 39), (32001, 32003), (LDS_MAX_V + 1, LDS_MAX_V + 3))                      # (V, ld)
ROWS = (1, 5, 128)
VARIANTS = {"plain": 5.0, "peaked": 20.0, "flat": 0.1}
TOPPS = (1e-6, 0.1, 0.5, 0.9, 0.999, 1.0)
MIN_KEEPS = (1, 3, 9)


def topks(V_):
    return tuple(k for k in (1, 2, 9, 10, V_ - 1, V_, V_ + 7) if k >= 1)


def random_cases():
    """(rows, V, ld, variant) of the random-input kernel cases: every shape and row count with randn * 5; the peaked and the
    flat variant on 5 rows; the 128-row blocks of the three longest rows stay with the plain variant (the checker's sort of
    128 x 32000 float64 values is what takes the time)."""
    out = []
    for V_, ld in SHAPES:
        out += [(rows, V_, ld, "plain") for rows in ROWS]
        out += [(5, V_, ld, v) for v in ("peaked", "flat")]
    return out


def random_logits(rows, V_, variant, seed=None):
    """fp32 [rows, V_]: randn * the variant's scale, from a seed fixed by the case."""
    seed = 1000 * rows + V_ + sorted(VARIANTS).index(variant) if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, V_, generator=g) * VARIANTS[variant]).to(torch.float32)


def random_settings(rows, V_):
    """(topk, topp, min_keep) of a random case: top-k alone, top-p alone, both where either may bind.  Rows of up to 1000
    logits take every min_keep with every setting; the long ones cycle through them, and their 128-row blocks take every
    third setting."""
    both = [(10, 0.9), (2, 0.999), (V_ + 7, 0.1), (9, 0.5), (1, 1.0), (V_, 1e-6)]
    base = [(k, 0.0) for k in topks(V_)] + [(0, p) for p in TOPPS] + both
    if V_ <= 1000:
        return [(k, p, mk) for k, p in base for mk in MIN_KEEPS]
    return [(k, p, MIN_KEEPS[i % 3]) for i, (k, p) in enumerate(base[::3] if rows > 5 else base)]


CONSTRUCTED_SHAPES = ((37, 40), (257, 264), (32000, 32000), (LDS_MAX_V + 1, LDS_MAX_V + 8), (32001, 32003))


def constructed(kind, V_):
    """The by-construction kernel cases: -> (x fp32 [5, V_], [(topk, topp, min_keep, kept tokens per row or None), ..]).
      ties        distinct integers 0, -1, .. shuffled, the value at ranks k - 1 .. k + 2 of row r (k = 3 + r) held by four
                  tokens: top-k with that k keeps all four, k + 3 tokens in that row;
      equal       every entry 0.375: everything is kept whatever the setting;
      two_level_50 / two_level_3   row r holds j = r + 2 zeros, the rest -50 (mass ~ 1e-17) resp. -3.  At -50 any p up to 0.999
                  keeps the zeros only.  At -3 the zeros hold m = j / (j + (V - j) e^-3) of the mass; the settings are per row
                  r: p = m / 2 keeps j tokens, p = (1 + m) / 2 everything -- wide of the boundary on either side;
      geometric   x_i = -i ln 2 shuffled: s = 1/2, 1/4, ..; M = 0, 1/2, 3/4: p = 0.7 keeps two tokens with min_keep 1, three
                  with min_keep 3;
      prebanned   randn * 5 with a third of every row at -1e8 (what the n-gram ban leaves) -- those stay, and the others are
                  ranked and weighed as if they were not there."""
    rng = np.random.default_rng(V_ + sorted(("ties", "equal", "two_level_50", "two_level_3", "geometric", "prebanned")).index(kind))
    rows = 5
    if kind == "ties":
        x = np.empty((rows, V_), np.float32)
        for r in range(rows):
            vals = -np.arange(V_, dtype=np.float32)
            k = 3 + r
            vals[k - 1:k + 3] = vals[k - 1]
            x[r] = rng.permutation(vals)
        return x, [(3 + r, 0.0, 1, {r: 6 + r}) for r in range(rows)]
    if kind == "equal":
        return np.full((rows, V_), 0.375, np.float32), [(1, 0.0, 1, V_), (0, 1e-6, 1, V_), (1, 0.5, 1, V_)]
    if kind in ("two_level_50", "two_level_3"):
        low = -50.0 if kind == "two_level_50" else -3.0
        x = np.full((rows, V_), low, np.float32)
        sets = []
        for r in range(rows):
            j = r + 2
            x[r, rng.choice(V_, j, replace=False)] = 0.0
            m = j / (j + (V_ - j) * np.exp(low))
            sets.append((0, 0.5 * m, 1, {r: j}))
            sets.append((0, 0.999, 1, {r: j}) if low < -10 else (0, 0.5 * (1 + m), 1, {r: V_}))
        return x, sets
    if kind == "geometric":
        base = (-np.arange(V_) * np.log(2.0)).astype(np.float32)
        return np.stack([rng.permutation(base) for _ in range(rows)]), [(0, 0.7, 1, 2), (0, 0.7, 3, 3)]
    assert kind == "prebanned"
    x = random_logits(rows, V_, "plain", seed=V_ + 3).numpy()
    banned = rng.random((rows, V_)) < 1.0 / 3
    banned[:, :12] = False
    x[banned] = -INF
    return x, [(10, 0.0, 1, 10), (0, 0.5, 3, None), (4, 0.9, 9, None)]


CONSTRUCTED = ("ties", "equal", "two_level_50", "two_level_3", "geometric", "prebanned")


# ---------------------------------------------------------------------------------------------- the reference's search
def truncated(decoding_fns, topk, topp, K, log=None):
    """decoding_fns(hp, P) -> (encoding_fn, decoding_fn) with the truncation on the step's logits (min_keep = 2 K + 1).  It
    wraps ngram_ref.constrained's result where both options are on: the ban comes first.  log: a list that receives
    (logits float64 [rows, V], kept bool [rows, V]) of every step."""
    if topk == 0 and topp == 0:
        return decoding_fns
    mk = min_keep_of(K)

    def fns(hp, P):
        enc, dec = decoding_fns(hp, P)

        def decoding_fn(target, state, time):
            logits, state = dec(target, state, time)
            x = logits.detach().cpu().numpy().astype(np.float64)
            k = kept(x, topk, topp, mk)
            if log is not None:
                log.append((x, k))
            logits = logits.clone()
            logits[torch.as_tensor(~k)] = -INF
            return logits, state

        return enc, decoding_fn
    return fns


SETTINGS = ((5, 0.0), (0, 0.4), (10, 0.4))        # (sampling_topk, sampling_topp) of the model tests
WITH_NGRAM = (3, (0, 0.4))       # (no_repeat_ngram_size, setting) of the combination test: of the settings x n in {2, 3} the one
                                 # whose candidate gaps exceed 4 x the fp32 error on all three models (10 x and more)
MODELS = ("transformer", "transformer_aan", "rnnsearch")
RTOL, ATOL = N.RTOL, N.ATOL


def fns_of(model, topk, topp, K, ngram=0, log=None):
    return truncated(N.constrained(N.MODELS[model]["fns"], ngram), topk, topp, K, log)


def decisions_decided(log64, log32, topk, topp, K, factor=4.0):
    """Every threshold decision of a float64 run is decided at factor x the fp32 error: the fp32 run takes the same decisions,
    the value gap at rank k exceeds factor x 2 x the largest logit difference and every mass is further from topp than factor
    x the largest mass difference.  -> (smallest value gap, largest logit error, smallest mass gap, largest mass error)"""
    mk = min_keep_of(K)
    gx, ex, gm, em = np.inf, 0.0, np.inf, 0.0
    assert len(log64) == len(log32)
    for (x64, k64), (x32, k32) in zip(log64, log32):
        assert np.array_equal(k64, k32), "the fp32 and the float64 reference truncate differently"
        live = np.abs(x64).max(axis=1) < 1e30
        for r in np.nonzero(live)[0]:
            fin = x64[r] > -1e7                 # (entries the n-gram ban took are far from every threshold)
            ex = max(ex, float(np.abs(x64[r] - x32[r])[fin].max()))
            c, M, s64 = rank_mass(x64[r])
            s32 = rank_mass(x32[r])[2]
            xs = np.sort(x64[r])[::-1]
            for k in sorted({mk} | ({topk} if topk else set())):
                if k < xs.size and xs[k - 1] != xs[k]:
                    gx = min(gx, float(xs[k - 1] - xs[k]))
            if 0 < topp < 1:
                # the mass of the first j tokens in rank order, for every j (per token the mass ahead of it moves by a whole
                # token's mass when two near-tied tokens swap ranks, far from the threshold or not)
                em = max(em, float(np.abs(np.cumsum(-np.sort(-s64)) - np.cumsum(-np.sort(-s32))).max()))
                gm = min(gm, float(np.abs(M - f32(topp)).min()))
    assert gx > factor * 2 * ex, (gx, ex)
    assert gm > factor * em, (gm, em)
    return gx, ex, gm, em


def make_fixture(model, settings=SETTINGS, beams=(1, 4)):
    """The tiny model of tests/ngram_ref.py (same seeds) with what the REFERENCE ALONE shows on it under every setting and
    beam: candidate_margin (float64 and fp32 token- and order-identical, gaps > 4 x the fp32 score error), decisions_decided,
    the x 6 sharpened model keeps its best hypotheses under the bf16 storage model, and `changed`: the sentences whose best
    hypothesis or beam order (the hypotheses in rank order) differs from the untruncated search at beam 4.  "with_ngram":
    candidate_margin of the WITH_NGRAM combination (ban first, then the truncation)."""
    hp, src = N.fixture(model)
    Pn = N.MODELS[model]["init"](hp, N.SEEDS[model])
    Ps = V.sharpen(hp, Pn)
    out = dict(hp=hp, src=src, Pn=Pn)
    plain, _ = V.search(N.MODELS[model]["fns"], hp, Pn, src, 4, torch.float32)
    for topk, topp in settings:
        f = V.candidate_margin(lambda hp_, P_, s_, K, dt: V.search(fns_of(model, topk, topp, K), hp_, P_, s_, K, dt), hp, Pn, src,
                               beams=beams, tol=(ATOL, RTOL))
        for K in beams:
            l64, l32 = [], []
            V.search(fns_of(model, topk, topp, K, log=l64), hp, Pn, src, K, torch.float64)
            V.search(fns_of(model, topk, topp, K, log=l32), hp, Pn, src, K, torch.float32)
            f["decided_%d" % K] = decisions_decided(l64, l32, topk, topp, K)
            a, _ = V.search(fns_of(model, topk, topp, K), hp, Ps, src, K, torch.float32)
            b, _ = V.search(fns_of(model, topk, topp, K), hp, Ps, src, K, torch.float32, store_bf16=True)
            assert N.rt.decode_hypothesis(a["seq"], hp) == N.rt.decode_hypothesis(b["seq"], hp), ("bf16 storage model", K)
        con, _ = V.search(fns_of(model, topk, topp, 4), hp, Pn, src, 4, torch.float32)
        f["changed"] = int(sum(not np.array_equal(con["seq"][b], plain["seq"][b]) for b in range(src.shape[0])))
        out[(topk, topp)] = f
    n, (topk, topp) = WITH_NGRAM
    out["with_ngram"] = V.candidate_margin(
        lambda hp_, P_, s_, K, dt: V.search(fns_of(model, topk, topp, K, ngram=n), hp_, P_, s_, K, dt), hp, Pn, src, beams=beams,
        tol=(ATOL, RTOL))
    return out
