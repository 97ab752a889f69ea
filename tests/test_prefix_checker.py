"""tgt_prefix_file on the CPU: the rule of tests/prefix_ref.py against an independent restatement, the planted defects, and what
the reference's search (oracle.ref_torch.beam_search) shows under the rule on the tiny fixtures of the GPU tests."""
import numpy as np
import pytest
import torch

from tests import ngram_ref as N
from tests import prefix_ref as PR
from tests import variant_ref as V


# ---------------------------------------------------------------------------------------------- the rule
def _restated(logits, V_, prefix, t, K, eos):
    """The rule once more, element by element."""
    out = np.array(logits, copy=True)
    for r in range(out.shape[0]):
        row = [int(v) for v in prefix[r // K]]
        n = len([v for v in row if v != 0])
        if not t < n:
            continue
        for v in range(V_):
            if v == row[t]:
                continue
            out[r, v] = -2e8 if v == eos else -1e8
    return out


@pytest.mark.parametrize("t", [0, 1, 2, 3, 4, 7])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_rule_against_the_restatement(K, t):
    rng = np.random.default_rng(10 * K + t)
    prefix = PR.prefixes(9, (2, 0, 3, 4), seed=K)
    logits = rng.normal(size=(4 * K, 12)).astype(np.float32)
    got = PR.force(logits, 9, prefix, t, K, -PR.INF, 2)
    assert np.array_equal(got.view(np.int32), _restated(logits, 9, prefix, t, K, 2).view(np.int32))
    assert np.array_equal(got[:, 9:].view(np.int32), logits[:, 9:].view(np.int32))
    n_b = PR.lengths(prefix)
    for r in range(4 * K):
        if t >= n_b[r // K]:
            assert np.array_equal(got[r].view(np.int32), logits[r].view(np.int32))


def test_rule_by_hand():
    logits = np.arange(12, dtype=np.float32).reshape(2, 6) + 0.5
    out = PR.force(logits, 5, np.array([[3, 4], [0, 0]]), 0, 1, -PR.INF, 2)
    assert out.tolist() == [[-1e8, -1e8, -2e8, 3.5, -1e8, 5.5], [6.5, 7.5, 8.5, 9.5, 10.5, 11.5]]
    assert np.array_equal(PR.force(logits, 5, np.array([[3, 4], [0, 0]]), 2, 1, -PR.INF, 2), logits)      # past the table
    assert PR.force(logits, 5, np.array([[3, 4], [0, 0]]), 1, 1, -PR.INF, -1)[0].tolist() == [-1e8] * 4 + [4.5, 5.5]
    assert np.array_equal(PR.force(logits, 5, np.array([[5, 0], [7, 0]]), 0, 1, -PR.INF, 2), logits)      # ids the rows lack
    # the forced token's log-probability is exactly 0, in fp32 and in float64
    for dt in (np.float32, np.float64):
        lp = PR.logprobs(out.astype(dt)[:, :5])
        assert lp[0, 3] == 0.0 and (lp[0, [0, 1, 4]] < -0.9 * PR.INF).all() and lp[0, 2] < -1.9 * PR.INF
        assert np.isfinite(lp).all()


@pytest.mark.parametrize("defect", sorted(PR.CASES))
def test_planted_defects_change_the_step(defect):
    prefix, t, K, V_, ld = PR.CASES[defect]
    rng = np.random.default_rng(3)
    logits = rng.normal(size=(prefix.shape[0] * K, ld)).astype(np.float32)
    good, bad = PR.force(logits, V_, prefix, t, K, -PR.INF, 2), PR.force(logits, V_, prefix, t, K, -PR.INF, 2, defect)
    assert not np.array_equal(good.view(np.int32), bad.view(np.int32)), defect
    assert np.array_equal(good.view(np.int32), _restated(logits, V_, prefix, t, K, 2).view(np.int32))


def test_every_defect_has_a_case():
    assert set(PR.DEFECTS) == set(PR.CASES) | {"before_ngram"}


def test_force_ahead_of_the_ban_lifts_a_banned_eos():
    """The defect "before_ngram" on its case: a history that holds the EOS id makes the ban write -INF over the -2 INF of the
    forced row, where EOS is then level with the fillers and, with its low id, among the first of them."""
    hist = np.array([[0, 5, 2, 5, 0, 0]])              # 5 was followed by 2: n = 2 bans 2 behind the second 5
    prefix = np.array([[5, 7, 5, 6]])
    logits = np.random.default_rng(1).normal(size=(1, 9)).astype(np.float32)
    good = PR.step(logits, 9, prefix, 3, 1, 2, hist=hist, n=2)
    bad = PR.step(logits, 9, prefix, 3, 1, 2, hist=hist, n=2, defect="before_ngram")
    assert good[0, 6] == logits[0, 6] and PR.logprobs(good)[0, 6] == 0.0
    assert good[0, 2] == -2 * PR.INF and bad[0, 2] == -PR.INF
    assert np.array_equal(np.delete(good, 2, axis=1), np.delete(bad, 2, axis=1))


def test_a_ban_of_the_forced_token_itself_is_not_undone():
    """What the force leaves "untouched" is what the ban left there: history a b a, the prefix forces b, the ban has taken b.
    The forced entry then ties with the fillers at log(1 / (V - 1)) instead of scoring 0 -- in either order of the two
    launches -- and the lowest ids win the tie.  Hence zero_amd refuses a prefix that holds an n-gram twice
    (models/_decode.py check_prefix_ngram)."""
    from zero_amd.models import _decode
    hist = np.array([[0, 5, 6, 5, 0, 0]])
    prefix = np.array([[5, 6, 5, 6]])
    logits = np.random.default_rng(1).normal(size=(1, 9)).astype(np.float32)
    for defect in (None, "before_ngram"):
        out = PR.step(logits, 9, prefix, 3, 1, 2, hist=hist, n=2, defect=defect)
        assert out[0, 6] == -PR.INF
        lp = PR.logprobs(out.astype(np.float64))
        assert np.allclose(lp[0, [0, 1, 3, 6]], -np.log(8.0)) and lp[0, 6] == lp[0, 0]
    with pytest.raises(ValueError, match=r"sentence 0 with no_repeat_ngram_size=2: the 2-gram \(5, 6\) at position 2 is already "
                                         r"at position 0"):
        _decode.check_prefix_ngram(prefix, 2)
    with pytest.raises(ValueError, match=r"sentence 1 with no_repeat_ngram_size=1: the 1-gram \(4,\) at position 2"):
        _decode.check_prefix_ngram(np.array([[3, 4, 5], [4, 3, 4]]), 1)
    _decode.check_prefix_ngram(prefix, 3)
    _decode.check_prefix_ngram(prefix, 0)
    _decode.check_prefix_ngram(None, 2)
    _decode.check_prefix_ngram(np.array([[5, 6, 5, 7], [0, 0, 0, 0]]), 2)


@pytest.mark.parametrize("topk, topp", [(3, 0.0), (0, 0.4), (2, 0.9)])
def test_a_step_with_a_truncation_forces_twice(topk, topp):
    """Forced tokens that are the least probable of their rows: the truncation ahead of a single force leaves them at -INF,
    level with the fillers; force, truncate, force is the rule applied to logits whose forced entries nobody touched."""
    rng = np.random.default_rng(5)
    prefix = np.array([[7, 5], [0, 0], [3, 4]])
    logits = rng.normal(size=(6, 12)).astype(np.float32)
    for r, tok in ((0, 7), (1, 7), (4, 3), (5, 3)):
        logits[r, tok] = -9.0
    want = PR.force(logits, 9, prefix, 0, 2, -PR.INF, 2)
    got = PR.step_truncated(logits, 9, prefix, 0, 2, 2, topk, topp, 5)
    assert np.array_equal(got[[0, 1, 4, 5]].view(np.int32), want[[0, 1, 4, 5]].view(np.int32))
    lp = PR.logprobs(got[:, :9].astype(np.float64))
    assert lp[0, 7] == 0.0 and lp[4, 3] == 0.0
    from tests import sampling_ref as S
    assert np.array_equal(got[[2, 3]], S.apply(logits, 9, topk, topp, 5)[[2, 3]])          # the free sentence: truncated as ever
    lost = PR.step_truncated(logits, 9, prefix, 0, 2, 2, topk, topp, 5, single=True)
    assert lost[0, 7] == -PR.INF and lost[4, 3] == -PR.INF
    assert PR.logprobs(lost[:, :9].astype(np.float64))[0, 7] == PR.logprobs(lost[:, :9].astype(np.float64))[0, 0]


# ---------------------------------------------------------------------------------------------- the reference's search
@pytest.fixture(scope="module")
def tf():
    """The transformer fixture with its plain and constrained fp32 searches at beam 4 (computed once, left unchanged)."""
    hp, src, prefix = PR.fixture("transformer")
    m = PR.MODELS["transformer"]
    Pn = m["init"](hp, PR.SEEDS["transformer"])
    plain = V.search(m["fns"], hp, Pn, src, 4, torch.float32)
    con = V.search(PR.constrained(m["fns"], prefix, 4), hp, Pn, src, 4, torch.float32)
    return dict(hp=hp, src=src, prefix=prefix, Pn=Pn, fns=m["fns"], plain=plain, con=con)


@pytest.mark.parametrize("model", sorted(PR.MODELS))
def test_reference_search_with_the_rule(model):
    """make_fixture's own assertions (float64 and fp32 identical on every beam and in the order of the real candidates, free
    gaps > 4 err, the bf16 storage model keeps the sharpened best hypotheses, every output hypothesis starts with its prefix,
    none ends inside it, no output score below -1e7, forced steps add exactly 0, the unconstrained best hypotheses do not
    start with their prefixes), and the fp32 reference within a quarter of the project's fp32 score tolerance, which the GPU
    tests then use."""
    f = PR.make_fixture(model)
    print("%s seed %d: gap %.2e err %.1e (x %.1f) rel %.3f forced %r over %d forced steps"
          % (model, PR.SEEDS[model], f["gap"], f["err"], f["gap"] / f["err"], f["rel"], f["forced"], f["forced_steps"]))
    assert f["gap"] > 4.0 * f["err"] and f["rel"] <= 0.25 and f["forced"] == 0.0
    assert f["forced_steps"] == 2 * sum(PR.PREFIX_LENGTHS)           # beams 1 and 4, every forced step of every sentence
    assert PR.score_tol(f["rel"], f["err"]) == (PR.RTOL, PR.ATOL)
    assert tuple(PR.lengths(f["prefix"])) == PR.PREFIX_LENGTHS


def test_all_empty_prefixes_are_the_plain_search(tf):
    """Through the wrapper itself (the shortcut of `constrained` is bypassed by a table whose only token no row can have)."""
    zero = np.zeros_like(tf["prefix"])
    assert PR.constrained(tf["fns"], zero, 4) is tf["fns"] and PR.constrained(tf["fns"], None, 4) is tf["fns"]
    hp = tf["hp"]
    off = zero.copy()
    off[1, 0] = hp.tgt_vocab.size()              # outside [1, V): forces nothing
    out, _ = V.search(PR.constrained(tf["fns"], off, 4), hp, tf["Pn"], tf["src"], 4, torch.float32)
    assert np.array_equal(out["seq"], tf["plain"][0]["seq"])
    assert np.array_equal(out["score"].view(np.int32), tf["plain"][0]["score"].view(np.int32))


def test_no_filler_finishes_and_fillers_are_displaced(tf):
    """From the trace of the constrained search: on a forced step a sentence keeps ONE real candidate, none of the 2K kept
    candidates is EOS, and from a sentence's first free step on all of its 2K kept candidates are real."""
    hp, prefix = tf["hp"], tf["prefix"]
    Vt, eos = hp.tgt_vocab.size(), hp.tgt_vocab.eos()
    n_b = PR.lengths(prefix)
    out, trace = tf["con"]
    mtl = (tf["src"] != 0).sum(1) + hp.decode_length       # behind it the search keeps no live row of the sentence
    seen_free = 0
    for t, (s, i) in enumerate(trace):
        for b in range(prefix.shape[0]):
            kept_s, kept_tok = s[b, :8], i[b, :8] % Vt
            if t < n_b[b]:
                assert (kept_s > PR.REAL).sum() == 1 and kept_tok[0] == prefix[b, t] and kept_s[0] == 0.0
                assert not (kept_tok == eos).any(), (t, b)
                assert (kept_s[1:] < -1e7).all()
            elif n_b[b] > 0 and t <= mtl[b]:
                assert (kept_s > PR.REAL).all(), (t, b, kept_s)
                seen_free += 1
    assert seen_free > 0


def test_eos_not_lowered_lets_a_filler_finish(tf):
    """The defect "eos_kept": EOS is the lowest-numbered filler but two, so behind step 0 (where the tail bans it anyway) a
    forced step keeps it among its 2K candidates, where it counts as a finished hypothesis of about -1e8."""
    hp, prefix = tf["hp"], tf["prefix"]
    Vt, eos = hp.tgt_vocab.size(), hp.tgt_vocab.eos()
    n_b = PR.lengths(prefix)
    _, trace = V.search(PR.constrained(tf["fns"], prefix, 4, "eos_kept"), hp, tf["Pn"], tf["src"], 4, torch.float32)
    hits = [(t, b) for t, (s, i) in enumerate(trace) for b in range(prefix.shape[0])
            if 1 <= t < n_b[b] and (i[b, :8] % Vt == eos).any()]
    assert hits


@pytest.mark.parametrize("defect", ["row_mod_k", "t_plus_1", "t_minus_1", "next_sentence", "resumed"])
def test_search_level_defects_break_a_property(tf, defect):
    """The defects that move WHO is forced WHEN: some hypothesis no longer starts with its prefix, or the sentence without a
    prefix no longer decodes what the plain search decodes for it."""
    hp, prefix = tf["hp"], tf["prefix"]
    out, _ = V.search(PR.constrained(tf["fns"], prefix, 4, defect), hp, tf["Pn"], tf["src"], 4, torch.float32)
    broken = any(not PR.starts_with(out["seq"][b, k], prefix[b], hp) for b in range(prefix.shape[0]) for k in range(4)
                 if out["score"][b, k] > -1e30)
    good = tf["con"][0]
    n = min(out["seq"].shape[2], good["seq"].shape[2])
    assert broken or not np.array_equal(out["seq"][:, :, :n], good["seq"][:, :, :n]), defect


def test_the_search_with_the_ban_and_the_rule(tf):
    """The fixture's prefixes (none holds a 2-gram twice) with no_repeat_ngram_size = 2: every hypothesis starts with its
    prefix, scores like a real one, and holds no 2-gram twice -- the prefix's own 2-grams count."""
    hp, prefix = tf["hp"], tf["prefix"]
    out, _ = V.search(PR.with_ngram(tf["fns"], prefix, 4, 2), hp, tf["Pn"], tf["src"], 4, torch.float32)
    plain_ban, _ = V.search(N.constrained(tf["fns"], 2), hp, tf["Pn"], tf["src"], 4, torch.float32)
    for b in range(prefix.shape[0]):
        for k in range(4):
            if out["score"][b, k] > -1e30:
                assert out["score"][b, k] > PR.REAL
                assert PR.starts_with(out["seq"][b, k], prefix[b], hp)
                assert not N.has_repeat(N.hypothesis(out["seq"][b, k], hp), 2)
    n = min(out["seq"].shape[2], plain_ban["seq"].shape[2])
    assert np.array_equal(out["seq"][0, :, :n], plain_ban["seq"][0, :, :n])          # the sentence without a prefix
    assert np.array_equal(out["score"][0], plain_ban["score"][0])
