"""zk_diverse_select called directly (zero_amd/csrc/zk_diverse.hip) against the rule of tests/diverse_ref.py.

Every buffer is a beam_ref.GuardedWords: the candidate lists must be bit-identical after the call, the outputs start as NaN words
and nothing outside them may be written.  (K, G) in diverse_ref.KG_SETTINGS, B in {1, 3, 33}, token ids up to 31999.
  * dyadic scores (multiples of 1/4), lambda a power of two, penalty 1: ts and ti are BIT-EQUAL to the rule -- every tie, within a
    row, across the rows of a group and between a penalised and an unpenalised candidate, falls as the rule says;
  * random scores: every group's result is judged by beam_ref.assert_topk (scores within the counted bound, order, completeness,
    exact indices where decisive) against the rule given the counts of the groups before it;
  * the length penalty read from a device word by ONE captured launch, replayed with the word changed;
  * refusals: -1 with a message, nothing launched, every buffer untouched;
  * the composed tail -- zk_beam_topk with B K "sentences" of beam 1 and k2 = K + K/G, then the selection -- on logits of
    V = 1000 and 32000 against the rule on the full score matrix.
tests/test_diverse_host.py shows that the rule rejects the planted defects.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import beam_ref as BR  # noqa: E402
from tests import diverse_ref as D  # noqa: E402
from tests.parity import PER_TERM  # noqa: E402
from tests.util_gpu import eng  # noqa: E402
from zero_amd.hip import ZeroHipError  # noqa: E402

f32, f64, i32 = np.float32, np.float64, np.int32
VMAX = 32000
BS = (1, 3, 33)


class _Call(object):
    """The four guarded buffers of one call."""

    def __init__(self, cs, ci, B, K, G):
        self.B, self.K, self.G, self.Kg, self.k2 = B, K, G, K // G, cs.shape[1]
        self.cs = BR.GuardedWords(cs.size, np.ascontiguousarray(cs, dtype=f32), "cuda")
        self.ci = BR.GuardedWords(ci.size, np.ascontiguousarray(ci, dtype=i32), "cuda")
        self.os = BR.GuardedWords(B * 2 * K, BR.NAN_WORD, "cuda")
        self.oi = BR.GuardedWords(B * 2 * K, BR.NAN_WORD, "cuda")

    def args(self, V, lam, pen, eos, pen_dev=None, **kw):
        a = dict(B=self.B, K=self.K, G=self.G, k2=self.k2, V=V, lam=lam, pen=pen)
        a.update(kw)
        return (self.cs.ptr, self.ci.ptr, self.os.ptr, self.oi.ptr, a["B"], a["K"], a["G"], a["k2"], a["V"], float(a["lam"]),
                float(a["pen"]), pen_dev, int(eos))

    def run(self, e, *a, **kw):
        e.lib.call("zk_diverse_select", *self.args(*a, **kw), e.stream)
        return self.result("call")

    def result(self, what):
        torch.cuda.synchronize()
        self.cs.check_intact(what + " [cand_scores]")
        self.ci.check_intact(what + " [cand_index]")
        self.os.check_guard(what + " [topk_scores]")
        self.oi.check_guard(what + " [topk_index]")
        shape = (self.B * self.G, 2 * self.Kg)
        return self.os.words().view(f32).reshape(shape), self.oi.words().reshape(shape)

    def untouched(self, what):
        torch.cuda.synchronize()
        for b in (self.cs, self.ci, self.os, self.oi):
            b.check_intact(what)


def _rule(cs, ci, B, K, G, V, lam, pen, eos):
    out = [D.select_lists(cs[b * K:(b + 1) * K], ci[b * K:(b + 1) * K], V, G, lam, pen, eos) for b in range(B)]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("K, G", D.KG_SETTINGS, ids=str)
def test_dyadic_scores_are_bit_equal_to_the_rule(K, G, B):
    e = eng()
    k2 = D.depth(K, G)
    changed = 0
    for n, lam in enumerate((0.5, 2.0, 0.0)):
        cs, ci = D.dyadic_lists(100 * K + 10 * G + B + n, B * K, k2, VMAX)
        assert ci.max() == VMAX - 1 and (ci == D.EOS).any()
        want_s, want_i = _rule(cs, ci, B, K, G, VMAX, lam, 1.0, D.EOS)
        got_s, got_i = _Call(cs, ci, B, K, G).run(e, VMAX, lam, 1.0, D.EOS)
        assert np.array_equal(got_i, want_i), (lam, got_i, want_i)
        assert np.array_equal(got_s.view(i32), want_s.astype(f32).view(i32)), (lam, got_s, want_s)
        plain_s, plain_i = _rule(cs, ci, B, K, G, VMAX, 0.0, 1.0, D.EOS)
        changed += not (np.array_equal(plain_i, want_i) and np.array_equal(plain_s, want_s))
    assert changed >= 1 or (K == 2 and B <= 3)          # the penalty decided something (one row per group: not always)


def _sequential_check(got_s, got_i, scores_of, bound_of, B, K, G, V, lam, pen, eos, what):
    """Every group judged by beam_ref.assert_topk given what the kernel itself counted in the groups before it.
    scores_of(b, g) / bound_of(b, g): float64 [Kg * V] reference scores before the penalty (-inf: not a candidate) and their
    bounds.  -> the share of decisive groups."""
    Kg = K // G
    ref = np.full((B * G, Kg * V), -np.inf)
    bnd = np.zeros((B * G, Kg * V))
    for b in range(B):
        counted = []
        for g in range(G):
            raw, rb = scores_of(b, g), bound_of(b, g)
            cnt = np.zeros(Kg * V)
            for t in counted:
                cnt[np.arange(Kg) * V + t] += 1
            sub = float(f32(lam)) * cnt / float(f32(pen))
            ref[b * G + g] = raw - sub
            # the product, the quotient (on |sub|) and the difference (on its result), one PER_TERM each
            bnd[b * G + g] = np.where(np.isfinite(raw), rb + PER_TERM * (2 * sub + np.abs(np.where(np.isfinite(raw), raw - sub, 0))),
                                      0.0)
            counted += [int(t % V) for t in got_i[b * G + g, :Kg] if t % V != eos]
    return BR.assert_topk(got_s, got_i, ref, bnd, Kg, V, what)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("K, G", D.KG_SETTINGS, ids=str)
def test_random_scores_pass_the_decisive_candidate_checker(K, G, B):
    e = eng()
    Kg, k2, V = K // G, D.depth(K, G), 1000
    rng = np.random.default_rng(7 * K + G + B)
    pool = np.unique(np.append(rng.choice(V, 3 * k2, replace=False), D.EOS))
    ci = np.stack([rng.choice(pool, k2, replace=False) for _ in range(B * K)]).astype(i32)
    cs = -np.sort(rng.gamma(2.0, 1.0, (B * K, k2)), axis=1).astype(f32)          # descending, as zk_beam_topk returns them
    lam, pen = 0.5, BR.PENALTY
    got_s, got_i = _Call(cs, ci, B, K, G).run(e, V, lam, pen, D.EOS)

    def scores_of(b, g):
        raw = np.full(Kg * V, -np.inf)
        for j in range(Kg):
            r = b * K + g * Kg + j
            raw[j * V + ci[r]] = cs[r].astype(f64)
        return raw
    share = _sequential_check(got_s, got_i, scores_of, lambda b, g: np.zeros(Kg * V), B, K, G, V, lam, pen, D.EOS,
                              "random K %d G %d B %d" % (K, G, B))
    print("decisive share %.3f" % share)
    assert share >= BR.DECISIVE_FLOOR


def test_the_penalty_is_read_from_the_device_at_replay():
    """ONE captured launch with penalty_dev; the word changes between the replays: every replay equals the rule under the
    length penalty the word holds at that time (dyadic scores, penalties 1, 2 and 4: exact)."""
    e = eng()
    B, K, G = 3, 6, 3
    cs, ci = D.dyadic_lists(5, B * K, D.depth(K, G), VMAX)
    c = _Call(cs, ci, B, K, G)
    word = torch.ones(1, dtype=torch.float32, device="cuda")
    with torch.cuda.stream(e.work_stream):
        torch.cuda.synchronize()
        g = e.graph_capture(lambda: e.lib.call("zk_diverse_select", *c.args(VMAX, 1.0, -1.0, D.EOS, pen_dev=word.data_ptr()),
                                               e.stream))
        try:
            assert e.last_graph_nodes == 1
            c.untouched("capturing must not run the kernel")
            seen = []
            for pen in (1.0, 2.0, 4.0, 1.0):
                word.fill_(pen)
                e.graph_launch(g)
                got_s, got_i = c.result("replay at penalty %g" % pen)
                want_s, want_i = _rule(cs, ci, B, K, G, VMAX, 1.0, pen, D.EOS)
                assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s.astype(f32)), pen
                seen.append(got_s.copy())
            assert not np.array_equal(seen[0], seen[1]) and np.array_equal(seen[0], seen[3])
        finally:
            e.lib.call("zk_graph_destroy", g)


ERRORS = [
    ("no multiple", dict(G=3)), ("bad shape", dict(G=0)), ("bad shape", dict(B=-1)), ("bad shape", dict(V=0)),
    ("k2=1 ", dict(k2=1)), ("k2=17", dict(k2=17)), ("more than 128", dict(K=16, G=1, k2=16)),
    ("lambda=-0.5", dict(lam=-0.5)), ("lambda=nan", dict(lam=float("nan"))), ("lambda=inf", dict(lam=float("inf"))),
    ("length_penalty=0", dict(pen=0.0)), ("length_penalty=nan", dict(pen=float("nan"))),
    ("overflows", dict(V=2 ** 30)), ("overflows", dict(K=2, G=2, V=2 ** 31 - 1)),
    ("counted tokens, more than 64", dict(K=80, G=80, k2=2)),
]


@pytest.mark.parametrize("word, kw", ERRORS, ids=["%s-%d" % (w.strip(), i) for i, (w, _) in enumerate(ERRORS)])
def test_refusals_name_the_argument_and_touch_nothing(word, kw):
    e = eng()
    B, K, G = 3, 4, 2
    cs, ci = D.dyadic_lists(6, 16 * B, 16, VMAX)          # large enough for every shape asked for below
    c = _Call(cs, ci, B, K, G)
    c.k2 = D.depth(K, G)
    kw = dict(kw)
    args = c.args(kw.pop("V", VMAX), kw.pop("lam", 0.5), kw.pop("pen", 1.0), D.EOS, **kw)
    with pytest.raises(ZeroHipError, match=word):
        e.lib.call("zk_diverse_select", *args, e.stream)
    c.untouched("refused call")
    with pytest.raises(ZeroHipError, match="required"):
        e.lib.call("zk_diverse_select", None, c.ci.ptr, c.os.ptr, c.oi.ptr, B, K, G, c.k2, VMAX, 0.5, 1.0, None, D.EOS, e.stream)
    e.lib.call("zk_diverse_select", None, None, None, None, 0, K, G, c.k2, VMAX, 0.5, 1.0, None, D.EOS, e.stream)    # B = 0
    c.untouched("B = 0")


@pytest.mark.parametrize("V", [1000, 32000])
@pytest.mark.parametrize("K, G", [(4, 2), (6, 3), (12, 3)], ids=str)
def test_the_composed_tail_equals_the_rule_on_the_full_matrix(K, G, V):
    """Logits -> zk_beam_topk (B K sentences of beam 1, k2 = K + K/G, the step's scalars from a device buffer) ->
    zk_diverse_select, against the rule applied to beam_ref.topk_ref's full score matrix (temperature 0.7, the EOS ban on,
    previous log-probs with dead beams)."""
    e = eng()
    B, Kg, k2 = 3, K // G, D.depth(K, G)
    rng = np.random.default_rng(K + G + V)
    logits = (rng.standard_normal((B * K, V)) * 3.0).astype(f32)
    hot = rng.choice(V, 6, replace=False)
    logits[:, hot] += 6.0                                   # the rows agree on a few tokens: the groups collide
    logits[:, D.EOS] += 8.0
    prev = -rng.gamma(2.0, 1.0, B * K).astype(f32)
    prev[K - 1] = BR.F32_MIN                                # a dead beam
    lam, pen, temp, fv = 1.0, BR.PENALTY, 0.7, BR.FORBID_VALUE
    for forbid in (D.EOS, -1):
        d_logits = torch.from_numpy(logits).cuda()
        d_prev = torch.from_numpy(prev).cuda()
        scal = torch.from_numpy(BR.scal_words(pen, forbid)).cuda()
        cand = _Call(np.zeros((B * K, k2), f32), np.zeros((B * K, k2), i32), B, K, G)
        ws = torch.zeros(BR.topk_workspace(B * K, 1, k2), dtype=torch.uint8, device="cuda")
        e.lib.call("zk_beam_topk", d_logits.data_ptr(), d_prev.data_ptr(), cand.cs.ptr, cand.ci.ptr, B * K, 1, V, V, k2, temp,
                   1.0, -1, fv, scal.data_ptr(), ws.data_ptr(), ws.numel(), e.stream)
        torch.cuda.synchronize()
        cand.cs.before, cand.ci.before = cand.cs.t.cpu().numpy().copy(), cand.ci.t.cpu().numpy().copy()
        e.lib.call("zk_diverse_select", *cand.args(V, lam, -1.0, D.EOS, pen_dev=scal.data_ptr()), e.stream)
        got_s, got_i = cand.result("composed tail")
        ref, bound = BR.topk_ref(logits, prev, 1, V, BR.inv_temp_of(temp), pen, forbid, fv)       # [B K, V]
        rows = lambda b, g: slice(b * K + g * Kg, b * K + (g + 1) * Kg)
        share = _sequential_check(got_s, got_i, lambda b, g: ref[rows(b, g)].reshape(-1),
                                  lambda b, g: bound[rows(b, g)].reshape(-1), B, K, G, V, lam, pen, D.EOS,
                                  "composed K %d G %d V %d forbid %d" % (K, G, V, forbid))
        assert share >= BR.DECISIVE_FLOOR
        # and the full-matrix rule itself, where it is decisive (float64 scores): the same indices
        want = [D.select_full(ref[b * K:(b + 1) * K], G, lam, pen, D.EOS) for b in range(B)]
        want_i = np.concatenate([w[1] for w in want])
        live = np.concatenate([w[0] for w in want]) > -1e30
        assert np.array_equal(got_i[live], want_i[live])
