"""zk_align_probs / zk_f32_align_probs (zero_amd/csrc/zk_align.hip) element by element against the float64 statement of the
rule in tests/align_ref.py, on guarded, NaN-prefilled, strided buffers (q a column slice of a [., 3 H] buffer, k the first H
columns of a [., 2 H] buffer, ldmask = Lk + 3, ldp = Lk + 5) with the inputs verified unchanged.

  probabilities   every element within align_bound (derived, no fitted constant); masked positions exactly 0.0
  arg-max         accept_best: every index eligible and able to be the arg-max of a result inside the bound; no row skipped
  outputs         probs NULL / best NULL give the other output bit for bit; two runs are bit-identical
  exact           one valid key: exactly 1.0 there; two bit-identical maximal key rows: the lower index
  refusals        by name, buffers untouched
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import align_ref as R  # noqa: E402
from tests import parity as PR  # noqa: E402
from tests.util_gpu import eng  # noqa: E402
from zero_amd import hip  # noqa: E402

BEST_GUARD = -7777
DT = {"bf16": torch.bfloat16, "fp32": torch.float32}


class _Bufs(object):
    def __init__(self, x, form):
        q, k = x["q"], x["k"]
        self.B, self.Lq, H = q.shape
        self.Lk = k.shape[1]
        self.nh, self.d, self.inf = x["nh"], x["d"], x["inf"]
        B, Lq, Lk = self.B, self.Lq, self.Lk
        self.q = PR.guarded(B * Lq, H, ld=3 * H, off=H, dtype=DT[form], prefill=q.reshape(B * Lq, H), device="cuda")
        self.k = PR.guarded(B * Lk, H, ld=2 * H, off=0, dtype=DT[form], prefill=k.reshape(B * Lk, H), device="cuda")
        self.ldmask, self.ldp = Lk + R.LD_EXTRA_MASK, Lk + R.LD_EXTRA_PROBS
        mk = lambda m: None if m is None else PR.guarded(B, Lk, ld=self.ldmask, dtype=torch.float32, prefill=m, device="cuda")
        self.km, self.am = mk(x["kmask"]), mk(x["amask"])
        self.inputs = [g for g in (self.q, self.k, self.km, self.am) if g is not None]

    def run(self, probs=True, best=True):
        """-> (probs Guarded or None, best tensor with 64 guard elements on either side, or None)"""
        B, Lq, Lk = self.B, self.Lq, self.Lk
        pg = PR.guarded(B * Lq, Lk, ld=self.ldp, dtype=torch.float32, device="cuda") if probs else None
        pv = torch.as_strided(pg.t, (B, Lq, Lk), (Lq * self.ldp, self.ldp, 1), PR.LEAD) if probs else None
        bt = torch.full((64 + B * Lq + 64,), BEST_GUARD, dtype=torch.int32, device="cuda") if best else None
        win = lambda g: None if g is None else g.window()
        eng().align_probs(self.q.mat, self.k.mat, B, self.nh, Lq, Lk, self.d, kmask=win(self.km), ldmask=self.ldmask,
                          amask=win(self.am), probs=pv, best=bt[64:64 + B * Lq].view(B, Lq) if best else None,
                          mask_inf=self.inf)
        torch.cuda.synchronize()
        for g in self.inputs:
            g.check_intact()
        if pg is not None:
            pg.check_guard("probs")
        if bt is not None:
            b = bt.cpu()
            assert (b[:64] == BEST_GUARD).all() and (b[-64:] == BEST_GUARD).all(), "best: written outside [B, Lq]"
        return pg, (bt[64:64 + B * Lq].view(B, Lq).cpu().numpy() if best else None)


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_elementwise(case, form):
    x = R.case_inputs(case, form)
    ref = R.case_reference(x)
    bound = R.align_bound(ref, form)
    bufs = _Bufs(x, form)
    B, Lq, Lk = bufs.B, bufs.Lq, bufs.Lk
    pg, best = bufs.run()
    P = pg.value().double().numpy().reshape(B, Lq, Lk)
    print("%s %s: worst |err| / bound %.3f" % (case, form, R.worst_ratio(P, ref["P"], bound)))
    PR.assert_elementwise(torch.as_tensor(P).reshape(B * Lq, Lk), torch.as_tensor(ref["P"]).reshape(B * Lq, Lk),
                          torch.as_tensor(bound).reshape(B * Lq, Lk), "%s %s probs" % (case, form))
    if x["kmask"] is not None and x["inf"] == R.MASK_INF:
        masked = np.broadcast_to((x["kmask"].numpy() == 0)[:, None, :], P.shape)
        assert (P[masked] == 0.0).all(), "a masked position is not exactly 0.0"
        for b, n in enumerate(R.CASES[case]["lengths"]):
            if n == 1:
                assert (P[b, :, 0] == 1.0).all() and (P[b, :, 1:] == 0.0).all(), "one valid key: exactly 1.0 expected"
    bad = R.accept_best(best, ref["P"], bound, ref["amask"])
    assert not bad, bad[:5]
    if R.CASES[case].get("amask") == "zero":
        assert (best == -1).all()
    if R.CASES[case].get("tie"):
        j1, j2 = R.CASES[case]["tie"]
        assert (P[:, :, j1] == P[:, :, j2]).all(), "bit-identical key rows gave different probabilities"
        assert (best == j1).all(), "equal maxima: the lower index %d expected, got %s" % (j1, np.unique(best))
    # a second run, and each output alone: bit for bit
    pg2, best2 = bufs.run()
    assert torch.equal(pg2.t.view(torch.int32), pg.t.view(torch.int32)) and np.array_equal(best, best2)
    pg3, none = bufs.run(best=False)
    assert none is None and torch.equal(pg3.t.view(torch.int32), pg.t.view(torch.int32))
    none, best4 = bufs.run(probs=False)
    assert none is None and np.array_equal(best, best4)


@pytest.mark.parametrize("form", R.FORMS)
def test_refusals_leave_the_buffers_untouched(form):
    x = R.case_inputs("q17_k17_hole", form)
    bufs = _Bufs(x, form)
    B, Lq, Lk, nh, d = bufs.B, bufs.Lq, bufs.Lk, bufs.nh, bufs.d
    H = nh * d
    name = "zk_align_probs" if form == "bf16" else "zk_f32_align_probs"
    pg = PR.guarded(B * Lq, Lk, ld=bufs.ldp, dtype=torch.float32, device="cuda")
    bt = torch.full((B * Lq,), BEST_GUARD, dtype=torch.int32, device="cuda")
    ok = dict(q=bufs.q.mat.ptr, ldq=3 * H, bsq=Lq * 3 * H, k=bufs.k.mat.ptr, ldk=2 * H, bsk=Lk * 2 * H,
              kmask=bufs.km.window().data_ptr(), ldmask=bufs.ldmask, amask=None, probs=pg.window().data_ptr(), ldp=bufs.ldp,
              bsp=Lq * bufs.ldp, best=bt.data_ptr(), B=B, nh=nh, Lq=Lq, Lk=Lk, d=d, scale=d ** -0.5, mask_inf=1e8)
    esz = 2 if form == "bf16" else 4
    bad = [(dict(probs=None, best=None), "neither probs nor best"),
           (dict(ldk=H - 8), "shorter than nh"), (dict(ldq=H - 8), "shorter than nh"),
           (dict(Lk=R.MAX_LK + 1, ldmask=R.MAX_LK + 1, ldp=R.MAX_LK + 1), "at most %d" % R.MAX_LK),
           (dict(ldmask=Lk - 1), "ldmask"), (dict(ldp=Lk - 1), "ldp"),
           (dict(k=ok["k"] + esz), "16-byte aligned"), (dict(ldk=2 * H + 1), "16-byte aligned"),
           (dict(d=d + 4 if form == "bf16" else d + 2, nh=1), "head size"), (dict(d=256, nh=1, ldq=256, ldk=256), "head size"),
           (dict(Lq=0), "bad arguments"), (dict(nh=0), "bad arguments")]
    if form == "bf16":
        bad += [(dict(q=ok["q"] + esz), "16-byte aligned"), (dict(bsq=Lq * 3 * H + 4), "16-byte aligned")]
    for change, text in bad:
        args = dict(ok, **change)
        with pytest.raises(hip.ZeroHipError, match=text):
            hip.lib().call(name, *(list(args.values()) + [eng().stream]))
    torch.cuda.synchronize()
    assert torch.isnan(pg.window()).all() and (bt == BEST_GUARD).all()
    pg.check_guard("probs")
    for g in bufs.inputs:
        g.check_intact()
