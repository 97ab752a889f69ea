"""The in-launch LayerNorm (chain) kernels -- zk_gemm_add_ln, zk_gemm_ln_bwd, zk_attn_out_ln, zk_proj_attn_out_ln -- element
by element against the staged float64 references and derived bounds of tests/chain_ref.py (tests/test_chain_checker.py
shows on the CPU that a correct computation passes them and that each planted defect does not).

Every case goes through the Engine entry points after ln_epoch_bump.  Operands are guarded buffers (tests/parity.py):
A, B / W, R (x, Wp, Wo, q / k / v) contiguous or column windows of wider buffers; every [M, N] output is a NaN-prefilled
window of M + 1 rows whose last row is a sentinel (a ragged block that also processed row M would overwrite it); mean /
rstd / lse and the partials buffer (sized exactly by zk_gemm_ln_bwd_partials) are guarded too.  After the call every output
element is written, every guard band and sentinel row is intact, every input is bit-identical, sync_ln_errors() == 0 and
every element is inside its stage's bound.  The dropout scale is what zk_dropout_mask gives for the seed and the site.

Refusals leave every buffer bit-identical.  The 16-byte alignment refusal names the operand class ("operands must be
16-byte aligned"), not the single pointer.

The epoch word is exercised at its legitimate values around the 24-bit wrap (0xfffffd .. 0xffffff, then 1: the bump skips
0x1000000), the site counter through the wrapper's own bump at 255, and one captured graph of [ln_epoch_bump, gemm_add_ln,
gemm_ln_bwd] is replayed against the eager calls.

Worst |err| / bound per tensor seen on an MI355X (a record, profiles/chain_parity_ratios.json; no constant is taken from it):

    gemm_add_ln  (60 cases + the memory route)   s 0.990   mean 0.0062   rstd 0.029   y 0.989
    gemm_ln_bwd  (60 cases + the memory route)   ds 0.845   dy 0.663   partials 0.964
    attn_out_ln  (31 cases)   q 0.989   k 0.989   v 0.988   att 4.31e-3 (row ratio, bar 7.9e-3)   lse 3.5e-5 of its bar
                              s 0.981   mean 0.0022   rstd 0.014   y 0.988

(the CPU stand-in's: tests/test_chain_checker.py; s, y, ds and the partials are near 1 in both because one half-ulp bf16
rounding, which a correct computation reaches, makes up nearly the whole bound).  Every stored s passed the exact check as
well.  No kernel defect was found with these checks: no kernel, launch or existing assertion changed.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng  # noqa: E402
from tests import chain_ref as C  # noqa: E402
from tests import parity as P  # noqa: E402
from zero_amd import hip  # noqa: E402
from zero_amd.func import Mat  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
SEED, SID_ATTN, SID = 4242, 7, 8


def _in(t, layout, pad, off):
    """A read-only operand: contiguous, or a column window of a wider guarded buffer."""
    rows, cols = t.shape
    if layout == "contig":
        pad, off = 0, 0
    return P.guarded(rows, cols, cols + pad, off, t.dtype, t, "cuda")


def _vec(t):
    return None if t is None else P.guarded(1, t.numel(), dtype=F32, prefill=t, device="cuda")


def _ptr(gd):
    return None if gd is None else gd.window().view(-1)


def _fvec(n):
    return P.guarded(1, n, dtype=F32, device="cuda")


def _mask(e, rows, cols, p, sid):
    if not p:
        return None
    msk = torch.zeros(rows * cols, device="cuda")
    e.lib.call("zk_dropout_mask", msk.data_ptr(), rows * cols, p, e.seed.data_ptr(), sid, e.stream)
    torch.cuda.synchronize()
    return msk.view(rows, cols).cpu()


def _written(gd, what):
    gd.check_guard(what)
    v = gd.value()
    assert bool(torch.isfinite(v).all()), "%s: %d element(s) nobody wrote" % (what, int((~torch.isfinite(v)).sum()))
    return v.reshape(-1)


def _show(what, worst):
    print(what, {k: "%.3g" % v for k, v in worst.items()})


# ------------------------------------------------------------------------------------------------------- forward
class Fwd(object):
    def __init__(self, c, x):
        M, K, N = c["M"], c["K"], c["N"]
        self.c, self.x = c, x
        self.A, self.B, self.R = _in(x["A"], c["layout"], 24, 8), _in(x["B"], c["layout"], 16, 16), _in(x["R"], c["layout"], 40, 24)
        self.bias, self.gamma, self.beta = _vec(x["bias"]), _vec(x["gamma"]), _vec(x["beta"])
        self.y = C.out_rows(M, N, device="cuda")
        self.s = C.out_rows(M, N, device="cuda") if c["save"] else None
        self.mean = _fvec(M) if c["save"] else None
        self.rstd = _fvec(M) if c["save"] else None
        self.inputs = [g for g in (self.A, self.B, self.R, self.bias, self.gamma, self.beta) if g is not None]
        self.outputs = [g for g in (self.y, self.s, self.mean, self.rstd) if g is not None]

    def call(self, e, **kw):
        c = self.c
        a = dict(A=self.A.mat, B=self.B.mat, M=c["M"], N=c["N"], K=c["K"], bias=_ptr(self.bias), residual=self.R.mat,
                 gamma=_ptr(self.gamma), beta=_ptr(self.beta), y=self.y.mat, s_out=self.s.mat if self.s else None,
                 mean=_ptr(self.mean), rstd=_ptr(self.rstd), drop_p=c["drop"], sid=SID)
        a.update(kw)
        e.gemm_add_ln(**a)

    def got(self):
        M = self.c["M"]
        g = {"y": C.out_value(self.y, M, "y"), "s": None, "mean": None, "rstd": None}
        if self.s is not None:
            g["s"] = C.out_value(self.s, M, "s")
            g["mean"], g["rstd"] = _written(self.mean, "mean"), _written(self.rstd, "rstd")
        return g

    def intact(self, outputs_too=False):
        for gd in self.inputs + (self.outputs if outputs_too else []):
            gd.check_intact("operand")


def run_fwd(c):
    e = eng()
    e.set_seed(SEED)
    f = Fwd(c, C.fwd_inputs(c))
    e.ln_epoch_bump()
    f.call(e)
    torch.cuda.synchronize()
    assert e.sync_ln_errors() == 0
    got = f.got()
    f.intact()
    worst = C.check_fwd(f.x, _mask(e, c["M"], c["N"], c["drop"], SID), got, "gemm_add_ln " + C.case_id(c))
    _show("gemm_add_ln " + C.case_id(c), worst)
    return worst


@pytest.mark.parametrize("c", C.FWD_CASES, ids=C.case_id)
def test_gemm_add_ln(c):
    run_fwd(c)


# ------------------------------------------------------------------------------------------------------ backward
class Bwd(object):
    def __init__(self, e, c, x):
        M, K, N = c["M"], c["K"], c["N"]
        self.c, self.x = c, x
        self.dY, self.W = _in(x["dY"], c["layout"], 24, 8), _in(x["W"], c["layout"], 16, 16)
        self.R = _in(x["R"], c["layout"], 40, 24) if x["R"] is not None else None
        self.s = _in(x["s"], "contig", 0, 0)
        self.mean, self.rstd, self.gamma = _vec(x["mean"]), _vec(x["rstd"]), _vec(x["gamma"])
        self.ds = C.out_rows(M, N, device="cuda")
        self.dy = C.out_rows(M, N, device="cuda") if c["drop"] else None
        nfl = e.lib.query("zk_gemm_ln_bwd_partials", M, N)
        assert nfl == C.nblocks(M) * 3 * N * 4
        self.part = _fvec(nfl // 4)
        self.inputs = [g for g in (self.dY, self.W, self.R, self.s, self.mean, self.rstd, self.gamma) if g is not None]
        self.outputs = [g for g in (self.ds, self.dy, self.part) if g is not None]

    def call(self, e, **kw):
        c = self.c
        a = dict(dY=self.dY.mat, W=self.W.mat, M=c["M"], N=c["N"], K=c["K"], residual=self.R.mat if self.R else None,
                 s=self.s.mat, mean=_ptr(self.mean), rstd=_ptr(self.rstd), gamma=_ptr(self.gamma), dsum=self.ds.mat,
                 dy_out=self.dy.mat if self.dy else None, partials=_ptr(self.part), drop_p=c["drop"], sid=SID)
        a.update(kw)
        e.gemm_ln_bwd(**a)

    def got(self):
        M, N = self.c["M"], self.c["N"]
        return {"ds": C.out_value(self.ds, M, "ds"), "dy": C.out_value(self.dy, M, "dy") if self.dy else None,
                "part": _written(self.part, "partials").view(C.nblocks(M), 3, N)}

    def intact(self, outputs_too=False):
        for gd in self.inputs + (self.outputs if outputs_too else []):
            gd.check_intact("operand")


def run_bwd(c):
    e = eng()
    e.set_seed(SEED)
    b = Bwd(e, c, C.bwd_inputs(c))
    e.ln_epoch_bump()
    b.call(e)
    torch.cuda.synchronize()
    assert e.sync_ln_errors() == 0
    got = b.got()
    b.intact()
    worst = C.check_bwd(b.x, _mask(e, c["M"], c["N"], c["drop"], SID), got, "gemm_ln_bwd " + C.case_id(c))
    _show("gemm_ln_bwd " + C.case_id(c), worst)
    return worst


@pytest.mark.parametrize("c", C.BWD_CASES, ids=C.case_id)
def test_gemm_ln_bwd(c):
    run_bwd(c)


def test_the_exchange_through_memory_on_a_grid_that_would_take_the_l2_route():
    """Tuning key 15 = 1 on M = 500 (eight row blocks, the last one ragged): forward and backward."""
    e = eng()
    c = C.MEM_ROUTE_CASE
    tune = e.lib.raw("zk_tune")
    tune(15, 1)
    try:
        run_fwd({k: v for k, v in c.items() if k != "res"})
        run_bwd({k: v for k, v in c.items() if k not in ("bias", "save")})
    finally:
        tune(15, 0)


# ----------------------------------------------------------------------------------------------------- attention
class Attn(object):
    def __init__(self, c, x):
        B, nh, Lq, Lk, G, pro, Kp = (c[n] for n in ("B", "nh", "Lq", "Lk", "G", "pro", "Kp"))
        H, Tq = nh * C.ATT_D, B * Lq
        self.c, self.x, self.H, self.Tq = c, x, H, Tq
        self.inputs, self.qkv_out = [], None
        if pro == 3:
            self.qkv_out = C.out_rows(Tq, 3 * H, 3 * H + 16, 8, device="cuda")
            self.q, self.k, self.v = (self.qkv_out.mat.cols_slice(i * H, (i + 1) * H) for i in range(3))
        else:
            if pro == 1:
                self.qkv_out = C.out_rows(Tq, H, H + 8, 8, device="cuda")
                self.q = self.qkv_out.mat
            if pro == 0 and Lq == Lk and G == 1:
                qkv = P.guarded(Tq, 3 * H, 3 * H + 16, 8, BF, torch.cat([x["q"], x["k"], x["v"]], 1), "cuda")
                self.q, self.k, self.v = (qkv.mat.cols_slice(i * H, (i + 1) * H) for i in range(3))
                self.inputs.append(qkv)
            else:
                if pro == 0:
                    qg = P.guarded(Tq, H, H + 8, 8, BF, x["q"], "cuda")
                    self.q = qg.mat
                    self.inputs.append(qg)
                kv = P.guarded(x["k"].shape[0], 2 * H, 2 * H + 24, 16, BF, torch.cat([x["k"], x["v"]], 1), "cuda")
                self.k, self.v = kv.mat.cols_slice(0, H), kv.mat.cols_slice(H, 2 * H)
                self.inputs.append(kv)
        self.proj = None
        if pro:
            self.xin, self.Wp, self.bp = _in(x["x"], "win", 8, 8), _in(x["Wp"], "win", 8, 0), _vec(x["bp"])
            self.inputs += [self.xin, self.Wp, self.bp]
            self.proj = (self.xin.mat, self.Wp.mat, _ptr(self.bp), pro)
        self.Wo, self.R = _in(x["Wo"], "win", 16, 8), _in(x["R"], "win", 40, 24)
        self.bias, self.gamma, self.beta = _vec(x["bias"]), _vec(x["gamma"]), _vec(x["beta"])
        self.kmask = None if x["kmask"] is None else _in(x["kmask"].float(), "contig", 0, 0)
        self.inputs += [g for g in (self.Wo, self.R, self.bias, self.gamma, self.beta, self.kmask) if g is not None]
        self.att = C.out_rows(Tq, H, H + 32, 8, device="cuda")
        self.lse = _fvec(B * nh * Lq)
        self.y = C.out_rows(Tq, H, device="cuda")
        self.s = C.out_rows(Tq, H, device="cuda") if c["save"] else None
        self.mean = _fvec(Tq) if c["save"] else None
        self.rstd = _fvec(Tq) if c["save"] else None
        self.outputs = [g for g in (self.qkv_out, self.att, self.lse, self.y, self.s, self.mean, self.rstd) if g is not None]

    def call(self, e, **kw):
        c = self.c
        a = dict(q=self.q, k=self.k, v=self.v, att=self.att.mat, lse=_ptr(self.lse), B=c["B"], nh=c["nh"], Lq=c["Lq"], Lk=c["Lk"],
                 d=C.ATT_D, kmask=None if self.kmask is None else self.kmask.window(), causal=c["causal"], attn_drop_p=c["drop"],
                 attn_sid=SID_ATTN, Wo=self.Wo.mat, bias=_ptr(self.bias), residual=self.R.mat, gamma=_ptr(self.gamma),
                 beta=_ptr(self.beta), y=self.y.mat, s_out=self.s.mat if self.s else None, mean=_ptr(self.mean),
                 rstd=_ptr(self.rstd), drop_p=c["drop"], sid=SID, kv_group=c["G"], proj=self.proj)
        a.update(kw)
        return e.attn_out_ln(**a)

    def got(self):
        c, H, Tq = self.c, self.H, self.Tq
        g = {"q": self.x["q"], "k": self.x["k"], "v": self.x["v"]}
        if c["pro"]:
            st = C.out_value(self.qkv_out, Tq, "projected q (k, v)")
            assert bool(torch.isfinite(st.float()).all()), "projected tiles: elements nobody wrote"
            for i, n in enumerate(("q", "k", "v")[:c["pro"]]):
                g[n] = st[:, i * H:(i + 1) * H].contiguous()
        g["att"], g["lse"] = C.out_value(self.att, Tq, "att"), _written(self.lse, "lse")
        g["y"] = C.out_value(self.y, Tq, "y")
        g["s"] = g["mean"] = g["rstd"] = None
        if self.s is not None:
            g["s"], g["mean"], g["rstd"] = C.out_value(self.s, Tq, "s"), _written(self.mean, "mean"), _written(self.rstd, "rstd")
        return g

    def intact(self, outputs_too=False):
        for gd in self.inputs + (self.outputs if outputs_too else []):
            gd.check_intact("operand")


@pytest.mark.parametrize("c", C.ATTN_CASES, ids=C.case_id)
def test_attn_out_ln_with_and_without_the_projection(c):
    e = eng()
    e.set_seed(SEED)
    B, nh, Lq, Lk = c["B"], c["nh"], c["Lq"], c["Lk"]
    a = Attn(c, C.attn_inputs(c))
    e.ln_epoch_bump()
    assert a.call(e) is True, "the shape is covered: the launch must not be refused"
    torch.cuda.synchronize()
    assert e.sync_ln_errors() == 0
    got = a.got()
    a.intact()
    am = _mask(e, B * nh * Lq, Lk, c["drop"], SID_ATTN)
    masks = {"attn": None if am is None else am.view(B, nh, Lq, Lk), "tail": _mask(e, B * Lq, nh * C.ATT_D, c["drop"], SID)}
    worst = C.check_attn(c, a.x, got, masks, "attn_out_ln " + C.case_id(c))
    _show("attn_out_ln " + C.case_id(c), worst)


# ------------------------------------------------------------------------------------------------------ refusals
REFUSAL_CASE = dict(M=65, K=64, N=128, layout="win", drop=0.0, bias=True, save=True, gamma="plain", res=True)


def _raw_fwd_args(e, f, site, slots_bytes=None):
    from zero_amd.utils import dtype as zdtype
    c = f.c
    slots, meta = e.sync_ln_state(c["M"], c["N"])
    return (f.A.mat.ptr, f.B.mat.ptr, c["M"], c["N"], c["K"], f.A.mat.ld, f.B.mat.ld, hip.ptr(_ptr(f.bias)), f.R.mat.ptr, f.R.mat.ld,
            0.0, e.seed.data_ptr(), SID, _ptr(f.gamma).data_ptr(), _ptr(f.beta).data_ptr(), zdtype.epsilon(), f.s.mat.ptr,
            f.y.mat.ptr, _ptr(f.mean).data_ptr(), _ptr(f.rstd).data_ptr(), slots.data_ptr(),
            slots.numel() if slots_bytes is None else slots_bytes, meta.data_ptr(), site, meta.data_ptr() + 4, e.stream)


def test_refused_calls_name_the_argument_and_touch_nothing():
    e = eng()
    e.set_seed(SEED)
    c = REFUSAL_CASE
    M, N = c["M"], c["N"]
    f = Fwd({k: v for k, v in c.items() if k != "res"}, C.fwd_inputs(c))
    b = Bwd(e, {k: v for k, v in c.items() if k not in ("bias", "save")}, C.bwd_inputs(c))
    e.ln_epoch_bump()
    bad_ld = lambda m: Mat(m.t, m.rows, m.cols, m.ld + 4, m.off)
    need = e.lib.query("zk_gemm_add_ln_workspace", M, N)
    refused = [
        ("N=96", lambda: f.call(e, N=96)), ("N=1088", lambda: f.call(e, N=1088)),
        ("residual", lambda: f.call(e, residual=bad_ld(f.R.mat))),
        ("site", lambda: e.lib.call("zk_gemm_add_ln", *_raw_fwd_args(e, f, 0))),
        ("site", lambda: e.lib.call("zk_gemm_add_ln", *_raw_fwd_args(e, f, 256))),
        ("slots", lambda: e.lib.call("zk_gemm_add_ln", *_raw_fwd_args(e, f, 1, need - 1))),
        ("16-byte aligned", lambda: f.call(e, y=Mat(f.y.t, M, N, N, f.y.mat.off + 1))),
        ("mean / rstd", lambda: f.call(e, rstd=None)),
        ("N=96", lambda: b.call(e, N=96)),
        ("residual", lambda: b.call(e, residual=bad_ld(b.R.mat))),
        ("dy_out", lambda: b.call(e, drop_p=0.25, dy_out=None)),
    ]
    for word, fn in refused:
        with pytest.raises(hip.ZeroHipError, match=word):
            fn()
    torch.cuda.synchronize()
    assert e.sync_ln_errors() == 0
    f.intact(outputs_too=True)
    b.intact(outputs_too=True)
    # the same buffers, the call as it should be: nothing above left a trace that breaks it
    e.ln_epoch_bump()
    f.call(e)
    b.call(e)
    torch.cuda.synchronize()
    assert e.sync_ln_errors() == 0
    C.check_fwd(f.x, None, f.got(), "after the refusals")
    C.check_bwd(b.x, None, b.got(), "after the refusals")


@pytest.mark.parametrize("change", [dict(Lq=65), dict(Lk=257), dict(d=32), dict(nh=17)], ids=lambda d: "%s=%d" % next(iter(d.items())))
def test_attn_out_ln_returns_2_for_a_shape_it_does_not_cover(change):
    e = eng()
    c = dict(B=5, nh=2, Lq=13, Lk=37, G=1, pro=0, Kp=64, causal=False, mask="ragged", drop=0.0, save=True)
    a = Attn(c, C.attn_inputs(c))
    e.ln_epoch_bump()
    assert a.call(e, **change) is False
    torch.cuda.synchronize()
    assert e.sync_ln_errors() == 0
    a.intact(outputs_too=True)


# ------------------------------------------------------------------------ epoch wrap, site exhaustion, captured graph
REPEAT_CASE = dict(M=130, K=72, N=512, layout="contig", drop=0.0, bias=True, save=True, gamma="plain")


def _plain_fwd(e, x, c):
    M, N, K = c["M"], c["N"], c["K"]
    dev = lambda t: t.cuda()
    out = {"y": torch.full((M, N), float("nan"), dtype=BF, device="cuda"), "s": torch.full((M, N), float("nan"), dtype=BF, device="cuda"),
           "mean": torch.full((M,), float("nan"), device="cuda"), "rstd": torch.full((M,), float("nan"), device="cuda")}
    ops = {k: dev(x[k]) for k in ("A", "B", "R", "bias", "gamma", "beta")}
    def call():
        e.gemm_add_ln(Mat(ops["A"], M, K), Mat(ops["B"], K, N), M, N, K, ops["bias"], Mat(ops["R"], M, N), ops["gamma"], ops["beta"],
                      Mat(out["y"], M, N), Mat(out["s"], M, N), out["mean"], out["rstd"])
    return ops, out, call


def _zero_exchange_state(e):
    torch.cuda.synchronize()
    e._sync_ln[0].zero_()
    if e.__dict__.get("_sync_flags") is not None:
        e._sync_flags.zero_()
    torch.cuda.synchronize()


def test_the_epoch_word_wraps_past_24_bits_without_a_trace():
    """0xfffffd -> fe, ff, 1 (0x1000000 is skipped: its low 24 bits are the never-published tag 0), 2, 3, 4: six launches on
    two alternating inputs, each bit-equal to the same input's result from before the wrap.  The slots are zero-filled
    around the test (as at the engine's start), since epochs that small have been used by this process before; the word
    is put back afterwards."""
    e = eng()
    c = REPEAT_CASE
    runs = [_plain_fwd(e, C.fwd_inputs(c, seed), c) for seed in (0, 1)]
    want = []
    for ops, out, call in runs:
        e.ln_epoch_bump()
        call()
        torch.cuda.synchronize()
        want.append({k: v.clone() for k, v in out.items()})
        C.check_fwd({k: v.cpu() for k, v in ops.items()}, None, {k: v.cpu() for k, v in out.items()}, "before the wrap")
    assert not torch.equal(want[0]["y"], want[1]["y"]) and e.sync_ln_errors() == 0
    meta = e.sync_ln_state(1, 64)[1]
    old = int(meta[0].item())
    _zero_exchange_state(e)
    try:
        meta[0:1].fill_(0xfffffd)
        torch.cuda.synchronize()
        words = []
        for it in range(6):
            ops, out, call = runs[it % 2]
            for t in out.values():
                t.fill_(float("nan"))
            e.ln_epoch_bump()
            call()
            torch.cuda.synchronize()
            words.append(int(meta[0].item()))
            for k in out:
                assert torch.equal(out[k], want[it % 2][k]), (it, k, hex(words[-1]))
        assert words == [0xfffffe, 0xffffff, 1, 2, 3, 4], [hex(w) for w in words]
        assert e.sync_ln_errors() == 0
    finally:
        _zero_exchange_state(e)
        meta[0:1].fill_(old)
        torch.cuda.synchronize()


def test_three_hundred_calls_without_a_manual_bump():
    """The wrapper bumps the epoch when the sites of a pass run out (255): the last call is bit-equal to the first."""
    e = eng()
    c = dict(REPEAT_CASE, M=65, N=128)
    ops, out, call = _plain_fwd(e, C.fwd_inputs(c), c)
    e.ln_epoch_bump()
    epoch0 = int(e.sync_ln_state(1, 64)[1][0].item())
    call()
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in out.items()}
    C.check_fwd({k: v.cpu() for k, v in ops.items()}, None, {k: v.cpu() for k, v in first.items()}, "first call")
    for it in range(299):
        if it == 298:
            for t in out.values():
                t.fill_(float("nan"))
        call()
    torch.cuda.synchronize()
    assert e.sync_ln_errors() == 0
    assert int(e.sync_ln_state(1, 64)[1][0].item()) == epoch0 + 1 and e._sync_site == 300 - 255
    for k in out:
        assert torch.equal(out[k], first[k]), k


def test_a_captured_graph_replays_the_eager_calls_bit_for_bit():
    """[ln_epoch_bump, gemm_add_ln, gemm_ln_bwd] captured once, replayed three times with the inputs overwritten in place."""
    e = eng()
    c = dict(REPEAT_CASE, M=130, N=256, res=True)
    M, N, K = c["M"], c["N"], c["K"]
    with torch.cuda.stream(e.work_stream):
        ops, out, fwd = _plain_fwd(e, C.fwd_inputs(c), c)
        xb = C.bwd_inputs(c)
        bops = {k: xb[k].cuda() for k in ("dY", "W", "R", "gamma")}
        bout = {"ds": torch.full((M, N), float("nan"), dtype=BF, device="cuda"),
                "part": torch.full((e.lib.query("zk_gemm_ln_bwd_partials", M, N) // 4,), float("nan"), device="cuda")}

        def body():
            e.ln_epoch_bump()
            fwd()
            e.gemm_ln_bwd(Mat(bops["dY"], M, K), Mat(bops["W"], N, K), M, N, K, Mat(bops["R"], M, N), Mat(out["s"], M, N),
                          out["mean"], out["rstd"], bops["gamma"], Mat(bout["ds"], M, N), None, bout["part"])

        def load(seed):
            x, xb2 = C.fwd_inputs(c, seed), C.bwd_inputs(c, seed)
            for k in ("A", "R"):
                ops[k].copy_(x[k].cuda())
            bops["dY"].copy_(xb2["dY"].cuda())
            for t in list(out.values()) + list(bout.values()):
                t.fill_(float("nan"))
            torch.cuda.synchronize()

        body()                                              # (eager once: sizes the exchange state)
        torch.cuda.synchronize()
        g = e.graph_capture(body)
        torch.cuda.synchronize()
        for seed in (1, 0, 2):
            load(seed)
            body()
            torch.cuda.synchronize()
            eager = {k: v.clone() for k, v in list(out.items()) + list(bout.items())}
            assert all(bool(torch.isfinite(v.float()).all()) for v in eager.values())
            load(seed)
            e.graph_launch(g)
            torch.cuda.synchronize()
            for k, v in list(out.items()) + list(bout.items()):
                assert torch.equal(v, eager[k]), (seed, k)
        assert e.sync_ln_errors() == 0
