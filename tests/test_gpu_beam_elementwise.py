"""The beam-search tail kernels of zero_amd/csrc/zk_decode.hip against the references, bounds and case tables of
tests/beam_ref.py: zk_beam_topk (every path: chunked NV = 4 / NV = 8, the row fallback, scalar loads, both sides of the two
topk_chunks boundaries), zk_beam_dev_prepare / zk_beam_dev_advance / zk_beam_topk_advance called directly on a guarded
arena, zk_gather_rows_ex byte for byte, zk_add_gumbel element by element.  Every operand sits between guard bands, every
output starts as NaN or as a sentinel, and every guard is checked after the call.  tests/test_beam_checker.py shows on
the CPU that the same checks fail for planted defects.  Logits are finite everywhere (the kernels' precondition)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng  # noqa: E402
from tests import beam_ref as R  # noqa: E402
from tests import parity as P  # noqa: E402

DEV = "cuda"
F32 = torch.float32
DECISIVE_FLOOR = R.DECISIVE_FLOOR    # (the c_exp needed and the largest ratios are printed: profiles/elemkernel_parity_constants.json)


def _sync():
    torch.cuda.synchronize()


def _logits(z, ld, off=0):
    return P.guarded(z.shape[0], z.shape[1], ld=ld, off=off, dtype=F32, prefill=torch.from_numpy(z), device=DEV)


class _TopkCall(object):
    """One zk_beam_topk call on guarded operands: logits (read-only), prev (read-only), NaN-prefilled scores,
    sentinel-prefilled indices, a workspace of exactly zk_beam_topk_workspace bytes (or ``ws_bytes``)."""

    def __init__(self, z, prev, B, K, V, ld, k2, off=0, ws_bytes=None):
        e = eng()
        self.B, self.K, self.V, self.ld, self.k2 = B, K, V, ld, k2
        self.need = e.lib.query("zk_beam_topk_workspace", B, K, min(k2, R.TOPK_MAX))
        assert self.need == R.topk_workspace(B, K, min(k2, R.TOPK_MAX))
        self.ws_bytes = self.need if ws_bytes is None else ws_bytes
        self.lg = _logits(z, ld, off)
        self.prev = R.GuardedWords(B * K, np.asarray(prev, dtype=np.float32), DEV)
        self.ts = R.GuardedWords(B * k2, R.NAN_WORD, DEV)
        self.ti = R.GuardedWords(B * k2, R.SENTINEL, DEV)
        self.ws = R.GuardedWords(self.need // 4, R.SENTINEL, DEV)

    def run(self, temp, pen, forbid, scal=None):
        e = eng()
        self.scal = None if scal is None else R.GuardedWords(2, scal, DEV)
        rc = e.lib.raw("zk_beam_topk")(self.lg.mat.ptr, self.prev.ptr, self.ts.ptr, self.ti.ptr, self.B, self.K, self.V,
                                       self.ld, self.k2, float(temp), float(pen), int(forbid), R.FORBID_VALUE,
                                       None if scal is None else self.scal.ptr, self.ws.ptr, self.ws_bytes, e.stream)
        _sync()
        return rc

    def check_guards(self, what):
        self.lg.check_intact(what + " logits")
        self.prev.check_intact(what + " prev")
        if self.scal is not None:
            self.scal.check_intact(what + " scal_dev")
        for name, g in (("scores", self.ts), ("indices", self.ti), ("workspace", self.ws)):
            g.check_guard(what + " " + name)

    def result(self):
        return (self.ts.words().view(np.float32).reshape(self.B, self.k2),
                self.ti.words().astype(np.int64).reshape(self.B, self.k2))


@functools.lru_cache(maxsize=None)
def _shape_inputs(i):
    return R.topk_inputs(R.TOPK_SHAPES[i])


@pytest.mark.parametrize("i", range(len(R.TOPK_SHAPES)), ids=lambda i: R.TOPK_SHAPES[i]["note"])
def test_beam_topk(i):
    s = R.TOPK_SHAPES[i]
    B, K, V, ld, k2 = s["B"], s["K"], s["V"], s["ld"], s["k2"]
    z, prev = _shape_inputs(i)
    worst, ratio = 0.0, 0.0
    for temp, pen, forbid, dev in R.topk_variants(s):
        what = "zk_beam_topk %s (%s) T=%g forbid=%d scal_dev=%d" % (s["note"], R.topk_path(K, V, k2), temp, forbid, dev)
        call = _TopkCall(z, prev, B, K, V, ld, k2, off=s["off"])
        if dev:                                               # the per-step scalars from the device: decoys in the arguments
            rc = call.run(temp, 99.0, -1, R.scal_words(pen, forbid))
        else:
            rc = call.run(temp, pen, forbid)
        assert rc == 0, what
        call.check_guards(what)
        gs, gi = call.result()
        ref, bound, fixed, shape = R.topk_ref(z, prev, K, V, R.inv_temp_of(temp), pen, forbid, R.FORBID_VALUE, terms=True)
        share = R.assert_topk(gs, gi, ref, bound, K, V, what)
        need = R.topk_c_exp_needed(gs, gi, ref, fixed, shape)
        worst = max(worst, need)
        ratio = max(ratio, R.topk_ratio(gs, gi, ref, bound))
        print("%s: decisive share %.2f, c_exp needed %.3g" % (what, share, need))
        assert share >= DECISIVE_FLOOR, what
        if s["kind"] == "step0":                              # every survivor of step 0 comes from beam 0
            assert (gi // V == 0).all(), what
    print("TOPK_C_EXP_NEEDED %s: %.4g of C_EXP = %g; largest |err| / bound %.4g" % (s["note"], worst, P.C_EXP, ratio))


@pytest.mark.parametrize("family", R.EXACT_FAMILIES)
@pytest.mark.parametrize("K,V,ld,k2", R.EXACT_SHAPES)
def test_beam_topk_exact_order(K, V, ld, k2, family):
    c = R.topk_exact_case(K, V, k2, family)
    what = "zk_beam_topk exact %s K=%d V=%d ld=%d (%s)" % (family, K, V, ld, R.topk_path(K, V, k2))
    call = _TopkCall(c["logits"], c["prev"], c["B"], K, V, ld, k2)
    assert call.run(1.0, c["penalty"], c["forbid"]) == 0, what
    call.check_guards(what)
    gs, gi = call.result()
    P.assert_exact(torch.from_numpy(gi), torch.from_numpy(c["expect"]), what)
    ref, bound = R.topk_ref(c["logits"], c["prev"], K, V, R.inv_temp_of(1.0), c["penalty"], c["forbid"], R.FORBID_VALUE)
    R.assert_topk(gs, gi, ref, bound, K, V, what)


@pytest.mark.parametrize("bad", ["k2 > 16", "V < k2", "workspace one byte short"])
def test_beam_topk_argument_errors_write_nothing(bad):
    B, K, V, k2 = 2, 2, 40, 4
    ws_bytes = None
    if bad == "k2 > 16":
        k2 = 17
    elif bad == "V < k2":
        V = 3
    else:
        ws_bytes = R.topk_workspace(B, K, k2) - 1
    rng = np.random.default_rng(3)
    z, prev = rng.standard_normal((B * K, V)).astype(np.float32), rng.standard_normal(B * K).astype(np.float32)
    call = _TopkCall(z, prev, B, K, V, V, k2, ws_bytes=ws_bytes)
    assert call.run(1.0, 1.5, -1) != 0, bad
    call.check_guards(bad)
    for g in (call.ts, call.ti, call.ws):
        g.check_intact(bad + ": prefilled output")


# ---------------------------------------------------------------------------------------------- bookkeeping
def _dev_call(name, arena, cfg):
    e = eng()
    e.lib.call(name, *(arena.args(cfg) + [e.stream]))
    _sync()


def _fused(arena, cfg, lg, ws, temp):
    e = eng()
    rc = e.lib.raw("zk_beam_topk_advance")(lg.mat.ptr, lg.ld, float(temp), R.FORBID_VALUE, ws.ptr, 4 * ws.n,
                                           *(arena.args(cfg) + [e.stream]))
    _sync()
    return rc


def _workspace(cfg):
    return R.GuardedWords(R.topk_workspace(cfg["B"], cfg["K"], 2 * cfg["K"]) // 4, R.SENTINEL, DEV)


@pytest.mark.parametrize("scenario", list(R.BOOK_SCENARIOS))
@pytest.mark.parametrize("B", R.BOOK_B)
@pytest.mark.parametrize("K", R.BOOK_K)
def test_beam_dev_prepare_and_advance_against_book_ref(K, B, scenario):
    """Several steps on synthetic survivors (sorted scores, exact ties, EOS symbols, length caps incl. 0 and 1), every array
    of the state bit for bit after each launch; then the stop: ctrl[1] = 1 and further launches change nothing."""
    cfg, finish_at = R.book_scenario(scenario, B, K)
    d = R.dev_init(cfg)
    arena = R.Arena(d, DEV)
    cause = None
    for step in range(cfg["Tcap"] + 1):
        what = "K=%d B=%d %s step %d" % (K, B, scenario, step)
        want, cause = R.dev_prepare_expected(d, cfg)
        _dev_call("zk_beam_dev_prepare", arena, cfg)
        R.assert_book_equal(arena.read(what), want, what + " prepare")
        if cause is not None:
            break
        time = int(want["ctrl"][0]) - 1
        assert list(want["stepbuf"][:3]) == [time, int(want["pen_table"][time:time + 1].view(np.int32)[0]),
                                             cfg["eos"] if time == 0 else -1]
        want["topk_scores"], want["topk_idx"] = R.book_survivors(cfg, time, seed=K, finish_at=finish_at)
        arena.write("topk_scores", want["topk_scores"])
        arena.write("topk_idx", want["topk_idx"])
        d = R.dev_advance_expected(want, cfg)
        _dev_call("zk_beam_dev_advance", arena, cfg)
        got = arena.read(what)
        R.assert_book_equal(got, d, what + " advance")
        n = time + 2                                          # the columns beyond time + 1 still hold the sentinel
        assert (got["seq"][:, :, n:] == R.SENTINEL).all() and (got["fin_seq"][:, :, n:] == R.SENTINEL).all(), what
    # (which cause the reference finds per scenario, K and B: tests/test_beam_checker.py test_book_scenarios_stop_for_their_cause)
    assert cause in ("length", "bound") and int(want["ctrl"][1]) == 1 and int(want["ctrl"][2]) == 0 and step >= 2
    # replays past the stop: a further prepare + advance and a further fused launch change no byte but the top-k scratch
    frozen = arena.read("frozen")
    _dev_call("zk_beam_dev_prepare", arena, cfg)
    _dev_call("zk_beam_dev_advance", arena, cfg)
    R.assert_book_equal(arena.read("replay"), frozen, "K=%d B=%d %s: prepare + advance past the stop" % (K, B, scenario))
    if 2 * K <= R.TOPK_MAX:
        z = (np.random.default_rng(K).standard_normal((B * K, cfg["V"])) * 2).astype(np.float32)
        lg, ws = _logits(z, cfg["V"] + 2), _workspace(cfg)
        assert _fused(arena, cfg, lg, ws, 1.0) == 0
        lg.check_intact("logits"); ws.check_guard("workspace")
        R.assert_book_equal(arena.read("fused replay"), frozen, "K=%d B=%d %s: zk_beam_topk_advance past the stop" %
                            (K, B, scenario), skip=R.BOOK_SCRATCH)


def test_beam_dev_last_legal_step_and_overflow_branch():
    """Tmax = 3 with sentences that would go on: the step time = Tmax - 1 writes column Tmax and not column Tmax + 1;
    the prepare after it finds ctrl[0] = Tmax, sets ctrl[1] = ctrl[2] = 1 and writes nothing else."""
    cfg = R.book_cfg(3, 4, R.BOOK_V, 3, [9, 9, 9])
    d = R.dev_init(cfg)
    arena = R.Arena(d, DEV)
    for time in range(cfg["Tmax"]):
        want, cause = R.dev_prepare_expected(d, cfg)
        assert cause is None
        _dev_call("zk_beam_dev_prepare", arena, cfg)
        want["topk_scores"], want["topk_idx"] = R.book_survivors(cfg, time, seed=1)
        want["topk_idx"][want["topk_idx"] % cfg["V"] == cfg["eos"]] += 1          # nobody finishes: the search would go on
        arena.write("topk_scores", want["topk_scores"])
        arena.write("topk_idx", want["topk_idx"])
        d = R.dev_advance_expected(want, cfg)
        _dev_call("zk_beam_dev_advance", arena, cfg)
        got = arena.read("step %d" % time)
        R.assert_book_equal(got, d, "Tmax = 3, step %d" % time)
    assert (got["seq"][:, :, cfg["Tmax"]] != R.SENTINEL).all() and (got["seq"][:, :, cfg["Tmax"] + 1] == R.SENTINEL).all()
    assert (got["fin_seq"][:, :, cfg["Tmax"] + 1] == R.SENTINEL).all()
    want, cause = R.dev_prepare_expected(d, cfg)
    assert cause == "overflow" and list(want["ctrl"][:3]) == [cfg["Tmax"], 1, 1]
    _dev_call("zk_beam_dev_prepare", arena, cfg)
    R.assert_book_equal(arena.read("overflow"), want, "the overflow branch")
    _dev_call("zk_beam_dev_advance", arena, cfg)
    R.assert_book_equal(arena.read("overflow"), want, "advance after the overflow")


@pytest.mark.parametrize("K,V,ld,off,temp", R.FUSED_CASES)
def test_beam_topk_advance_equals_the_two_calls(K, V, ld, off, temp):
    """zk_beam_topk_advance against zk_beam_topk(scal_dev = stepbuf + 1, penalty 1, forbid -1) + zk_beam_dev_advance on the
    same logits and the same starting arena: every byte equal, at step 0 (the ban on) and at a later step.  The survivors
    are also held against topk_ref and the state against book_ref."""
    e = eng()
    B = 3
    cfg = R.book_cfg(B, K, V, 4, [9, 9, 9])
    a, b = R.Arena(R.dev_init(cfg), DEV), R.Arena(R.dev_init(cfg), DEV)
    for step in range(2):
        what = "fused K=%d V=%d ld=%d off=%d (%s) step %d" % (K, V, ld, off, R.topk_path(K, V, 2 * K), step)
        z = (np.random.default_rng(50 + step + V + K).standard_normal((B * K, V)) * 2).astype(np.float32)
        lg, wa, wb = _logits(z, ld, off), _workspace(cfg), _workspace(cfg)
        _dev_call("zk_beam_dev_prepare", a, cfg)
        _dev_call("zk_beam_dev_prepare", b, cfg)
        before = a.read(what)
        assert int(before["ctrl"][1]) == 0 and int(before["stepbuf"][0]) == step
        assert _fused(a, cfg, lg, wa, temp) == 0, what
        e.lib.call("zk_beam_topk", lg.mat.ptr, b.buf["prev"].ptr, b.buf["topk_scores"].ptr, b.buf["topk_idx"].ptr, B, K, V,
                   ld, 2 * K, float(temp), 1.0, -1, R.FORBID_VALUE, b.buf["stepbuf"].ptr + 4, wb.ptr, 4 * wb.n, e.stream)
        _dev_call("zk_beam_dev_advance", b, cfg)
        lg.check_intact(what + " logits"); wa.check_guard(what + " workspace"); wb.check_guard(what + " workspace")
        ga, gb = a.read(what), b.read(what)
        R.assert_book_equal(ga, gb, what + ": fused against split")
        # the survivors against the float64 reference, the state against book_ref on the kernel's own survivors
        pen = before["stepbuf"][1:2].view(np.float32)[0]
        forbid = int(before["stepbuf"][2])
        assert forbid == (cfg["eos"] if step == 0 else -1)
        ref, bound = R.topk_ref(z, before["prev"], K, V, R.inv_temp_of(temp), pen, forbid, R.FORBID_VALUE)
        share = R.assert_topk(ga["topk_scores"], ga["topk_idx"], ref, bound, K, V, what)
        assert share >= DECISIVE_FLOOR, what
        before["topk_scores"], before["topk_idx"] = ga["topk_scores"], ga["topk_idx"]
        R.assert_book_equal(ga, R.dev_advance_expected(before, cfg), what + ": book_ref on the kernel's survivors")
        # and book_ref on topk_ref's survivors, wherever the sentence is decisive
        order = R.topk_order(ref, 2 * K)
        want = R.dev_advance_expected(before, cfg, ts=np.take_along_axis(ref, order, 1).astype(np.float32),
                                      ti=order.astype(np.int32))
        dec = R.topk_decisive(ref, bound, 2 * K)
        for name in ("seq", "flat_idx", "next_tok"):
            g, w = ga[name].reshape(B, -1), want[name].reshape(B, -1)
            assert np.array_equal(g[dec], w[dec]), (what, name)


def test_beam_topk_advance_returns_minus_2_where_the_top_k_is_not_chunked():
    e = eng()
    B, K, V = 1, 8, 16379
    assert R.topk_chunks(K, V, 2 * K) == 0 and R.topk_chunks(K, V - 1, 2 * K) == 2
    cfg = R.book_cfg(B, K, V, 4, [9])
    arena = R.Arena(R.dev_init(cfg), DEV)
    _dev_call("zk_beam_dev_prepare", arena, cfg)
    before = arena.read("before")
    z = np.random.default_rng(1).standard_normal((B * K, V)).astype(np.float32)
    lg, ws = _logits(z, V), _workspace(cfg)
    assert _fused(arena, cfg, lg, ws, 1.0) == -2
    ws.check_intact("workspace after -2")
    R.assert_book_equal(arena.read("after"), before, "the arena after the -2 return")
    for buf in arena.buf.values():
        buf.check_guard("arena after -2")


# ---------------------------------------------------------------------------------------------- zk_gather_rows_ex
def _gather(rows, src_rows, row_bytes, index, period, pad=8, off=4):
    e = eng()
    cols = row_bytes // 4
    g = torch.Generator(device="cpu"); g.manual_seed(rows + cols)
    src = P.guarded(src_rows, cols, ld=cols + pad, off=off, dtype=F32, prefill=torch.randn(src_rows, cols, generator=g), device=DEV)
    dst = P.guarded(rows, cols, ld=cols + 2 * pad, off=2 * off, dtype=F32, device=DEV)
    idx = None if index is None else R.GuardedWords(len(index), np.asarray(index, dtype=np.int32), DEV)
    rc = e.lib.raw("zk_gather_rows_ex")(src.mat.ptr, 4 * src.ld, None if idx is None else idx.ptr, dst.mat.ptr, 4 * dst.ld,
                                        rows, row_bytes, period, e.stream)
    _sync()
    src.check_intact("gather src")
    if idx is not None:
        idx.check_intact("gather index")
    dst.check_guard("gather dst")
    return rc, src.value().view(torch.int32), dst.value().view(torch.int32)


@pytest.mark.parametrize("row_bytes", [16, 4096, 4112, 266240])
def test_gather_rows_ex_byte_exact(row_bytes):
    """4112 bytes: gridDim.y = 2 with a ragged tail; 266 240 bytes = 16 640 uint4 > 64 * 256: the gy = 64 cap, the inner loop
    iterates.  period = 0 with repeats and with a NULL index; period = 5: three tables, each gathers from its own block."""
    index = [3, 3, 0, 5]
    rc, s, d = _gather(4, 6, row_bytes, index, 0)
    assert rc == 0 and torch.equal(d, s[index]), "period 0"
    rc, s, d = _gather(4, 4, row_bytes, None, 0)
    assert rc == 0 and torch.equal(d, s), "NULL index"
    if row_bytes <= 4112:
        index = [4, 0, 0, 3, 1]
        rc, s, d = _gather(15, 15, row_bytes, index, 5)
        want = torch.cat([s[5 * t + torch.tensor(index)] for t in range(3)])
        assert rc == 0 and torch.equal(d, want), "period 5"


def test_gather_rows_ex_empty_and_argument_errors():
    e = eng()

    def call(rows, row_bytes, period, src_stride=None, dst_stride=None):
        src = P.guarded(6, 16, ld=24, off=4, dtype=F32, prefill=torch.ones(6, 16), device=DEV)
        dst = P.guarded(6, 16, ld=32, off=8, dtype=F32, device=DEV)
        idx = R.GuardedWords(6, np.array([3, 3, 0, 5, 1, 2], dtype=np.int32), DEV)
        rc = e.lib.raw("zk_gather_rows_ex")(src.mat.ptr, 96 if src_stride is None else src_stride, idx.ptr, dst.mat.ptr,
                                            128 if dst_stride is None else dst_stride, rows, row_bytes, period, e.stream)
        _sync()
        dst.check_intact("dst of a call that must write nothing")
        return rc
    assert call(0, 64, 0) == 0 and call(4, 0, 0) == 0
    assert call(4, 60, 0) != 0 and call(4, 64, 0, src_stride=100) != 0 and call(4, 64, 0, dst_stride=120) != 0
    assert call(4, 64, 3) != 0                               # rows % period != 0


# ---------------------------------------------------------------------------------------------- zk_add_gumbel
def _gumbel(case, x0, sid=None):
    e = eng()
    rows, V, ld, seed, sid0 = case
    lg = P.guarded(rows, V, ld=ld, off=0, dtype=F32, prefill=x0, device=DEV)
    e.set_seed(seed)
    e.lib.call("zk_add_gumbel", lg.mat.ptr, rows, V, ld, R.GUMBEL_EPS, e.seed.data_ptr(), sid0 if sid is None else sid,
               e.stream)
    _sync()
    lg.check_guard("zk_add_gumbel %r" % (case,))             # the pad columns [V, ld) are outside the window
    return lg.value()


@pytest.mark.parametrize("case", R.GUMBEL_CASES, ids=lambda c: "%dx%d" % c[:2])
def test_add_gumbel_elementwise(case):
    """out = x + noise: gumbel_ref's bound plus one rounding of the addition (PER_TERM of the result).  The reference
    counter is r * V + c: a kernel that formed it with ld would miss every row but the first."""
    rows, V, ld, seed, sid = case
    g = torch.Generator(device="cpu"); g.manual_seed(rows * V)
    x0 = torch.randn(rows, V, generator=g) * 3
    ref, bound = R.gumbel_case_ref(case)
    assert R.gumbel_wide_share(bound) <= R.GUMBEL_CAP_SHARE
    want = torch.from_numpy(ref) + x0.double()
    tol = torch.from_numpy(bound) + P.PER_TERM * want.abs()
    got = _gumbel(case, x0)
    P.assert_elementwise(got, want, tol, "zk_add_gumbel %r" % (case,))
    print("GUMBEL_RATIO %r: largest |err| / bound %.4g" % (case, P.ratio(got, want, tol)))
    assert torch.equal(_gumbel(case, x0), got)               # the same seed and sid add the same noise
    assert not torch.equal(_gumbel(case, x0, sid=sid + 1), got)      # another sid, other noise
