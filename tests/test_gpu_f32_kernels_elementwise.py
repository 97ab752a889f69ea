"""The fp32 decode kernels of zero_amd/csrc/zk_f32.hip, called through the C ABI on the tables of tests/f32_ref.py: zk_f32_gemm
(all 17 instantiations under the default dispatch), zk_f32_add_ln / zk_f32_ln_fused, zk_f32_embed / zk_f32_embed_step,
zk_f32_aan_step / zk_f32_gate and zk_f32_attn / zk_f32_attn_kb.  Every operand and output is a parity.guarded window: outputs
are prefilled with NaN, nothing outside a window may change, every input must be bit-identical after the call, and every row
stride an entry point takes is larger than the row (GEMM and attention; the row kernels take none).  Results are held to the
derived element-wise bounds of f32_ref (nothing there is fitted to these kernels) or to bit equality; a refused call must
leave every buffer untouched.  tests/test_f32_checker.py shows on the CPU that these checks pass on what a correct kernel
computes and fail on each planted defect.  Every test prints the largest |err| / bound it saw (pytest -s).

Found: nothing wrong in any kernel; every bound is met with room and every bit-for-bit check holds.  Largest |err| / bound on an
MI355X: gemm 0.042 (random data; the integer data is exact in all 17 forms, both layouts), LayerNorm 0.064 (H = 4) falling to
0.001 at H = 2048 (the bound counts H worst-case roundings), embedding 0.47 of the 2 ulp the fused multiply-add is allowed,
gate 0.49, attention 0.006 (score_f32_ref's worst-case bound; fp32 errors grow like the root of the term count)."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng  # noqa: E402
from tests import parity as P  # noqa: E402
from tests import f32_ref as R  # noqa: E402
from zero_amd.hip import ZeroHipError  # noqa: E402

LEAD = P.LEAD


def G(rows, cols, ld=None, off=0, prefill=None):
    return P.guarded(rows, cols, ld, off, torch.float32, None if prefill is None else torch.as_tensor(np.asarray(prefill, np.float32)),
                     "cuda")


class IntBuf(object):
    """An int32 operand (ids, a device scalar) with LEAD guard words on both sides."""

    def __init__(self, data):
        data = np.asarray(data, np.int32).reshape(-1)
        raw = np.full(data.size + 2 * LEAD, 0x4ACE4ACE, np.int32)
        raw[LEAD:LEAD + data.size] = data
        self.before = raw.copy()
        self.t = torch.as_tensor(raw).cuda()
        self.ptr = self.t.data_ptr() + 4 * LEAD

    def check_intact(self, what):
        assert np.array_equal(self.t.cpu().numpy(), self.before), "%s: a read-only int32 operand changed" % what


def ptr(buf):
    return None if buf is None else (buf.ptr if isinstance(buf, IntBuf) else buf.mat.ptr)


def val(buf):
    return buf.value().numpy()


def call(name, *args):
    e = eng()
    return e.lib.call(name, *(args + (e.stream,)))


def finish(inputs=(), outputs=()):
    """After a call: every input bit-identical, nothing written outside an output's window."""
    torch.cuda.synchronize()
    for i, b in enumerate(b for b in inputs if b is not None):
        b.check_intact("input %d" % i)
    for i, b in enumerate(b for b in outputs if b is not None):
        b.check_guard("output %d" % i)


def dev_or_host(where, value, wrong):
    """-> (host argument, device buffer or None): a value given on the device comes with a WRONG host argument."""
    return (value, None) if where == "host" else (wrong, IntBuf([value]))


# ---------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("name", list(R.GEMM_CASES))
def test_gemm(name):
    M, N, K, tb = R.GEMM_CASES[name]
    assert eng().lib.raw("zk_f32_gemm_legacy")(-1) == 0, "the A/B switch is not at its default"
    rb, cb = (N, K) if tb else (K, N)
    worst = 0.0
    for data in R.GEMM_DATA:
        x = R.gemm_inputs(name, data)
        refs = {(bias, act): R.gemm_ref(name, x, bias, act) for bias in (0, 1) for act in (0, 1)}
        bv = G(1, N, prefill=x["bias"])
        for lay in R.GEMM_LAYOUTS:
            L = R.gemm_layout(M, N, K, tb, lay)
            A, B = G(M, K, L["lda"], L["offa"], x["a"]), G(rb, cb, L["ldb"], L["offb"], x["b"])
            for bias, act in itertools.product((0, 1), (0, 1)):
                C = G(M, N, L["ldc"], L["offc"])
                call("zk_f32_gemm", ptr(A), ptr(B), ptr(C), M, N, K, L["lda"], L["ldb"], L["ldc"], tb, ptr(bv) if bias else None, act)
                finish((A, B, bv), (C,))
                ref, bound = refs[(bias, act)]
                what = "gemm %s %s %s bias=%d act=%d (%s)" % (name, lay, data, bias, act, "/".join(map(str, R.route(M, N, K, tb, L["ldb"]))))
                worst = max(worst, R.gemm_check(val(C), ref, bound, data, what))
    print("gemm %s: largest |err| / bound %.3f (random data; the integer data is exact)" % (name, worst))


# ---------------------------------------------------------------------------------------------- LayerNorm family
def _ln_run(cs, x):
    rows, H = cs["rows"], cs["H"]
    gam, bet, out = G(1, H, prefill=x["gamma"]), G(1, H, prefill=x["beta"]), G(rows, H)
    cache = cat = tdev = None
    time = cs["time"]
    if cs.get("aan"):
        cache, cat = G(rows, H, prefill=x["cache0"]), G(rows, 2 * H)
        time, tdev = dev_or_host(cs["aan"], cs["time"], cs["time"] + 93)
    if cs.get("gate"):
        ins = [G(rows, 2 * H, prefill=x["z"]), G(rows, 2 * H, prefill=x["cat_in"])]
        args = (None, None, ptr(ins[0]), ptr(ins[1]))
    else:
        ins = [G(rows, H, prefill=x["x"]), None if x["y"] is None else G(rows, H, prefill=x["y"])]
        args = (ptr(ins[0]), ptr(ins[1]), None, None)
    if cs["entry"] == "add_ln":
        call("zk_f32_add_ln", args[0], args[1], ptr(gam), ptr(bet), ptr(out), rows, H, cs["eps"])
    else:
        call("zk_f32_ln_fused", *(args + (ptr(gam), ptr(bet), ptr(out), rows, H, cs["eps"], ptr(cache), ptr(cat), time, ptr(tdev))))
    finish(ins + [gam, bet, tdev], (out, cache, cat))
    got = {"out": val(out)}
    if cache is not None:
        got["cache"], got["cat"] = val(cache), val(cat)
    return got


LN_GROUPS = {}
for _n in R.ln_case_names():
    LN_GROUPS.setdefault("/".join(_n.split("/")[:2]), []).append(_n)


@pytest.mark.parametrize("group", list(LN_GROUPS))
def test_layernorm(group):
    worst = 0.0
    for name in LN_GROUPS[group]:
        cs = R.ln_case(name)
        x = R.ln_inputs(cs)
        worst = max(worst, R.ln_check(cs, x, _ln_run(cs, x)))
    print("ln %s: largest |err| / bound %.3f over %d cases" % (group, worst, len(LN_GROUPS[group])))


# ---------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("name", list(R.EMBED_CASES))
def test_embed(name):
    cs, x = R.EMBED_CASES[name], R.embed_inputs(name)
    rows, H = cs["rows"], cs["H"]
    ids, table, bias = IntBuf(x["ids"]), G(R.EMB_V, H, prefill=x["table"]), G(1, H, prefill=x["bias"])
    timing, out = G(R.EMB_TIMING_ROWS, H, prefill=x["timing"]), G(rows, H)
    pos0, pdev = dev_or_host(cs["pos"][0], cs["pos"][1], cs["pos"][1] + 1)
    cache = cat = flag = None
    if cs["entry"] == "embed":
        flag = None if cs["flag"] is None else IntBuf([cs["flag"]])
        call("zk_f32_embed", ids.ptr, rows, cs["L"], ptr(table), ptr(bias), ptr(timing), R.EMB_TIMING_ROWS, ptr(out), H,
             float(x["scale"]), pos0, ptr(pdev), ptr(flag))
    else:
        if cs["aan"]:
            cache, cat = G(rows, H, prefill=x["cache0"]), G(rows, 2 * H)
        call("zk_f32_embed_step", ids.ptr, rows, ptr(table), ptr(bias), ptr(timing), R.EMB_TIMING_ROWS, ptr(out), H,
             float(x["scale"]), pos0, ptr(pdev), cs["pad_id"], ptr(cache), ptr(cat))
    finish((ids, table, bias, timing, pdev, flag), (out, cache, cat))
    got = {"out": val(out)}
    if cache is not None:
        got["cache"], got["cat"] = val(cache), val(cat)
    print("embed %s: largest |err| / bound %.3f" % (name, R.embed_check(name, x, got)))


# ---------------------------------------------------------------------------------------------- aan_step / gate
@pytest.mark.parametrize("where", ["host", "dev"])
@pytest.mark.parametrize("name", list(R.ROW_SHAPES))
def test_aan_step(name, where):
    rows, H = R.ROW_SHAPES[name]
    x = R.row_inputs(name)
    xb, cache, cat = G(rows, H, prefill=x["x"]), G(rows, H, prefill=x["cache0"]), G(rows, 2 * H)
    time, tdev = dev_or_host(where, R.LN_TIME, R.LN_TIME + 93)
    call("zk_f32_aan_step", ptr(xb), ptr(cache), ptr(cat), rows, H, time, ptr(tdev))
    finish((xb, tdev), (cache, cat))
    want_cache, want_cat = R.aan_np(name, x, R.LN_TIME)
    R.assert_bits(val(cache), want_cache, "aan_step %s [cache]" % name)
    R.assert_bits(val(cat), want_cat, "aan_step %s [cat = x | cache / (t + 1)]" % name)


@pytest.mark.parametrize("name", list(R.ROW_SHAPES))
def test_gate(name):
    rows, H = R.ROW_SHAPES[name]
    x = R.row_inputs(name)
    z, cat, g = G(rows, 2 * H, prefill=x["z"]), G(rows, 2 * H, prefill=x["cat"]), G(rows, H)
    call("zk_f32_gate", ptr(z), ptr(cat), ptr(g), rows, H)
    finish((z, cat), (g,))
    ref, bound = R.gate_f64(name, x)
    print("gate %s: largest |err| / bound %.3f" % (name, R.assert_within(val(g), ref, bound, "gate " + name)))


# ---------------------------------------------------------------------------------------------- attention
def _attn_bufs(cs, x):
    B, nh, Lq, Lk, d, group = (cs[k] for k in ("B", "nh", "Lq", "Lk", "d", "group"))
    H, Bk = nh * d, B // group
    if cs["slices"]:
        rows = max(B * Lq, Bk * Lk)
        m = np.zeros((rows, 3 * H), np.float32)
        m[:B * Lq, :H], m[:Bk * Lk, H:2 * H], m[:Bk * Lk, 2 * H:] = x["q"], x["k"], x["v"]
        qkv = G(rows, 3 * H, prefill=m)                     # ldq = ldk = ldv = 3H: the fused q / k / v projection's output
        ins, ld = [qkv], qkv.ld
        q, k, v = (qkv.mat.ptr + 4 * H * i for i in range(3))
    else:
        ins, ld = [G(B * Lq, H, prefill=x["q"]), G(Bk * Lk, H, prefill=x["k"]), G(Bk * Lk, H, prefill=x["v"])], H
        q, k, v = (ptr(b) for b in ins)
    return ins, (q, k, v), ld


def _attn_call(cs, x, Lk=None, refused=None):
    B, nh, Lq, d, group = (cs[k] for k in ("B", "nh", "Lq", "d", "group"))
    Lk_data = cs["Lk"]
    Lk = Lk_data if Lk is None else Lk
    H, Bk, ldm = nh * d, B // group, R.attn_ldmask(cs)
    ins, (q, k, v), ld = _attn_bufs(cs, x)
    out = G(B * Lq, H, H + 4, 0)
    mask = None if x["kmask"] is None else G(Bk, Lk_data, ldm, 0, x["kmask"])
    kbias = None if x["kbias"] is None else G(Bk, Lk_data, ldm, 0, x["kbias"])
    nkeys = None if cs["nkeys"] is None else IntBuf([cs["nkeys"]])
    rk = None if cs["rpr"] is None else G(2 * cs["rpr"] + 1, d, prefill=x["rk"])
    rv = None if cs["rpr"] is None else G(2 * cs["rpr"] + 1, d, prefill=x["rv"])
    qp0, qpdev = dev_or_host(cs["q_pos"][0], cs["q_pos"][1], cs["q_pos"][1] + 50)
    head = (q, k, v, ptr(out), B, nh, Lq, Lk, d, ld, ld, ld, out.ld, Lq * ld, Lk_data * ld, Lk_data * ld, Lq * out.ld, ptr(mask), ldm)
    tail = (group, float(x["scale"]), R.MASK_INF, ptr(nkeys), ptr(rk), ptr(rv), cs["rpr"] or 0, qp0, ptr(qpdev))
    ins = ins + [mask, kbias, nkeys, rk, rv, qpdev]
    name, args = ("zk_f32_attn_kb", head + (ptr(kbias),) + tail) if kbias is not None else ("zk_f32_attn", head + tail)
    if refused is not None:
        _refused([b for b in ins if b is not None] + [out], refused, name, *args)
    else:
        call(name, *args)
        finish(ins, (out,))
    return out


@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_attention(name):
    cs, x = R.ATTN_CASES[name], R.attn_inputs(name)
    out = _attn_call(cs, x)
    ref, bound = R.attn_bound(name, x)
    print("attn %s: largest |err| / bound %.4f" % (name, R.assert_within(val(out), ref, bound, "attn " + name)))


def test_attention_refuses_more_than_64k_of_lds():
    cs, x = R.ATTN_CASES["lds_limit"], R.attn_inputs("lds_limit")
    _attn_call(cs, x, Lk=cs["Lk"] + 1, refused="LDS")     # (refused before anything is read: the buffers hold Lk keys)


# ---------------------------------------------------------------------------------------------- refusals and empty calls
def _refused(bufs, match, name, *args):
    with pytest.raises(ZeroHipError, match=match):
        call(name, *args)
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        b.check_intact("%s refused: buffer %d" % (name, i))


def test_gemm_refusals_and_empty():
    M, N, K = 5, 7, 8
    g = np.random.default_rng(1)
    A, B, C, bias = G(M, K + 4, K + 8, 4, g.standard_normal((M, K + 4))), G(K, N, N + 3, 2, g.standard_normal((K, N))), G(M, N, N + 3, 2), \
        G(1, N, prefill=g.standard_normal(N))
    bufs = (A, B, C, bias)
    gemm = lambda **kw: tuple({**dict(A=ptr(A), B=ptr(B), C=ptr(C), M=M, N=N, K=K, lda=A.ld, ldb=B.ld, ldc=C.ld, tb=0, bias=ptr(bias),
                                      act=0), **kw}.values())
    _refused(bufs, "multiple of 4", "zk_f32_gemm", *gemm(K=6))
    _refused(bufs, "leading dimensions", "zk_f32_gemm", *gemm(lda=K + 6))
    _refused(bufs, "16-byte aligned", "zk_f32_gemm", *gemm(A=ptr(A) + 4))
    _refused(bufs, "act must be", "zk_f32_gemm", *gemm(act=2))
    call("zk_f32_gemm", *gemm(M=0))
    finish(bufs)


def test_row_kernel_refusals_and_empty():
    rows, H = 3, 8
    g = np.random.default_rng(2)
    n = lambda r, c: G(r, c, prefill=g.standard_normal((r, c)))
    x, y, z, cat_in, gam, bet, cache = n(rows, 2064), n(rows, 2064), n(rows, 2 * H), n(rows, 2 * H), n(1, 2064), n(1, 2064), n(rows, H)
    out, cat = G(rows, 2064), G(rows, 2 * H)
    bufs = (x, y, z, cat_in, gam, bet, cache, out, cat)
    fused = lambda **kw: tuple({**dict(x=ptr(x), ybuf=ptr(y), z=None, cat_in=None, gamma=ptr(gam), beta=ptr(bet), out=ptr(out), rows=rows,
                                       H=H, eps=1e-8, cache=None, cat_out=None, time=0, time_dev=None), **kw}.values())
    _refused(bufs, "multiple of 4", "zk_f32_ln_fused", *fused(H=6))
    _refused(bufs, "multiple of 4, at most", "zk_f32_ln_fused", *fused(H=2052))
    _refused(bufs, "go together", "zk_f32_ln_fused", *fused(cache=ptr(cache)))
    _refused(bufs, "either", "zk_f32_ln_fused", *fused(z=ptr(z), cat_in=ptr(cat_in)))
    _refused(bufs, "either", "zk_f32_ln_fused", *fused(x=None, ybuf=None, cat_in=ptr(cat_in)))
    _refused(bufs, "at most 2048", "zk_f32_add_ln", ptr(x), ptr(y), ptr(gam), ptr(bet), ptr(out), 1, 2049, 1e-8)
    call("zk_f32_ln_fused", *fused(rows=0))
    call("zk_f32_add_ln", ptr(x), ptr(y), ptr(gam), ptr(bet), ptr(out), 0, H, 1e-8)
    call("zk_f32_aan_step", ptr(x), ptr(cache), ptr(cat), 0, H, 0, None)
    call("zk_f32_gate", ptr(z), ptr(cat_in), ptr(out), 0, H)
    ids = IntBuf([1, 2, 3])
    call("zk_f32_embed", ids.ptr, 0, 1, ptr(x), ptr(gam), ptr(y), 3, ptr(out), H, 1.0, 0, None, None)
    call("zk_f32_embed_step", ids.ptr, 0, ptr(x), ptr(gam), ptr(y), 3, ptr(out), H, 1.0, 0, None, 0, None, None)
    finish(bufs + (ids,))


def test_attention_refusals_and_empty():
    g = np.random.default_rng(3)
    n = lambda r, c: G(r, c, prefill=g.standard_normal((r, c)))
    q, k, v, out, rk = n(4, 24), n(4, 24), n(4, 24), G(4, 24), n(9, 12)
    bufs = (q, k, v, out, rk)
    attn = lambda **kw: tuple({**dict(q=ptr(q), k=ptr(k), v=ptr(v), out=ptr(out), B=2, nh=2, Lq=2, Lk=2, d=12, ldq=24, ldk=24, ldv=24, ldo=24,
                                      bsq=48, bsk=48, bsv=48, bso=48, kmask=None, ldmask=2, group=1, scale=0.5, mask_inf=1e8, nkeys=None,
                                      rk=None, rv=None, max_rel=0, q_pos0=0, q_pos_dev=None), **kw}.values())
    _refused(bufs, "bad shape", "zk_f32_attn", *attn(nh=4, d=6))
    _refused(bufs, "both tables", "zk_f32_attn", *attn(rk=ptr(rk), max_rel=4))
    _refused(bufs, "both tables", "zk_f32_attn", *attn(rv=ptr(rk), max_rel=4))
    call("zk_f32_attn", *attn(B=0))
    finish(bufs)
