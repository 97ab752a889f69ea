"""References of the fp32 decode kernels of zero_amd/csrc/zk_f32.hip (a plain module, no pytest in it), in the manner of
tests/direct_ref.py: per family a float64 statement (``defect=`` plants ONE defect, each something a kernel could do), the
DERIVED element-wise bound or bit-equality a kernel is held to, a fp32 stand-in of what a correct kernel computes, and the case
table.  tests/test_f32_checker.py (CPU) shows on these tables that every stand-in passes and that every defect fails on the
case named for it (``*_DEFECTS``: defect -> case); tests/test_gpu_f32_kernels_elementwise.py runs the same tables through the
C ABI on parity.guarded windows.

    gemm      zk_f32_gemm                    C = act(A op(B) + bias).  ``route`` restates the dispatch; GEMM_CASES reaches all 17
                                             instantiations.  Random data under parity.gemm_bound (fp32 out); small integers
                                             BIT FOR BIT (every partial sum is exact).  The stand-in and its defects work on flat
                                             guarded buffers, as the kernel sees them: a wrong stride is a wrong element or a
                                             write outside the window.
    ln        zk_f32_add_ln, zk_f32_ln_fused out = gamma (s - mean) / sqrt(var + eps) + beta under ``ln_bound``; the average-
                                             attention tail (cache, cat_out) bit for bit from the kernel's own ``out``.
    embed     zk_f32_embed, zk_f32_embed_step  (table[id] scale + bias) + timing[pos] under ``embed_bound``; tail bit for bit.
    aan/gate  zk_f32_aan_step, zk_f32_gate   bit-equal to numpy fp32 (true division) / ``gate_bound``.
    attn      zk_f32_attn, zk_f32_attn_kb    func.py:218-256 under score_f32_ref.attn_bound_from.

Units.  U = parity.PER_TERM = 2^-23 per fp32 operation, TWICE its half-ulp error, as parity.gemm_bound / ln_fwd_bound count.
Division and sqrtf are IEEE in this build (half an ulp each, one U together).  Every expf is charged parity.C_EXP U relative
(the constant measured for the row kernels; nothing is measured here, and no bound below holds a constant fitted to these kernels).

The embedding.  The compiler contracts ``e * scale + bias`` of k_f32_embed into ONE fused multiply-add (v_fmac_f32 in the gfx950
code object; the build does not switch contraction off), so the result is fl(fl(e scale + bias) + timing), not the three separate
roundings; a fused and an unfused kernel are both right.  The kernel is therefore held to 2 ulp of the magnitudes,
``embed_bound`` = 2 U (|e scale| + |bias| + |timing|), which both forms meet (the stand-in is the unfused one), and the zeroed
form (0 + timing) to the timing row's bits.
"""
import numpy as np
import torch

from tests import parity as P
from tests import score_f32_ref as S

U = P.PER_TERM
LEAD = P.LEAD
GUARD32 = np.array([P.GUARD_I16 << 16 | P.GUARD_I16], np.uint32).view(np.float32)[0]      # what parity.guarded puts outside
F32 = np.float32


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a))


def _seed(name, base):
    return base + sum((i + 1) * ord(c) for i, c in enumerate(name)) % 100003


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def assert_bits(got, want, what):
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.nonzero(g != w)[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError("%s: %d of %d elements differ in their bits; the first at flat index %d: got %r want %r" %
                             (what, bad.size, g.size, i, float(np.asarray(got, np.float32).reshape(-1)[i]),
                              float(np.asarray(want, np.float32).reshape(-1)[i])))


def assert_within(got, ref, bound, what):
    P.assert_elementwise(_t(np.asarray(got, np.float64)), _t(np.asarray(ref, np.float64)), _t(np.asarray(bound, np.float64)), what)
    return S.worst_ratio(got, ref, bound)


def fails(check, *args):
    """True when ``check(*args)`` raises AssertionError: a planted defect is seen."""
    try:
        check(*args)
    except AssertionError:
        return True
    return False


# ---- flat guarded buffers in numpy, laid out as parity.Guarded lays them out
def flat(rows, cols, ld, off, data=None):
    buf = np.full(LEAD + rows * ld + LEAD, GUARD32, np.float32)
    win(buf, rows, cols, ld, off)[...] = np.nan if data is None else np.asarray(data, np.float32).reshape(rows, cols)
    return buf


def win(buf, rows, cols, ld, off):
    return np.lib.stride_tricks.as_strided(buf[LEAD + off:], (rows, cols), (4 * ld, 4))


def assert_guard(buf, rows, cols, ld, off, what):
    inside = np.zeros(buf.shape, bool)
    idx = (LEAD + off + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]).reshape(-1)
    inside[idx] = True
    bad = np.nonzero((bits(buf) != bits(GUARD32)) & ~inside)[0]
    assert bad.size == 0, "%s: %d element(s) outside the %d x %d window (ld %d) were written; the first at flat index %d" % (
        what, bad.size, rows, cols, ld, int(bad[0]) if bad.size else -1)


# ================================================================================================ GEMM
def route(M, N, K, tb, ldb):
    """The dispatch rule of zk_f32_gemm (zero_amd/csrc/zk_f32.hip) with the A/B switch at 0 -> (kernel, TB, KS, per): kernel in
    "plain" (k_f32_gemm), "ks" (k_f32_gemm_ks), "t16" (k_f32_gemm_t16), "tb_lds" (k_f32_gemm_tb_lds); per = the k range of
    one wave.  It mirrors, in order:

        if (tb && N >= 2048 && K % 32 == 0 && ldb % 4 == 0 && ...)                              -> k_f32_gemm_tb_lds
        const long tiles16 = (long)((M + 15) / 16) * ((N + 15) / 16);
        if (tiles16 <= 2048 && K >= 64 && K <= 2048 && ...) {
          int ks = 4;
          while (ks < 16 && (((K + ks * 16 - 1) / (ks * 16)) * 16 > 128 || tiles16 * ks < 2048) && K / (ks * 2) >= 32) ks *= 2;
          const int per = ((K + ks * 16 - 1) / (ks * 16)) * 16;
          if (per <= 128) ...                                                                  -> k_f32_gemm_t16<tb, ks>
        if (tiles < 2048 && K >= 64 && K <= 2048 && ...) { the same loop with `tiles * ks < 1024`; if (per <= 128) ...
                                                                                               -> k_f32_gemm_ks<tb, ks>
        const bool split = tiles < 2048 && K >= 256;                                           -> k_f32_gemm<tb, split ? 4 : 1>

    A change of that rule means revisiting GEMM_CASES: tests/test_f32_checker.py asserts through this function that the table
    reaches all 17 instantiations, and the slice defects below take KS and per from it."""
    per_of = lambda ks: ((K + ks * 16 - 1) // (ks * 16)) * 16
    tb = int(bool(tb))
    if tb and N >= 2048 and K % 32 == 0 and ldb % 4 == 0:
        return ("tb_lds", 1, 1, K)
    tiles = ((M + 31) // 32) * ((N + 31) // 32)
    tiles16 = ((M + 15) // 16) * ((N + 15) // 16)
    for kernel, count, few, waves in (("t16", tiles16, tiles16 <= 2048, 2048), ("ks", tiles, tiles < 2048, 1024)):
        if few and 64 <= K <= 2048:
            ks = 4
            while ks < 16 and (per_of(ks) > 128 or count * ks < waves) and K // (ks * 2) >= 32:
                ks *= 2
            if per_of(ks) <= 128:
                return (kernel, tb, ks, per_of(ks))
    if tiles < 2048 and K >= 256:
        return ("plain", tb, 4, per_of(4))
    return ("plain", tb, 1, K)


GEMM_FORMS = ([("plain", tb, ks) for tb in (0, 1) for ks in (1, 4)] + [(kn, tb, ks) for kn in ("ks", "t16") for tb in (0, 1)
                                                                         for ks in (4, 8, 16)] + [("tb_lds", 1, 1)])
assert len(GEMM_FORMS) == 17
_GEMM_SHAPES = [        # (form the shape is in the table for, M, N, K, the values of tb)
    ("plain1_colmajor", 33, 70, 36, (0, 1)), ("plain1_rowmajor", 70, 33, 36, (0, 1)), ("plain1_deadtiles", 1100, 2100, 36, (0, 1)),
    ("plain4_K2052", 33, 70, 2052, (0, 1)),
    ("t16k4_emptywave", 5, 104, 68, (0, 1)), ("t16k4", 17, 40, 128, (0, 1)),
    ("t16k8", 33, 50, 260, (0, 1)), ("t16k8_big", 129, 520, 516, (0, 1)),
    ("t16k16", 50, 36, 1028, (0, 1)), ("t16k16_big", 128, 512, 2048, (0, 1)),
    ("ks4", 520, 1030, 68, (0, 1)), ("ks8", 520, 1030, 600, (0, 1)), ("ks16_refill", 520, 1030, 1028, (0, 1)),
    ("tblds", 130, 2050, 96, (1,)), ("tblds_onerow", 1, 2048, 32, (1,)), ("tblds_fallthrough", 130, 2050, 100, (1,)),
]
GEMM_CASES = {"%s_tb%d" % (n, tb): (M, N, K, tb) for n, M, N, K, tbs in _GEMM_SHAPES for tb in tbs}
GEMM_LAYOUTS = ("tight", "strided")
GEMM_DATA = ("random", "int")
GEMM_CONFIGS = [(lay, bias, act, data) for lay in GEMM_LAYOUTS for bias in (0, 1) for act in (0, 1) for data in GEMM_DATA]
# defect -> (case, layout, bias, act, data): the case it must fail on
GEMM_DEFECTS = {
    "lda_from_K": ("t16k8_tb0", "strided", 1, 0, "random"),
    "ldb_from_width": ("t16k8_tb1", "strided", 1, 0, "random"),
    "ldc_from_N": ("ks4_tb0", "strided", 0, 0, "random"),
    "k_tail_dropped": ("plain1_colmajor_tb0", "tight", 1, 0, "random"),
    "last_slice_dropped": ("t16k4_tb1", "tight", 0, 0, "random"),
    "empty_wave_reads": ("t16k4_emptywave_tb1", "strided", 1, 0, "random"),
    "relu_before_bias": ("plain1_rowmajor_tb0", "tight", 1, 1, "random"),
    "clamped_row_stored": ("t16k4_emptywave_tb0", "strided", 1, 0, "int"),
    "col_tail_untouched": ("plain1_colmajor_tb1", "strided", 0, 1, "int"),
}


def gemm_layout(M, N, K, tb, layout):
    """Row strides and column offsets of the three operands (A and a transposed B are read with 16-byte loads: their strides
    and offsets stay multiples of 4)."""
    wb = K if tb else N
    if layout == "tight":
        return dict(lda=K, offa=0, ldb=wb, offb=0, ldc=N, offc=0)
    return dict(lda=K + 8, offa=4, ldb=wb + (4 if tb else 3), offb=0 if tb else 2, ldc=N + 3, offc=2)


def gemm_inputs(name, data):
    """a [M, K], b ([N, K] when tb, else [K, N]), bias [N] as fp32 numpy.  "int": integers in [-4, 4], so that every partial
    sum of every summation order is an integer below 2^24 (16 K + 4 <= 16 * 2052 + 4) and the fp32 result IS the float64 one."""
    M, N, K, tb = GEMM_CASES[name]
    g = np.random.default_rng(_seed(name + data, 5100))
    bs = (N, K) if tb else (K, N)
    if data == "int":
        return dict(a=g.integers(-4, 5, (M, K)).astype(F32), b=g.integers(-4, 5, bs).astype(F32), bias=g.integers(-4, 5, N).astype(F32))
    return dict(a=g.standard_normal((M, K)).astype(F32), b=g.standard_normal(bs).astype(F32), bias=g.standard_normal(N).astype(F32))


def gemm_ref(name, x, bias, act):
    """(ref, bound) float64 numpy through parity.gemm_bound with the fp32 output unit."""
    M, N, K, tb = GEMM_CASES[name]
    b = _t(x["b"]).t() if tb else _t(x["b"])
    ref, bound = P.gemm_bound(_t(x["a"]), b, K, torch.float32, bias=_t(x["bias"]) if bias else None, act=act)
    return ref.numpy(), bound.numpy()


def gemm_check(got, ref, bound, data, what):
    if data == "int":
        P.assert_exact(_t(np.asarray(got, np.float64)), _t(ref), what)
        return 0.0
    return assert_within(got, ref, bound, what)


def gemm_standin(name, x, layout, bias, act, defect=None):
    """What a correct kernel leaves in the flat C buffer (torch fp32 product, fp32 epilogue) -> the flat buffer.  defect:
      lda_from_K / ldb_from_width   the row stride of A / B taken from the width, not from its argument
      ldc_from_N                    rows of C stored N apart
      k_tail_dropped                the last K % 16 terms missing
      last_slice_dropped            the k range of the last wave of a K-sliced workgroup missing
      empty_wave_reads              a wave whose k range starts past K adds the last float4 of the row once more (its first
                                    chunk, clamped into the row)
      relu_before_bias              max(A B, 0) + bias
      clamped_row_stored            row M - 1 (what the clamped loads of a dead row hold) stored again one row below
      col_tail_untouched            the last N % 16 columns never stored"""
    M, N, K, tb = GEMM_CASES[name]
    L = gemm_layout(M, N, K, tb, layout)
    rb, cb = (N, K) if tb else (K, N)
    fa, fb, fc = flat(M, K, L["lda"], L["offa"], x["a"]), flat(rb, cb, L["ldb"], L["offb"], x["b"]), flat(M, N, L["ldc"], L["offc"])
    a = win(fa, M, K, K if defect == "lda_from_K" else L["lda"], L["offa"])
    b = win(fb, rb, cb, cb if defect == "ldb_from_width" else L["ldb"], L["offb"])
    bm = b.T if tb else b
    _, _, KS, per = route(M, N, K, tb, L["ldb"])
    keep = np.ones(K, bool)
    if defect == "k_tail_dropped":
        assert K % 16
        keep[K - K % 16:] = False
    if defect == "last_slice_dropped":
        assert KS > 1 and (KS - 1) * per < K
        keep[(KS - 1) * per:] = False
    v = _t(a[:, keep]) @ _t(bm[keep])
    if defect == "empty_wave_reads":
        empty = sum(1 for w in range(KS) if w * per >= K)
        assert KS > 1 and empty
        v = v + empty * (_t(a[:, K - 4:]) @ _t(bm[K - 4:]))
    bv = _t(x["bias"]) if bias else torch.zeros(N)
    if defect == "relu_before_bias":
        v = torch.relu(v) + bv
    else:
        v = v + bv
        if act:
            v = torch.relu(v)
    v = v.numpy().copy()
    if defect == "col_tail_untouched":
        assert N % 16
        v[:, N - N % 16:] = np.nan
    ldc = N if defect == "ldc_from_N" else L["ldc"]
    win(fc, M, N, ldc, L["offc"])[...] = v
    if defect == "clamped_row_stored":
        at = LEAD + L["offc"] + M * ldc
        n = min(N, fc.size - at)
        fc[at:at + n] = v[M - 1, :n]
    return fc


def gemm_check_flat(fc, name, layout, ref, bound, data, what="gemm"):
    M, N, K, tb = GEMM_CASES[name]
    L = gemm_layout(M, N, K, tb, layout)
    assert_guard(fc, M, N, L["ldc"], L["offc"], what)
    return gemm_check(win(fc, M, N, L["ldc"], L["offc"]), ref, bound, data, what)


# ================================================================================================ LayerNorm family
LN_ROWS = (1, 5, 131)
LN_H = (4, 60, 64, 68, 256, 620, 1000, 2044, 2048)
LN_H_ODD = (1, 63, 65)                       # zk_f32_add_ln only
LN_TIME = 6
# form -> flags.  entry: the entry point; y: the residual operand; gate: (z, cat_in); aan: (cache, cat_out), time from "host"
# or from the "dev"ice (the host argument then holds LN_TIME + 93, which must be ignored)
LN_FORMS = {
    "add_ln": dict(entry="add_ln", y=False), "add_ln_y": dict(entry="add_ln", y=True),
    "fused": dict(entry="fused", y=False), "fused_y": dict(entry="fused", y=True),
    "fused_aan_host": dict(entry="fused", y=True, aan="host"), "fused_aan_dev": dict(entry="fused", y=True, aan="dev"),
    "fused_gate": dict(entry="fused", gate=True), "fused_gate_aan": dict(entry="fused", gate=True, aan="dev"),
}
LN_KINDS = ("random", "constant", "narrow")
LN_EPS = {k: float(np.float32(v)) for k, v in (("random", 1e-8), ("constant", 1e-8), ("narrow", 1e-3))}     # as the kernel gets them
LN_CONST, LN_CONST_Y = 2.5, 0.25             # k * 2.75 is a fp32 number for every k <= 2048: the row sums are exact


def ln_case_names():
    """form/H/rows/kind.  "constant" (the output is beta, bit for bit) not for the gate forms; "narrow" (a row of spread 0.05
    around 5 with eps = 1e-3: where eps sits matters) at 5 rows and H = 60, 620 only."""
    out = []
    for form, fl in LN_FORMS.items():
        for H in LN_H + (LN_H_ODD if fl["entry"] == "add_ln" else ()):
            for rows in LN_ROWS:
                for kind in LN_KINDS:
                    if (kind == "constant" and fl.get("gate")) or (kind == "narrow" and (rows != 5 or H not in (60, 620))):
                        continue
                    out.append("%s/%d/%d/%s" % (form, H, rows, kind))
    return out


def ln_case(name):
    form, H, rows, kind = name.split("/")
    cs = dict(LN_FORMS[form], form=form, H=int(H), rows=int(rows), kind=kind, eps=LN_EPS[kind], time=LN_TIME, name=name)
    return cs


LN_DEFECTS = {
    "unbiased_variance": "add_ln_y/60/5/random", "eps_outside_root": "fused_y/60/5/narrow", "tail_left_out": "add_ln_y/68/5/random",
    "tail_left_out_fused": "fused_y/620/5/random", "y_ignored": "fused_y/256/131/random", "gate_halves_swapped": "fused_gate/68/5/random",
    "div_by_t": "fused_aan_dev/620/5/random", "cache_from_input": "fused_aan_host/64/1/random",
}


def ln_inputs(cs):
    rows, H, kind = cs["rows"], cs["H"], cs["kind"]
    g = np.random.default_rng(_seed(cs["name"], 5200))
    n = lambda *s: g.standard_normal(s).astype(F32)
    x = dict(gamma=(1.0 + 0.2 * n(H)).astype(F32), beta=(0.1 * n(H)).astype(F32))
    if cs.get("gate"):
        z = (2.0 * n(rows, 2 * H)).astype(F32)
        z[:, 0::5], z[:, 1::5] = 30.0, -30.0              # saturated gates beside moderate ones, in both halves
        x["z"], x["cat_in"] = z, (5.0 + 3.0 * n(rows, 2 * H)).astype(F32)
    elif kind == "constant":
        x["x"] = np.full((rows, H), LN_CONST, F32)
        x["y"] = np.full((rows, H), LN_CONST_Y, F32) if cs["y"] else None
    else:
        x["x"] = (5.0 + (0.05 if kind == "narrow" else 3.0) * n(rows, H)).astype(F32)
        x["y"] = ((0.01 if kind == "narrow" else 1.0) * n(rows, H)).astype(F32) if cs["y"] else None
    if cs.get("aan"):
        x["cache0"] = n(rows, H)
    return x


def _sig64(z):
    return 1.0 / (1.0 + np.exp(-z))


def gate_terms(z, cat, swapped=False):
    """transformer_aan.py:186-189 in float64 -> (g, bound).  sigmoid(z) = 1 / (1 + expf(-z)): expf is off by C_EXP U of E =
    e^-z, which moves s = 1 / (1 + E) by C_EXP U E / (1 + E) = C_EXP U (1 - s) relative; the sum 1 + E and the division are
    one U together, the product with the operand and the final sum (each at most half a U of a magnitude below the sum of the
    two products) one more; 3 U is charged.  At z = +30 the sum rounds to 1 and s to 1, at -30 s = e^-30: both inside.
        gate_bound = U sum over the two halves of (C_EXP (1 - s) + 3) s |operand|"""
    z, cat = np.asarray(z, np.float64), np.asarray(cat, np.float64)
    H = z.shape[1] // 2
    si, sf = _sig64(z[:, :H]), _sig64(z[:, H:])
    if swapped:
        si, sf = sf, si
    g = si * cat[:, :H] + sf * cat[:, H:]
    bound = U * ((P.C_EXP * (1 - si) + 3) * si * np.abs(cat[:, :H]) + (P.C_EXP * (1 - sf) + 3) * sf * np.abs(cat[:, H:]))
    return g, bound


def ln_f64(cs, x, defect=None):
    """The float64 statement -> dict out, v (the row that is normalised), e (how far a correct kernel's fp32 v may be from it)
    and, with the average-attention tail, cache and cat [rows, 2H].

    defect:  unbiased_variance (H / (H - 1));  eps_outside_root (1 / (sqrt(var) + eps));  tail_left_out (the channels beyond
    the last multiple of 64 -- of 256 for the fused kernel, whose lanes hold four channels each -- missing from the two row
    sums);  y_ignored;  gate_halves_swapped (z = [f | i]);  div_by_t (cache / t);  cache_from_input (cache += s, the row
    before it is normalised)."""
    H, eps = cs["H"], cs["eps"]
    d = lambda a: np.asarray(a, np.float64)
    if cs.get("gate"):
        xc = d(x["cat_in"])[:, :H]
        g, gb = gate_terms(x["z"], x["cat_in"], swapped=defect == "gate_halves_swapped")
        v, e = xc + g, gb + U * (np.abs(xc) + np.abs(g))
    elif x["y"] is not None and defect != "y_ignored":
        v, e = d(x["x"]) + d(x["y"]), U * (np.abs(d(x["x"])) + np.abs(d(x["y"])))
    else:
        v, e = d(x["x"]), np.zeros_like(d(x["x"]))
    n = H
    if defect in ("tail_left_out", "tail_left_out_fused"):
        n = H // (256 if cs["entry"] == "fused" else 64) * (256 if cs["entry"] == "fused" else 64)
        assert 0 < n < H
    mean = v[:, :n].sum(1, keepdims=True) / H
    var = ((v[:, :n] - mean) ** 2).sum(1, keepdims=True) / H
    if defect == "unbiased_variance":
        var = var * H / (H - 1.0)
    rs = 1.0 / (np.sqrt(var) + eps) if defect == "eps_outside_root" else 1.0 / np.sqrt(var + eps)
    out = d(x["gamma"])[None] * (v - mean) * rs + d(x["beta"])[None]
    res = dict(out=out, v=v, e=e)
    if cs.get("aan"):
        t = cs["time"]
        cache = (v if defect == "cache_from_input" else out) + d(x["cache0"])
        res["cache"] = cache
        res["cat"] = np.concatenate([out, cache / (t if defect == "div_by_t" else t + 1)], 1)
    return res


def ln_bound(cs, x):
    """-> (ref out, bound), float64.  parity.ln_fwd_bound restated for an all-fp32 kernel: v is the kernel's fp32 row, off the
    float64 one by e (one addition: U (|x| + |y|); the gate form: gate_bound + U (|x_c| + |g|), so the fused launch is held to the
    SUM of the bounds of zk_f32_gate and of the LayerNorm that follow each other in the launches it replaces).
      mean  = fl(sum v) / H, H - 1 additions in any order and the division:   bound_mean = (H + C_LN) U mean|v| + mean(e)
      var   = sum (v - mean)^2 / H; sum (v - m)^2 = H var + H (m - mu)^2: the error of the mean enters squared, e as
              2 sqrt(var mean(e^2)) + mean(e^2) (Cauchy-Schwarz):   var_abs = bound_mean^2 + 2 sqrt(var mean(e^2)) + mean(e^2),
              and (H + C_LN) U relative for its own roundings
      rs    = 1 / sqrtf(var + eps), both IEEE: half the relative error of var + eps and one U
      out   = gamma (v - mean) rs + beta:  U |ref| + (H + C_LN) U (|gamma| rs (|v - mu| + mean|v|) + |beta|)
              + |gamma| rs (mean(e) + e + |v - mu| var_abs / (2 (var + eps)))
    (the counts are those of parity.ln_fwd_bound with RSQRT_ULP = 2 replaced by the one U of an IEEE root and division, and the
    output unit 2^-8 by 2^-23; C_LN is parity's, not tuned).  A constant row has var = 0 and a bound worth nothing (rs = 1e4): it
    is held to beta's bits instead (ln_check)."""
    r = ln_f64(cs, x)
    v, e, H, eps = r["v"], r["e"], cs["H"], cs["eps"]
    g, b = np.asarray(x["gamma"], np.float64)[None], np.asarray(x["beta"], np.float64)[None]
    kd = dict(axis=1, keepdims=True)
    mu, ma = v.mean(**kd), np.abs(v).mean(**kd)
    lin = (H + P.C_LN) * U
    mean_bound = lin * ma + e.mean(**kd)
    dv = v - mu
    var = (dv * dv).mean(**kd)
    e2 = (e * e).mean(**kd)
    var_abs = mean_bound ** 2 + 2 * np.sqrt(var * e2) + e2
    gr = np.abs(g) / np.sqrt(var + eps)
    bound = (U * np.abs(r["out"]) + lin * (gr * (np.abs(dv) + ma) + np.abs(b))
             + gr * (e.mean(**kd) + e + np.abs(dv) * 0.5 * var_abs / (var + eps)))
    return r["out"], bound


def aan_tail(out32, cache0, t):
    """transformer_aan.py:110-112 on fp32 numbers, as numpy forms them: cache = out + cache0, cat = [out | cache / (t + 1)]
    with a TRUE division (torch on a GPU would multiply by a reciprocal)."""
    out32, cache0 = np.asarray(out32, F32), np.asarray(cache0, F32)
    cache = (out32 + cache0).astype(F32)
    return cache, np.concatenate([out32, (cache / F32(t + 1)).astype(F32)], 1)


def ln_standin(cs, x):
    """torch fp32: one sum per row in torch's own order, the two passes of func.py:289-303, IEEE division and root."""
    H = cs["H"]
    f = lambda a: _t(np.asarray(a, F32))
    if cs.get("gate"):
        z, cat = f(x["z"]), f(x["cat_in"])
        sg = lambda t: 1.0 / (1.0 + torch.exp(-t))
        v = cat[:, :H] + (sg(z[:, :H]) * cat[:, :H] + sg(z[:, H:]) * cat[:, H:])
    else:
        v = f(x["x"]) + f(x["y"]) if x["y"] is not None else f(x["x"])
    Hf = torch.tensor(float(H))
    mean = v.sum(1, keepdim=True) / Hf
    dv = v - mean
    var = (dv * dv).sum(1, keepdim=True) / Hf
    out = (f(x["gamma"])[None] * dv * (1.0 / torch.sqrt(var + F32(cs["eps"]))) + f(x["beta"])[None]).numpy()
    res = dict(out=out)
    if cs.get("aan"):
        res["cache"], res["cat"] = aan_tail(out, x["cache0"], cs["time"])
    return res


def ln_check(cs, x, got, what=None):
    """got: dict out (and cache, cat) as fp32 arrays -> the largest |err| / bound of out."""
    what = what or cs["name"]
    ref, bound = ln_bound(cs, x)
    out = np.asarray(got["out"], F32)
    if cs["kind"] == "constant":
        assert_bits(out, np.broadcast_to(np.asarray(x["beta"], F32)[None], out.shape), what + ": a constant row gives beta")
        r = 0.0
    else:
        r = assert_within(out, ref, bound, what + " [out]")
    if cs.get("aan"):
        cache, cat = aan_tail(out, x["cache0"], cs["time"])
        assert_bits(got["cache"], cache, what + " [cache = out + cache]")
        assert_bits(np.asarray(got["cat"])[:, :cs["H"]], out, what + " [cat_out[:, :H] = out]")
        assert_bits(np.asarray(got["cat"])[:, cs["H"]:], cat[:, cs["H"]:], what + " [cat_out[:, H:] = cache / (t + 1)]")
    return r


# ================================================================================================ embedding
EMB_V, EMB_PAD = 11, 2
EMB_TIMING_ROWS = 12


def _emb(entry, rows, H, L=1, pos=("host", 0), ids="no_pad", pad_id=-1, flag=None, aan=False):
    return dict(entry=entry, rows=rows, H=H, L=L, pos=pos, ids=ids, pad_id=pad_id, flag=flag, aan=aan)


# entry "embed" = zk_f32_embed (L > 1; all_pad flag None / 0 / 1, pad_id is -1 by construction), "step" = zk_f32_embed_step.
# pos = (where the position comes from, its value): "dev" passes the other number on the host, which must be ignored;
# positions past EMB_TIMING_ROWS - 1 are clipped.  ids: all_pad, one_live (row 100 of 131, or the last row), some_pad, no_pad.
EMBED_CASES = {
    "embed_H4_L3": _emb("embed", 3, 4, L=3), "embed_H68_2x3_dev": _emb("embed", 6, 68, L=3, pos=("dev", 4)),
    "embed_H620_L131_clip": _emb("embed", 131, 620, L=131, pos=("host", 3)),
    "embed_H1024_L3_clip_dev": _emb("embed", 3, 1024, L=3, pos=("dev", 10)),
    "embed_flag0_allpad": _emb("embed", 6, 68, L=3, ids="all_pad", flag=0), "embed_flag1": _emb("embed", 6, 68, L=3, flag=1),
    "embed_flag1_host_pos": _emb("embed", 131, 620, L=131, pos=("host", 5), ids="some_pad", flag=1),
    "step_H4_1": _emb("step", 1, 4, pad_id=EMB_PAD), "step_H68_3_dev": _emb("step", 3, 68, pos=("dev", 5), pad_id=EMB_PAD, ids="some_pad"),
    "step_H620_131_allpad": _emb("step", 131, 620, pos=("dev", 7), pad_id=EMB_PAD, ids="all_pad"),
    "step_H620_131_onelive": _emb("step", 131, 620, pos=("host", 7), pad_id=EMB_PAD, ids="one_live"),
    "step_H1024_131_nopad_clip": _emb("step", 131, 1024, pos=("dev", 40), pad_id=EMB_PAD),
    "step_H68_3_allpad_nopadid": _emb("step", 3, 68, pos=("host", 2), pad_id=-1, ids="all_pad"),
    "step_H68_1_allpad": _emb("step", 1, 68, pos=("host", 0), pad_id=EMB_PAD, ids="all_pad"),
    "step_aan_H68_3": _emb("step", 3, 68, pos=("dev", 5), pad_id=EMB_PAD, ids="some_pad", aan=True),
    "step_aan_H620_131_allpad": _emb("step", 131, 620, pos=("host", 3), pad_id=EMB_PAD, ids="all_pad", aan=True),
    "step_aan_H1024_131_clip": _emb("step", 131, 1024, pos=("dev", 40), pad_id=EMB_PAD, ids="one_live", aan=True),
    "step_aan_H4_1": _emb("step", 1, 4, pos=("host", 0), pad_id=EMB_PAD, aan=True),
}
EMBED_DEFECTS = {
    "scale_after_bias": "step_H68_3_dev", "zero_keeps_bias": "step_H620_131_allpad", "zero_if_any_pad": "step_H68_3_dev",
    "zero_per_row": "step_H68_3_dev", "pos_per_row_ignored": "embed_H68_2x3_dev", "pos_unclipped": "embed_H620_L131_clip",
    "pad_scan_64": "step_H620_131_onelive",
}


def embed_inputs(name):
    cs = EMBED_CASES[name]
    rows, H = cs["rows"], cs["H"]
    g = np.random.default_rng(_seed(name, 5300))
    live = np.array([i for i in range(EMB_V) if i != EMB_PAD])
    ids = live[g.integers(0, len(live), rows)]
    if cs["ids"] == "all_pad":
        ids[:] = EMB_PAD
    elif cs["ids"] == "one_live":
        ids[:] = EMB_PAD
        ids[min(100, rows - 1)] = 7
    elif cs["ids"] == "some_pad":
        ids[::2] = EMB_PAD
        ids[-1] = 5
    x = dict(ids=ids.astype(np.int32), table=g.standard_normal((EMB_V, H)).astype(F32), bias=(0.3 * g.standard_normal(H)).astype(F32),
             timing=g.standard_normal((EMB_TIMING_ROWS, H)).astype(F32), scale=F32(float(H) ** 0.5))
    if cs["aan"]:
        x["cache0"] = g.standard_normal((rows, H)).astype(F32)
    return x


def embed_zeroed(cs, ids, defect=None):
    """Whether the embedding part is zeroed -> bool per row (transformer.py:113-115: all rows or none)."""
    rows = len(ids)
    if defect == "zero_per_row":
        return (ids == cs["pad_id"]) & (cs["pad_id"] >= 0)
    if cs["pad_id"] >= 0:
        seen = ids[:64] if defect == "pad_scan_64" else ids
        hit = (seen == cs["pad_id"]).any() if defect == "zero_if_any_pad" else (seen == cs["pad_id"]).all()
    else:
        hit = bool(cs["flag"])
    return np.full(rows, bool(hit))


def embed_f64(name, x, defect=None):
    """out[r] = (table[ids[r]] scale + bias) + timing[min(t0 + r % L, timing_rows - 1)] in float64 -> dict out, mag, zero.
    defect:  scale_after_bias ((e + bias) scale);  zero_keeps_bias (a zeroed step keeps the bias);  zero_if_any_pad;
    zero_per_row;  pos_per_row_ignored (every row at t0);  pos_unclipped (rows past the table read what lies behind it);
    pad_scan_64 (only the first 64 ids are looked at)."""
    cs = EMBED_CASES[name]
    d = lambda a: np.asarray(a, np.float64)
    ids, s = x["ids"].astype(np.int64), float(x["scale"])
    t0 = cs["pos"][1]
    pos = t0 + (0 if defect == "pos_per_row_ignored" else np.arange(cs["rows"]) % cs["L"])
    tim = d(x["timing"])
    if defect == "pos_unclipped":
        tim = np.concatenate([tim, np.full((int(pos.max()) + 1, cs["H"]), float(GUARD32))], 0)
    else:
        pos = np.minimum(pos, EMB_TIMING_ROWS - 1)
    e, b = d(x["table"])[ids], d(x["bias"])[None]
    body, mag = ((e + b) * s if defect == "scale_after_bias" else e * s + b), np.abs(e) * s + np.abs(b)
    zero = embed_zeroed(cs, x["ids"], defect)[:, None]
    body = np.where(zero, b if defect == "zero_keeps_bias" else 0.0, body)
    mag = np.where(zero, 0.0, mag)
    return dict(out=body + tim[pos], mag=mag + np.abs(tim[pos]), zero=zero, t0=t0)


def embed_bound(r):
    """2 ulp of the magnitudes (module docstring: the product-sum may or may not be fused); a zeroed row is 0 + timing: 0."""
    return np.where(r["zero"], 0.0, 2 * U * r["mag"])


def embed_standin(name, x):
    """fl(fl(e scale) + bias) + timing, every step rounded on its own (torch fp32 does not fuse)."""
    cs = EMBED_CASES[name]
    f = lambda a: _t(np.asarray(a, F32))
    pos = np.minimum(cs["pos"][1] + np.arange(cs["rows"]) % cs["L"], EMB_TIMING_ROWS - 1)
    v = f(x["table"])[_t(x["ids"].astype(np.int64))] * torch.tensor(float(x["scale"]))
    v = v + f(x["bias"])[None]
    v = torch.where(_t(embed_zeroed(cs, x["ids"]))[:, None], torch.zeros_like(v), v)
    out = (v + f(x["timing"])[_t(pos)]).numpy()
    res = dict(out=out)
    if cs["aan"]:
        res["cache"], res["cat"] = aan_tail(out, x["cache0"], cs["pos"][1])
    return res


def embed_check(name, x, got, what=None):
    cs, what = EMBED_CASES[name], what or name
    r = embed_f64(name, x)
    out = np.asarray(got["out"], F32)
    ratio = assert_within(out, r["out"], embed_bound(r), what + " [out]")
    if cs["aan"]:
        cache, cat = aan_tail(out, x["cache0"], r["t0"])
        assert_bits(got["cache"], cache, what + " [cache]")
        assert_bits(got["cat"], cat, what + " [cat_out = out | cache / (t + 1)]")
    return ratio


# ================================================================================================ aan_step / gate
ROW_SHAPES = {"1x4": (1, 4), "12x256": (12, 256), "7x620": (7, 620), "257x2048": (257, 2048)}     # the last: rows H > 2048 * 256
ROW_GRID = 2048 * 256                        # threads of the largest grid: elements beyond take the second trip
AAN_DEFECTS = {"second_trip_dropped": "257x2048", "row_stride_H": "7x620", "div_by_t": "12x256"}
GATE_DEFECTS = {"second_trip_dropped": "257x2048", "row_stride_H": "7x620"}


def row_inputs(name):
    rows, H = ROW_SHAPES[name]
    g = np.random.default_rng(_seed(name, 5400))
    n = lambda *s: g.standard_normal(s).astype(F32)
    z = (2.0 * n(rows, 2 * H)).astype(F32)
    z[:, 0::5], z[:, 1::5] = 30.0, -30.0                              # saturated gates beside moderate ones
    return dict(x=n(rows, H), cache0=n(rows, H), z=z, cat=n(rows, 2 * H))


def _wide(flat2, rows, H, defect):
    """[rows, H] halves of a 2H-wide operand given flat; row_stride_H: rows taken H apart."""
    ld = H if defect == "row_stride_H" else 2 * H
    at = np.arange(rows)[:, None] * ld + np.arange(H)[None]
    return flat2.reshape(-1)[at], flat2.reshape(-1)[at + H]


def aan_np(name, x, t, defect=None):
    """zk_f32_aan_step in numpy fp32 (statement and stand-in: the kernel is held to its bits) -> (cache, cat [rows, 2H]).
    defect:  second_trip_dropped (elements from ROW_GRID on never visited);  row_stride_H (cat rows H apart);  div_by_t."""
    rows, H = ROW_SHAPES[name]
    cache, cat = aan_tail(x["x"], x["cache0"], t - 1 if defect == "div_by_t" else t)
    if defect == "row_stride_H":
        fl = np.full(rows * 2 * H, np.nan, F32)
        for r in range(rows):
            fl[r * H:r * H + H], fl[r * H + H:r * H + 2 * H] = cat[r, :H], cat[r, H:]
        cat = fl.reshape(rows, 2 * H)
    if defect == "second_trip_dropped":
        assert rows * H > ROW_GRID
        dead = (np.arange(rows * H) >= ROW_GRID).reshape(rows, H)
        cache = np.where(dead, np.asarray(x["cache0"], F32), cache)
        cat = np.where(np.concatenate([dead, dead], 1), np.nan, cat).astype(F32)
    return cache, cat


def gate_f64(name, x, defect=None):
    """-> (g, bound) float64 (gate_terms); the defects of aan_np on the read side: z and cat taken with row stride H."""
    rows, H = ROW_SHAPES[name]
    zi, zf = _wide(np.asarray(x["z"], np.float64), rows, H, defect)
    ci, cf = _wide(np.asarray(x["cat"], np.float64), rows, H, defect)
    g, bound = gate_terms(np.concatenate([zi, zf], 1), np.concatenate([ci, cf], 1))
    if defect == "second_trip_dropped":
        assert rows * H > ROW_GRID
        g = np.where((np.arange(rows * H) >= ROW_GRID).reshape(rows, H), np.nan, g)
    return g, bound


def gate_standin(name, x):
    rows, H = ROW_SHAPES[name]
    z, cat = _t(x["z"]), _t(x["cat"])
    sg = lambda t: 1.0 / (1.0 + torch.exp(-t))
    return (sg(z[:, :H]) * cat[:, :H] + sg(z[:, H:]) * cat[:, H:]).numpy()


# ================================================================================================ attention
MASK_INF = S.MASK_INF
ATTN_PAD_ROWS = 8                            # rows of ones behind the keys / values of the statement (nkeys_unclipped)
_C = {"c1": (1, 1, 1, 1, 4, 1), "c2": (3, 2, 9, 64, 64, 1), "c3": (3, 2, 9, 65, 68, 1), "c4": (8, 2, 1, 23, 128, 4),
      "c5": (2, 1, 5, 130, 32, 1), "lds": (1, 1, 1, 4032, 64, 1)}


def _at(shape, **kw):
    B, nh, Lq, Lk, d, group = _C[shape]
    cs = dict(B=B, nh=nh, Lq=Lq, Lk=Lk, d=d, group=group, mask=False, dead=None, nkeys=None, kbias=None, rpr=None, q_pos=("host", 0),
              slices=False)
    cs.update(kw)
    return cs


# mask: a holed key mask with ldmask = Lk + 3, sentence `dead` masked entirely.  nkeys: *nkeys_dev.  kbias: "slot0" / "spread".
# rpr: max_rel; q_pos = (where the query position comes from, its value) -- "dev" passes value + 50 on the host.
# slices: q, k, v are the column slices of one [rows, 3H] buffer.  out is always a window with ldo = H + 4.
ATTN_CASES = {
    "c1_plain": _at("c1"), "c1_slices_rpr0": _at("c1", slices=True, rpr=0),
    "c2_plain": _at("c2", slices=True), "c3_plain": _at("c3"), "c4_plain": _at("c4"), "c5_plain": _at("c5", slices=True),
    "c2_mask": _at("c2", mask=True, dead=2), "c3_mask": _at("c3", mask=True, dead=1, slices=True),
    "c4_mask": _at("c4", mask=True, dead=1), "c5_mask": _at("c5", mask=True, dead=0),
    "c4_nk0": _at("c4", nkeys=0), "c4_nk7": _at("c4", nkeys=7, slices=True), "c4_nk22": _at("c4", nkeys=22),
    "c4_nk28_clipped": _at("c4", nkeys=28), "c3_nk21_Lq9": _at("c3", nkeys=21), "c3_nk70_clipped_Lq9": _at("c3", nkeys=70),
    "c5_nk0_Lq5": _at("c5", nkeys=0),
    "c3_kbias_slot0": _at("c3", mask=True, kbias="slot0"), "c3_kbias_spread": _at("c3", mask=True, dead=1, kbias="spread"),
    "c4_kbias_spread": _at("c4", kbias="spread"),
    "c2_rpr4_host": _at("c2", rpr=4, q_pos=("host", 20)), "c2_rpr4_dev": _at("c2", rpr=4, q_pos=("dev", 20)),
    "c2_rpr0": _at("c2", rpr=0, q_pos=("host", 20)), "c3_rpr4_host": _at("c3", rpr=4, q_pos=("host", 30), slices=True),
    "c4_rpr4_cached": _at("c4", rpr=4, q_pos=("dev", 12), nkeys=12), "c5_rpr4_mask": _at("c5", rpr=4, q_pos=("host", 60), mask=True),
    "lds_limit": _at("lds"),
}
ATTN_DEFECTS = {
    "neighbour_sentence": "c4_plain", "nkeys_off_by_one": "c4_nk7", "nkeys_unclipped": "c4_nk28_clipped", "mask_stride_Lk": "c3_mask",
    "rpr_sign": "c2_rpr4_host", "clip_m_minus_1": "c2_rpr4_host", "q_pos0_ignored": "c2_rpr4_host", "kbias_dropped": "c3_kbias_slot0",
    "head_tail_dropped": "c3_plain", "softmax_not_normalised": "c2_plain",
}


def attn_inputs(name):
    """fp32 numpy: q [B Lq, H], k, v [Bk Lk, H], kmask / kbias [Bk, Lk] or None, rk, rv [2 m + 1, d] or None, scale.
    The queries of a `dead` sentence are scaled by 0.4 so that every score of it stays below 4 = half an ulp of 1e8 (a fully masked row is uniform in fp32; asserted in
    attn_f64); the mask keeps key 0 of every sentence that is not `dead`; kbias holds log-counts log(1 .. 5)."""
    cs = ATTN_CASES[name]
    B, nh, Lq, Lk, d, group = (cs[k] for k in ("B", "nh", "Lq", "Lk", "d", "group"))
    H, Bk = nh * d, B // group
    g = np.random.default_rng(_seed(name, 5500))
    n = lambda *s: g.standard_normal(s).astype(F32)
    x = dict(q=n(B * Lq, H), k=n(Bk * Lk, H), v=n(Bk * Lk, H), kmask=None, kbias=None, rk=None, rv=None,
             scale=F32(d ** -0.5))
    if cs["mask"]:
        km = (g.random((Bk, Lk)) < 0.6).astype(F32)
        km[:, 0] = 1
        if cs["dead"] is not None:
            km[cs["dead"]] = 0
            x["q"].reshape(B, Lq * H)[np.arange(B) // group == cs["dead"]] *= F32(0.4)
        x["kmask"] = km
    if cs["kbias"] is not None:
        kb = np.zeros((Bk, Lk), F32)
        if cs["kbias"] == "slot0":
            kb[:, 0] = np.log(5.0)
        else:
            kb[:] = np.log(g.integers(1, 6, (Bk, Lk))).astype(F32)
        x["kbias"] = kb
    if cs["rpr"] is not None:
        x["rk"], x["rv"] = (0.3 * n(2 * cs["rpr"] + 1, d)).astype(F32), (0.3 * n(2 * cs["rpr"] + 1, d)).astype(F32)
    return x


def attn_ldmask(cs):
    return cs["Lk"] + 3


def attn_f64(name, x, defect=None):
    """zk_f32_attn_kb in float64 -> the dict of score_f32_ref.attn_f64 (out [B Lq, H] and the pieces attn_bound_from needs).
    The mask term is added as fp32 adds it (func.py:372-387): 0 for a valid key; a masked key of a row with valid keys has
    probability exactly 0; a row whose every key is masked has all scores rounded to -1e8 and is uniform.

    defect:  neighbour_sentence (sentence b's memory instead of b / group's);  nkeys_off_by_one (*nkeys_dev keys);
    nkeys_unclipped (*nkeys_dev + 1 keys although Lk are there: the rows behind);  mask_stride_Lk (mask rows Lk apart);
    rpr_sign (clip(j - i));  clip_m_minus_1;  q_pos0_ignored;  kbias_dropped;  head_tail_dropped (channels 64 .. of a head
    never written);  softmax_not_normalised (exp(s - max) without the division)."""
    cs = ATTN_CASES[name]
    B, nh, Lq, Lk, d, group = (cs[k] for k in ("B", "nh", "Lq", "Lk", "d", "group"))
    H, Bk, m = nh * d, B // group, cs["rpr"]
    f = lambda a: np.asarray(a, np.float64)
    own = np.arange(B) % Bk if defect == "neighbour_sentence" else np.arange(B) // group
    nk = Lk
    if cs["nkeys"] is not None:
        nk = cs["nkeys"] + (0 if defect == "nkeys_off_by_one" else 1)
        if defect != "nkeys_unclipped":
            nk = min(nk, Lk)
    Le = max(Lk, nk)                                             # keys the statement looks at (> Lk only with the defect)
    assert Le - Lk <= ATTN_PAD_ROWS
    rows = own[:, None] * Lk + np.arange(Le)[None]               # flat key / value rows of every sentence
    kf, vf = (np.concatenate([f(x[t]), np.ones((ATTN_PAD_ROWS, H))], 0) for t in ("k", "v"))
    qh = (f(x["q"]) * float(x["scale"])).reshape(B, Lq, nh, d).transpose(0, 2, 1, 3)
    kh = kf[rows].reshape(B, Le, nh, d).transpose(0, 2, 1, 3)
    vh = vf[rows].reshape(B, Le, nh, d).transpose(0, 2, 1, 3)
    s = qh @ kh.transpose(0, 1, 3, 2)
    s_abs = np.abs(qh) @ np.abs(kh).transpose(0, 1, 3, 2)
    idx, rv = None, None
    if m is not None:
        i = np.arange(Lq)[:, None] + (0 if defect == "q_pos0_ignored" else cs["q_pos"][1])
        j = np.arange(Le)[None, :]
        mm = m - 1 if defect == "clip_m_minus_1" else m
        idx = np.clip((j - i) if defect == "rpr_sign" else (i - j), -mm, mm) + m
        rk, rv = f(x["rk"]), f(x["rv"])
        s = s + np.einsum("bhqd,qkd->bhqk", qh, rk[idx])
        s_abs = s_abs + np.einsum("bhqd,qkd->bhqk", np.abs(qh), np.abs(rk[idx]))
    ld = attn_ldmask(cs)
    at = own[:, None] * (Lk if defect == "mask_stride_Lk" else ld) + np.arange(Le)[None]
    if x["kbias"] is not None and defect != "kbias_dropped":
        kb = flat(Bk, Lk, ld, 0, x["kbias"])[LEAD:].astype(np.float64)[at][:, None, None, :]
        s, s_abs = s + kb, s_abs + np.abs(kb)
    live = np.broadcast_to((np.arange(Le) < nk)[None, None, None, :], s.shape)
    lg = np.where(live, s, -np.inf)
    full = np.zeros(B, bool)
    if x["kmask"] is not None:
        term = (1.0 - flat(Bk, Lk, ld, 0, x["kmask"])[LEAD:].astype(np.float64)[at]) * -MASK_INF          # [B, Le]
        masked = np.broadcast_to((term < -1e6)[:, None, None, :], s.shape)
        lg = np.where(masked, -np.inf, lg + np.where(term < -1e6, 0.0, term)[:, None, None, :])          # (garbage: added as it is)
        full = (term < -1e6)[:, :nk].all(1)
        if full.any():
            assert float(np.abs(s[full]).max()) < 4.0
            lg[full] = np.where(live[full], 0.0, -np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(lg - np.max(lg, -1, keepdims=True))
    e = np.where(np.isfinite(e), e, 0.0)
    p = e if defect == "softmax_not_normalised" else e / np.maximum(e.sum(-1, keepdims=True), 1e-300)
    o, ov_abs = p @ vh, p @ np.abs(vh)
    if m is not None:
        o = o + np.einsum("bhqk,qkd->bhqd", p, rv[idx])
        ov_abs = ov_abs + np.einsum("bhqk,qkd->bhqd", p, np.abs(rv[idx]))
    if defect == "head_tail_dropped":
        assert d > 64
        o = o.copy()
        o[..., 64:] = np.nan
    out = o.transpose(0, 2, 1, 3).reshape(B * Lq, H)
    return {"out": out, "s": s, "s_abs": s_abs, "p": p, "vh": vh, "ov_abs": ov_abs, "full": full, "lg": lg, "idx": idx, "rv": rv}


def attn_bound(name, x):
    """-> (ref, bound) float64: score_f32_ref.attn_bound_from (derivation there) on this statement.  The key bias is one more
    addition to the score, counted in S_j; the kernel's softmax is the plain two-pass one, which the bound's online form
    covers; expf is charged there as 4 U = C_EXP U."""
    cs = ATTN_CASES[name]
    r = attn_f64(name, x)
    return r["out"], S.attn_bound_from(r, cs["B"], cs["nh"], cs["Lq"], cs["d"])


def attn_standin(name, x):
    """torch fp32 with the keys in DESCENDING order through matrix products, the finite additive mask in fp32, torch.softmax."""
    cs = ATTN_CASES[name]
    B, nh, Lq, Lk, d, group = (cs[k] for k in ("B", "nh", "Lq", "Lk", "d", "group"))
    m = cs["rpr"]
    nk = Lk if cs["nkeys"] is None else min(cs["nkeys"] + 1, Lk)
    rev = torch.arange(nk - 1, -1, -1)
    own = torch.arange(B) // group
    f = lambda a: _t(np.asarray(a, F32))
    qh = (f(x["q"]) * torch.tensor(float(x["scale"]))).view(B, Lq, nh, d).permute(0, 2, 1, 3)
    kh = f(x["k"]).view(B // group, Lk, nh, d).permute(0, 2, 1, 3)[own][:, :, rev]
    vh = f(x["v"]).view(B // group, Lk, nh, d).permute(0, 2, 1, 3)[own][:, :, rev]
    lg = qh @ kh.transpose(-1, -2)
    if m is not None:
        idx = (torch.arange(Lq)[:, None] + cs["q_pos"][1] - rev[None, :]).clamp(-m, m) + m
        lg = lg + torch.einsum("bhqd,qkd->bhqk", qh, f(x["rk"])[idx])
    if x["kmask"] is not None:
        lg = lg + ((1.0 - f(x["kmask"])[own][:, rev]) * torch.tensor(-MASK_INF, dtype=torch.float32))[:, None, None, :]
    if x["kbias"] is not None:
        lg = lg + f(x["kbias"])[own][:, rev][:, None, None, :]
    w = torch.softmax(lg, -1)
    o = w @ vh
    if m is not None:
        o = o + torch.einsum("bhqk,qkd->bhqd", w, f(x["rv"])[idx])
    return o.permute(0, 2, 1, 3).reshape(B * Lq, nh * d).numpy()


def attn_lds_bytes(Lk, d):
    """The launch's dynamic LDS: four waves of (Lk + d) floats; zk_f32_attn refuses more than 64 KiB."""
    return 4 * (Lk + d) * 4


assert attn_lds_bytes(4032, 64) == 64 * 1024 and attn_lds_bytes(4033, 64) > 64 * 1024
