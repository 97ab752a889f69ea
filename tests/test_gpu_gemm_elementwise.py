"""Element-wise parity of every GEMM family against the float64 reference and the derived bound of tests/parity.py
(gemm_bound: u_out |ref| + (K + 8) 2^-23 mag; nothing measured, nothing excused), on guarded operands:

  * the output is a NaN-prefilled window of a larger buffer: an element nobody wrote, or a write outside the window
    (pad columns, rows past the last, the bytes in front) fails;
  * A, B, an un-aliased residual, aux and the bias are bit-identical after the call;
  * layouts: contiguous; every operand a column window of a wider buffer (own ld, own offset, all multiples of 8: the
    16-byte epilogue); the scalar epilogue (ldc % 8 != 0, C offset by 1-4 elements, ldr % 8 != 0, N = 517 in ld 520 and
    in ld 517, odd M, arbitrary K); tile edges (tile - 1, tile + 1, 2 tile + 7, M = 1, K = 8, K below one K tile, K tail);
    split-K with N % 4 != 0;
  * epilogues: bias, residual (aliasing C or not), act 1 / 2, dropout, alpha != 1, fp32 output by a pairwise covering
    (EPILOGUES).  Each family gives layout slot i row (start + i) of it with a start of its own (FAMILIES), so every
    layout class meets every row over the families, and the two MFMA kernels also run every row on every class in
    one test (tests/test_parity_checker.py asserts the former on the CPU).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng  # noqa: E402
from tests.parity import guarded, assert_elementwise, gemm_bound, pairwise  # noqa: E402
from zero_amd import hip  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32

# (pad, off) per operand A, B, C, residual, aux: the window starts `off` columns into a row of ld = cols + off + pad
CONTIG = dict(A=(0, 0), B=(0, 0), C=(0, 0), R=(0, 0), X=(0, 0))
STRIDED = dict(A=(8, 8), B=(16, 24), C=(8, 16), R=(24, 8), X=(16, 32))
SCALAR_LAYOUTS = {
    "ldr%8": dict(STRIDED, R=(3, 0)), "ldc%8": dict(STRIDED, C=(5, 0)),
    "c_off1": dict(STRIDED, C=(7, 1)), "c_off2": dict(CONTIG, C=(6, 2)),
    "c_off3": dict(STRIDED, C=(13, 3)), "c_off4": dict(CONTIG, C=(4, 4)),
}

EPILOGUES = pairwise(
    dict(bias=[0, 1], res=["none", "alias", "own"], act=[0, 1, 2], drop=[0.0, 0.3], alpha=[1.0, 0.5], f32=[0, 1]),
    valid=lambda r: not (r["res"] == "alias" and r["f32"]))       # the residual is bf16: it can alias a bf16 C only
PLAIN = dict(bias=0, res="none", act=0, drop=0.0, alpha=1.0, f32=0)


def _rand(rows, cols, seed, scale=1.0):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return (torch.randn(rows, cols, generator=g) * scale).to(BF)


def _bias(N, seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.randn(N, generator=g)


def _operand(rows, cols, lay, seed, dtype=BF, prefill="rand"):
    pad, off = lay
    data = _rand(rows, cols, seed) if isinstance(prefill, str) else prefill
    return guarded(rows, cols, cols + pad + off, off, dtype, data, "cuda")


def _dropout_mask(e, M, N, p, sid):
    msk = torch.zeros(M * N, device="cuda")
    e.lib.call("zk_dropout_mask", msk.data_ptr(), M * N, p, e.seed.data_ptr(), sid, e.stream)
    torch.cuda.synchronize()
    return msk.view(M, N).cpu()


def run_gemm(impl, M, N, K, ta, tb, lay=CONTIG, epi=PLAIN, seed=0, what=""):
    """One zk_gemm call on guarded operands, checked element by element."""
    e = eng()
    what = "%s impl=%#x %dx%dx%d ta=%d tb=%d lay=%s epi=%s" % (what, impl, M, N, K, ta, tb, lay, epi)
    A = _operand(*((K, M) if ta else (M, K)), lay["A"], seed + 1)
    B = _operand(*((N, K) if tb else (K, N)), lay["B"], seed + 2)
    out_dtype = F32 if epi["f32"] else BF
    res_v = _rand(M, N, seed + 3) if epi["res"] != "none" else None
    C = _operand(M, N, lay["C"], 0, out_dtype, prefill=res_v if epi["res"] == "alias" else None)
    R = _operand(M, N, lay["R"], 0, BF, prefill=res_v) if epi["res"] == "own" else None
    X = _operand(M, N, lay["X"], seed + 4) if epi["act"] == 2 else None
    bias = guarded(1, N, N, 0, F32, _bias(N, seed + 5), "cuda") if epi["bias"] else None
    e.set_seed(1234)
    e.gemm(A.mat, B.mat, C.mat, M, N, K, ta, tb, alpha=epi["alpha"],
           bias=bias.window().view(-1) if bias else None,
           residual=C.mat if epi["res"] == "alias" else (R.mat if R else None), act=epi["act"],
           aux=X.mat if X else None, aux_scale=1.25, drop_p=epi["drop"], sid=77, impl=impl)
    torch.cuda.synchronize()
    mask = _dropout_mask(e, M, N, epi["drop"], 77) if epi["drop"] > 0 else None
    a = A.value().t() if ta else A.value()
    b = B.value().t() if tb else B.value()
    ref, bound = gemm_bound(a, b, K, out_dtype, alpha=epi["alpha"], bias=bias.value().view(-1) if bias else None,
                            res=res_v, act=epi["act"], aux=X.value() if X else None, aux_scale=1.25, mask=mask)
    C.check_guard(what + " C")
    assert_elementwise(C.value(), ref, bound, what)
    for name, g in (("A", A), ("B", B), ("residual", R), ("aux", X), ("bias", bias)):
        if g is not None:
            g.check_intact(what + " " + name)


def _mfma_shape(M, N, K, ta, tb):
    """The nearest shape mfma_ok (zk_gemm.hip) accepts: the contiguous dimension of A and of B a multiple of 8."""
    r8 = lambda x: max(8, (x + 7) // 8 * 8)
    if ta:
        M = r8(M)
    if not ta or tb:
        K = r8(K)
    if not tb:
        N = r8(N)
    return M, N, K


TRANS = [(0, 0), (0, 1), (1, 0), (1, 1)]
SPLIT_EPILOGUES = [dict(PLAIN, alpha=al, f32=f) for al in (1.0, 0.5) for f in (0, 1)]   # all a split launch may carry
N517_LD520 = dict(CONTIG, C=(3, 0), R=(3, 0), X=(3, 0))


def _layout_slots(bm, bn, split):
    """(layout class, M, N, K, ta, tb, layout) of one family; ta = None: any transposition.  Split-K families run
    K = 2048 (the automatic rule wants K >= 1024), have no residual (so no ldr % 8 class) and no tile edges."""
    k = 2048 if split else 200
    slots = [("contiguous", 328, 200, k, None, None, CONTIG), ("contiguous", 328, 200, k, None, None, CONTIG),
             ("strided", 328, 200, k, None, None, STRIDED), ("strided", 328, 200, k, None, None, STRIDED)]
    slots += [(name, 136, 72, k, None, None, lay) for name, lay in SCALAR_LAYOUTS.items() if not (split and name == "ldr%8")]
    # N % 8 != 0 (tb = 1): ld 520 = the 16-byte path with a ragged last chunk, ld 517 = the scalar path; odd M; any K
    slots += [("n517_ld520", 72, 517, k, 0, 1, N517_LD520), ("n517_ld517", 72, 517, k, 0, 1, CONTIG),
              ("odd_m", 133, 200, k, 0, 0, STRIDED), ("any_k", 136, 200, k + 77, 1, 0, STRIDED)]
    if not split:
        # tile edges: M, N at tile - 1, tile + 1, 2 tile + 7 and M = 1; K = 8, K below one K tile, K with a tail
        edges = [(bm - 1, bn + 1, 8), (bm + 1, bn - 1, 40), (2 * bm + 7, bn + 1, 200), (1, 2 * bn + 7, 72),
                 (bm + 1, 2 * bn + 7, 136), (bm - 1, bn - 1, 64)]
        slots += [("edge%d" % i, M, N, K, None, None, CONTIG if i % 2 else STRIDED) for i, (M, N, K) in enumerate(edges)]
    return slots


def _family_cases(bm, bn, split=False, start=0):
    """(layout class, M, N, K, ta, tb, layout, epilogue) of one kernel family: every layout class, slot i with epilogue
    row (start + i) of the covering.  A family has more slots than the covering has rows, so it runs every row; the
    families' starts differ (FAMILIES), so that over the families EVERY layout class meets EVERY row, i.e. every level
    and every pair of levels of the epilogue (tests/test_parity_checker.py asserts it).  Split-K is taken with the plain
    epilogue only (zk_gemm.hip): those families rotate alpha x fp32 output."""
    rows = SPLIT_EPILOGUES if split else EPILOGUES
    cases = []
    for i, (cls, M, N, K, ta, tb, lay) in enumerate(_layout_slots(bm, bn, split)):
        epi = rows[(start + i) % len(rows)]
        if cls == "ldr%8":
            epi = dict(epi, res="own")         # the residual's leading dimension matters where it has a buffer of its own
        if ta is None:
            ta, tb = TRANS[(start + i + (start + i) // 4) % 4]
            if cls in ("contiguous", "strided"):
                K += 8 * ta
            if cls.startswith("edge"):
                # the nearest shape mfma_ok accepts in this transposition, and the exact one in ta = 0, tb = 1
                cases.append((cls, M, N, K, 0, 1, CONTIG if lay is STRIDED else STRIDED, epi))
                M, N, K = _mfma_shape(M, N, K, ta, tb)
        cases.append((cls, M, N, K, ta, tb, lay, epi))
    return cases


TILES = {1: (128, 128), 2: (128, 64), 3: (64, 128), 4: (64, 64), 5: (256, 128), 6: (256, 128), 7: (128, 256)}
AUTO = [(impl, 0) for impl in (1, 2, 3)]
TILE_OVERRIDES = [(2, t) for t in range(1, 8)] + [(3, t) for t in range(1, 5)]
RING2 = [6, 7]
TWO_WAVE = [2, 4]
PRODUCER = [(4, 0), (4, 2), (4, 8), (1, 0), (1, 2 << 4), (1, 8 << 4), (1, (4 << 4) | 256), (2, 4 << 12), (3, 8 << 12)]
SPLITS = [(impl, s) for impl in (2, 3) for s in (0, 3, 8)]
# every family of this file: name -> (bm, bn, split-K?, start).  The unsplit families' starts run on from 0, so with
# more of them than covering rows each layout slot meets each row; likewise the split families over their four.
FAMILIES = {}
for _kind, _keys, _tile in (("auto", AUTO, lambda k: (64, 64)), ("tile", TILE_OVERRIDES, lambda k: TILES[k[1]]),
                            ("ring2", RING2, lambda k: TILES[k]), ("two_wave", TWO_WAVE, lambda k: (64, 64)),
                            ("producer", PRODUCER, lambda k: TILES[k[0]])):
    for _k in _keys:
        FAMILIES[(_kind, _k)] = _tile(_k) + (False, len(FAMILIES))
for _i, _k in enumerate(SPLITS):
    FAMILIES[("split", _k)] = (64, 64, True, _i)


def _run_family(key, impl, what=""):
    bm, bn, split, start = FAMILIES[key]
    for i, (cls, M, N, K, ta, tb, lay, epi) in enumerate(_family_cases(bm, bn, split, start)):
        run_gemm(impl, M, N, K, ta, tb, lay, epi, seed=10 * i + start, what="%s %s" % (what, cls))


# impl 1 = the reference kernel (any shape), 2 = LDS-DMA ring kernel, 3 = register-staged kernel; automatic tile
@pytest.mark.parametrize("impl", [1, 2, 3])
def test_gemm_elementwise_auto_tile(impl):
    _run_family(("auto", (impl, 0)), impl)


@pytest.mark.parametrize("impl", [2, 3])
def test_gemm_elementwise_every_epilogue_row_on_every_layout_class(impl):
    """One kernel, the whole covering on one representative of each layout class (contiguous, strided, every scalar
    variant, N = 517 in ld 520 and in ld 517, odd M, any K, one tile edge) -- not only over the families together.
    The two MFMA kernels: theirs is the 16-byte / scalar epilogue of zk_gemm2_dev.h; the reference kernel stores
    element by element and runs the whole covering in test_reference_kernel_takes_unaligned_operands."""
    seen = set()
    for i, (cls, M, N, K, ta, tb, lay) in enumerate(_layout_slots(64, 64, False)):
        if cls in seen or (cls.startswith("edge") and cls != "edge2"):
            continue
        seen.add(cls)
        for j, epi in enumerate(EPILOGUES):
            if cls == "ldr%8":
                epi = dict(epi, res="own")
            t = (ta, tb) if ta is not None else TRANS[(i + j) % 4]
            m, n, k = _mfma_shape(M, N, K, *t)
            run_gemm(impl, m, n, k, t[0], t[1], lay, epi, seed=1000 + 20 * i + j, what="%s row %d" % (cls, j))


def test_reference_kernel_takes_unaligned_operands():
    """impl 1 beyond mfma_ok: odd leading dimensions and offsets of A and B, odd K"""
    lay = dict(A=(2, 1), B=(2, 3), C=(6, 1), R=(1, 2), X=(4, 5))
    for i, epi in enumerate(EPILOGUES):
        ta, tb = TRANS[i % 4]
        run_gemm(1, 67, 45, 51, ta, tb, lay, epi, seed=i)
    with pytest.raises(hip.ZeroHipError):
        run_gemm(2, 67, 45, 51, 0, 0, lay, PLAIN)            # the MFMA kernels refuse what mfma_ok does not accept


@pytest.mark.parametrize("impl,tile", TILE_OVERRIDES)
def test_gemm_elementwise_tile_overrides(impl, tile):
    _run_family(("tile", (impl, tile)), impl | (tile << 8))


@pytest.mark.parametrize("tile", RING2)
def test_gemm_elementwise_wide_tiles_ring_depth_2(tile):
    _run_family(("ring2", tile), 2 | (tile << 8) | (2 << 24))


@pytest.mark.parametrize("variant", TWO_WAVE)
def test_gemm_elementwise_two_wave_workgroups(variant):
    e = eng()
    old = e.lib.raw("zk_tune")(4, variant)
    try:
        _run_family(("two_wave", variant), 2 | (4 << 8), what="two-wave %d" % variant)
    finally:
        e.lib.raw("zk_tune")(4, old)


@pytest.mark.parametrize("tile,tune", PRODUCER)
def test_gemm_elementwise_producer_wave_workgroups(tile, tune):
    e = eng()
    old = e.lib.raw("zk_tune")(6, tune)
    try:
        _run_family(("producer", (tile, tune)), 2 | (tile << 8) | (1 << 16), what="producer waves %#x" % tune)
    finally:
        e.lib.raw("zk_tune")(6, old)


@pytest.mark.parametrize("impl,split", SPLITS)
def test_gemm_elementwise_split_k(impl, split):
    """split 0: the automatic rule splits these (few tiles, K >= 1024); else impl bits [23:16]"""
    _run_family(("split", (impl, split)), impl | (split << 16))
    # the slab branch with N % 4 != 0, and the wide tiles' split
    run_gemm(impl | (split << 16), 200, 517, 2048, 0, 1, dict(CONTIG, C=(3, 0)), PLAIN)
    run_gemm(impl | (split << 16), 200, 517, 2048, 0, 1, CONTIG, dict(PLAIN, f32=1, alpha=0.5))
    if impl == 2 and split:
        for tile in (5, 6, 7):
            run_gemm(impl | (tile << 8) | (split << 16), 264, 520, 2048 + 72, 1, 0, STRIDED, dict(PLAIN, f32=1))


def test_gemm_elementwise_automatic_split_is_taken():
    """the plans of the split-0 family's shapes really split (so that family is not the unsplit kernel again)"""
    e = eng()
    for cls, M, N, K, ta, tb, lay, epi in _family_cases(64, 64, True):
        assert (e.lib.raw("zk_gemm_plan")(M, N, K, epi["f32"], 1) >> 24) & 15 > 1, (cls, M, N, K, epi)


# ------------------------------------------------------------------ K-segmented
@pytest.mark.parametrize("tb", [0, 1])
@pytest.mark.parametrize("shape", [(200, 264, 128, 3), (72, 40, 64, 1), (130, 512, 192, 16), (63, 520, 64, 2),
                                   (65, 72, 64, 5), (1, 136, 128, 2)])
@pytest.mark.parametrize("lay", ["contig", "strided"])
def test_gemm_kseg_elementwise(tb, shape, lay):
    e = eng()
    M, N, kseg, nseg = shape
    L = CONTIG if lay == "contig" else STRIDED
    A = [_operand(M, kseg, L["A"], 10 + i) for i in range(nseg)]
    Bm = [_operand(*((N, kseg) if tb else (kseg, N)), L["B"], 40 + i) for i in range(nseg)]
    a = torch.cat([x.value() for x in A], 1)
    b = torch.cat([(x.value().t() if tb else x.value()) for x in Bm], 0)
    res_v = _rand(M, N, 99)
    for res in ("none", "alias", "own"):
        C = _operand(M, N, L["C"], 0, BF, prefill=res_v if res == "alias" else None)
        R = _operand(M, N, L["R"], 0, BF, prefill=res_v) if res == "own" else None
        e.gemm_kseg([(x.mat, y.mat) for x, y in zip(A, Bm)], C.mat, M, N, kseg, tb,
                    residual=C.mat if res == "alias" else (R.mat if R else None))
        torch.cuda.synchronize()
        ref, bound = gemm_bound(a, b, kseg * nseg, BF, res=None if res == "none" else res_v)
        what = "kseg %s tb=%d %s res=%s" % (shape, tb, lay, res)
        C.check_guard(what)
        assert_elementwise(C.value(), ref, bound, what)
        if R is not None:
            R.check_intact(what + " residual")
    for x in A + Bm:
        x.check_intact("kseg operand")


def test_gemm_kseg_refuses_what_its_vector_epilogue_cannot_store():
    """zk_gemm_kseg has the 16-byte epilogue only: ldc % 8 != 0, a C offset by one element and ldr % 8 != 0 are errors"""
    e = eng()
    M, N, kseg = 72, 64, 64
    A, Bm = _operand(M, kseg, (0, 0), 1), _operand(kseg, N, (0, 0), 2)
    for layC, layR in (((5, 0), None), ((7, 1), None), ((0, 0), (3, 0))):
        C = _operand(M, N, layC, 0, BF, prefill=None)
        R = _operand(M, N, layR, 3) if layR else None
        with pytest.raises(hip.ZeroHipError):
            e.gemm_kseg([(A.mat, Bm.mat)], C.mat, M, N, kseg, 0, residual=R.mat if R else None)
        torch.cuda.synchronize()
        C.check_guard("refused call")
        assert torch.isnan(C.value().float()).all()


# ------------------------------------------------------------------ grouped
def _grouped(tile, ta, tb, specs, what):
    """specs: (M, N, K, f32, bias, res ('none' | 'alias' | 'own'), colsum, layout dict or per-problem C Mat factory)"""
    e = eng()
    probs, checks = [], []
    for i, (M, N, K, f32, bias, res, cs, lay) in enumerate(specs):
        A = _operand(*((K, M) if ta else (M, K)), lay["A"], 10 + i)
        Bm = _operand(*((N, K) if tb else (K, N)), lay["B"], 20 + i)
        res_v = _rand(M, N, 30 + i) if res != "none" else None
        C = lay["Cmat"](i) if "Cmat" in lay else _operand(M, N, lay["C"], 0, F32 if f32 else BF,
                                                           prefill=res_v if res == "alias" else None)
        R = _operand(M, N, lay["R"], 0, BF, prefill=res_v) if res == "own" else None
        bias_g = guarded(1, N, N, 0, F32, _bias(N, 50 + i), "cuda") if bias else None
        cs_g = guarded(1, N, N, 0, F32, None, "cuda") if cs else None
        Cm = C if not hasattr(C, "mat") else C.mat
        probs.append((A.mat, Bm.mat, Cm, M, N, K, bias_g.window().view(-1) if bias_g else None,
                      Cm if res == "alias" else (R.mat if R else None), cs_g.window().view(-1) if cs_g else None))
        checks.append((A, Bm, C, R, bias_g, cs_g, res_v))
    e.gemm_grouped(probs, ta, tb, tile=tile)
    torch.cuda.synchronize()
    for i, ((M, N, K, f32, bias, res, cs, lay), (A, Bm, C, R, bias_g, cs_g, res_v)) in enumerate(zip(specs, checks)):
        w = "%s tile=%s ta=%d tb=%d problem %d (%dx%dx%d)" % (what, tile, ta, tb, i, M, N, K)
        a = A.value().t() if ta else A.value()
        b = Bm.value().t() if tb else Bm.value()
        ref, bound = gemm_bound(a, b, K, F32 if f32 else BF, bias=bias_g.value().view(-1) if bias_g else None, res=res_v)
        if hasattr(C, "mat"):
            C.check_guard(w)
            got = C.value()
        else:
            got = C.torch().cpu()
        assert_elementwise(got, ref, bound, w)
        if cs_g is not None:
            # column sums of B over K (fp32 accumulation of bf16 values, fp32 out)
            ones = torch.ones(1, K, dtype=BF)
            cref, cbound = gemm_bound(ones, b, K, F32)
            cs_g.check_guard(w + " column sums")
            assert_elementwise(cs_g.value().view(-1), cref.view(-1), cbound.view(-1), w + " column sums")
        for g in (A, Bm, R, bias_g):
            if g is not None:
                g.check_intact(w)


SCALAR_C = [dict(STRIDED, C=(5, 0)), dict(STRIDED, C=(7, 1)), dict(CONTIG, C=(5, 3)), dict(STRIDED, R=(3, 0))]


@pytest.mark.parametrize("tile", [128, 64])
@pytest.mark.parametrize("ta,tb", TRANS)
def test_gemm_grouped_elementwise(tile, ta, tb):
    t = tile
    shapes = [(t - 1, t + 1, 200), (t + 1, t - 1, 40), (2 * t + 7, t + 1, 8), (1, 2 * t + 7, 72), (136, 520, 264),
              (264, 72, 1000)]
    for lays, what in (([CONTIG] * 6, "contiguous"), ([STRIDED] * 6, "strided"),
                       (SCALAR_C + SCALAR_C[:2], "scalar epilogue")):
        specs = []
        for i, ((M, N, K), lay) in enumerate(zip(shapes, lays)):
            M, N, K = _mfma_shape(M, N, K, ta, tb)
            res = ("none", "alias", "own")[i % 3]
            f32 = 1 if (i % 2 == 0 and res != "alias") else 0
            if lay["R"][0] % 8:
                res, f32 = "own", 0
            specs.append((M, N, K, f32, i % 2, res, False, lay))
        _grouped(tile, ta, tb, specs, what)


@pytest.mark.parametrize("tile", [128, 64])
def test_gemm_grouped_writes_the_three_slices_of_one_qkv_buffer(tile):
    """the model's own layout (zero_amd/models/_core.py): three H-wide products into the column slices of one [T, 3H]
    buffer by one grouped launch -- every slice correct, nothing outside the buffer's window touched"""
    T, H = 200, 136
    qkv = guarded(T, 3 * H, 3 * H + 16, 8, BF, None, "cuda")
    lay = dict(CONTIG, Cmat=lambda i: qkv.mat.cols_slice(i * H, (i + 1) * H))
    _grouped(tile, 0, 0, [(T, H, 264, 0, 1, "none", False, lay)] * 3, "qkv slices")
    qkv.check_guard("qkv buffer")
    assert torch.isfinite(qkv.value().float()).all()


@pytest.mark.parametrize("tile", [(256, 128), (128, 256), (256, 256), (256, 256, 0)])
@pytest.mark.parametrize("lay", ["contig", "strided", "scalar"])
def test_gemm_grouped_wide_tiles_with_column_sums_elementwise(tile, lay):
    """weight-gradient form (ta = 1, tb = 0, fp32 out) with the bias gradient as column sums; a problem without them"""
    bm, bn = tile[:2]
    L = {"contig": CONTIG, "strided": STRIDED, "scalar": dict(STRIDED, C=(2, 3))}[lay]
    shapes = [(bm - 8, bn + 8, 1000, True), (bm + 8, bn - 8, 264, True), (2 * bm + 8, 72, 40, False), (8, 2 * bn + 8, 8, True),
              (264, 304, 72, True)]
    _grouped(tile, 1, 0, [(M, N, K, 1, 0, "none", cs, L) for M, N, K, cs in shapes], lay)


@pytest.mark.parametrize("tile", [(256, 128), (128, 256)])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 1)])
def test_gemm_grouped_wide_tiles_other_transpositions(tile, ta, tb):
    bm, bn = tile
    specs = []
    for i, (M, N, K) in enumerate([(bm - 1, bn + 1, 200), (bm + 1, bn - 1, 40), (2 * bm + 7, 72, 8), (1, 2 * bn + 7, 72)]):
        M, N, K = _mfma_shape(M, N, K, ta, tb)
        specs.append((M, N, K, i % 2, i % 2, ("none", "own", "alias", "none")[i] if not i % 2 else "none", False,
                      (CONTIG, STRIDED, SCALAR_C[0], SCALAR_C[1])[i]))
    _grouped(tile, ta, tb, specs, "wide")
