"""The checker of tests/parity.py has teeth (CPU only): a correct stand-in passes with no element excused, and each
planted defect of the kind tiled kernels have -- each touching ONE element, one 8-wide store or one guard element -- fails.

GEMM stand-in: torch fp32 product, the epilogue in fp32, one rounding to the output type (parity.cpu_gemm_standin) over
the shapes, transpositions, layouts and epilogues of tests/test_gpu_gemm_elementwise.py.
Attention stand-in: the fp32 / bf16 emulation (parity.attn_math(emulate=True)) over parity.ATTN_CASES against the
constants c_x of tests/test_gpu_attention_elementwise.py.
"""
import pytest
import torch

from tests import parity as P
from tests.test_gpu_gemm_elementwise import (EPILOGUES, SPLIT_EPILOGUES, PLAIN, STRIDED, CONTIG, SCALAR_LAYOUTS, FAMILIES,
                                             _family_cases, _rand, _bias)
from tests.test_gpu_attention_elementwise import C_X

BF, F32 = torch.bfloat16, torch.float32


def _standin_case(M, N, K, ta, tb, lay, epi, seed=0):
    """The operands of run_gemm (test_gpu_gemm_elementwise.py) on the CPU -> (guarded C holding the stand-in's result,
    ref, bound, the pieces a defect needs)."""
    a = _rand(*((K, M) if ta else (M, K)), seed + 1)
    b = _rand(*((N, K) if tb else (K, N)), seed + 2)
    a = a.t() if ta else a
    b = b.t() if tb else b
    out_dtype = F32 if epi["f32"] else BF
    res = _rand(M, N, seed + 3) if epi["res"] != "none" else None
    aux = _rand(M, N, seed + 4) if epi["act"] == 2 else None
    bias = _bias(N, seed + 5) if epi["bias"] else None
    mask = None
    if epi["drop"] > 0:
        g = torch.Generator(); g.manual_seed(seed + 6)
        mask = (torch.rand(M, N, generator=g) >= epi["drop"]).float() / (1 - epi["drop"])
    kw = dict(alpha=epi["alpha"], bias=bias, res=res, act=epi["act"], aux=aux, aux_scale=1.25, mask=mask)
    ref, bound = P.gemm_bound(a, b, K, out_dtype, **kw)
    good = P.cpu_gemm_standin(a, b, out_dtype, **kw)
    pad, off = lay["C"]
    C = P.guarded(M, N, N + pad + off, off, out_dtype, res if epi["res"] == "alias" else None)
    return C, good, ref, bound, (a, b, out_dtype, kw)


def _all_cases():
    """Every distinct (shape, transposition, layout, epilogue) of every family of the GPU file."""
    seen, out = set(), []
    for bm, bn, split, start in FAMILIES.values():
        for c in _family_cases(bm, bn, split, start):
            key = repr(c[1:])
            if key not in seen:
                seen.add(key)
                out.append(c[1:])
    return out


def test_every_layout_class_meets_every_epilogue_level_and_pair():
    """Over the families of tests/test_gpu_gemm_elementwise.py: each layout class runs with every row of the covering
    (hence with every level and every pair of levels), and every single family runs every row somewhere."""
    import itertools
    names = list(PLAIN)
    for split, rows in ((False, EPILOGUES), (True, SPLIT_EPILOGUES)):
        by_class = {}
        for (bm, bn, sp, start) in (f for f in FAMILIES.values() if f[2] == split):
            fam = _family_cases(bm, bn, sp, start)
            assert all(any(c[7] == r for c in fam if c[0] != "ldr%8") for r in rows), (bm, bn, sp, start)
            for c in fam:
                by_class.setdefault(c[0], []).append(c[7])
        classes = {"contiguous", "strided", "n517_ld520", "n517_ld517", "odd_m", "any_k"} | set(SCALAR_LAYOUTS)
        classes = classes - {"ldr%8"} if split else classes | {"edge%d" % i for i in range(6)}
        assert set(by_class) == classes
        for cls, epis in by_class.items():
            want = [dict(r, res="own") for r in rows] if cls == "ldr%8" else rows
            for r in want:
                assert r in epis, (cls, r)
            for n1, n2 in itertools.combinations(names, 2):
                have = {(e[n1], e[n2]) for e in epis}
                for r in want:                      # every valid pair of levels is in some row of the covering
                    assert (r[n1], r[n2]) in have
            for n1 in names:
                assert {e[n1] for e in epis} == {r[n1] for r in want}, (cls, n1)


def test_pairwise_covering_covers_every_valid_pair():
    import itertools
    names = list(EPILOGUES[0])
    for n1, n2 in itertools.combinations(names, 2):
        have = {(r[n1], r[n2]) for r in EPILOGUES}
        for l1 in {r[n1] for r in EPILOGUES}:
            for l2 in {r[n2] for r in EPILOGUES}:
                if {n1: l1, n2: l2} in ({"res": "alias", "f32": 1}, {"f32": 1, "res": "alias"}):
                    continue
                assert (l1, l2) in have, (n1, l1, n2, l2)
    assert len(EPILOGUES) < 20          # a covering, not the product of 144


def test_correct_gemm_standin_passes_everywhere_with_nothing_excused():
    cases = _all_cases()
    assert len(cases) > 60
    for i, (M, N, K, ta, tb, lay, epi) in enumerate(cases):
        C, good, ref, bound, _ = _standin_case(M, N, K, ta, tb, lay, epi, seed=10 * i)
        C.window().copy_(good)
        C.check_guard()
        P.assert_elementwise(C.value(), ref, bound, "stand-in %s" % ((M, N, K, ta, tb, epi),))


DEFECT_CASES = [(328, 200, 208, 0, 0, STRIDED, PLAIN), (136, 72, 200, 0, 1, SCALAR_LAYOUTS["ldc%8"], dict(PLAIN, f32=1)),
                (72, 517, 200, 0, 1, CONTIG, dict(PLAIN, bias=1, res="own")),
                (200, 517, 2048, 0, 1, CONTIG, dict(PLAIN, alpha=0.5, f32=1)),
                (263, 129, 136, 1, 1, STRIDED, dict(PLAIN, bias=1, res="alias", act=1, alpha=0.5)),
                (136, 200, 277, 1, 0, STRIDED, dict(PLAIN, act=2, drop=0.3))]


DEFECTS = ["zeroed", "stale", "k_tail", "shifted_store", "double_rounding", "guard"]


# (rounding twice to bf16 is a defect of a bf16 output)
@pytest.mark.parametrize("case,defect", [(c, d) for c in DEFECT_CASES for d in DEFECTS
                                         if not (d == "double_rounding" and c[6]["f32"])])
def test_each_planted_gemm_defect_fails(case, defect):
    M, N, K, ta, tb, lay, epi = case
    C, good, ref, bound, (a, b, out_dtype, kw) = _standin_case(M, N, K, ta, tb, lay, epi)
    got = good.clone()
    # the element where the reference is largest against its bound: a defect is planted where it is NOT hidden by a
    # reference near zero (a masked / gated element is exactly 0 in any kernel)
    live = ref.abs() / bound.clamp_min(1e-300)
    r, c = divmod(int(live.argmax()), N)
    if defect == "zeroed":
        got[r, c] = 0
    elif defect == "stale":
        got[r, c] = float("nan")
    elif defect == "k_tail":
        short = P.cpu_gemm_standin(a, b, out_dtype, k_limit=K - 8, **kw)
        delta = (short.double() - good.double()).abs() / bound.clamp_min(1e-300)
        r, c = divmod(int(delta.argmax()), N)
        got[r, c] = short[r, c]
    elif defect == "shifted_store":
        c8 = min(c // 8 * 8, N - 8)
        r = min(r, M - 2)
        got[r + 1, c8:c8 + 8] = good[r, c8:c8 + 8]
    elif defect == "double_rounding":
        bits = got.view(torch.int16)
        bits[r, c] = bits[r, c] - 2          # two ulp toward zero (sign-magnitude: the integer below)
    C.window().copy_(got)
    if defect == "guard":
        rel = P.LEAD + C.off + C.cols if C.ld > C.off + C.cols else P.LEAD + C.off + C.rows * C.ld     # pad column / row past the end
        C.t.view(torch.int16)[rel * (2 if out_dtype == F32 else 1)] = 0
        with pytest.raises(AssertionError, match="outside the"):
            C.check_guard()
        return
    C.check_guard()
    with pytest.raises(AssertionError, match="outside their bound") as info:
        P.assert_elementwise(C.value(), ref, bound, defect)
    assert "row % 64" in str(info.value) and "col % 256" in str(info.value)


def test_guard_names_the_touched_element_and_inputs_are_compared_whole():
    g = P.guarded(5, 16, 24, 3, BF, torch.zeros(5, 16))
    g.check_guard(); g.check_intact()
    g.t[P.LEAD + 2 * 24 + 3 + 16] = 1.0          # first pad column behind row 2
    with pytest.raises(AssertionError, match=r"row 2, col 16"):
        g.check_guard()
    g = P.guarded(5, 16, 24, 3, F32, torch.zeros(5, 16))
    g.t[P.LEAD - 1] = 0.0                          # the element in front of the window's first row
    with pytest.raises(AssertionError, match=r"row -1"):
        g.check_guard()
    g = P.guarded(5, 16, 24, 3, BF, torch.zeros(5, 16))
    g.window()[4, 15] = 1.0                        # inside the window: the guard is intact, the operand is not
    g.check_guard()
    with pytest.raises(AssertionError, match=r"row 4, col 15"):
        g.check_intact()
    assert torch.isnan(P.guarded(3, 8, 8, 0, BF).value().float()).all()
    assert P.guarded(3, 8, 9, 1, F32).mat.ld == 9


# ---------------------------------------------------------------------------------------------- attention
def _attn_pair(case):
    B, nh, Lq, Lk, mask, causal, rpr, drop = case
    x = P.attn_inputs(case)
    dm = None
    if drop > 0:
        g = torch.Generator(); g.manual_seed(5)
        dm = (torch.rand(B, nh, Lq, Lk, generator=g) >= drop).float() / (1 - drop)
    kw = dict(kmask=x["kmask"], causal=causal, rk=x["rk"], rv=x["rv"], max_rel=P.ATTN_MAX_REL, drop_mask=dm)
    ref = P.attn_math(x["q"], x["k"], x["v"], x["dout"], B, nh, Lq, Lk, P.ATTN_D, **kw)
    emu = P.attn_math(x["q"], x["k"], x["v"], x["dout"], B, nh, Lq, Lk, P.ATTN_D, emulate=True, **kw)
    return ref, emu


@pytest.mark.parametrize("case", P.ATTN_CASES)
def test_attention_emulation_is_inside_c_x_and_planted_row_defects_are_not(case):
    nh = case[1]
    ref, emu = _attn_pair(case)
    for key in C_X:
        if key not in ref:
            continue
        heads = nh if key in ("out", "dq", "dk", "dv") else 1
        worst = P.assert_attn_rows(emu[key], ref[key], P.ATTN_D, C_X[key], key, heads=heads)
        assert worst <= C_X[key] / 2 * 1.001, (key, worst)      # c_x is TWICE the emulation's worst ratio
        if ref[key].shape[0] < 2:
            continue
        for name, bad in P.plant_attn_defects(emu[key], P.ATTN_D, heads).items():
            with pytest.raises(AssertionError, match="beyond c"):
                P.assert_attn_rows(bad, ref[key], P.ATTN_D, C_X[key], "%s %s" % (key, name), heads=heads)
    assert float((emu["lse"] - ref["lse"]).abs().max()) < 2e-2
