"""The decode-kernel checks of tests/test_gpu_decode_elementwise.py have teeth and their constants are measured (CPU only).

Measured: for every case of the tables of tests/decode_parity.py the row ratio of the emulation (float32, bf16 rounding
of q, k, v, P, ctx; of y and the output for the LayerNorm) against the float64 reference, per kind of output.  The
constants of the GPU file must be between once and twice the worst ratio, so they cannot drift.  C_LN_ELEM likewise from
float32 LayerNorms that sum in forward, reversed, pairwise and 64-strided order.

Planted: each defect of decode_parity.ATTN_DEFECTS / LN_DEFECTS on the case built for it must exceed FOUR times the
constant of the output it is judged on (run with -s for the table):
    neighbour_k / neighbour_v / neighbour_mask   one row of a group that straddles two sentences reads the other sentence
    stale_slot, skip_t, past_t                   slot t stale / left out / slot t + 1 let in (self-attention, t = 33)
    clip_off1, sign_flip, no_rpr_v               relative positions (tables of order 0.5, max_rel 4, position 9, 33 keys)
    zero_head                                    one head's part zeroed
    drop_last_part, no_bias                      the LayerNorm's partial sums (judged on the LayerNorm rows)
    cache_twice                                  the running sum updated twice: the exact fp32 check fails, and the
                                                 average half of cat_out is far outside its element bound
"""
import pytest
import torch

from tests import parity as P
from tests import decode_parity as DP
from tests.test_gpu_decode_elementwise import C_PART, C_SUM, C_LN, C_LN_ELEM


def _between(worst, c, what):
    print("%s: worst emulation ratio %.4g, constant %.4g (= %.3f x)" % (what, worst, c, c / worst))
    assert worst <= c <= 2 * worst * 1.0005, (what, worst, c)


@pytest.fixture(scope="module")
def attn_ratios():
    out = []
    for kind, cases, inputs, math in (("cross", DP.cross_cases(), DP.cross_inputs, DP.cross_math),
                                      ("self", DP.SELF_CASES, DP.self_inputs, DP.self_math)):
        for case in cases:
            x = inputs(case)
            ref, emu = math(case, x), math(case, x, emulate=True)
            out.append((kind, case, ref["smax"], DP.parts_ratio(emu["parts"], ref["parts"]),
                        DP.row_ratio(emu["sum"], ref["sum"])))
    return out


def test_scores_stay_below_four(attn_ratios):
    worst = max(r[2] for r in attn_ratios)
    print("largest |score| over %d cases: %.3f" % (len(attn_ratios), worst))
    assert worst < 4.0


def test_attention_constants_are_twice_the_measured_emulation(attn_ratios):
    for kind, case, smax, rp, rs in attn_ratios:
        print("%-5s %-90s part %.3e  sum %.3e" % (kind, {k: v for k, v in case.items()}, rp, rs))
    assert sum(1 for r in attn_ratios if r[1]["H"] == 2048) == 2          # one H = 2048 case per entry point
    _between(max(r[3] for r in attn_ratios), C_PART, "head part")
    _between(max(r[4] for r in attn_ratios), C_SUM, "head sum")


def _ln_table():
    """Every LayerNorm the GPU file runs: zk_ln_decode alone and the prologues."""
    for c in DP.ln_cases():
        yield "alone %s" % (c,), DP.ln_inputs(c["rows"], c["H"], c["form"], c["cache"])
    for case in (DP.PRO_CROSS, DP.PRO_SELF):
        (B, R), H = case["BR"], case["H"]
        for form, cache, tdev in DP.PROLOGUE_CASES:
            yield "prologue %s cache=%d" % (form, cache), DP.ln_inputs(B * R, H, form, cache, seed=1,
                                                                        nparts=H // DP.D if form == "parts4" else None)


def test_layernorm_constants_are_twice_the_measured_emulation():
    worst_row, worst_elem = 0.0, 0.0
    for name, a in _ln_table():
        ref, emu = DP.ln_run(a), DP.ln_run(a, emulate=True)
        r = DP.row_ratio(emu["out"], ref["out"])
        worst_row = max(worst_row, r)
        line = "%-100s rows %.3e" % (name, r)
        y = DP.ln_exact_y(a)
        if y is not None:
            ref_e, unit = DP.ln_unit(a["x"], y, a["gamma"], a["beta"], DP.EPS)
            v = a["x"].float() + y.float()
            ru = max(float(((DP.ln32(v, a["gamma"], a["beta"], DP.EPS, o) - ref_e).abs() / unit.clamp_min(1e-300)).max())
                     for o in DP.LN_ORDERS)
            worst_elem = max(worst_elem, ru)
            line += "  elements %.3g units" % ru
            # the emulation's bf16 output is inside the element bound built on the constant
            _, bound = DP.ln_elem(a["x"], y, a["gamma"], a["beta"], DP.EPS, C_LN_ELEM)
            P.assert_elementwise(emu["out"], ref_e, bound, name)
        print(line)
        if a["cache"] is not None:
            DP.assert_running_sum(a["cache"], emu["out"].to(torch.bfloat16), emu["cache"], name)
            ref_c, bound_c = DP.cat_bound(emu["cache"], a["inv_count"])
            P.assert_elementwise(emu["cat"][:, a["x"].shape[1]:], ref_c, bound_c, name + " cat")
    _between(worst_row, C_LN, "LayerNorm rows")
    _between(worst_elem, C_LN_ELEM, "LayerNorm elements (units of 2^-23 (|gamma| |xhat| + |beta|))")


@pytest.mark.parametrize("name", list(DP.ATTN_DEFECTS))
def test_each_planted_attention_defect_fails(name):
    rp, rs = DP.attn_defect_ratios(name)
    print("%-16s head part %.3e (%.1f c)   head sum %.3e (%.1f c)" % (name, rp, rp / C_PART, rs, rs / C_SUM))
    assert rp >= 4 * C_PART, (name, rp)
    assert rs >= 4 * C_SUM, (name, rs)


def test_the_correct_emulation_passes_the_defect_cases():
    for name, (kind, case) in DP.ATTN_DEFECTS.items():
        x = DP.cross_inputs(case) if kind == "cross" else DP.self_inputs(case, stale=True)
        math = DP.cross_math if kind == "cross" else DP.self_math
        ref, emu = math(case, x), math(case, x, emulate=True)
        assert DP.parts_ratio(emu["parts"], ref["parts"]) <= C_PART / 2 * 1.0005
        assert DP.row_ratio(emu["sum"], ref["sum"]) <= C_SUM / 2 * 1.0005


@pytest.mark.parametrize("name", list(DP.LN_DEFECTS))
def test_each_planted_layernorm_defect_fails(name):
    form, cache = DP.LN_DEFECTS[name]
    a = DP.ln_inputs(12, 128, form, cache, seed=1)
    ref, bad = DP.ln_run(a), DP.ln_run(a, emulate=True, defect=name)
    if name == "cache_twice":
        with pytest.raises(AssertionError, match="running sum"):
            DP.assert_running_sum(a["cache"], bad["out"].to(torch.bfloat16), bad["cache"], name)
        # and the average the next layer reads, judged from the CORRECT running sum
        good = DP.ln_run(a, emulate=True)
        ref_c, bound_c = DP.cat_bound(good["cache"], a["inv_count"])
        with pytest.raises(AssertionError, match="outside their bound"):
            P.assert_elementwise(bad["cat"][:, 128:], ref_c, bound_c, name)
        r = DP.row_ratio(bad["cat"][:, 128:], ref["cat"][:, 128:])
        print("%-16s cat average rows %.3e (%.1f c)" % (name, r, r / C_LN))
        assert r >= 4 * C_LN
        return
    r = DP.row_ratio(bad["out"], ref["out"])
    print("%-16s LayerNorm rows %.3e (%.1f c)" % (name, r, r / C_LN))
    assert r >= 4 * C_LN, (name, r)
    _, bound = DP.ln_elem(a["x"], DP.ln_exact_y(a), a["gamma"], a["beta"], DP.EPS, C_LN_ELEM)
    with pytest.raises(AssertionError, match="outside their bound"):
        P.assert_elementwise(bad["out"], ref["out"], bound, name)


def test_gemm_parts_ranges_are_multiples_of_64():
    assert [len(DP.gemm_parts_ranges(K, s)) for _, _, K, s in DP.GEMM_PARTS_CASES] == [3, 1, 4, 3]
    assert DP.gemm_parts_ranges(512, 3) == [(0, 192), (192, 384), (384, 512)]


def test_cross_table_covers_every_pair_and_the_forced_cases():
    import itertools
    cases = DP.cross_cases()
    small = [c for c in cases if c["H"] != 2048]
    for n1, n2 in itertools.combinations(list(DP.CROSS_FACTORS), 2):
        have = {(repr(c[n1]), repr(c[n2])) for c in small}
        for l1 in DP.CROSS_FACTORS[n1]:
            for l2 in DP.CROSS_FACTORS[n2]:
                if 2048 in (l1, l2) and "H" in (n1, n2):
                    continue
                assert (repr(l1), repr(l2)) in have, (n1, l1, n2, l2)
    rows = lambda c: c["BR"][0] * c["BR"][1]
    assert any(c["group"] == 16 and rows(c) == 12 for c in cases) and any(c["group"] == 16 and rows(c) == 20 for c in cases)
    assert any(c["group"] == 3 and c["BR"][1] == 4 for c in cases)
    assert any(c["group"] == 16 and rows(c) >= 16 and c["Lk"] == 130 for c in cases)
    assert any(c["mask"] == "allmasked" for c in cases)
    assert len(cases) < 80
