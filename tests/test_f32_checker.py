"""The checks of tests/test_gpu_f32_kernels_elementwise.py, shown on the CPU (tests/f32_ref.py): what a correct fp32 kernel
computes passes every case of every table, and every planted defect fails on the case named for it -- so that a pass on the
device says something.  Also: the GEMM table reaches all 17 instantiations of zk_f32_gemm through ``route``, the integer GEMM
data is exact in float64, and the data has the properties the cases rely on (ReLU inputs with negative values, holed masks with
a live key, relative positions clipped on both sides)."""
import numpy as np
import pytest

from tests import f32_ref as R


# ---------------------------------------------------------------------------------------------- GEMM
def test_gemm_table_reaches_all_17_instantiations():
    seen = {}
    for name, (M, N, K, tb) in R.GEMM_CASES.items():
        for lay in R.GEMM_LAYOUTS:
            L = R.gemm_layout(M, N, K, tb, lay)
            assert K % 4 == 0 and L["lda"] % 4 == 0 and L["offa"] % 4 == 0 and (not tb or (L["ldb"] % 4 == 0 and L["offb"] % 4 == 0))
            kernel, TB, KS, per = R.route(M, N, K, tb, L["ldb"])
            assert R.route(M, N, K, tb, R.gemm_layout(M, N, K, tb, "tight")["ldb"])[:3] == (kernel, TB, KS), "layouts part"
            seen.setdefault((kernel, TB, KS), []).append(name)
    assert set(seen) == set(R.GEMM_FORMS), set(R.GEMM_FORMS) ^ set(seen)
    r = lambda n: R.route(*R.GEMM_CASES[n], R.GEMM_CASES[n][2])
    # the properties the table's names promise
    assert r("t16k4_emptywave_tb1")[2:] == (4, 32) and 3 * 32 >= 68 and 68 % 16 == 4            # empty last wave, 4-wide k tail
    assert r("plain4_K2052_tb0")[2:] == (4, 528)
    assert r("ks16_refill_tb0")[2:] == (16, 80)                                                 # five chunks: the refill round
    assert (35 * 66) > 2048 and (35 * 66) % 4 != 0                                              # 1100 x 2100: dead tiles
    assert r("tblds_fallthrough_tb1")[0] != "tb_lds" and r("tblds_tb1")[0] == "tb_lds"


@pytest.mark.parametrize("name", list(R.GEMM_CASES))
def test_gemm_standin_passes_and_integers_are_exact(name):
    M, N, K, tb = R.GEMM_CASES[name]
    xi = R.gemm_inputs(name, "int")
    a, b = xi["a"].astype(np.float64), (xi["b"].T if tb else xi["b"]).astype(np.float64)
    assert float((np.abs(a) @ np.abs(b)).max()) + 4 < 2 ** 24, "a partial sum could leave the exact integers"
    for data in R.GEMM_DATA:
        x = R.gemm_inputs(name, data)
        pre, _ = R.gemm_ref(name, x, 1, 0)
        assert (pre < 0).mean() >= 0.25, "too few negative values in front of the ReLU"
        for lay, bias, act in (("strided", 1, 1), ("tight", 0, 0)):
            ref, bound = R.gemm_ref(name, x, bias, act)
            R.gemm_check_flat(R.gemm_standin(name, x, lay, bias, act), name, lay, ref, bound, data, name)


@pytest.mark.parametrize("defect", list(R.GEMM_DEFECTS))
def test_gemm_defect_fails_on_its_case(defect):
    name, lay, bias, act, data = R.GEMM_DEFECTS[defect]
    x = R.gemm_inputs(name, data)
    ref, bound = R.gemm_ref(name, x, bias, act)
    R.gemm_check_flat(R.gemm_standin(name, x, lay, bias, act), name, lay, ref, bound, data)
    assert R.fails(R.gemm_check_flat, R.gemm_standin(name, x, lay, bias, act, defect=defect), name, lay, ref, bound, data)


# ---------------------------------------------------------------------------------------------- LayerNorm family
def test_ln_standin_passes_every_case():
    worst = 0.0
    for name in R.ln_case_names():
        cs = R.ln_case(name)
        x = R.ln_inputs(cs)
        worst = max(worst, R.ln_check(cs, x, R.ln_standin(cs, x)))
    print("ln: largest |err| / bound of the stand-in %.3f" % worst)


def _rounded(r):
    return {k: v.astype(np.float32) for k, v in r.items() if k in ("out", "cache", "cat")}


@pytest.mark.parametrize("defect", list(R.LN_DEFECTS))
def test_ln_defect_fails_on_its_case(defect):
    cs = R.ln_case(R.LN_DEFECTS[defect])
    assert cs["name"] in R.ln_case_names()
    x = R.ln_inputs(cs)
    R.ln_check(cs, x, R.ln_standin(cs, x))
    assert R.fails(R.ln_check, cs, x, _rounded(R.ln_f64(cs, x, defect=defect)))


# ---------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("name", list(R.EMBED_CASES))
def test_embed_standin_passes(name):
    x = R.embed_inputs(name)
    R.embed_check(name, x, R.embed_standin(name, x))
    cs, r = R.EMBED_CASES[name], R.embed_f64(name, x)
    ids = x["ids"]
    assert {"all_pad": (ids == R.EMB_PAD).all(), "no_pad": (ids != R.EMB_PAD).all(),
            "one_live": (ids != R.EMB_PAD).sum() == 1, "some_pad": 0 < (ids == R.EMB_PAD).sum() < len(ids)}[cs["ids"]]
    if cs["ids"] == "one_live" and cs["rows"] > 64:
        assert (ids[:64] == R.EMB_PAD).all()               # the live id sits in the second trip of the pad scan
    if "clip" in name:
        assert cs["pos"][1] + (cs["rows"] - 1) % cs["L"] > R.EMB_TIMING_ROWS - 1
    assert bool(r["zero"].all()) == (name in ("embed_flag1", "embed_flag1_host_pos", "step_H620_131_allpad", "step_H68_1_allpad",
                                              "step_aan_H620_131_allpad"))


@pytest.mark.parametrize("defect", list(R.EMBED_DEFECTS))
def test_embed_defect_fails_on_its_case(defect):
    name = R.EMBED_DEFECTS[defect]
    x = R.embed_inputs(name)
    got = {"out": R.embed_f64(name, x, defect=defect)["out"].astype(np.float32)}
    if R.EMBED_CASES[name]["aan"]:
        got["cache"], got["cat"] = R.aan_tail(got["out"], x["cache0"], R.EMBED_CASES[name]["pos"][1])
    assert R.fails(R.embed_check, name, x, got)


# ---------------------------------------------------------------------------------------------- aan_step / gate
def _aan_check(name, x, got):
    cache, cat = R.aan_np(name, x, R.LN_TIME)
    R.assert_bits(got[0], cache, "cache")
    R.assert_bits(got[1], cat, "cat")


def _gate_check(name, x, got):
    ref, bound = R.gate_f64(name, x)
    return R.assert_within(got, ref, bound, "gate " + name)


@pytest.mark.parametrize("name", list(R.ROW_SHAPES))
def test_row_standins_pass(name):
    x = R.row_inputs(name)
    _aan_check(name, x, R.aan_np(name, x, R.LN_TIME))
    print("gate %s: stand-in |err| / bound %.3f" % (name, _gate_check(name, x, R.gate_standin(name, x))))
    z = x["z"]
    assert (z == 30).any() and (z == -30).any() and (np.abs(z) < 3).any()


@pytest.mark.parametrize("kernel,defect", [("aan", d) for d in R.AAN_DEFECTS] + [("gate", d) for d in R.GATE_DEFECTS])
def test_row_defect_fails_on_its_case(kernel, defect):
    name = (R.AAN_DEFECTS if kernel == "aan" else R.GATE_DEFECTS)[defect]
    x = R.row_inputs(name)
    if kernel == "aan":
        assert R.fails(_aan_check, name, x, R.aan_np(name, x, R.LN_TIME, defect=defect))
    else:
        assert R.fails(_gate_check, name, x, R.gate_f64(name, x, defect=defect)[0].astype(np.float32))


# ---------------------------------------------------------------------------------------------- attention
def _attn_check(name, x, got):
    ref, bound = R.attn_bound(name, x)
    return R.assert_within(got, ref, bound, "attn " + name)


@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_attn_standin_passes(name):
    cs, x = R.ATTN_CASES[name], R.attn_inputs(name)
    print("attn %s: stand-in |err| / bound %.3f" % (name, _attn_check(name, x, R.attn_standin(name, x))))
    if cs["mask"]:
        live = x["kmask"].sum(1) > 0
        assert all(bool(live[b]) != (b == cs["dead"]) for b in range(len(live))), "a sentence that is not meant to be dead is"
        assert (x["kmask"] == 0).any()
        if cs["dead"] is not None:                         # the dead sentence is uniform over its keys
            p = R.attn_f64(name, x)["p"][cs["dead"] * cs["group"]]
            assert np.allclose(p, 1.0 / cs["Lk"], rtol=0, atol=1e-15)
    if cs["rpr"] and cs["nkeys"] is None:                  # (the cached decode form has keys behind the query only)
        rel = cs["q_pos"][1] + np.arange(cs["Lq"])[:, None] - np.arange(cs["Lk"] if cs["nkeys"] is None else cs["nkeys"] + 1)[None]
        assert rel.max() > cs["rpr"] and rel.min() < -cs["rpr"], "nothing is clipped on one side"


@pytest.mark.parametrize("defect", list(R.ATTN_DEFECTS))
def test_attn_defect_fails_on_its_case(defect):
    name = R.ATTN_DEFECTS[defect]
    x = R.attn_inputs(name)
    _attn_check(name, x, R.attn_standin(name, x))
    assert R.fails(_attn_check, name, x, R.attn_f64(name, x, defect=defect)["out"].astype(np.float32))


def test_attn_lds_limit():
    cs = R.ATTN_CASES["lds_limit"]
    assert R.attn_lds_bytes(cs["Lk"], cs["d"]) == 64 * 1024 < R.attn_lds_bytes(cs["Lk"] + 1, cs["d"])
