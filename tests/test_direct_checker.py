"""The references of tests/direct_ref.py checked on their own, on the CPU: on every case the GPU tests run
(tests/test_gpu_direct_kernels.py) the stand-in of a correct kernel passes its check, and every planted defect fails on the
case that exists to catch it (*_CAUGHT_BY names it).  TorchBucketOps, the stand-in the host tests of the row-sparse exchange
plug in (tests/test_parallel_gloo.py), agrees bit for bit with the pack / scatter statement, so the host tests and the device
are held to ONE statement.  C_TANH is re-measured on every run."""
import json
import os

import numpy as np
import pytest
import torch

from tests import direct_ref as D

FORMS = ("bf16", "fp32")


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---------------------------------------------------------------------------------------------- embed
EMBED_CAUGHT_BY = {"no_bias": "r1", "bias_bf16": "r300", "zero_if_any_pad": "r5_pad0", "zero_per_row": "r5_pad0",
                   "pad_scan_256": "all_pad_but_last", "pad_rule_without_pad": "no_pad_all_equal"}


def _embed_kernel(x, form, defect=None):
    """What a kernel with the defect stores: the statement's sum rounded to fp32 (t and b are fp32 values: the float64 sum
    is exact, so this IS the fp32 add), then to the storage type."""
    return D.st(D.f32(D.embed_ref(defect=defect, **x)), form)


@pytest.mark.parametrize("form", FORMS)
def test_embed_standin_and_defects(form):
    cases = D.embed_cases(form)
    assert set(EMBED_CAUGHT_BY) == set(D.EMBED_DEFECTS)
    for name, x in cases.items():
        ref = D.embed_ref(**x)
        got = D.embed_standin(form=form, **x)
        assert not D.exceeds(got, ref, D.embed_bound(ref, form)), name
        assert D.same_bits(_embed_kernel(x, form), got, form), name           # (the defect-free path adds no artefact)
        assert (not ref.any()) == (name == "all_pad"), name
    assert (cases["r300"]["ids"][4:6] == (-3, D.EMBED_V + 5)).all()            # the clamped ids are in
    x = cases["r300"]
    assert _eq(D.embed_ref(**x)[4:6], x["table"][[0, D.EMBED_V - 1]] + x["bias"][None, :])
    for d, name in EMBED_CAUGHT_BY.items():
        x = cases[name]
        assert not D.same_bits(_embed_kernel(x, form, d), D.embed_standin(form=form, **x), form), "%s on case %s" % (d, name)


# ---------------------------------------------------------------------------------------------- bias_tanh
TANH_CAUGHT_BY = {"no_bias": (5, 72, 3, True), "rep_interleaved": (5, 72, 3, True), "f32_out_rounded": (5, 72, 3, True),
                  "tanh_naive": (5, 72, 3, True), "copy_from_x": (33, 300, 4, True)}


def _measure_c_tanh():
    need = 0.0
    for key, x in D.tanh_cases().items():
        ref = D.bias_tanh_ref(**x)
        need = max(need, D.tanh_need(D.bias_tanh_standin(form="fp32", **x)["out"], ref))
    return need


def test_c_tanh_is_remeasured_and_recorded():
    need = _measure_c_tanh()
    print("C_TANH: the torch-fp32 stand-in needs %.4f; the rule gives %.1f; recorded %.4f / %.1f"
          % (need, D.c_tanh_rule(need), D.C_TANH_MEASURED, D.C_TANH))
    assert np.isfinite(need) and D.c_tanh_rule(need) <= D.C_TANH and D.c_tanh_rule(D.C_TANH_MEASURED) == D.C_TANH
    with open(os.path.join(os.path.dirname(__file__), "..", "profiles", "elemkernel_parity_constants.json")) as f:
        rec = json.load(f)["direct_kernels"]
    assert rec["C_TANH"] == D.C_TANH and rec["c_tanh_measured_cpu"] == D.C_TANH_MEASURED
    assert D.c_tanh_rule(rec["c_tanh_needed_gpu"]) <= D.C_TANH     # (recorded beside it; it does not set the constant)


@pytest.mark.parametrize("form", FORMS)
def test_bias_tanh_standin_and_defects(form):
    cases = D.tanh_cases()
    assert set(TANH_CAUGHT_BY) == set(D.TANH_DEFECTS)
    for key, x in cases.items():
        ref = D.bias_tanh_ref(form=form, **x)
        got = D.bias_tanh_standin(form=form, **x)
        assert not D.exceeds(got["out"], ref["out"], D.tanh_bound(ref, form)), key
        assert not D.exceeds(got["copy"], ref["copy"], D.tanh_bound(ref, form, copy=True)), key
        big = np.abs(ref["z"]) >= 60
        assert big.sum() >= 2 * x["rep"] and (np.abs(got["out"][big]) == 1).all(), key          # saturated: exactly +-1
    for d, key in TANH_CAUGHT_BY.items():
        x = cases[key]
        ref, bad = D.bias_tanh_ref(form=form, **x), D.bias_tanh_ref(form=form, defect=d, **x)
        which = "copy" if d == "copy_from_x" else "out"
        assert D.exceeds(bad[which], ref[which], D.tanh_bound(ref, form, copy=which == "copy")), "%s on case %s" % (d, key)
    # tanh_naive: at |z| = 2^-12 it misses the RELATIVE term, at z = 60 it is not finite (TANH_SPECIALS 0 / 5 and 1).  With the
    # bias z = fl(2^-12 - b) + b is 2^-12 to an ulp, not the power of two: AT the power of two e^2z = 1 + 2^-11 + 2^-23 + ..
    # happens to be an fp32 number to 2^-35 and the naive form is right by luck (0.04 of the bound; 228 x at -2^-12 + ulp).
    x = cases[TANH_CAUGHT_BY["tanh_naive"]]
    ref, bad = D.bias_tanh_ref(**x), D.bias_tanh_ref(defect="tanh_naive", **x)
    small = np.abs(np.abs(ref["z"][0, :6]) * 2.0 ** 12 - 1) < 2.0 ** -20
    assert small[0] and small[5] and np.abs(ref["z"][0, 1] - 60.0) < 1e-5
    miss = np.abs(bad["out"] - ref["y"])[0, :6] > D.tanh_bound(ref, "fp32")[0, :6]
    assert np.isfinite(bad["out"][0, :6][small]).all() and (miss & small).any(), "tanh_naive at |z| = 2^-12"
    assert not np.isfinite(bad["out"][0, 1]), "tanh_naive at z = 60"


# ---------------------------------------------------------------------------------------------- aan_decode
AAN_CAUGHT_BY = {"cache_holds_mean": "time6_wrong_arg", "inv_from_argument": "time6_wrong_arg", "count_off_by_one": "time0",
                 "halves_swapped": "arg_only", "cache_bf16": "time0"}


def test_aan_decode_standin_and_defects():
    assert set(AAN_CAUGHT_BY) == set(D.AAN_DEFECTS)
    for rows, H in D.AAN_SHAPES:
        for name, (tdev, inv) in D.AAN_TIMES.items():
            cache = D.aan_inputs(rows, H)["cache"]
            for call in (0, 1):                                  # two chained calls: the second adds to the first's sum
                x = D.aan_inputs(rows, H, call)["x"]
                ref = D.aan_decode_ref(x, cache, inv, tdev)
                got = D.aan_decode_standin(x, cache, inv, tdev)
                b = D.aan_bound(ref)
                assert not D.exceeds(got["cache"], ref["cache"], b["cache"]), (rows, H, name, call)
                assert not D.exceeds(got["cat"], ref["cat"], b["cat"]), (rows, H, name, call)
                assert D.same_bits(got["cat"][:, :H], x, "bf16")
                cache = got["cache"]
    rows, H = D.AAN_SHAPES[1]
    for d, name in AAN_CAUGHT_BY.items():
        tdev, inv = D.AAN_TIMES[name]
        x = D.aan_inputs(rows, H)
        ref, bad = D.aan_decode_ref(x["x"], x["cache"], inv, tdev), D.aan_decode_ref(x["x"], x["cache"], inv, tdev, defect=d)
        b = D.aan_bound(ref)
        assert D.exceeds(bad["cache"], ref["cache"], b["cache"]) or D.exceeds(bad["cat"], ref["cat"], b["cat"]), \
            "%s on case %s" % (d, name)


# ---------------------------------------------------------------------------------------------- add_rows
ADD_ROWS_CAUGHT_BY = {"b_stride_from_out": ((5, 20), True), "cols_from_ld": ((1, 1), True)}


def test_add_rows_standin_and_defects():
    assert set(ADD_ROWS_CAUGHT_BY) == set(D.ADD_ROWS_DEFECTS)
    for rows, cols in D.ADD_ROWS_SHAPES:
        for in_place in (False, True):
            x = D.add_rows_case(rows, cols, in_place)
            assert len({x["lda"], x["ldb"], x["ldo"]}) == (2 if in_place else 3) and min(x["lda"], x["ldb"], x["ldo"]) > cols
            before = x["obuf"].copy()
            out = D.add_rows_flat(**x)
            win = D.window(out, rows, cols, x["ldo"], x["o0"] - D.LEAD)
            assert D.same_bits(win, D.add_rows_standin(x)), (rows, cols, in_place)
            D.window(out, rows, cols, x["ldo"], x["o0"] - D.LEAD)[:] = D.window(before, rows, cols, x["ldo"], x["o0"] - D.LEAD)
            assert _eq(out, before), "nothing outside the window is written"
    for d, ((rows, cols), in_place) in ADD_ROWS_CAUGHT_BY.items():
        x = D.add_rows_case(rows, cols, in_place)
        assert not _eq(D.add_rows_flat(defect=d, **x), D.add_rows_flat(**x)), "%s on case %s" % (d, (rows, cols, in_place))


# ---------------------------------------------------------------------------------------------- transpose
TRANSPOSE_CAUGHT_BY = {"copy": (5, 72, 80, 8), "tiles_not_swapped": (65, 130, 136, 72), "ld_swapped": (5, 72, 80, 8)}


def test_transpose_statement_and_defects():
    assert set(TRANSPOSE_CAUGHT_BY) == set(D.TRANSPOSE_DEFECTS)
    for shape in D.TRANSPOSE_SHAPES:
        rows, cols, ld_src, ld_dst = shape
        x = D.transpose_case(*shape)
        out = D.transpose_flat(**x)
        src = torch.as_tensor(D.window(x["src"], rows, cols, ld_src).copy())
        assert _eq(D.window(out, cols, rows, ld_dst), src.T.contiguous().numpy()), shape
        D.window(out, cols, rows, ld_dst)[:] = np.nan
        assert _eq(out, x["dst"]), "the padding columns keep their NaN, the guards their value"
    for d, shape in TRANSPOSE_CAUGHT_BY.items():
        x = D.transpose_case(*shape)
        assert not _eq(D.transpose_flat(defect=d, **x), D.transpose_flat(**x)), "%s on case %s" % (d, shape)
    # why the cases of more than one tile are there: inside one tile, a tile transposed where it stands is right
    x = D.transpose_case(64, 64, 64, 64)
    assert _eq(D.transpose_flat(defect="tiles_not_swapped", **x), D.transpose_flat(**x))


# ---------------------------------------------------------------------------------------------- rows pack / scatter
# defect -> (case, bf16 payload, clear_rows)
ROWS_CAUGHT_BY = {"stale_uid_packed": ("n3_of_4", False, 0), "ids_not_minus_one": ("n3_of_4", False, 1),
                  "no_clear": ("full_H260", False, 1), "clear_every_slot": ("n3_of_4", True, 1),
                  "no_poison": ("overflow", False, 1), "scatter_overwrites": ("n3_of_4", False, 1),
                  "scatter_ignores_vocab_rows": ("n3_of_4", False, 1), "bf16_halves_swapped": ("n3_of_4", True, 1),
                  "second_column_trip_dropped": ("full_H260", True, 1)}


def _pack_args(x, bf16, clear):
    return dict(table=x["table"], uid=x["uid"], n=x["n"], R=x["R"], H=x["H"], bf16=bf16, clear_rows=clear)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(D.ROWS_CASES))
def test_rows_standins_and_bucket_ops_match_the_statement(name, bf16):
    from tests.test_parallel_gloo import TorchBucketOps
    ops = TorchBucketOps()
    x = D.rows_case(name)
    R, H, V, n = x["R"], x["H"], x["V"], x["n"]
    assert D.payload_words(R, H, bf16) == ops.payload_words(R, H, bf16)
    for clear in (0, 1):
        words, table = D.rows_pack_ref(**_pack_args(x, bf16, clear))
        w2, t2 = D.rows_pack_standin(**_pack_args(x, bf16, clear))
        assert np.array_equal(words, w2) and np.array_equal(table.view(np.int32), t2.view(np.int32)), (name, clear)
        rows = D.payload_rows(words, R, H, bf16)
        nu = min(n, R)
        assert (words[nu:R] == -1).all() and not rows[nu:].any()
        touched = np.zeros(len(table), bool)
        touched[x["uid"][:nu]] = True
        assert _eq(table[~touched], x["table"][~touched]) and (not table[touched].any() if clear else _eq(table, x["table"]))
        if n > R:
            exact = D.payload_rows(D.rows_pack_ref(**_pack_args(dict(x, n=R), bf16, clear))[0], R, H, bf16)
            assert np.isnan(rows[0]).any() and _eq(rows[1:], exact[1:])
            after = D.rows_scatter_ref(np.ones_like(x["table"]), words, R, H, bf16, V)
            assert np.isnan(after[x["uid"][0]]).any() and np.isfinite(np.delete(after, x["uid"][0], 0)).all()
        elif clear:                                   # TorchBucketOps always clears and knows no overflow
            tt = torch.as_tensor(x["table"].copy())
            out = torch.zeros(D.payload_words(R, H, bf16), dtype=torch.int32)
            ops.rows_pack(tt, torch.as_tensor(x["uid"]), torch.tensor([n], dtype=torch.int32), out, R, H, bf16)
            assert np.array_equal(out.numpy(), words) and np.array_equal(tt.numpy().view(np.int32), table.view(np.int32)), name
    s = D.scatter_case(name, bf16)
    ref = D.rows_scatter_ref(s["table"], s["words"], R, H, bf16, V)
    assert np.array_equal(ref.view(np.int32), D.rows_scatter_standin(s["table"], s["words"], R, H, bf16, V).view(np.int32))
    tt = torch.as_tensor(s["table"].copy())
    ops.rows_scatter_add(tt, torch.as_tensor(s["words"]), R, H, bf16, V)
    assert np.array_equal(tt.numpy().view(np.int32), ref.view(np.int32)), name
    assert _eq(ref[V:], s["table"][V:]) and set(s["words"][:R].tolist()) >= {-1, V, V + 3}


def test_rows_defects():
    assert set(ROWS_CAUGHT_BY) == set(D.ROWS_DEFECTS)
    for d, (name, bf16, clear) in ROWS_CAUGHT_BY.items():
        x, s = D.rows_case(name), D.scatter_case(name, bf16)
        R, H, V = x["R"], x["H"], x["V"]
        what = "%s on case %s (%s payload, clear_rows = %d)" % (d, name, "bf16" if bf16 else "fp32", clear)
        caught = False
        if d in D.PACK_ONLY or d == "second_column_trip_dropped":
            good, bad = D.rows_pack_ref(**_pack_args(x, bf16, clear)), D.rows_pack_ref(defect=d, **_pack_args(x, bf16, clear))
            if d == "no_poison":
                caught = not np.isnan(D.payload_rows(bad[0], R, H, bf16)[0]).any()
            else:
                caught = not (np.array_equal(good[0], bad[0]) and _eq(good[1], bad[1]))
            if d == "second_column_trip_dropped":     # the pack AND the scatter must each show it
                assert caught, what + ": pack"
                caught = False
        if d not in D.PACK_ONLY:
            caught = not _eq(D.rows_scatter_ref(s["table"], s["words"], R, H, bf16, V),
                             D.rows_scatter_ref(s["table"], s["words"], R, H, bf16, V, defect=d))
        assert caught, what


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_rows_two_rank_round_trip(bf16):
    """Two dense tables with overlapping row sets, each packed with clear, both payloads scattered into both tables in rank
    order: the tables are bit-identical to each other and to the sum of the (once rounded) rows in rank order."""
    t, uid, R, H, V = D.two_rank_inputs()
    words, tabs = zip(*(D.rows_pack_standin(t[k], uid[k], len(uid[k]), R, H, bf16, 1) for k in (0, 1)))
    expect = D.two_rank_expect(t, bf16)
    for k in (0, 1):
        tab = tabs[k]
        for w in words:
            tab = D.rows_scatter_standin(tab, w, R, H, bf16, V)
        assert np.array_equal(tab.view(np.int32), expect.view(np.int32)), k


# ---------------------------------------------------------------------------------------------- seed
def test_seed_statement():
    assert D.seed_advance_ref(5, 0) == 5 and D.seed_advance_ref(2 ** 32 - 1, 1) == 2 ** 32
    assert D.seed_advance_ref(2 ** 64 - 1, 2) == 1
