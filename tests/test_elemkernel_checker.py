"""The element-kernel references and bounds of tests/parity_elem.py have teeth (CPU only).  Over the case lists of
tests/test_gpu_elemkernels_elementwise.py:

  * a correct stand-in (parity_elem.*_standin: the kernel's arithmetic in fp32, bf16 at the storage sites, torch's
    summation order) passes every case with nothing excused; the worst |err| / bound is printed and is below 1;
  * each planted defect fails at every case it applies to (at least five each), and the checker's message names an
    output and a position inside the defect.
"""
import pytest
import torch

from tests import parity as P
from tests import parity_elem as PE
from tests.test_rowkernel_checker import _fails, _report
from tests.test_gpu_elemkernels_elementwise import (
    EMB_FWD_CASES, EMB_PAIR_CASES, embed_inputs, cpu_timing, cpu_mask, EMB_BWD_V, EMB_BWD_CASES, embed_bwd_inputs,
    EMB_ATOMIC_CASES, EMB_ATOMIC_V, EMB_ATOMIC_B, EMB_ATOMIC_L, SCAN_CASES, SCAN_B, SCAN_EXACT, scan_inputs,
    scan_bwd_case, aan_bwd_operands, GATE_CASES, GATE_ROW, gate_inputs, ADAM_SIZES, ADAM_CLIP_CASES, ADAM_DEFAULT, HYPER,
    adam_inputs)

F32 = torch.float32


def _merge(worst, new):
    for k, v in new.items():
        worst[k] = max(worst.get(k, 0.0), v)


def _cases(cases, applies, least=5):
    out = [c for c in cases if applies(c)]
    assert len(out) >= least, len(out)
    return out


# ---------------------------------------------------------------------------------------------- embedding forward
def _emb_fwd(case, defect=None):
    H, B, L, (pos0, _) = case["H"], case["B"], case["L"], case["pos"]
    inp = embed_inputs(H, B, L)
    a = (inp["ids"], inp["table"], inp["bias"], cpu_timing(H), PE.embed_scale(H), case["shift"], pos0, bool(case["zf"]),
         cpu_mask(B * L, H, case["drop"]))
    return PE.embed_fwd_standin(*a, defect=defect), PE.embed_fwd_bound(*a)


def test_embed_fwd_standin_passes_everywhere():
    assert {c["H"] for c in EMB_FWD_CASES} == {8, 64, 504, 512, 520, 1024} and any(c["B"] * c["L"] == 8200 for c in EMB_FWD_CASES)
    worst = {}
    for case in EMB_FWD_CASES:
        got, bounds = _emb_fwd(case)
        _merge(worst, P.check_all(got, bounds, "stand-in %s" % case))
    for H, La, Lb, drop in EMB_PAIR_CASES:                       # the pair: side b is shifted, each side has its own mask
        for L, shift, seed in ((La, 0, 1), (Lb, 1, 2)):
            inp = embed_inputs(H, 3, L, seed=seed)
            a = (inp["ids"], inp["table"], inp["bias"], cpu_timing(H), PE.embed_scale(H), shift, 0, False,
                 cpu_mask(3 * L, H, drop, seed))
            _merge(worst, P.check_all(PE.embed_fwd_standin(*a), PE.embed_fwd_bound(*a), "stand-in pair"))
    _report("embedding forward stand-in", worst)


_T0 = lambda c: set(range(0, c["B"] * c["L"], c["L"]))                       # the rows with t = 0
_ALLROWS = lambda c: set(range(c["B"] * c["L"]))
EMB_FWD_DEFECTS = {            # defect -> (the cases, the rows the message may name)
    "bias_scaled": (lambda c: not c["zf"], lambda c: _ALLROWS(c) - (_T0(c) if c["shift"] else set())),
    "shift_reads_r": (lambda c: c["shift"] and not c["zf"], lambda c: _ALLROWS(c) - _T0(c)),
    "bias_on_empty": (lambda c: c["shift"] or c["zf"], lambda c: _ALLROWS(c) if c["zf"] else _T0(c)),
    "pos0_ignored": (lambda c: c["pos"][0] == 4, _ALLROWS),
    "drop_no_row": (lambda c: c["drop"] > 0, lambda c: _ALLROWS(c) - {0}),
}


@pytest.mark.parametrize("defect", list(EMB_FWD_DEFECTS))
def test_each_planted_embed_fwd_defect_fails(defect):
    applies, rows = EMB_FWD_DEFECTS[defect]
    cases = _cases(EMB_FWD_CASES, applies)
    for case in cases:
        got, bounds = _emb_fwd(case, defect)
        _fails(lambda: P.check_all(got, bounds, "%s %s" % (defect, case)), ("out",), rows(case))
    print("embedding forward defect %s: fails at each of its %d cases" % (defect, len(cases)))


# ---------------------------------------------------------------------------------------------- embedding backward
def _emb_bwd(case, defect=None):
    H, shift, kind = case["H"], case["shift"], case["kind"]
    inp = embed_bwd_inputs(H, shift, kind)
    a = (inp["ids"], inp["dout"], EMB_BWD_V, PE.embed_scale(H), shift, cpu_mask(inp["ids"].numel(), H, case["drop"]),
         inp["prev"], case["acc"])
    bounds = PE.embed_bwd_bound(*a)
    return PE.embed_bwd_standin(*a, defect=defect), bounds, (tuple(bounds) if kind == "exact" else ())


def test_embed_bwd_standin_passes_everywhere():
    worst = {}
    for case in EMB_BWD_CASES:
        got, bounds, exact = _emb_bwd(case)
        _merge(worst, P.check_all(got, bounds, "stand-in %s" % case, exact=exact))
    for H, shift, drop in EMB_ATOMIC_CASES:                      # the atomic form: always added to, with dbias
        inp = embed_inputs(H, EMB_ATOMIC_B, EMB_ATOMIC_L, EMB_ATOMIC_V, seed=3)
        prev, pb = torch.full((EMB_ATOMIC_V, H), 0.75), torch.linspace(-1, 1, H)
        a = (inp["ids"], inp["dout"], EMB_ATOMIC_V, PE.embed_scale(H), shift,
             cpu_mask(EMB_ATOMIC_B * EMB_ATOMIC_L, H, drop), prev, 1, pb)
        _merge(worst, P.check_all(PE.embed_bwd_standin(*a), PE.embed_bwd_bound(*a), "stand-in atomic"))
    _report("embedding backward stand-in", worst)


EMB_BWD_DEFECTS = {            # defect -> (the cases, the table rows (ids) the message may name; None: any)
    "drop_ignored": (lambda c: c["drop"] > 0, None),
    "no_scale": (lambda c: True, None),
    "past64": (lambda c: True, {7, 8}),                          # the runs of 65 and 150 rows
    "acc_ignored": (lambda c: c["acc"], None),
}


@pytest.mark.parametrize("defect", list(EMB_BWD_DEFECTS))
def test_each_planted_embed_bwd_defect_fails(defect):
    applies, rows = EMB_BWD_DEFECTS[defect]
    cases = _cases(EMB_BWD_CASES, applies)
    for case in cases:
        got, bounds, exact = _emb_bwd(case, defect)
        _fails(lambda: P.check_all(got, bounds, "%s %s" % (defect, case), exact=exact), ("dtable",), rows)
    print("embedding backward defect %s: fails at each of its %d cases" % (defect, len(cases)))


def test_a_written_row_of_an_absent_id_fails():
    case = EMB_BWD_CASES[0]
    got, bounds, exact = _emb_bwd(case)
    got["dtable"][0, 3] = 0.0                                     # id 0 is absent: the sentinel must stay
    _fails(lambda: P.check_all(got, bounds, "absent %s" % case, exact=exact), ("dtable",), {0}, {3})


# ---------------------------------------------------------------------------------------------- scan forward
SCAN_FORMS = [(L, H, um, att) for (L, H) in SCAN_CASES for um, att in ((0, 0), (1, 0), (1, 1))]      # att: k_cumavg_add_fwd


def _scan_fwd(form, defect=None, kind="random"):
    L, H, um, att = form
    inp, mask = scan_inputs(L, H, kind), PE.scan_masks(L)
    a = (inp["x"], mask, um, inp["att"] if att else None)
    ref, bound = PE.scan_fwd_bound(*a, exact=kind == "exact")
    return {"avg": PE.scan_fwd_standin(*a, defect=defect)}, {"avg": (ref, bound)}, mask


def test_scan_fwd_standin_passes_everywhere():
    assert {L for L, _ in SCAN_CASES} == {1, 2, 3, 4, 5, 7, 8, 9, 64, 130}
    worst = {}
    for form in SCAN_FORMS:
        got, bounds, _ = _scan_fwd(form)
        _merge(worst, P.check_all(got, bounds, "stand-in %s" % (form,)))
    for um, att in ((0, 0), (1, 0), (1, 1)):
        got, bounds, _ = _scan_fwd(SCAN_EXACT + (um, att), kind="exact")
        _merge(worst, P.check_all(got, bounds, "stand-in exact"))
    _report("scan forward stand-in", worst)


def _rows_cnt0(form, mask):
    """The token rows whose count of live steps is still 0."""
    return set(torch.nonzero(mask.cumsum(1).reshape(-1) == 0).reshape(-1).tolist())


def _rows_segment(form, mask):
    """The token rows of the steps of the segment whose carry is dropped."""
    t0, t1 = PE.scan_segment(form[0])
    return {b * form[0] + t for b in range(SCAN_B) for t in range(t0, t1)}


_rows_of = lambda *sentences: (lambda form, mask: {b * form[0] + t for b in sentences for t in range(form[0])})
SCAN_FWD_DEFECTS = {           # defect -> (the forms, the rows(form, mask), the columns(form) the message may name)
    "carry_dropped": (lambda f: f[0] >= 2, _rows_segment, None),
    "exclusive": (lambda f: True, None, None),
    "cnt_counts_masked": (lambda f: f[0] >= 2, _rows_of(1, 2, 3), None),          # (the full sentence has nothing masked)
    "den_unclamped": (lambda f: True, _rows_cnt0, None),
    "u1_under_mask": (lambda f: f[2] == 1 and f[0] >= 2, _rows_of(2), None),      # (the hole: a masked step before a live one)
    "last8": (lambda f: True, None, lambda f: range(f[1] - 8, f[1])),
}


@pytest.mark.parametrize("defect", list(SCAN_FWD_DEFECTS))
def test_each_planted_scan_fwd_defect_fails(defect):
    applies, rows, cols = SCAN_FWD_DEFECTS[defect]
    forms = _cases(SCAN_FORMS, applies)
    for form in forms:
        got, bounds, mask = _scan_fwd(form, defect)
        _fails(lambda: P.check_all(got, bounds, "%s %s" % (defect, form)), ("avg",), rows and rows(form, mask), cols and cols(form))
    if defect != "u1_under_mask":                                 # the integers (the hole's steps are what u = 1 would add)
        got, bounds, _ = _scan_fwd(SCAN_EXACT + (1, 0), defect, kind="exact")
        _fails(lambda: P.check_all(got, bounds, "%s exact" % defect), ("avg",))
    print("scan forward defect %s: fails at each of its %d forms" % (defect, len(forms)))


# ---------------------------------------------------------------------------------------------- scan backward
SCAN_BWD_FORMS = [(L, H, fl) for (L, H) in SCAN_CASES for fl in (0, 1, 2, 3, None)]        # None: k_cumavg_bwd


def _scan_bwd(form, defect=None, kind="random"):
    L, H, flags = form
    inp, mask = scan_bwd_case(L, H, kind, 1 if flags is None else flags & 1)
    ex = kind == "exact"
    if flags is None:
        ref, bound = PE.scan_bwd_bound(inp["x"], inp["x"].double().abs(), mask, 1, exact=ex)
        return {"dx": PE.scan_bwd_standin(inp["x"], mask, 1, defect=defect)}, {"dx": (ref, bound)}
    dcat = aan_bwd_operands(inp, H, flags)
    extra = (inp["ds"], inp["dxg"], dcat[:, :H])
    g, gmag = PE.aan_bwd_g(inp["dyg"], dcat, H, flags)
    ref, bound = PE.scan_bwd_bound(g, gmag, mask, flags & 1, extra=extra, exact=ex)
    dc2 = defect if defect in ("dc2_added", "dc2_dropped") else None
    gs, _ = PE.aan_bwd_g(inp["dyg"], dcat, H, flags, F32, dc2)
    return {"dx": PE.scan_bwd_standin(gs, mask, flags & 1, extra, None if dc2 else defect)}, {"dx": (ref, bound)}


def test_scan_bwd_standin_passes_everywhere():
    worst = {}
    for form in SCAN_BWD_FORMS:
        got, bounds = _scan_bwd(form)
        _merge(worst, P.check_all(got, bounds, "stand-in %s" % (form,)))
    for fl in (0, 1, 2, 3, None):
        got, bounds = _scan_bwd(SCAN_EXACT + (fl,), kind="exact")
        _merge(worst, P.check_all(got, bounds, "stand-in exact"))
    _report("scan backward stand-in", worst)


SCAN_BWD_DEFECTS = {
    "cnt_early": lambda f: f[0] >= 2,
    "carry_wrong_side": lambda f: f[0] >= 2,
    "dc2_added": lambda f: f[2] in (2, 3),
    "dc2_dropped": lambda f: f[2] in (0, 1),
}


@pytest.mark.parametrize("defect", list(SCAN_BWD_DEFECTS))
def test_each_planted_scan_bwd_defect_fails(defect):
    forms = _cases(SCAN_BWD_FORMS, SCAN_BWD_DEFECTS[defect])
    for form in forms:
        got, bounds = _scan_bwd(form, defect)
        _fails(lambda: P.check_all(got, bounds, "%s %s" % (defect, form)), ("dx",))
    if defect == "carry_wrong_side":                              # the integers: every step of every segment counts
        for fl in (0, 1, 2, 3, None):
            got, bounds = _scan_bwd(SCAN_EXACT + (fl,), defect, kind="exact")
            _fails(lambda: P.check_all(got, bounds, "%s exact" % defect), ("dx",))
    print("scan backward defect %s: fails at each of its %d forms" % (defect, len(forms)))


# ---------------------------------------------------------------------------------------------- gate
GATE_FORMS = [(rows, H, seed) for rows, H in GATE_CASES for seed in (0, 1)]


def _gate(form, defect=None):
    rows, H, seed = form
    inp = gate_inputs(rows, H)
    if seed:
        inp["cat"], inp["dg"] = inp["cat"].flip(0), inp["dg"].flip(1)          # other operands beside the same z
    t = PE.gate_terms(inp["z"], inp["cat"], inp["dg"])
    return PE.gate_standin(inp["z"], inp["cat"], inp["dg"], defect), t


def test_gate_standin_passes_everywhere_and_is_finite_at_the_saturated_z():
    worst, need = {}, 0.0
    for form in GATE_FORMS:
        got, t = _gate(form)
        _merge(worst, P.check_all(got, PE.gate_bound(t), "stand-in %s" % (form,)))
        need = max([need] + list(PE.gate_c_needed(t, got).values()))
        assert all(bool(torch.isfinite(v.float()[GATE_ROW]).all()) for v in got.values())
    print("gate stand-in (torch's exp, not the GPU's): c needed %.3g, C_GATE %g" % (need, PE.C_GATE))
    _report("gate stand-in", worst)


def test_a_floor_of_one_denormal_step_cannot_hold_at_z_minus_90():
    """Why gate_terms' floor is 2^-126 times the multiplying magnitude: with 2^-149 alone the CORRECT fp32 evaluation is
    outside the bound at z = -90, where sigmoid = 8.2e-40 and 1 / (1 + e^90) is 0 in fp32."""
    got, t = _gate(GATE_FORMS[2])
    tiny = {k: (ref, shape, torch.full_like(ref, 2.0 ** -149)) for k, (ref, shape, _) in t.items()}
    _fails(lambda: P.check_all(got, PE.gate_bound(tiny), "denormal-step floor"), ("dz", "dxg", "dyg", "out"), {GATE_ROW})


GATE_DEFECTS = {"swapped": ("out", "dz", "dxg", "dyg"), "no_1ms": ("dz",)}


@pytest.mark.parametrize("defect", list(GATE_DEFECTS))
def test_each_planted_gate_defect_fails(defect):
    for form in _cases(GATE_FORMS, lambda f: True):
        got, t = _gate(form, defect)
        _fails(lambda: P.check_all(got, PE.gate_bound(t), "%s %s" % (defect, form)), GATE_DEFECTS[defect])
    print("gate defect %s: fails at each of its %d forms with C_GATE = %g" % (defect, len(GATE_FORMS), PE.C_GATE))


# ---------------------------------------------------------------------------------------------- optimiser
def _adam(n, key10, defect=None, norm_free=1, hyper=HYPER, gnorm=None, seed=0):
    """The stand-in's outputs against every bound the GPU test applies (p staged on the stand-in's own m and v)."""
    inp = adam_inputs(n, seed)
    hy = torch.tensor(hyper, dtype=F32)
    got = PE.adam_standin(inp["p"], inp["g"], inp["m"], inp["v"], hy, norm_free, gnorm, defect)
    bounds = PE.adam_bound(inp["p"], inp["g"], inp["m"], inp["v"], hy, norm_free, gnorm, got["m"], got["v"])
    grid = PE.adam_grid(n, key10)
    T = PE.adam_terms_per_thread(n, grid, ADAM_DEFAULT[9] != 0)
    bounds["pnorm"] = PE.norm_bound(inp["p"], 1.0, T, grid)
    if norm_free:
        bounds["gnorm"] = PE.norm_bound(inp["g"], hyper[4], T, grid)
    bounds["shadow"] = (got["p"].to(torch.bfloat16).double(), torch.zeros(n, dtype=torch.float64))
    got = dict(got, shadow=got["shadow"].float())
    return got, bounds


def test_adam_standin_passes_everywhere():
    worst = {}
    for n, key10 in ADAM_SIZES:
        got, bounds = _adam(n, key10)
        _merge(worst, P.check_all(got, bounds, "stand-in n=%d" % n, exact=("shadow",)))
    for n, api, clip in ADAM_CLIP_CASES:
        inp = adam_inputs(n, seed=1)
        gn = PE.f32(HYPER[4] * float(inp["g"].double().norm()))
        hyper = list(HYPER)
        hyper[5] = {"off": 0.0, "on": 0.5 * gn, "slack": 2.0 * gn}[clip]
        got, bounds = _adam(n, 0, None, 0, hyper, gn, seed=1)
        _merge(worst, P.check_all(got, bounds, "stand-in n=%d clip %s" % (n, clip), exact=("shadow",)))
    _report("Adam stand-in", worst)


_TAIL = lambda n: range(n - n % 4, n)
ADAM_DEFECTS = {               # defect -> (the sizes, the outputs, the elements(n) the message may name)
    "eps_inside": (lambda n: True, ("p",), None),
    "v_unscaled": (lambda n: True, ("v",), None),
    "no_1mb1": (lambda n: True, ("m",), None),
    "shadow_old": (lambda n: True, ("shadow",), None),
    "tail_skipped": (lambda n: n % 4 != 0, ("m", "v", "p"), _TAIL),
    "pnorm_after": (lambda n: True, ("pnorm",), None),
    "clip_on_normfree": (lambda n: True, ("m", "v"), None),
}


@pytest.mark.parametrize("defect", list(ADAM_DEFECTS))
def test_each_planted_adam_defect_fails(defect):
    applies, names, cols = ADAM_DEFECTS[defect]
    sizes = _cases(ADAM_SIZES, lambda c: applies(c[0]))
    for n, key10 in sizes:
        got, bounds = _adam(n, key10, defect)
        _fails(lambda: P.check_all(got, bounds, "%s n=%d" % (defect, n), exact=("shadow",)), names, {0}, cols and cols(n),
               index_is_col=())
    print("Adam defect %s: fails at each of its %d sizes" % (defect, len(sizes)))


def test_small_kernel_bounds_hold_for_the_fp32_evaluation():
    e, p = torch.randn(4003, generator=torch.Generator().manual_seed(1)), torch.randn(4003, generator=torch.Generator().manual_seed(2))
    d = PE.f32(0.999)
    one = torch.tensor(1.0)
    worst = P.check_all({"ema": e - (one - d) * (e - p)}, {"ema": PE.ema_bound(e, p, d)}, "ema stand-in")
    a, b = PE.f32(0.75), PE.f32(-1.3)
    worst.update(P.check_all({"y": b * e + a * p}, {"y": PE.axpby_bound(e, p, a, b)}, "axpby stand-in"))
    _report("ema / axpby stand-in", worst)
    _fails(lambda: P.check_all({"ema": e - (one - d) * (p - e)}, {"ema": PE.ema_bound(e, p, d)}, "ema sign"), ("ema",), index_is_col=())
