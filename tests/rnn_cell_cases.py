"""The dense recurrent cell launches of zero_amd/csrc/zk_rnn.hip -- the ATR step, the two GRU launches and a deepnmt layer's
ff + residual, bf16 and fp32 forms -- on parity.guarded buffers: the input generators and run helpers of
tests/test_gpu_rnnsearch_kernels.py, test_gpu_deepatt_kernels.py and test_gpu_deepnmt_kernels.py, and the table of cases
whose output BYTES tests/golden/make_rnn_cell_golden.py pins and tests/test_gpu_rnn_cells_image.py recomputes.

Inputs come from CPU generators with fixed seeds.  Every operand and output is a guarded buffer: outputs are prefilled with
NaN, nothing outside their windows may change, inputs must be bit-identical after the call; every row stride is larger than
the row.  The *_call functions return the guarded outputs, the *_run functions their values as float64 arrays."""
import functools
import hashlib
import json
import os

import numpy as np
import torch

from tests import deepnmt_ref as DN
from tests import parity as P
from tests.util_gpu import eng

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rnn_cells_parent.json")
BF, F32 = torch.bfloat16, torch.float32
ST = {"bf16": BF, "fp32": F32}


def G(rows, cols, ld=None, off=0, dtype=BF, prefill=None):
    return P.guarded(rows, cols, ld, off, dtype, prefill, "cuda")


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def _values(bufs):
    return {k: b.value().double().numpy() for k, b in bufs.items()}


# ---------------------------------------------------------------------------------------------- the ATR step
def atr_inputs(Rn, H, form, seed, n_prev, u_zero=False):
    """float64 arrays whose values are exactly representable where the kernel reads them: U and p in the storage type, the
    state and the bias in fp32."""
    g = np.random.default_rng(100 + seed)
    st = lambda a: _t(a).float().to(ST[form]).double().numpy()
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    x = dict(h_prev=f32(g.normal(0, 1, (n_prev, H))), U=st(g.normal(0, H ** -0.5, (H, H))), b=f32(g.normal(0, 0.3, H)),
             p=st(g.normal(0, 1, (Rn, H))), mask=(np.arange(Rn) % 3 != 1).astype(np.float64),
             idx=g.integers(0, n_prev, Rn))
    x["idx"][:3] = (n_prev - 1, n_prev - 1, 0)         # repeated rows
    if u_zero:
        x["U"] = np.zeros((H, H))
        x["h_prev"] = f32(x["h_prev"] * (1 + 2.0 ** -12))
        assert not np.array_equal(_t(x["h_prev"]).float().to(BF).double().numpy(), x["h_prev"])
    return x


def atr_call(x, form, with_state=True, with_idx=True, with_mask=True):
    """-> dict out, out_copy (guarded buffers) of one Engine.rnn_atr_step."""
    e = eng()
    st = ST[form]
    Rn, H = x["p"].shape
    n_prev = x["h_prev"].shape[0]
    # (R = 5: a row stride that is no multiple of 4 floats -- the scalar loads of the state; else the 16-byte ones)
    hp = G(n_prev, H, H + (13 if Rn == 5 else 12), 4, F32, _t(x["h_prev"]))
    U = G(H, H, H + 8, 0, st, _t(x["U"]))
    b = G(1, H, dtype=F32, prefill=_t(x["b"]))
    p = G(Rn, H, 2 * H + 8, 8, st, _t(x["p"]))
    m = G(Rn, 1, 3, 1, F32, _t(x["mask"]))
    idx = torch.as_tensor(x["idx"].astype(np.int32)).cuda()
    out, cp = G(Rn, H, 3 * H + 4, 4, F32), G(Rn, H, H + 16, 8, st)
    e.rnn_atr_step(hp.mat if with_state else None, U.mat, b.t[P.LEAD:P.LEAD + H], p.mat, out.mat, cp.mat,
                   idx=idx if (with_idx and with_state) else None, mask=m.mat if with_mask else None)
    torch.cuda.synchronize()
    for buf, what in ((hp, "h_prev"), (U, "U"), (b, "b"), (p, "p"), (m, "mask")):
        buf.check_intact("atr_step " + what)
    out.check_guard("atr_step state")
    cp.check_guard("atr_step copy")
    return dict(out=out, out_copy=cp)


def atr_run(x, form, **kw):
    got = _values(atr_call(x, form, **kw))
    return got["out"], got["out_copy"]


# ---------------------------------------------------------------------------------------------- the GRU step
def gru_inputs(Rn, H, form, seed, n_prev, u_zero=False):
    """float64 arrays whose values are exactly representable where the kernels read them: Ug, Uh, xg and xh in the storage
    type, the state and the biases in fp32."""
    g = np.random.default_rng(200 + seed)
    st = lambda a: _t(a).float().to(ST[form]).double().numpy()
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    x = dict(h_prev=f32(g.normal(0, 1, (n_prev, H))), Ug=st(g.normal(0, H ** -0.5, (H, 2 * H))), bg=f32(g.normal(0, 0.3, 2 * H)),
             Uh=st(g.normal(0, H ** -0.5, (H, H))), bh=f32(g.normal(0, 0.3, H)), xg=st(g.normal(0, 1, (Rn, 2 * H))),
             xh=st(g.normal(0, 1, (Rn, H))), mask=(np.arange(Rn) % 3 != 1).astype(np.float64), idx=g.integers(0, n_prev, Rn))
    x["idx"][:3] = (n_prev - 1, n_prev - 1, 0)         # repeated rows
    if u_zero:
        x["Ug"], x["Uh"] = np.zeros((H, 2 * H)), np.zeros((H, H))
        x["h_prev"] = f32(x["h_prev"] * (1 + 2.0 ** -12))
        assert not np.array_equal(_t(x["h_prev"]).float().to(BF).double().numpy(), x["h_prev"])
    return x


def gru_call(x, form, with_state=True, with_idx=True, with_mask=True):
    """-> dict z, rh, out, out_copy (guarded buffers) of one Engine.rnn_gru_step."""
    e = eng()
    st = ST[form]
    Rn, H = x["xh"].shape
    n_prev = x["h_prev"].shape[0]
    # (R = 5: row strides that are no multiple of 16 bytes -- the scalar loads of the state and of rh; else the 16-byte ones)
    odd = Rn == 5
    hp = G(n_prev, H, H + (13 if odd else 12), 4, F32, _t(x["h_prev"]))
    Ug = G(H, 2 * H, 2 * H + 8, 0, st, _t(x["Ug"]))
    Uh = G(H, H, H + 8, 0, st, _t(x["Uh"]))
    bg = G(1, 2 * H, dtype=F32, prefill=_t(x["bg"]))
    bh = G(1, H, dtype=F32, prefill=_t(x["bh"]))
    xg = G(Rn, 2 * H, 3 * H + 8, 8, st, _t(x["xg"]))
    xh = G(Rn, H, 2 * H + 8, 8, st, _t(x["xh"]))
    m = G(Rn, 1, 3, 1, F32, _t(x["mask"]))
    idx = torch.as_tensor(x["idx"].astype(np.int32)).cuda()
    z, rh = G(Rn, H, H + 4, 4, F32), G(Rn, H, H + (11 if odd else 16), 8, st)
    out, cp = G(Rn, H, 3 * H + 4, 4, F32), G(Rn, H, H + 16, 8, st)
    e.rnn_gru_step(hp.mat if with_state else None, Ug.mat, bg.t[P.LEAD:P.LEAD + 2 * H], Uh.mat, bh.t[P.LEAD:P.LEAD + H], xg.mat,
                   xh.mat, z.mat, rh.mat, out.mat, cp.mat, idx=idx if (with_idx and with_state) else None,
                   mask=m.mat if with_mask else None)
    torch.cuda.synchronize()
    for buf, what in ((hp, "h_prev"), (Ug, "Ug"), (Uh, "Uh"), (bg, "bg"), (bh, "bh"), (xg, "xg"), (xh, "xh"), (m, "mask")):
        buf.check_intact("gru_step " + what)
    for buf, what in ((z, "z"), (rh, "rh"), (out, "state"), (cp, "copy")):
        buf.check_guard("gru_step " + what)
    return dict(z=z, rh=rh, out=out, out_copy=cp)


def gru_run(x, form, **kw):
    """-> dict z, rh, out, copy (float64 arrays)."""
    got = _values(gru_call(x, form, **kw))
    got["copy"] = got.pop("out_copy")
    return got


# ---------------------------------------------------------------------------------------------- ff + residual
def ff_call(x, form, in_place=False, with_copy=True):
    """-> dict out (and out_copy) (guarded buffers) of one Engine.rnn_ff_residual."""
    e = eng()
    st = ST[form]
    R, K = x["a"].shape
    N = x["W"].shape[1]
    odd = R % 2 == 1          # a row stride of a that is no multiple of 16 bytes: the scalar loads of the bf16 form
    a = G(R, K, K + (13 if odd else 16), 5 if odd else 8, st, _t(x["a"]))
    W = G(K, N, N + 8, 0, st, _t(x["W"]))
    b = G(1, N, dtype=F32, prefill=_t(x["b"]))
    xs = G(R, N, N + 4, 4, F32, _t(x["x"]))
    out = xs if in_place else G(R, N, 2 * N + 4, 4, F32)
    cp = G(R, N, N + K + 16, 8, st) if with_copy else None        # the x columns of a wider [. | x | c] operand
    e.rnn_ff_residual(a.mat, W.mat, b.t[P.LEAD:P.LEAD + N], xs.mat, out.mat, cp.mat if with_copy else None)
    torch.cuda.synchronize()
    for buf, what in ((a, "a"), (W, "W"), (b, "b")) + (() if in_place else ((xs, "x"),)):
        buf.check_intact("ff_residual " + what)
    for buf, what in ((out, "out"),) + (((cp, "copy"),) if with_copy else ()):
        buf.check_guard("ff_residual " + what)
    return dict(out=out, out_copy=cp) if with_copy else dict(out=out)


def ff_run(x, form, **kw):
    """-> (out, copy or None) as float64 arrays."""
    got = _values(ff_call(x, form, **kw))
    return got["out"], got.get("out_copy")


# ---------------------------------------------------------------------------------------------- the pinned cases
# ATR and GRU: the shapes of the kernel tests x three variants.  R = 5 has a state stride that is no multiple of 4 floats (the
# scalar loads of the A operand; the other shapes take the 16-byte loads).  GRU bf16 with H = 1000 and 2048: LDS images above
# 64 KB, which the launch has to ask for.
CELL_SHAPES = [("bf16", 5, 72), ("bf16", 33, 128), ("bf16", 70, 40), ("fp32", 5, 20), ("fp32", 33, 128)]
VARIANTS = {"gather+mask": {}, "null_state": dict(with_state=False), "plain": dict(with_idx=False, with_mask=False)}
# ff + residual, shapes of test_gpu_deepnmt_kernels._shapes(): (form, R, K, N, the call).  bf16 K = 4096 is the largest LDS
# image, fp32 N = 620 no multiple of the tile; odd R has an lda that is no multiple of 8 (the scalar A path of the bf16 form).
FF_MODES = {"apart": {}, "in_place": dict(in_place=True), "no_copy": dict(with_copy=False)}
FF_SHAPES = [
    ("bf16", 1, 4096, 24, "apart"), ("bf16", 65, 40, 64, "in_place"), ("bf16", 65, 2048, 8, "no_copy"),
    ("bf16", 130, 4096, 8, "apart"), ("bf16", 130, 1000, 616, "in_place"), ("bf16", 64, 40, 616, "apart"),
    ("bf16", 17, 8, 24, "no_copy"),
    ("fp32", 1, 40, 620, "apart"), ("fp32", 65, 8, 620, "in_place"), ("fp32", 65, 1000, 24, "no_copy"),
    ("fp32", 130, 8, 620, "apart"), ("fp32", 130, 2048, 64, "in_place"), ("fp32", 64, 2048, 620, "apart"),
    ("fp32", 17, 1000, 616, "no_copy"),
]


def _table():
    t = {}
    for cell in ("atr", "gru"):
        for form, Rn, H in CELL_SHAPES:
            for v in VARIANTS:
                t["%s-%s-R%d-H%d-%s" % (cell, form, Rn, H, v)] = (cell, form, Rn, H, v)
    for H in (1000, 2048):
        t["gru-bf16-R5-H%d-gather+mask" % H] = ("gru", "bf16", 5, H, "gather+mask")
    for form, R, K, N, mode in FF_SHAPES:
        t["ff-%s-R%d-K%d-N%d-%s" % (form, R, K, N, mode)] = ("ff", form, R, K, N, mode)
    return t


TABLE = _table()
CASES = list(TABLE)


@functools.lru_cache(maxsize=4)
def inputs(name):
    """The float64 arrays a case feeds its launch; the same values on every call."""
    c = TABLE[name]
    if c[0] == "ff":
        _, form, R, K, N, _ = c
        return DN.ff_inputs(R, K, N, form, R + K + N)
    cell, form, Rn, H, _ = c
    return (atr_inputs if cell == "atr" else gru_inputs)(Rn, H, form, Rn + H, n_prev=Rn + 2)


def run(name):
    """-> dict output name -> guarded buffer, after the guard checks"""
    c = TABLE[name]
    if c[0] == "ff":
        return ff_call(inputs(name), c[1], **FF_MODES[c[5]])
    return (atr_call if c[0] == "atr" else gru_call)(inputs(name), c[1], **VARIANTS[c[4]])


def digest(t):
    """t: a window as a contiguous CPU tensor (Guarded.value())"""
    raw = t.contiguous().view(torch.int16).numpy().tobytes()
    return {"sha256": hashlib.sha256(raw).hexdigest(), "head": [float(x) for x in t.reshape(-1)[:8].float()]}


def record(name):
    return {k: digest(b.value()) for k, b in run(name).items()}


def load(path=GOLDEN):
    with open(path) as f:
        return json.load(f)
