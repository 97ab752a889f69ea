"""The kernels of transformer_l0drop called directly (zero_amd/csrc/zk_l0drop.hip, zk_dec_cross_kb, zk_f32_attn_kb) and
compared with the float64 reference of tests/l0drop_ref.py.  Every operand and output is a parity.guarded buffer: outputs
are prefilled with NaN, nothing outside their windows may change, inputs must be bit-identical after the call.

zk_l0_gate + zk_l0_compact: B = 4, H = 128, Ls = 16 and 72 (the second crosses a wave in the scan), bf16 and fp32
storage; the sentences of l0drop_ref.gate_inputs (keeps all / none / an interleaved subset / a padded tail with positive
gates).  pos, counts, kmax and gmask exact, kbias within 1e-6, the gate within l0drop_ref.gate_bound, mem within one
rounding of its storage type of the float64 product (+ the gate's bound times |x|); Lm = Ls + 3, so fillers exist and
must be exact zeros.  tests/test_l0drop_host.py asserts the inputs' distance from the threshold and shows that the same
check rejects planted defects.

zk_dec_cross_kb / zk_f32_attn_kb: the smallest cross shape of tests/test_gpu_decode_elementwise.py (H 128, 3 sentences
x 4 rows) with Lk = 9 and 17; sentence 0 has the zero slot masked, sentence 1 count 5.  kbias = NULL: bit-identical to
the old entry point.  With kbias: the row check of the cross sub-layer with its constants C_PART / C_SUM.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng  # noqa: E402
from tests import decode_parity as DP  # noqa: E402
from tests import l0drop_ref as L  # noqa: E402
from tests.test_gpu_decode_elementwise import C_PART, C_SUM, G, ptr, Group, weights, check_attn  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32


def _ints(g):
    return g.value().contiguous().view(torch.int32).numpy()


@pytest.mark.parametrize("storage", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("Ls", [16, 72])
def test_gate_and_compact(Ls, storage):
    e = eng()
    B, H, Lm = 4, 128, Ls + 3
    enc, W, b0, smask = L.gate_inputs(Ls, storage)
    f32 = 1 if storage == F32 else 0
    encg = G(B * Ls, H, H + 8, 4, storage, enc.reshape(B * Ls, H))
    Wg, b0g = G(1, H, dtype=F32, prefill=W), G(1, 1, 4, 0, F32, b0.reshape(1, 1))
    smg = G(B, Ls, dtype=F32, prefill=smask)
    gate, pos = G(B, Ls, dtype=F32), G(B, Ls, dtype=F32)
    nk, nd, km = G(1, B, dtype=F32), G(1, B, dtype=F32), G(1, 1, dtype=F32)
    e.lib.call("zk_l0_gate", ptr(encg), encg.ld, f32, ptr(smg), ptr(Wg), ptr(b0g), B, Ls, H, ptr(gate), ptr(pos), ptr(nk),
               ptr(nd), ptr(km), e.stream)
    torch.cuda.synchronize()
    for g in (gate, pos, nk, nd, km):
        g.check_guard("zk_l0_gate output")
        g.rebase()
    mem = G(B * Lm, H, H + 4, 0, storage)
    gmask, kbias = G(B, Lm, dtype=F32), G(B, Lm, dtype=F32)          # [B, Lm] contiguous: the attention's ldmask = Lm
    e.lib.call("zk_l0_compact", ptr(encg), encg.ld, f32, ptr(gate), ptr(pos), ptr(nk), ptr(nd), B, Ls, H, Lm, ptr(mem), mem.ld,
               ptr(gmask), ptr(kbias), e.stream)
    torch.cuda.synchronize()
    for g in (encg, Wg, b0g, smg, gate, pos, nk, nd, km):
        g.check_intact("zk_l0_gate / zk_l0_compact operand")
    for g in (mem, gmask, kbias):
        g.check_guard("zk_l0_compact output")
    x64 = enc.double().numpy()
    la, g64 = L.gate(x64, W.numpy(), float(b0))
    _, g_bound = L.gate_bound(x64, W.numpy(), float(b0))
    got_gate = gate.value().double().numpy()
    assert np.isfinite(got_gate).all() and (np.abs(got_gate - g64) <= g_bound).all(), np.abs(got_gate - g64).max()
    assert np.array_equal(got_gate != 0, g64 != 0)
    ref = L.compact(x64, g64, smask.numpy(), Lm=Lm)
    got = {"pos": _ints(pos), "nkeep": _ints(nk)[0], "ndrop": _ints(nd)[0], "kmax": int(_ints(km)[0, 0]),
           "gmask": gmask.value().numpy(), "kbias": kbias.value().numpy(),
           "mem": mem.value().double().numpy().reshape(B, Lm, H)}
    L.assert_compact(got, ref, x64, g_bound, storage, "Ls %d %s" % (Ls, storage))
    assert (got["mem"][:, 0] == 0).all() and (got["mem"][1] == 0).all()      # the zero slot; the sentence that keeps nothing


def _run_cross(case, x, entry, kbias=None):
    """One zk_dec_cross / zk_dec_cross_kb call on guarded operands (column halves of one [B*Lk, 2H] buffer)."""
    e = eng()
    H, (B, R), Lk = case["H"], case["BR"], case["Lk"]
    nh, rows = H // DP.D, B * R
    w = weights(H, False)
    ld = 2 * H + 16
    kv = G(B * Lk, 2 * H, ld, 8, prefill=torch.cat([x["keys"].reshape(B * Lk, H), x["vals"].reshape(B * Lk, H)], 1))
    mask = G(B, Lk, Lk + 3, 0, F32, x["kmask"])
    kb = G(B, Lk, Lk + 3, 0, F32, kbias) if kbias is not None else None
    xin = G(rows, H, prefill=x["x"])
    out = G(nh * rows, H, dtype=F32)
    head = (ptr(xin), None, None, None, None, H, DP.EPS, None, None, None, 0, 0, None, None, None, 1.0, None,
            ptr(w["wqt"]), w["wqt"].ld, ptr(w["bq"]), kv.mat.ptr, kv.mat.cols_slice(H, 2 * H).ptr, ld, ld, Lk * ld, Lk * ld,
            ptr(mask), mask.ld)
    tail = (ptr(w["wot"]), w["wot"].ld, ptr(out), B, R, nh, Lk, DP.SCALE, DP.MASK_INF, None, None, 0, 0, None, e.stream)
    with Group(case["group"]):
        if entry == "zk_dec_cross":
            e.lib.call(entry, *head, *tail)
        else:
            e.lib.call(entry, *head, ptr(kb), *tail)
        torch.cuda.synchronize()
    for g in (w["wqt"], w["bq"], w["wot"], xin, mask, kb, kv):
        if g is not None:
            g.check_intact(entry + " operand")
    out.check_guard(entry + ": out_parts")
    return out


@pytest.mark.parametrize("group", [0, 3, 16])
@pytest.mark.parametrize("Lk", [9, 17])
def test_dec_cross_kb(Lk, group):
    case, gmask, kbias = L.kb_case(Lk)
    case = dict(case, group=group)
    x = L.kb_inputs(case, gmask)
    (B, R), H = case["BR"], case["H"]
    old = _run_cross(case, x, "zk_dec_cross")
    null = _run_cross(case, x, "zk_dec_cross_kb", None)
    assert torch.equal(old.value().view(torch.int32), null.value().view(torch.int32)), "kbias = NULL is not zk_dec_cross"
    ref = L.kb_math(case, x, kbias)
    assert ref["smax"] < 4.0
    out = _run_cross(case, x, "zk_dec_cross_kb", kbias)
    check_attn("zk_dec_cross_kb Lk %d group %d" % (Lk, group), out, ref, H // DP.D, B * R, H)


@pytest.mark.parametrize("Lk", [9, 17])
def test_f32_attn_kb(Lk):
    e = eng()
    case, gmask, kbias = L.kb_case(Lk)
    x = L.kb_inputs(case, gmask)
    (B, R), H = case["BR"], case["H"]
    nh, d, rows = H // DP.D, DP.D, B * R
    gq = torch.Generator().manual_seed(5)
    q = torch.randn(rows, H, generator=gq)
    qg = G(rows, H, H + 4, 0, F32, q)
    kg, vg = G(B * Lk, H, H + 8, 4, F32, x["keys"].reshape(B * Lk, H)), G(B * Lk, H, H + 8, 4, F32, x["vals"].reshape(B * Lk, H))
    mask, kb = G(B, Lk, Lk + 3, 0, F32, gmask), G(B, Lk, Lk + 3, 0, F32, kbias)

    def run(entry, kbp):
        out = G(rows, H, H + 4, 0, F32)
        head = (ptr(qg), ptr(kg), ptr(vg), ptr(out), rows, nh, 1, Lk, d, qg.ld, kg.ld, kg.ld, out.ld, qg.ld, Lk * kg.ld,
                Lk * kg.ld, out.ld, ptr(mask), mask.ld)
        tail = (R, DP.SCALE, DP.MASK_INF, None, None, None, 0, 0, None, e.stream)
        if entry == "zk_f32_attn":
            e.lib.call(entry, *head, *tail)
        else:
            e.lib.call(entry, *head, kbp, *tail)
        torch.cuda.synchronize()
        for g in (qg, kg, vg, mask, kb):
            g.check_intact(entry + " operand")
        out.check_guard(entry + " output")
        return out.value()
    old, null = run("zk_f32_attn", None), run("zk_f32_attn_kb", None)
    assert torch.equal(old.view(torch.int32), null.view(torch.int32)), "kbias = NULL is not zk_f32_attn"
    got = run("zk_f32_attn_kb", ptr(kb))
    k64, v64 = x["keys"].double().numpy(), x["vals"].double().numpy()
    ref = np.zeros((rows, H))
    for h in range(nh):
        sl = slice(h * d, (h + 1) * d)
        ref[:, sl] = L.count_attention(q.double().numpy().reshape(B, R, H)[:, :, sl], k64[:, :, sl], v64[:, :, sl],
                                       gmask.numpy(), np.exp(kbias.double().numpy()), DP.SCALE).reshape(rows, d)
    r = DP.row_ratio(got.double(), torch.as_tensor(ref))
    err = float((got.double() - torch.as_tensor(ref)).abs().max())
    print("zk_f32_attn_kb Lk %d: row ratio %.3e (c %.3e), max abs err %.3e" % (Lk, r, C_SUM, err))
    assert r <= C_SUM
    assert err < 5e-6            # the bound of tests/test_gpu_decode_f32.py::test_attention_f32 for this kernel
    # the count matters at this tolerance: without it the rows of sentence 1 are far off
    no = run("zk_f32_attn", None)
    assert DP.row_ratio(no.double(), torch.as_tensor(ref)) >= 4 * C_SUM
