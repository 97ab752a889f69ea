"""transformer_l0drop on the CPU: the variable layout and the registry, the float64 reference against a dense
formulation, and the checks of the GPU files (tests/test_gpu_l0drop_kernels.py) shown to reject planted defects.

Planted (tests/l0drop_ref.py ``defect`` arguments), each judged by the check the GPU file applies to the kernels:
    no_kbias         the count of slot 0 ignored: the cross sub-layer's row check (C_PART / C_SUM of
                     tests/test_gpu_decode_elementwise.py, measured in tests/test_decode_parity_checker.py)
    count_padding    n_dropped counted over padded positions as well          exact counts, kbias within 1e-6
    zero_slot_open   the zero slot left valid when nothing was dropped        exact gmask
    filler_valid     a filler slot left valid                                 exact gmask
    descending       kept positions in descending order                      exact pos
"""
import numpy as np
import pytest
import torch

from tests import l0drop_ref as L
from tests import decode_parity as DP
from tests.common import make_hp
from tests.test_gpu_decode_elementwise import C_PART, C_SUM


def test_variable_specs_registry_and_refusals():
    from zero_amd.variables import variable_specs
    from zero_amd.models import model as registry, load_all
    load_all()
    for shared in (False, True):
        hp = make_hp("transformer_l0drop", shared_source_target_embedding=shared)
        if shared:
            hp.tgt_vocab = hp.src_vocab
        names = [s[0] for s in variable_specs(hp, "transformer_l0drop")]
        base = [s[0] for s in variable_specs(hp, "transformer")]
        i = names.index("source_pruning/W_0_0")
        # created by the decoder after its embedding (and the shared "bias") and before decoder/layer_0
        assert names[i + 1] == "source_pruning/b_0" and names[i + 2].startswith("decoder/layer_0/")
        assert names[i - 1] == ("tgt_embedding" if not shared else
                                "encoder/layer_%d/feed_forward/layer_norm/offset" % (hp.num_encoder_layer - 1))
        assert names[:i] + names[i + 2:] == base
        shapes = {s[0]: s[1] for s in variable_specs(hp, "transformer_l0drop")}
        assert shapes["source_pruning/W_0_0"] == (hp.hidden_size, 1) and shapes["source_pruning/b_0"] == (1,)
    triple = registry.get_model("transformer_l0drop")
    assert callable(triple.train_fn) and callable(triple.score_fn) and callable(triple.infer_fn)
    hp = make_hp("transformer_l0drop")
    with pytest.raises(NotImplementedError, match="decode only"):
        triple.train_fn({"source": np.ones((1, 2)), "target": np.ones((1, 2))}, hp)
    with pytest.raises(NotImplementedError, match="decode only"):
        triple.score_fn({"source": np.ones((1, 2)), "target": np.ones((1, 2))}, hp)
    hp.search_mode = "dev"
    with pytest.raises(NotImplementedError, match="search_mode=cache"):
        triple.infer_fn(hp)


def test_ensemble_refuses_an_l0drop_member():
    from zero_amd.hip import ZeroHipError
    from zero_amd.models import _ensemble
    hp = make_hp("transformer_l0drop")
    with pytest.raises(ZeroHipError, match="transformer_l0drop"):
        _ensemble.check_members([make_hp("transformer"), hp])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_compacted_attention_equals_the_dense_formulation(seed):
    rng = np.random.default_rng(seed)
    B, Ls, H, d, R = 5, 13, 32, 16, 3
    enc = rng.normal(size=(B, Ls, H))
    W = rng.normal(size=H) * 0.5
    smask = np.ones((B, Ls))
    for b in range(1, B):
        smask[b, Ls - 2 * b:] = 0
    b0 = L.LOG_ALPHA_0
    la, g = L.gate(enc, W, b0)
    g[0] = np.maximum(g[0], 0.3)                      # sentence 0 keeps everything: its zero slot is masked
    g[1] = 0.0                                        # sentence 1 keeps nothing: only the zero slot
    Wk, Wv = rng.normal(size=(H, d)), rng.normal(size=(H, d))
    bk, bv = rng.normal(size=d), rng.normal(size=d)
    q = rng.normal(size=(B, R, d))
    c = L.compact(enc, g, smask, Lm=Ls + 3)
    assert c["ndrop"][0] == 0 and c["nkeep"][1] == 0 and 0 < c["nkeep"][2] < (smask[2] != 0).sum()
    out = L.count_attention(q, c["mem"] @ Wk + bk, c["mem"] @ Wv + bv, c["gmask"], c["count"], d ** -0.5)
    mem_all = np.concatenate([enc * g[..., None], np.zeros((B, 1, H))], 1)
    dense = L.dense_attention(q, mem_all @ Wk + bk, mem_all @ Wv + bv, g, smask, d ** -0.5)
    assert np.abs(out - dense).max() <= 1e-12
    # and the log-count form the kernels use: exp(l + log c) = exp(l) c
    l = np.einsum("brd,bjd->brj", q, c["mem"] @ Wk + bk) * d ** -0.5 + ((1 - c["gmask"]) * -L.MASK_INF + c["kbias"])[:, None]
    e = np.exp(l - l.max(-1, keepdims=True))
    out2 = np.einsum("brj,bjd->brd", e / e.sum(-1, keepdims=True), c["mem"] @ Wv + bv)
    assert np.abs(out2 - dense).max() <= 1e-12


# ---------------------------------------------------------------------------------------------- the checks have teeth
@pytest.mark.parametrize("storage", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("Ls", [16, 72])
def test_gate_inputs_keep_their_distance_and_the_standin_passes(Ls, storage):
    enc, W, b0, smask = L.gate_inputs(Ls, storage)
    la, g = L.gate(enc.double().numpy(), W.numpy(), float(b0))
    valid = smask.numpy() != 0
    assert np.abs(la - L.LOG_ALPHA_0)[valid].min() >= 0.05
    la_bound, g_bound = L.gate_bound(enc.double().numpy(), W.numpy(), float(b0))
    assert la_bound.max() < 0.05 / 4              # the fp32 dot product cannot move log_alpha that far
    ref = L.compact(enc.double().numpy(), g, smask.numpy(), Lm=1 + Ls)
    assert ref["nkeep"][0] == Ls and ref["nkeep"][1] == 0 and 0 < ref["nkeep"][2] < Ls
    assert ((g[3] != 0) & ~valid[3]).any() and ref["kmax"] == Ls          # positive gates in the padded tail
    L.assert_compact(L.standin_compact(ref, Ls, storage), ref, enc.double().numpy(), g_bound, storage, "stand-in")


@pytest.mark.parametrize("defect", ["count_padding", "zero_slot_open", "filler_valid", "descending"])
def test_each_planted_compaction_defect_fails(defect):
    Ls, storage = 16, torch.bfloat16
    enc, W, b0, smask = L.gate_inputs(Ls, storage)
    la, g = L.gate(enc.double().numpy(), W.numpy(), float(b0))
    _, g_bound = L.gate_bound(enc.double().numpy(), W.numpy(), float(b0))
    ref = L.compact(enc.double().numpy(), g, smask.numpy(), Lm=1 + Ls)
    bad = L.compact(enc.double().numpy(), g, smask.numpy(), Lm=1 + Ls, defect=defect)
    with pytest.raises(AssertionError):
        L.assert_compact(L.standin_compact(bad, Ls, storage), ref, enc.double().numpy(), g_bound, storage, defect)


@pytest.mark.parametrize("Lk", [9, 17])
def test_the_cross_tolerance_catches_a_dropped_count(Lk):
    case, gmask, kbias = L.kb_case(Lk)
    x = L.kb_inputs(case, gmask)
    ref = L.kb_math(case, x, kbias)
    assert ref["smax"] < 4.0
    emu = L.kb_math(case, x, kbias, emulate=True)
    rp, rs = DP.parts_ratio(emu["parts"], ref["parts"]), DP.row_ratio(emu["sum"], ref["sum"])
    print("Lk %d: correct emulation head part %.3e, head sum %.3e" % (Lk, rp, rs))
    # (the constants are twice the worst emulation ratio over the tables of tests/decode_parity.py; these two cases are
    # not in those tables and sit at 0.45 c / 0.51 c)
    assert rp <= 0.6 * C_PART and rs <= 0.6 * C_SUM
    bad = L.kb_math(case, x, kbias, emulate=True, defect="no_kbias")
    bp, bs = DP.parts_ratio(bad["parts"], ref["parts"]), DP.row_ratio(bad["sum"], ref["sum"])
    print("Lk %d: count ignored   head part %.3e (%.1f c), head sum %.3e (%.1f c)" % (Lk, bp, bp / C_PART, bs, bs / C_SUM))
    assert bp >= 4 * C_PART and bs >= 4 * C_SUM
