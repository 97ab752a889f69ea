"""zk_rnn_atr_step / zk_add_attn and their fp32 forms called directly (zero_amd/csrc/zk_rnn.hip) and compared element by
element with the float64 references of tests/rnnsearch_ref.py under their derived bounds.  Every operand and output is a
parity.guarded buffer: outputs are prefilled with NaN, nothing outside their windows may change, inputs must be
bit-identical after the call; every row stride is larger than the row.

atr_step   bf16: R = 5, H = 72 (edge tiles in rows and columns, K not a multiple of 32), R = 33, H = 128 (three waves) and
           R = 70, H = 40 (two row blocks);
           fp32: R = 5, H = 20 and R = 33, H = 128 (two row blocks, two column tiles).  Each with a gather index that repeats
           rows + a mixed 0 / 1 mask, and with a null h_prev.  U = 0 with a state that is not bf16-representable: the carried
           term to fp32 accuracy.  The aliasing refusal.
add_attn   R = 6, kv_group = 3, M = 72, Ls = 17, lengths (17, 6), sentence 1's masked keys the hottest;  kv_group = 1, Ls = 1;
           Ls = 130, M = 128 (three key tiles);  fp32 with M = 20;  kv_group = 6 (two workgroups per sentence, 4 + 2 rows).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng  # noqa: E402
from tests import parity as P  # noqa: E402
from tests import rnnsearch_ref as R  # noqa: E402
from tests import variant_ref as V  # noqa: E402
from tests.rnn_cell_cases import atr_inputs as _atr_inputs, atr_run as _atr_run  # noqa: E402
from zero_amd.func import Mat  # noqa: E402
from zero_amd.hip import ZeroHipError  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
ST = {"bf16": BF, "fp32": F32}


def G(rows, cols, ld=None, off=0, dtype=BF, prefill=None):
    return P.guarded(rows, cols, ld, off, dtype, prefill, "cuda")


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64))


# ---------------------------------------------------------------------------------------------- the ATR step
ATR_SHAPES = [("bf16", 5, 72), ("bf16", 33, 128), ("bf16", 70, 40), ("fp32", 5, 20), ("fp32", 33, 128)]


@pytest.mark.parametrize("form,Rn,H", ATR_SHAPES)
@pytest.mark.parametrize("variant", ["gather+mask", "null_state", "plain"])
def test_atr_step(form, Rn, H, variant):
    x = _atr_inputs(Rn, H, form, Rn + H, n_prev=Rn + 2)
    if variant == "gather+mask":
        kw, ref = {}, R.atr_step(**x)
    elif variant == "null_state":
        kw, ref = dict(with_state=False), R.atr_step(**dict(x, h_prev=None, idx=None))
    else:
        kw, ref = dict(with_idx=False, with_mask=False), R.atr_step(**dict(x, idx=None, mask=None))
    out, cp = _atr_run(x, form, **kw)
    r1 = V.assert_within(out, ref["out"], R.atr_bound(ref, form), "%s R=%d H=%d %s state" % (form, Rn, H, variant))
    r2 = V.assert_within(cp, ref["out"], R.atr_bound(ref, form, copy=True), "%s R=%d H=%d %s copy" % (form, Rn, H, variant))
    print("%s R=%d H=%d %s: largest |err| / bound %.3f (state), %.3f (copy)" % (form, Rn, H, variant, r1, r2))
    if variant == "gather+mask":
        carried = x["mask"] == 0
        assert np.array_equal(out[carried], ref["h"][carried]), "a carried row must be the gathered state, bit for bit"


@pytest.mark.parametrize("form", ["bf16", "fp32"])
def test_atr_step_keeps_the_state_in_fp32(form):
    """U = 0: q = b exactly; the state enters through f h and the carry only.  With a state that is not bf16-representable
    the bound has no bf16 term left, so a kernel that rounds the state fails it (tests/test_rnnsearch_host.py shows that)."""
    x = _atr_inputs(5, 72 if form == "bf16" else 20, form, 7, n_prev=6, u_zero=True)
    ref = R.atr_step(**x)
    out, _ = _atr_run(x, form)
    bound = R.atr_bound(ref, form)
    assert bound.max() < 2.0 ** -16                 # (a bf16 state is off by about 2^-9 f |h|)
    V.assert_within(out, ref["out"], bound, "%s U = 0" % form)


@pytest.mark.parametrize("form", ["bf16", "fp32"])
def test_atr_step_refuses_an_output_that_overlaps_the_state(form):
    e = eng()
    st = ST[form]
    Rn, H = 4, 24
    buf = torch.zeros(2 * Rn * 2 * H, dtype=F32, device="cuda")
    U = Mat(torch.zeros(H, H, dtype=st, device="cuda"), H, H)
    b = torch.zeros(H, dtype=F32, device="cuda")
    p = Mat(torch.zeros(Rn, H, dtype=st, device="cuda"), Rn, H)
    state = Mat(buf, Rn, H, 2 * H, 0)
    with pytest.raises(ZeroHipError, match="out overlaps h_prev"):
        e.rnn_atr_step(state, U, b, p, state)                                   # in place
    with pytest.raises(ZeroHipError, match="out overlaps h_prev"):
        e.rnn_atr_step(state, U, b, p, Mat(buf, Rn, H, 2 * H, H - 1))           # one column shared per row
    # rows of one [B, L, H] sequence buffer at two positions interleave without sharing an element: a scan's own layout
    e.rnn_atr_step(state, U, b, p, Mat(buf, Rn, H, 2 * H, H))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- the additive attention
ADD_CASES = {
    "beam3": dict(Rn=6, Gp=3, M=72, Ls=17, lengths=(17, 6), forms=("bf16", "fp32")),
    "one_key": dict(Rn=3, Gp=1, M=72, Ls=1, lengths=(1, 1, 1), forms=("bf16", "fp32")),
    "three_tiles": dict(Rn=4, Gp=2, M=128, Ls=130, lengths=(130, 67), forms=("bf16", "fp32")),
    "fp32_M20": dict(Rn=4, Gp=2, M=20, Ls=11, lengths=(11, 4), forms=("fp32",)),
    "beam6": dict(Rn=12, Gp=6, M=24, Ls=5, lengths=(5, 3), forms=("bf16", "fp32")),
}


def _add_inputs(name, form):
    cs = ADD_CASES[name]
    Rn, Gp, M, Ls = cs["Rn"], cs["Gp"], cs["M"], cs["Ls"]
    nB = Rn // Gp
    g = torch.Generator().manual_seed(900 + sum(map(ord, name)))
    st = lambda t: t.to(ST[form]).double().numpy()
    qa, pm, mem = torch.randn(Rn, M, generator=g), torch.randn(nB, Ls, M, generator=g), torch.randn(nB, Ls, M, generator=g)
    v = (torch.randn(M, generator=g) * 0.5).double().numpy()
    mask = torch.zeros(nB, Ls)
    for s_, n in enumerate(cs["lengths"]):
        mask[s_, :n] = 1
    b = nB - 1
    n = cs["lengths"][b]
    if n < Ls:     # the masked keys of the last sentence are the hottest: every tanh at about +-1 with v's sign
        pm[b, n:] = 3.0 * torch.sign(torch.as_tensor(v)).float()[None, :] - qa[b * Gp:(b + 1) * Gp].mean(0)[None, :]
    return dict(qa=st(qa), pm=st(pm), mem=st(mem), v=v, mask=mask.double().numpy(), kv_group=Gp)


def _add_run(x, form, Ls):
    e = eng()
    st = ST[form]
    Rn, M = x["qa"].shape
    nB = x["pm"].shape[0]
    qa = G(Rn, M, M + 8, 0, st, _t(x["qa"]))
    both = G(nB * Ls, 2 * M, 2 * M + 16, 8, st, torch.cat([_t(x["pm"]).reshape(nB * Ls, M), _t(x["mem"]).reshape(nB * Ls, M)], 1))
    v = G(1, M, dtype=F32, prefill=_t(x["v"]))
    mask = G(nB, Ls, Ls, 0, F32, _t(x["mask"]))
    ctx, cp = G(Rn, M, 2 * M + 4, 4, F32), G(Rn, M, M + 24, 8, st)
    e.add_attn(qa.mat, both.mat.cols_slice(0, M), both.mat.cols_slice(M, 2 * M), v.t[P.LEAD:P.LEAD + M],
               mask.t[P.LEAD:P.LEAD + nB * Ls].view(nB, Ls), ctx.mat, cp.mat, x["kv_group"], Ls)
    torch.cuda.synchronize()
    for buf, what in ((qa, "qa"), (both, "pm | mem"), (v, "v"), (mask, "mask")):
        buf.check_intact("add_attn " + what)
    ctx.check_guard("add_attn context")
    cp.check_guard("add_attn copy")
    return ctx.value().double().numpy(), cp.value().double().numpy()


ADD_RUNS = [(n, f) for n, cs in ADD_CASES.items() for f in cs["forms"]]


@pytest.mark.parametrize("name,form", ADD_RUNS, ids=["%s-%s" % r for r in ADD_RUNS])
def test_add_attn(name, form):
    x = _add_inputs(name, form)
    Ls = ADD_CASES[name]["Ls"]
    ref = R.add_attention(**x)
    ctx, cp = _add_run(x, form, Ls)
    r1 = V.assert_within(ctx, ref["out"], R.add_bound(ref, form), "%s %s context" % (name, form))
    r2 = V.assert_within(cp, ref["out"], R.add_bound(ref, form, copy=True), "%s %s copy" % (name, form))
    print("%s %s: largest |err| / bound %.3f (fp32 context), %.3f (copy)" % (name, form, r1, r2))
    if name == "one_key":
        assert np.array_equal(ctx, x["mem"][:, 0]), "one key: the weight is 1, the context the memory row"


@pytest.mark.parametrize("form", ["bf16", "fp32"])
def test_add_attn_tanh_saturates(form):
    """Projected queries of +-3e38 (and their sum with the memory beyond the fp32 range): tanh is +-1, nothing is NaN."""
    x = _add_inputs("beam3", form)
    big = np.where(np.arange(x["qa"].shape[1])[None, :] % 2 == 0, 3e38, -3e38) * np.ones_like(x["qa"])
    x = dict(x, qa=_t(big).float().to(ST[form]).double().numpy(), pm=np.abs(x["pm"]) * np.sign(big[0])[None, None, :] * 1e38)
    x["pm"] = _t(x["pm"]).float().to(ST[form]).double().numpy()
    ctx, _ = _add_run(x, form, 17)
    assert np.isfinite(ctx).all()
    with np.errstate(over="ignore"):
        ref = R.add_attention(**x)
    V.assert_within(ctx, ref["out"], R.add_bound(ref, form), "%s saturated" % form)


def test_bf16_forms_refuse_sizes_that_are_not_multiples_of_8():
    e = eng()
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device="cuda")
    H = 20
    with pytest.raises(ZeroHipError, match="zk_f32_rnn_atr_step takes any H"):
        e.rnn_atr_step(None, Mat(z(H, H), H, H), z(H, dt=F32), Mat(z(2, H), 2, H), Mat(z(2, H, dt=F32), 2, H))
    with pytest.raises(ZeroHipError, match="zk_f32_add_attn takes any M"):
        e.add_attn(Mat(z(2, H), 2, H), Mat(z(6, H), 6, H), Mat(z(6, H), 6, H), z(H, dt=F32), None, Mat(z(2, H, dt=F32), 2, H),
                   None, 1, 3)
