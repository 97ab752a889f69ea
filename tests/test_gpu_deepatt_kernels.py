"""zk_rnn_gru_gates + zk_rnn_gru_out and their fp32 forms called directly (zero_amd/csrc/zk_rnn.hip, through
Engine.rnn_gru_step) and compared element by element with the float64 reference of tests/deepatt_ref.py under its derived
bounds.  Every operand and output is a parity.guarded buffer: outputs are prefilled with NaN, nothing outside their windows
may change, inputs must be bit-identical after the call; every row stride is larger than the row.

Shapes (those of the ATR step's tests: the smallest that hit every edge)
    bf16: R = 5, H = 72 (edge tiles in rows and columns, K not a multiple of 32), R = 33, H = 128 (three waves) and
          R = 70, H = 40 (two row blocks);
    fp32: R = 5, H = 20 and R = 33, H = 128 (two row blocks, two column tiles).
Each with a gather index that repeats rows + a mixed 0 / 1 mask, with a null h_prev, and plain.  z, rh, the fp32 state and
the copy are each held to gru_bound; carried rows are bit-equal.  Ug = Uh = 0 with a state that is not bf16-representable:
the z h term to fp32 accuracy.  bf16 with H = 1000 and H = 2048: the LDS images past 64 KB.  The aliasing refusal; the
H % 8 and H > 2048 refusals of the bf16 forms name the fp32 forms.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util_gpu import eng  # noqa: E402
from tests import deepatt_ref as D  # noqa: E402
from tests import variant_ref as V  # noqa: E402
from tests.rnn_cell_cases import gru_inputs as _gru_inputs, gru_run as _gru_run  # noqa: E402
from zero_amd.func import Mat  # noqa: E402
from zero_amd.hip import ZeroHipError  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
ST = {"bf16": BF, "fp32": F32}


def _check(got, ref, form, label):
    worst = {}
    for what in ("z", "rh", "out", "copy"):
        worst[what] = V.assert_within(got[what], ref["out" if what == "copy" else what], D.gru_bound(ref, form, what),
                                      "%s %s" % (label, what))
    print("%s: largest |err| / bound %s" % (label, "  ".join("%s %.3f" % kv for kv in worst.items())))


GRU_SHAPES = [("bf16", 5, 72), ("bf16", 33, 128), ("bf16", 70, 40), ("fp32", 5, 20), ("fp32", 33, 128)]


@pytest.mark.parametrize("form,Rn,H", GRU_SHAPES)
@pytest.mark.parametrize("variant", ["gather+mask", "null_state", "plain"])
def test_gru_step(form, Rn, H, variant):
    x = _gru_inputs(Rn, H, form, Rn + H, n_prev=Rn + 2)
    if variant == "gather+mask":
        kw, ref = {}, D.gru_step(**x)
    elif variant == "null_state":
        kw, ref = dict(with_state=False), D.gru_step(**dict(x, h_prev=None, idx=None))
    else:
        kw, ref = dict(with_idx=False, with_mask=False), D.gru_step(**dict(x, idx=None, mask=None))
    got = _gru_run(x, form, **kw)
    _check(got, ref, form, "%s R=%d H=%d %s" % (form, Rn, H, variant))
    if variant == "gather+mask":
        carried = x["mask"] == 0
        assert np.array_equal(got["out"][carried], ref["h"][carried]), "a carried row must be the gathered state, bit for bit"
    if variant == "null_state":
        assert not got["rh"].any(), "the zero state: rh = 0"


@pytest.mark.parametrize("H", [1000, 2048])
def test_gru_step_bf16_large_lds_images(H):
    """The sizes at which the launches ask for more dynamic LDS than the 64 KB a kernel gets without asking: H = 1000 (the
    recipe's hidden size; the gates image [32][1032] bf16 is 66 KB, the second launch's 33 KB) and H = 2048, the largest H of
    the bf16 forms (129 KB and 66 KB).  Four rows, a gather index and a mixed mask."""
    x = _gru_inputs(4, H, "bf16", H, n_prev=5)
    ref = D.gru_step(**x)
    got = _gru_run(x, "bf16")
    _check(got, ref, "bf16", "bf16 R=4 H=%d" % H)
    carried = x["mask"] == 0
    assert np.array_equal(got["out"][carried], ref["h"][carried])


@pytest.mark.parametrize("form", ["bf16", "fp32"])
def test_gru_step_keeps_the_state_in_fp32(form):
    """Ug = Uh = 0: both products vanish; the state enters through z h and the carry only.  With a state that is not
    bf16-representable the bound has no bf16 term left, so a kernel that rounds the state fails it
    (tests/test_deepatt_host.py shows that)."""
    x = _gru_inputs(5, 72 if form == "bf16" else 20, form, 7, n_prev=6, u_zero=True)
    ref = D.gru_step(**x)
    got = _gru_run(x, form)
    bound = D.gru_bound(ref, form)
    assert bound.max() < 2.0 ** -16                 # (a bf16 state is off by about 2^-9 z |h|)
    V.assert_within(got["out"], ref["out"], bound, "%s U = 0" % form)


@pytest.mark.parametrize("form", ["bf16", "fp32"])
def test_gru_step_refuses_an_output_that_overlaps_the_state(form):
    e = eng()
    st = ST[form]
    Rn, H = 4, 24
    buf = torch.zeros(2 * Rn * 2 * H, dtype=F32, device="cuda")
    zt = lambda *s, dt=st: torch.zeros(*s, dtype=dt, device="cuda")
    Ug, Uh = Mat(zt(H, 2 * H), H, 2 * H), Mat(zt(H, H), H, H)
    bg, bh = zt(2 * H, dt=F32), zt(H, dt=F32)
    xg, xh = Mat(zt(Rn, 2 * H), Rn, 2 * H), Mat(zt(Rn, H), Rn, H)
    z, rh = Mat(zt(Rn, H, dt=F32), Rn, H), Mat(zt(Rn, H), Rn, H)
    state = Mat(buf, Rn, H, 2 * H, 0)
    with pytest.raises(ZeroHipError, match="zk_(f32_)?rnn_gru_out: out overlaps h_prev"):
        e.rnn_gru_step(state, Ug, bg, Uh, bh, xg, xh, z, rh, state)                                   # in place
    with pytest.raises(ZeroHipError, match="zk_(f32_)?rnn_gru_out: out overlaps h_prev"):
        e.rnn_gru_step(state, Ug, bg, Uh, bh, xg, xh, z, rh, Mat(buf, Rn, H, 2 * H, H - 1))           # one column shared per row
    with pytest.raises(ZeroHipError, match="zk_(f32_)?rnn_gru_gates: z overlaps h_prev"):
        e.rnn_gru_step(state, Ug, bg, Uh, bh, xg, xh, state, rh, Mat(buf, Rn, H, 2 * H, H))
    # rows of one [B, L, H] sequence buffer at two positions interleave without sharing an element: a scan's own layout
    e.rnn_gru_step(state, Ug, bg, Uh, bh, xg, xh, z, rh, Mat(buf, Rn, H, 2 * H, H))
    torch.cuda.synchronize()


def test_bf16_forms_refuse_sizes_they_do_not_take():
    e = eng()
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device="cuda")

    def call(H, Rn=2):
        e.rnn_gru_step(None, Mat(z(H, 2 * H), H, 2 * H), z(2 * H, dt=F32), Mat(z(H, H), H, H), z(H, dt=F32),
                       Mat(z(Rn, 2 * H), Rn, 2 * H), Mat(z(Rn, H), Rn, H), Mat(z(Rn, H, dt=F32), Rn, H), Mat(z(Rn, H), Rn, H),
                       Mat(z(Rn, H, dt=F32), Rn, H))
    with pytest.raises(ZeroHipError, match="multiple of 8.*zk_f32_rnn_gru_gates takes any H"):
        call(20)
    with pytest.raises(ZeroHipError, match="at most 2048.*zk_f32_rnn_gru_gates takes any H"):
        call(2056)                                    # past the LDS image: refused by name, nothing launched
    with pytest.raises(ZeroHipError, match="multiple of 8.*zk_f32_rnn_gru_out takes any H"):
        H = 20                                        # (the second launch alone: the first refused above)
        rh, Uh, bh, xh, zg, out = z(2, H), z(H, H), z(H, dt=F32), z(2, H), z(2, H, dt=F32), z(2, H, dt=F32)
        e.lib.call("zk_rnn_gru_out", rh.data_ptr(), H, Uh.data_ptr(), H, bh.data_ptr(), xh.data_ptr(), H, zg.data_ptr(), H,
                   None, 0, 0, None, None, 0, out.data_ptr(), H, None, 0, 2, H, e.stream)
