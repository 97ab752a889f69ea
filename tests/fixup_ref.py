"""References of transformer_fixup (a plain module, no pytest in it).

Reference arithmetic (modules/fixup.py; models/transformer_fixup.py is models/transformer.py with every LayerNorm removed,
a scalar shift in front of every sub-layer, a scalar scale behind it and no bias in any linear map):

    shift_layer(x) = x - offset          scale_layer(y) = y * scale          offset, scale: [1]
    attention sub-layer     x <- x + scale * o_map(attention(shift(x)))
    feed-forward sub-layer  x <- x + scale * output(relu(enlarge(shift(x)) - offset) - offset)      ONE offset, three uses
    encoder output          scale(shift(x))          decoder output   shift(x)

``residual`` / ``relu_shift``   the float64 numpy statements of the two kernels (zk_fixup_residual, zk_fixup_relu_shift) with
                     everything ``*_bound`` needs; ``defect=`` plants ONE defect.
``residual_bound`` / ``relu_shift_bound``   the element-wise bounds (derivation in the docstrings).
``standin_*``        what a correct kernel computes, in torch float32 with another evaluation order.
``CASES`` / ``case_inputs``   the operands of the kernel tests (tests/test_gpu_fixup_kernels.py), built on the CPU.
``encoder`` / ``decoding_fns`` / ``full_decoder`` / ``score``   the model restated on oracle.ref_torch's linear (bias=False),
                     dot_attention, embedding, timing, beam search and storage sites (rt._st).
``init_params`` / ``make_fixture``   the tiny model of the GPU model tests: every parameter matters, and the reference alone
                     is shown to be far from a tie on it.
"""
import copy
import functools
from collections import OrderedDict

import numpy as np
import torch

from oracle import ref_torch as rt
from tests import variant_ref as V

RES_DEFECTS = ("shift_before_residual", "scale_on_x", "scale2_dropped", "xs_from_rounded", "host_baked")
FFN_DEFECTS = ("second_shift_dropped", "shift_inside_only", "host_baked")


def _round_st(v, st):
    """float64 array rounded to the storage type (round to nearest even) and back."""
    return torch.as_tensor(np.asarray(v, np.float64)).to(torch.float32 if st == torch.float32 else st).double().numpy()


# ---------------------------------------------------------------------------------------------- numpy, float64
def residual(x, y, a, o, b, st=torch.bfloat16, defect=None, stale=None):
    """x [rows, H] or None (0), y [rows, H] or None (0); a, o, b floats or None (1, 0, 1).  -> dict of float64 arrays:
    x_out, xs, and the magnitudes the bounds need.

    defect (one at a time; each is something a kernel or its caller could do):
      shift_before_residual   the shifted operand formed from x, before the branch is added: xs = b (x - o)
      scale_on_x              x_out = a x + y
      scale2_dropped          xs = x_out - o
      xs_from_rounded         xs formed from x_out rounded to the storage type (two roundings)
      host_baked              the scalars are the values `stale` = (a, o, b) from before a change"""
    if defect == "host_baked":
        a, o, b = stale
    a = 1.0 if a is None else float(a)
    o = 0.0 if o is None else float(o)
    b = 1.0 if b is None else float(b)
    ref = x if x is not None else y
    x = np.zeros_like(np.asarray(ref, np.float64)) if x is None else np.asarray(x, np.float64)
    y = np.zeros_like(x) if y is None else np.asarray(y, np.float64)
    x_out = a * x + y if defect == "scale_on_x" else x + a * y
    base = x if defect == "shift_before_residual" else x_out
    if defect == "xs_from_rounded":
        base = _round_st(base, st)
    xs = (base - o) * (1.0 if defect == "scale2_dropped" else b)
    mag = np.abs(x) + np.abs(a * y)
    return {"x_out": x_out, "xs": xs, "mag_x": mag, "mag_xs": abs(b) * (mag + abs(o))}


def residual_bound(ref, st):
    """Element-wise bounds of a kernel that forms everything in fp32 from exactly representable inputs, against residual().

      x_out = x + a y        two roundings (the product, the sum), each at most 2^-24 of a magnitude that never exceeds
                             |x| + |a y|: with PER_TERM = 2^-23 per rounding (TWICE the unit roundoff, as
                             tests/parity.py:gemm_bound counts)          |dx_out| <= 2 * 2^-23 (|x| + |a y|)
      xs = b (x_out - o)     two more roundings (the difference, the product) on magnitudes within |b| (|x| + |a y| + |o|),
                             and the error of x_out carried through b:   4 * 2^-23 |b| (|x| + |a y| + |o|)
                             + u_out |xs|: ONE rounding to the storage type, half an ulp at the exact value (2^-8 bf16,
                             2^-23 fp32).
    The constants are the operation counts; nothing is measured on a kernel.  -> (bound of x_out, bound of xs)."""
    from tests import parity as PR
    return 2 * PR.PER_TERM * ref["mag_x"], PR.U_OUT[st] * np.abs(ref["xs"]) + 4 * PR.PER_TERM * ref["mag_xs"]


def relu_shift(h, o, defect=None, stale=None):
    """out = relu(h - o) - o (fixup.py:45-50: shift, ReLU, shift, with the one offset of the scope).
    defect: second_shift_dropped  relu(h - o);  shift_inside_only  relu(h - o - o);  host_baked  o = stale."""
    if defect == "host_baked":
        o = stale
    o = 0.0 if o is None else float(o)
    h = np.asarray(h, np.float64)
    if defect == "second_shift_dropped":
        out = np.maximum(h - o, 0.0)
    elif defect == "shift_inside_only":
        out = np.maximum(h - o - o, 0.0)
    else:
        out = np.maximum(h - o, 0.0) - o
    return {"out": out, "mag": np.abs(h) + 2 * abs(o)}


def relu_shift_bound(ref, st):
    """Two fp32 roundings (the two differences; the ReLU is exact) on magnitudes within |h| + 2 |o|, and one rounding to the
    storage type:  u_out |out| + 2 * 2^-23 (|h| + 2 |o|)."""
    from tests import parity as PR
    return PR.U_OUT[st] * np.abs(ref["out"]) + 2 * PR.PER_TERM * ref["mag"]


def standin_residual(x, y, a, o, b, st):
    """torch float32 in another evaluation order: x_out = a y + x; xs = (b x_out) - (b o), rounded once.  -> (x_out, xs)."""
    f = lambda v, d: torch.tensor(d if v is None else float(v), dtype=torch.float32)
    a, o, b = f(a, 1.0), f(o, 0.0), f(b, 1.0)
    ref = x if x is not None else y
    xf = torch.zeros_like(ref.float()) if x is None else x.float()
    yf = torch.zeros_like(xf) if y is None else y.float()
    x_out = a * yf + xf
    return x_out, (b * x_out - b * o).to(st)


def standin_relu_shift(h, o, st):
    o = torch.tensor(0.0 if o is None else float(o), dtype=torch.float32)
    return (torch.relu(h.float() + (-o)) + (-o)).to(st)


# ---------------------------------------------------------------------------------------------- kernel-test cases
# name -> one direct call of zk_fixup_residual.  rows / H / ld: the shape (ld: row stride of every operand, > H = a column
# slice of a wider matrix); null: the arguments passed as NULL; alias: x_out is x; small: the branch is below half a bf16
# ulp of x everywhere.  The three shapes are the smallest that can go wrong: one row of one workgroup's worth of lanes; an
# odd number of rows of a width that is no multiple of 64 lanes' 8 columns, strided; more rows than a decode step has
# (several workgroups per row block, the widest hidden size the project decodes).
SCALARS = (1.25, 0.375, 0.8125)                    # a, o, b of every case; (0.5, -1.5, 2.0) after "a change"
STALE = (0.5, -1.5, 2.0)
CASES = OrderedDict([
    ("one_row", dict(rows=1, H=128, ld=128)),
    ("strided", dict(rows=5, H=136, ld=200)),
    ("wide", dict(rows=130, H=2048, ld=2048)),
    ("x_null", dict(rows=5, H=136, ld=200, null=("x", "scale"))),                 # the shift of an embedding
    ("y_null", dict(rows=5, H=136, ld=200, null=("y", "scale"))),
    ("xs_null", dict(rows=5, H=136, ld=200, null=("xs_out", "offset", "scale2"))),
    ("scale_null", dict(rows=5, H=136, ld=200, null=("scale",))),
    ("offset_null", dict(rows=5, H=136, ld=200, null=("offset",))),
    ("scale2_null", dict(rows=5, H=136, ld=200, null=("scale2",))),               # residual + the next shift
    ("final", dict(rows=5, H=136, ld=200, null=("x_out",))),                      # the encoder's last boundary
    ("alias", dict(rows=130, H=2048, ld=2048, alias=True, null=("scale2",))),
    ("small_update", dict(rows=5, H=136, ld=200, small=True, null=("scale2",))),
])
FFN_CASES = OrderedDict([("one_row", dict(rows=1, H=128, ld=128)), ("strided", dict(rows=5, H=136, ld=200)),
                         ("wide", dict(rows=130, H=2048, ld=2048)), ("offset_null", dict(rows=5, H=136, ld=200, null=("offset",)))])


def case_inputs(name, form, seed=0, ffn=False):
    """-> dict x (fp32 values) / y (values exactly representable in the storage type of `form`) [rows, H] torch float32, the
    scalars a, o, b (None where the case passes NULL), or h / o for a feed-forward case."""
    cs = (FFN_CASES if ffn else CASES)[name]
    st = V.STORAGE[form]
    g = torch.Generator().manual_seed(7100 + seed + sum(map(ord, name)) + (1000 if ffn else 0))
    rows, H = cs["rows"], cs["H"]
    null = cs.get("null", ())
    if ffn:
        return {"h": torch.randn(rows, H, generator=g).to(st).float(), "o": None if "offset" in null else SCALARS[1]}
    x = torch.randn(rows, H, generator=g) * 3.0
    y = torch.randn(rows, H, generator=g)
    if cs.get("small"):
        # |x| in [1, 2): half a bf16 ulp of x is 2^-9; the branch a y is at most 1.25 * 2^-11
        x = 1.0 + torch.rand(rows, H, generator=g) * 0.99
        y = (torch.rand(rows, H, generator=g) * 0.5 + 0.5) * 2.0 ** -11
    a, o, b = SCALARS
    return {"x": None if "x" in null else x, "y": None if "y" in null else y.to(st).float(),
            "a": None if "scale" in null else a, "o": None if "offset" in null else o, "b": None if "scale2" in null else b}


def case_reference(name, x, form, defect=None, ffn=False):
    st = V.STORAGE[form]
    n = lambda t: None if t is None else t.double().numpy()
    if ffn:
        return relu_shift(n(x["h"]), x["o"], defect=defect, stale=STALE[1])
    return residual(n(x["x"]), n(x["y"]), x["a"], x["o"], x["b"], st=st, defect=defect, stale=STALE)


# ---------------------------------------------------------------------------------------------- ref_torch model
class _NoBias(dict):
    """The parameters as rt.dot_attention reads them: a linear map of this model has no b_0, adding 0.0 is exact."""

    def __missing__(self, key):
        if key.endswith("/b_0"):
            return 0.0
        raise KeyError(key)


def _boundary(x, y, P, scale, offset, scale2=None):
    """What one zk_fixup_residual launch computes: the stream stays unrounded (fp32 on the device in both modes), the
    shifted operand rows are stored (site "ln": they stand where the LayerNorm output stood)."""
    if y is not None:
        x = x + y * P[scale]
    xs = x - P[offset]
    if scale2 is not None:
        xs = xs * P[scale2]
    return x, rt._st(xs, "ln")


def _ffn(xs, P, scope):
    """fixup.py:29-55 behind its first shift (already in xs): enlarge, shift, ReLU, shift (the SAME offset), output."""
    o = P[scope + "/ffn_layer/shift/offset"]
    h = rt.linear(xs, P, scope + "/ffn_layer/enlarge", bias=False)
    h = rt._st(torch.relu(h - o) - o, "linear")
    return rt.linear(h, P, scope + "/ffn_layer/output", bias=False)


def _sublayers(side, n, cross):
    out = []
    for l in range(n):
        pre = "%s/layer_%d" % (side, l)
        out.append((pre + "/self_attention", pre + "/self_attention", "sa", l))
        if cross:
            out.append((pre + "/cross_attention", pre + "/cross_attention", "ca", l))
        out.append((pre + "/feed_forward/ffn_layer", pre + "/feed_forward", "ff", l))
    return out


def _stack(x0, P, subs, run, final_offset, final_scale2):
    """x0: the stored embedding rows.  run(kind, scope, l, xs) -> the sub-layer's output before its scale."""
    if not subs:
        return _boundary(x0, None, P, None, final_offset, final_scale2)[1]
    x, xs = _boundary(x0, None, P, None, subs[0][0] + "/shift/offset")
    for i, (pair, scope, kind, l) in enumerate(subs):
        y = run(kind, scope, l, xs)
        if i + 1 < len(subs):
            x, xs = _boundary(x, y, P, pair + "/scale/scale", subs[i + 1][0] + "/shift/offset")
        else:
            x, xs = _boundary(x, y, P, pair + "/scale/scale", final_offset, final_scale2)
    return xs


def encoder(source, hp, P):
    """models/transformer_fixup.py:16-88."""
    dt = P["bias"].dtype
    H = hp.hidden_size
    Pz = _NoBias(P)
    mask = (source != 0).to(dt)
    source, mask = rt.remove_invalid_seq(source, mask)
    x = rt._st_fwd(P[rt._emb_name(hp, "src")])[source] * (H ** 0.5) + P["bias"]
    x0 = rt._st(x + rt.timing_signal(x.shape[1], x.shape[2], dt), "embed")
    bias = rt.attention_bias(mask, "masking")

    def run(kind, scope, l, xs):
        if kind == "ff":
            return _ffn(xs, P, scope)
        return rt.dot_attention(xs, None, bias, H, Pz, scope, hp.num_heads)["output"]
    out = _stack(x0, P, _sublayers("encoder", hp.num_encoder_layer, False), run, "encoder/shift/offset", "encoder/scale/scale")
    return {"encodes": out, "decoder_initializer": V.empty_caches(out.shape[0], H, hp.num_decoder_layer, dt), "mask": mask}


def _decoder_layers(x0, state, hp, P, self_bias, caches):
    H, nh = hp.hidden_size, hp.num_heads
    Pz = _NoBias(P)
    mem_bias = rt.attention_bias(state["mask"], "masking")

    def run(kind, scope, l, xs):
        if kind == "ff":
            return _ffn(xs, P, scope)
        lc = None if caches is None else caches["layer_%d" % l]
        if kind == "sa":
            r = rt.dot_attention(xs, None, self_bias, H, Pz, scope, nh, cache=lc)
        else:       # the memory is the encoder's scaled, shifted output: not shifted again (transformer_fixup.py:73, 160)
            r = rt.dot_attention(xs, state["encodes"], mem_bias, H, Pz, scope, nh, cache=lc)
        if lc is not None:
            lc.update(r["cache"])
        return r["output"]
    feat = _stack(x0, P, _sublayers("decoder", hp.num_decoder_layer, True), run, "decoder/shift/offset", None)
    return torch.matmul(feat.reshape(-1, hp.embed_size), rt._st_fwd(P[rt._emb_name(hp, "softmax")]).t())


def decoding_fns(hp, P):
    """(encoding_fn, decoding_fn) of models/transformer_fixup.py:261-294 (search_mode = cache) for rt.beam_search."""
    hp = rt.closing_dropout(copy.copy(hp))

    def encoding_fn(source):
        return V.cached_state(encoder(source, hp, P))

    def decoding_fn(target, state, time):
        x0 = V.embed_step(target, time, hp, P)
        logits = _decoder_layers(x0, state, hp, P, rt.attention_bias(1, "causal").to(P["bias"].dtype), state["decoder"]["state"])
        return logits, state

    return encoding_fn, decoding_fn


def full_decoder(target, state, hp, P):
    """The training-path decoder (models/transformer_fixup.py:91-203 with is_training): shifted inputs, causal bias.
    target [B, Lt] -> logits [B, Lt, V]."""
    x0 = V.embed_shifted(target, hp, P)
    logits = _decoder_layers(x0, state, hp, P, rt.attention_bias(target.shape[1], "causal").to(P["bias"].dtype), None)
    return logits.reshape(target.shape[0], target.shape[1], -1)


def score(hp, Pn, src, tgt, dtype=torch.float64, store_bf16=False):
    """score_fn (models/transformer_fixup.py:244-258): per-sample cross entropy without label smoothing over the target
    positions that are not padding.  -> float64 numpy [B]."""
    hp = rt.closing_dropout(copy.copy(hp))
    P = rt.to_torch(Pn, dtype=dtype)
    with V.storage_model(store_bf16), torch.no_grad():
        target = torch.as_tensor(tgt)
        mask = (target != 0).to(dtype)
        target, mask = rt.remove_invalid_seq(target, mask)
        logits = full_decoder(target, encoder(torch.as_tensor(src), hp, P), hp, P)
        ce = -torch.log_softmax(logits, dim=-1).gather(-1, target[..., None])[..., 0]
        return ((ce * mask).sum(-1) / mask.sum(-1)).double().numpy()


def param_names(hp):
    """[(name, shape, kind)] written out from models/transformer_fixup.py and modules/fixup.py in creation order.  kind:
    embed, vec, offset, scale, att (x L^-1/6), ffn (x L^-1/2); the zero-initialised ones are marked by a trailing 0."""
    H, F = hp.hidden_size, hp.filter_size
    shared = hp.shared_source_target_embedding
    out = [("embedding" if shared else "src_embedding", (hp.src_vocab.size(), H), "embed", None), ("bias", (H,), "vec", None)]

    def att(p, maps, l):
        a = p + "/dot_attention/"
        return [(p + "/shift/offset", (1,), "offset", l)] + [(a + m + "/W_0_0", (H, w), "att", l) for m, w in maps] + \
            [(a + "o_map/W_0_0", (H, H), "att0", l), (p + "/scale/scale", (1,), "scale", l)]

    def ffn(p, l):
        f = p + "/ffn_layer/"
        return [(f + "shift/offset", (1,), "offset", l), (f + "enlarge/W_0_0", (H, F), "ffn", l),
                (f + "output/W_0_0", (F, H), "ffn0", l), (f + "scale/scale", (1,), "scale", l)]
    for l in range(hp.num_encoder_layer):
        out += att("encoder/layer_%d/self_attention" % l, [("qkv_map", 3 * H)], l) + ffn("encoder/layer_%d/feed_forward" % l, l)
    out += [("encoder/shift/offset", (1,), "offset", None), ("encoder/scale/scale", (1,), "scale", None)]
    if not shared:
        out.append(("tgt_embedding", (hp.tgt_vocab.size(), H), "embed", None))
    for l in range(hp.num_decoder_layer):
        out += att("decoder/layer_%d/self_attention" % l, [("qkv_map", 3 * H)], l)
        out += att("decoder/layer_%d/cross_attention" % l, [("q_map", H), ("k_map", H), ("v_map", H)], l)
        out += ffn("decoder/layer_%d/feed_forward" % l, l)
    out.append(("decoder/shift/offset", (1,), "offset", None))
    if not shared and not hp.shared_target_softmax_embedding:
        out.append(("softmax_embedding", (hp.tgt_vocab.size(), H), "embed0", None))
    return out


def init_params(hp, seed):
    """Every parameter matters: the zero-initialised matrices (o_map, the FFN output, a separate softmax_embedding) are drawn
    like their non-zero siblings (the scope initialiser times L^-1/6 or L^-1/2, the layer initialiser under
    deep_transformer_init; embeddings N(0, H^-1/2)), offsets ~ N(0, 0.1), scales ~ 1 + N(0, 0.1)."""
    rng = np.random.default_rng(seed)
    L = 2 * hp.num_encoder_layer + 3 * hp.num_decoder_layer
    Pn = OrderedDict()
    for name, shape, kind, l in param_names(hp):
        if kind.startswith("embed"):
            v = rng.normal(0.0, hp.hidden_size ** -0.5, size=shape)
        elif kind == "offset":
            v = rng.normal(0.0, 0.1, size=shape)
        elif kind == "scale":
            v = 1.0 + rng.normal(0.0, 0.1, size=shape)
        else:
            if l is not None and hp.deep_transformer_init:
                v = rt._scope_init(rng, shape, "uniform_unit_scaling", hp.initializer_gain * (l + 1) ** -0.5)
            else:
                v = rt._scope_init(rng, shape, hp.initializer, hp.initializer_gain)
            v = v * (L ** (-1.0 / 6.0) if kind.startswith("att") else L ** (-1.0 / 2.0) if kind.startswith("ffn") else 1.0)
        Pn[name] = np.asarray(v, np.float32)
    return Pn


def make_fixture(hp, src, seed, factor=4.0):
    """The tiny model of the GPU model tests, with the proof that the REFERENCE ALONE is far from a tie on it
    (variant_ref.candidate_margin, beam 1 and 4): the float64 and the fp32 run of the restated reference give identical
    hypotheses and candidate orders, and the smallest gap between a kept candidate and its runner-up exceeds factor x the
    largest fp32 - float64 score difference.
    -> dict Pn, gap, err (the worst over both beams)."""
    Pn = init_params(hp, seed)
    return dict(V.candidate_margin(functools.partial(V.search, decoding_fns), hp, Pn, src, factor=factor, seed=seed), Pn=Pn)


# ---------------------------------------------------------------------------------------------- the GPU model tests' fixture
FIXTURE_SEED = 45                 # chosen among 41 .. 52 for the widest gap / err (tests/test_gpu_fixup_model.py quotes it)
FIXTURE_LENGTHS = (14, 5, 9, 11)
TARGET_LENGTHS = (10, 4, 7, 6)
SOURCE_SEED, TARGET_SEED = 5, 9     # variant_ref.ragged(FIXTURE_LENGTHS, Vs, SOURCE_SEED) / (TARGET_LENGTHS, Vt, TARGET_SEED)
# largest relative error of score() under ref_torch's bf16 storage model against its float64 run on the fixture (measured on
# the CPU; tests/test_fixup_host.py re-measures it): the floor the device's bf16 score_fn is held to 4 x of
SCORE_FLOOR = 4.966e-4
