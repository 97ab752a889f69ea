# coding: utf-8
"""``deepnmt`` at inference: the encoder stack and the cached decoder step on the kernels of zero_amd/csrc/zk_rnn.hip, in the
bf16 mode and in ``decode_dtype=float32``, for ``cell`` in {atr, gru, lrn, olrn}.

Reference: models/deepnmt.py:16-100 (encoder), 103-194 (decoder); rnns/rnn.py (rnn, cond_rnn); rnns/atr.py, rnns/gru.py,
rnns/cell.py; func.py:14-65, 107-161, 289-303.  With carry(m, a, b) = m a + (1 - m) b, NE = num_encoder_layer, ND =
num_decoder_layer, ff_l(o) = o W_ff,l + b_ff,l:

  encoder   x_t = src_emb[source_t] + bias                              (no scale, no timing signal; one `bias` for both sides)
            layer l:   f_t = carry(m_t, cell_f(f_{t-1}, x_t), f_{t-1})                                       t = 0 .. Ls-1
              l = 0, caencoder:   s = carry(m_t, lower(g, x_t), g);  g = carry(m_t, higher(s, f_t), s);  y_t = g   t = Ls-1 .. 0
              l = 0, otherwise:   b_t the plain backward scan;  y_t = [f_t | b_t]
              l >= 1:             y_t = f_t
              x_t = x_t + ff_l(y_t)
            z = the state after the last scanned position of layer NE - 1 (g_0; [f_{Ls-1} | b_0]; f_{Ls-1})
            memory = x, or LayerNorm(x W_map + b_map) when embed_size != hidden_size: H wide in every case
            h0_l = z W_init,l + b_init,l  (NO tanh);   pm_l = memory W_ca,l for every attention-form layer (once per batch)
  step      x = tgt_emb[tok] + bias (zeros when every token is pad)
            layer l, by form:
              attention (l = 0; every l under use_deep_att):
                          s = lower(h_l, x);  qa = s Wq + bq;  c = add_attention(qa, pm_l, memory, v, mask);  h_l' = higher(s, c)
              one-to-one (caencoder, l >= 1):      s = lower(h_l, x);  h_l' = higher(s, c)
              plain (no caencoder, l >= 1):        h_l' = cell(h_l, [x | c])
              x = x + ff_l(h_l')
            feature = tanh([x | c] W_ff + b_ff) with dl4mt_redict, else x;   logits = feature E^T

The residual stream x is fp32 in BOTH modes (with layer_norm off nothing re-normalises it); ff, bias
and the add are ONE launch (zk_rnn_ff_residual), which also writes x in the storage type where the next product reads it: the
x columns of one [x | c] buffer, whose c columns the attention writes.  In the fp32 mode the stream IS those x columns and the
launch runs in place.  Launches of a captured step, without the search's own (n_p = n_c = 1 for atr, 2 for gru):
  embed                1 (fp32), 2 (bf16: the fp32 stream and its bf16 copy)
  attention-form layer 2 n_p + 2 n_c + 2 (feed_query, attention) + 1 (ff)
  one-to-one layer     2 n_p + 2 n_c + 1
  plain layer          n_p + n_c + 1
  tail                 3 with dl4mt_redict (product, tanh, logits), else 1
With lrn / olrn (n_p = n_c = 1, no recurrent product: models/_deepatt.py Cells) a one-to-one layer is 2 projections + ONE paired
launch + 1, and every scan of the encoder -- plain or one-to-one pair -- is one launch whatever Ls.

The state is one fp32 ping-pong pair [BK, H] per decoder layer (DeepNmtState); the beam reorder is the row index of every
layer's first cell launch.  A step that follows no reorder (time 0 of the host-side search, an eager decoding_fn call) reads
the current half with rows as they are and writes the other: a plain-form layer is ONE cell launch, and the cell launches
refuse an output that overlaps the state they read.
"""

import numpy as np
import torch

from zero_amd.func import Mat
from zero_amd.models import _decode as _dec
from zero_amd.models import _decode_f32 as _f32
from zero_amd.models._deepatt import GRU_MAX_H, Cells, _ops
from zero_amd.models._rnnsearch import RN, RnnSearchCore, RnnState, _at
from zero_amd.utils import dtype as zdtype

F32 = torch.float32


class DeepNmtCore(RnnSearchCore):
    """RnnSearchCore with this model's sizes: the memory is H wide, NE encoder and ND decoder layers."""

    def __init__(self, params, model_name, store=None, device=None):
        RnnSearchCore.__init__(self, params, model_name, store, device)
        self.M = self.H
        self.cell = str(params.cell).lower()
        self.NE, self.ND = int(params.num_encoder_layer), int(params.num_decoder_layer)
        self.deep_att, self.redict = bool(params.use_deep_att), bool(params.dl4mt_redict)

    def form(self, l):
        """The form of decoder layer l: "att", "one2one" or "plain" (models/deepnmt.py:140-162)."""
        if l == 0 or self.deep_att:
            return "att"
        return "one2one" if self.ca else "plain"


def check_shape(core, f32):
    """The sizes the kernels take; nothing here depends on the data, so encoding_fn refuses before the encoder pass."""
    H, E = core.H, core.E
    if not f32 and (H % 8 != 0 or E % 8 != 0):
        raise ValueError("deepnmt in bf16 needs hidden_size and embed_size to be multiples of 8 -- got %d and %d -- (rows are "
                         "loaded 16 bytes at a time); decode_dtype=float32 takes these sizes" % (H, E))
    if f32 and (H % 4 != 0 or E % 4 != 0):
        raise ValueError("deepnmt with decode_dtype=float32 needs hidden_size and embed_size to be multiples of 4 -- got %d "
                         "and %d -- (zk_f32_gemm reads rows 16 bytes at a time)" % (H, E))
    if H > 2048:
        raise ValueError("deepnmt: the additive attention kernel takes a memory width of at most 2048, and the bf16 ff of "
                         "encoder layer 0 a [forward | backward] input of at most 4096 (got hidden_size %d)" % H)
    if not f32 and core.cell == "gru" and H > GRU_MAX_H:
        raise ValueError("deepnmt with cell=gru in bf16 takes a hidden_size of at most %d (got %d); decode_dtype=float32 "
                         "has no such limit" % (GRU_MAX_H, H))


def embed(core, o, ids, rows, name, xs, xc, pad=-1):
    """The embedding lookup into the fp32 stream xs and its storage-type copy xc (in the fp32 mode they are one Mat)."""
    e = core.eng
    e.rnn_embed(ids, rows, o.table(name), o.b("bias"), xc, pad=pad)
    if xs is not xc:
        e.rnn_embed(ids, rows, core.store.w(name), o.b("bias"), xs, pad=pad)


def ff_residual(o, pre, a, xs, xc):
    """x = x + linear(a, embed_size, scope=pre + "ff") on the fp32 stream, in place, with its storage-type copy."""
    o.e.rnn_ff_residual(a, o.W(pre + "ff/W_0_0"), o.b(pre + "ff/b_0"), xs, xs, None if xs is xc else xc)


def encode(core, o, batch, K):
    """-> (memory Mat [B * Ls, H], [projected memory Mat [B * Ls, H] or None per decoder layer]); writes h0_l into layer l's
    state buffer of parity 0, tiled K times per sentence."""
    e, H, E, NE, ND, c, ca = core.eng, core.H, core.E, core.NE, core.ND, core.cell, core.ca
    f32 = o.storage.dtype == F32
    esz = o.storage.esz
    B, Ls = batch["B"], batch["Ls"]
    T = B * Ls
    smask = batch["smask"]
    mask_at = lambda t: Mat(smask, B, 1, Ls, t)
    at = lambda inp, t: tuple(_at(m, B, t, Ls) for m in inp)
    cells = Cells(core, o)
    whole = Mat(smask, B, Ls, Ls)
    xc = o.mat("enc.x", T, E)
    xs = xc if f32 else o.mat("enc.xs", T, E, F32)
    embed(core, o, batch["src"], T, core.src_emb, xs, xc)
    hs = [Mat(e.buf(o.pre + "enc.h%d" % i, (B, H), F32), B, H) for i in (0, 1)]
    hf = o.mat("enc.hf", T, H)
    y2 = None if ca else o.mat("enc.y2", T, 2 * H)           # [forward | backward] of layer 0

    def scan(pre, s, x, reverse, dest, tag):
        """A plain rnn.rnn scan of x from the zero state, over t = Ls-1 .. 0 with `reverse`; dest: the [B * Ls, H] Mat (maybe a
        column slice) that takes every position's state in the storage type."""
        inp = cells.fetch(x, pre, s, tag)
        if cells.lrn:
            cells.scan(inp, None, hs[0], dest, whole, Ls, reverse)
            return
        prev = None
        for n, t in enumerate(range(Ls - 1, -1, -1) if reverse else range(Ls)):
            cells.step(pre, s, prev, at(inp, t), hs[n & 1], _at(dest, B, t, Ls), mask=mask_at(t), tag="enc.")
            prev = hs[n & 1]
    for l in range(NE):
        pre = "encoder/layer_%d/" % l
        first = l == 0
        fw = y2.cols_slice(0, H) if first and not ca else hf
        scan(pre + "forward/", c, xc, False, fw, "enc.lo")
        y = fw
        if first and ca:              # cond_rnn(one2one=True) on the reversed sequence: the lower cell on x_t, the higher on f_t
            b = pre + "backward/"
            y = o.mat("enc.g", T, H)
            lo = cells.fetch(xc, b, c + "_lower", "enc.lo")
            hi = cells.fetch(hf, b, c + "_higher", "enc.hi")
            g, s = hs
            if cells.lrn:
                cells.scan(lo, hi, g, y, whole, Ls, True)
            else:
                for t in range(Ls - 1, -1, -1):
                    cells.step(b, c + "_lower", None if t == Ls - 1 else g, at(lo, t), s, mask=mask_at(t), tag="enc.")
                    cells.step(b, c + "_higher", s, at(hi, t), g, _at(y, B, t, Ls), mask=mask_at(t), tag="enc.")
        elif first:
            bw = y2.cols_slice(H, 2 * H)
            scan(pre + "backward/", c, xc, True, bw, "enc.lo")
            y = y2
        if l == NE - 1:               # z: the state after the last scanned position, before y's buffer is used again
            if first and ca:
                z = _at(y, B, 0, Ls)
            elif first:
                z = o.mat("enc.z", B, 2 * H)
                for t, c0 in ((Ls - 1, 0), (0, H)):        # [f_{Ls-1} | b_0]
                    src = _at(y2, B, t, Ls, c0, H)
                    e.lib.call("zk_gather_rows", src.ptr, src.ld * esz, None, z.ptr + c0 * esz, 2 * H * esz, B, H * esz,
                               e.stream)
            else:
                z = _at(y, B, Ls - 1, Ls)
        ff_residual(o, pre, y, xs, xc)
    if E != H:                        # layer_norm(linear(x, hidden_size, scope="x_map")), models/deepnmt.py:83-84
        enc = o.mat("enc", T, H)
        xm = o.project(xc, "x_map/W_0_0", o.mat("enc.xm", T, H, F32), bias=o.b("x_map/b_0"))
        ln = enc if f32 else o.mat("enc.ln", T, H, F32)
        e.lib.call("zk_f32_add_ln", xm.ptr, None, o.b("layer_norm/scale").data_ptr(), o.b("layer_norm/offset").data_ptr(),
                   ln.ptr, T, H, zdtype.epsilon(), e.stream)
        if not f32:
            e.lib.call("zk_cast_f32_bf16", ln.ptr, enc.ptr, T * H, e.stream)
    else:
        enc = xc
    rep = e.buf(o.pre + "enc.rep", (B * K,), torch.int32)
    e.h2d(rep, np.repeat(np.arange(B, dtype=np.int32), K))
    pms = []
    for l in range(ND):
        i = "layer_%d_init/" % l          # (at model scope: models/deepnmt.py:91-98 runs outside `decoder_initializer`)
        h0 = o.project(z, i + "W_0_0", o.mat("enc.init", B, H, F32), bias=o.b(i + "b_0"))
        state0 = e.buf(o.pre + "hs.l%d.0" % l, (B * K, H), F32)
        e.buf(o.pre + "hs.l%d.1" % l, (B * K, H), F32)
        e.lib.call("zk_gather_rows", h0.ptr, H * 4, rep.data_ptr(), state0.data_ptr(), H * 4, B * K, H * 4, e.stream)
        pms.append(o.project(enc, "decoder/layer_%d/context_att/W_0_0" % l, o.mat("pm.l%d" % l, T, H))
                   if core.form(l) == "att" else None)
    return enc, pms


class DeepNmtState(RnnState):
    """RnnState with one fp32 ping-pong pair [BK, H] per decoder layer: state["decoder"]["state"]["layer_l"].  reorder() hands
    the row index to the first cell launch of every layer."""

    def _half(self, pp, l=0):
        core = self["_core"]
        return Mat(core.eng.buf(self.storage.prefix + RN + "hs.l%d.%d" % (l, pp), (self["BK"], core.H), F32), self["BK"], core.H)

    def reorder(self, index_dev, time_dev=None, defer_aan=False):
        pp = self["_pp"]
        self["_gather"] = ([self._half(pp, l) for l in range(self["_core"].ND)], index_dev)
        self["_pp"] = 1 - pp
        self.bind_caches()

    def bind_caches(self):
        self["decoder"]["state"] = {"layer_%d" % l: self._half(self["_pp"], l) for l in range(self["_core"].ND)}


def step(state, target, time, time_dev, hp):
    """One cached decoder step -> (logits Mat fp32 [BK, Vpad], state)."""
    core = state["_core"]
    o = _ops(core, state["f32"])
    f32 = o.storage.dtype == F32
    e, H, E, c = core.eng, core.H, core.E, core.cell
    BK, K, Ls = state["BK"], state["K"], state["Ls"]
    if time_dev is None and time >= state["Tmax"]:
        raise RuntimeError("decode step %d exceeds the allocated cache length %d" % (time, state["Tmax"]))
    if "_gather" not in state:        # no reorder since the last step: the current half with rows as they are -> the other half
        state.reorder(None)
    srcs, idx = state.pop("_gather")
    cells = Cells(core, o)
    xcc = o.mat("xc", BK, E + H)                      # [x | c]: the operand of a plain-form cell and of the dl4mt ff
    xc, cc = xcc.cols_slice(0, E), xcc.cols_slice(E, E + H)
    xs = xc if f32 else o.mat("xs", BK, E, F32)
    embed(core, o, target, BK, core.tgt_emb, xs, xc, pad=hp.tgt_vocab.pad())
    s = o.mat("s", BK, H, F32)
    sc = o.mat("sc", BK, H)
    hc = o.mat("hc", BK, H)                           # a layer's new state in the storage type: the operand of its ff
    for l in range(core.ND):
        pre = "decoder/layer_%d/" % l
        src, dst = srcs[l], state["decoder"]["state"]["layer_%d" % l]
        form = core.form(l)
        if form == "plain":
            cells.step(pre, c, src, cells.fetch(xcc, pre, c, "lo"), dst, hc, idx=idx)
        elif form == "one2one" and cells.lrn:         # no attention between the two cells: ONE paired launch
            cells.pair(src, cells.fetch(xc, pre, c + "_lower", "lo"), cells.fetch(cc, pre, c + "_higher", "hi"), dst, hc, idx)
        else:
            att = form == "att"
            cells.step(pre, c + "_lower", src, cells.fetch(xc, pre, c + "_lower", "lo"), s, sc if att else None, idx=idx)
            if att:
                a = pre + "attention/"
                qa = o.project(sc, a + "feed_query/W_0_0", o.mat("qa", BK, H), bias=o.b(a + "feed_query/b_0"))
                v = o.b(a + "feed_logits/W_0_0")
                if f32:       # the fp32 context is of the storage type already: no separate fp32 buffer
                    e.add_attn(qa, state["pms"][l], state["encodes"], v, state["mask"], cc, None, K, Ls)
                else:
                    e.add_attn(qa, state["pms"][l], state["encodes"], v, state["mask"], o.mat("ctx", BK, H, F32), cc, K, Ls)
            cells.step(pre, c + "_higher", s, cells.fetch(cc, pre, c + "_higher", "hi"), dst, hc)
        ff_residual(o, pre, hc, xs, xc)
    if core.redict:
        pre = o.project(xcc, "ff/W_0_0", o.mat("pre", BK, E, F32))
        feat = o.mat("feat", BK, E)
        e.rnn_bias_tanh(pre, o.b("ff/b_0"), out_copy=feat, f32=f32)
    else:
        feat = xc
    logits = o.mat("logits", BK, core.Vpad, F32)
    o.gemm(feat, o.W(core.soft_emb), logits, BK, core.V, E, 1)
    if time_dev is None:
        state["time_filled"] = time + 1
    return logits, state


def build_state(core, hp, source, K, max_steps):
    """encoding_fn: source batch -> DeepNmtState, as models/_rnnsearch.py:build_state (source padding and the rounding of the
    step count follow models/_decode.py: a padded position has mask 0, so every scan carries the state over it and the
    attentions give it the weight 0)."""
    f32 = _f32.wanted(hp)
    check_shape(core, f32)
    o = _ops(core, f32)
    e = core.eng
    batch, max_steps = _dec.shape_batch(core, hp, source, max_steps)
    B, Ls = batch["B"], batch["Ls"]
    enc, pms = encode(core, o, batch, K)
    mask_keep = e.buf(o.pre + "smask", (B, Ls), F32)
    mask_keep.copy_(batch["smask"])
    state = DeepNmtState()
    state.storage = o.storage
    state.update({"_core": core, "B": B, "K": K, "BK": B * K, "Ls": Ls, "Tmax": max_steps, "encodes": enc, "pm": pms[0],
                  "pms": pms, "mask": mask_keep, "time_filled": 0, "decoder": {}, "f32": f32, "_pp": 0})
    state.bind_caches()
    return _dec.finish_state(state)


def make_infer_fns(params, model_name):
    hp = params
    from zero_amd.models._factory import get_core

    def encoding_fn(source, beam_size=None, max_steps=None):
        core = get_core(hp, model_name)
        return build_state(core, hp, source, hp.beam_size if beam_size is None else beam_size, max_steps)

    def step_static(state, temperature, forbid_value):
        _dec.static_step(state, hp, lambda st, time_dev: step(st, st["tok"], None, time_dev, hp)[0], True, temperature,
                         forbid_value)

    def decoding_fn(target, state, time):
        return step(state, target, time, None, hp)

    decoding_fn.step_static = step_static
    return encoding_fn, decoding_fn
