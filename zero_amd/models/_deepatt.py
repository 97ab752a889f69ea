# coding: utf-8
"""``rnnsearch_deepatt`` at inference: the encoder stack and the cached deep-attention decoder step on the kernels of
zero_amd/csrc/zk_rnn.hip, in the bf16 mode and in ``decode_dtype=float32``, for ``cell`` in {atr, gru, lrn, olrn}.

Reference: models/rnnsearch_deepatt.py:68-128, 132-236, 240-303; rnns/rnn.py (rnn, cond_rnn one2one); rnns/atr.py, rnns/gru.py,
rnns/cell.py; func.py:14-65, 107-161.  With carry(m, a, b) = m a + (1 - m) b, NE = num_encoder_layer, D = num_decoder_layer:

  encoder   x_t = src_emb[source_t] + bias                              (no scale, no timing signal; one `bias` for both sides)
            layer 0:        h0_t = carry(m_t, cell(h0_{t-1}, x_t), h0_{t-1})                              t = 0 .. Ls-1
            layer l >= 1:   s = carry(m_t, lower_l(g, x_t), g);  g = carry(m_t, higher_l(s, h^{l-1}_t), s);  h^l_t = g
                            from the zero state, t = Ls-1 .. 0 for odd l and 0 .. Ls-1 for even l (positions stay un-reversed)
            memory = h^NE (width H);  feature = the state after the last scanned position of layer NE
            h_0 = feature W_init + b_init  (NO tanh);   pm = memory W_ca  (once per batch, shared by all D attentions)
  step      y = tgt_emb[tok] + bias (zeros when every token is pad);  s = lower(h, y)
            l = 0 .. D-1:   qa = s Wq_l + bq_l;  c_l = add_attention(qa, pm, memory, v_l, mask);  s = higher_l(s, c_l)
            h' = s;   logits = tanh([h', c_0 .. c_{D-1}, y] W_ff + b_ff) E^T

A cell is its input projections (products over all rows at once) and its recurrence per time step:
  atr   p = x Wp;                      one launch  (zk_rnn_atr_step)
  gru   xg = x Wg [., 2 H], xh = x Wh;  two launches (zk_rnn_gru_gates, zk_rnn_gru_out: Engine.rnn_gru_step)
  lrn   [p | q | r] = x W [., 3 H];  olrn  [p | q | r | s] = x W [., 4 H]      (rnns/lrn.py, rnns/olrn.py: NO recurrent product)
        one launch for a WHOLE scan, single or lower / higher pair (zk_rnn_lrn_scan: Engine.rnn_lrn_scan); a step is T = 1
`Cells` is that dispatch, shared by encode() and step().  Launches of a captured decoder step (without the search's own):
  atr, lrn, olrn   embed, 1 projection, lower cell, D x (feed_query, attention, 1 projection, higher cell), ff, tanh, logits
        = 6 + 4 D
  gru   embed, 2 projections, 2 cell launches, D x (feed_query, attention, 2 projections, 2 cell launches), ff, tanh, logits
        = 8 + 6 D
and of the encoder: 1 embed + (1 + 2 NE) x n_p projections + (1 + 2 NE) x Ls x n_c cell launches (n_p = n_c = 1 for atr, 2 for
gru) + the initial state (1 product, 1 row gather) + the projected memory.  With lrn / olrn the cell launches of the encoder
are 1 + NE scans, whatever Ls: 1 embed + (1 + 2 NE) projections + (1 + NE) scans + the same tail.

The state is models/_rnnsearch.py's: a ping-pong pair of fp32 [BK, H] buffers (RnnState), the beam reorder is the row index
of the step's first cell launch.  The attention contexts and the final state are written straight into column slices of one
[BK, H + D H + E] buffer in the order [h' | c_0 .. c_{D-1} | y], so ff is one product.
"""

import numpy as np
import torch

from zero_amd.func import Mat
from zero_amd.models import _decode as _dec
from zero_amd.models import _decode_f32 as _f32
from zero_amd.models._ops import ops_for
from zero_amd.models._rnnsearch import RN, RnnSearchCore, RnnState, _at

F32 = torch.float32
GRU_MAX_H = 2048        # zk_rnn_gru_gates: the LDS image of its columns of the gate matrix (include/zero_hip.h)
LRN_CELLS = ("lrn", "olrn")      # the cells without a recurrent product: a whole scan is one launch


class DeepAttCore(RnnSearchCore):
    """RnnSearchCore with this model's sizes: the memory is H wide, NE conditional encoder layers, D attention layers."""

    def __init__(self, params, model_name, store=None, device=None):
        RnnSearchCore.__init__(self, params, model_name, store, device)
        self.ca, self.M = True, self.H
        self.cell = str(params.cell).lower()
        self.NE, self.D = int(params.num_encoder_layer), int(params.num_decoder_layer)


def check_shape(core, f32):
    """The sizes the kernels take; nothing here depends on the data, so encoding_fn refuses before the encoder pass."""
    H, E = core.H, core.E
    if not f32 and (H % 8 != 0 or E % 8 != 0):
        raise ValueError("rnnsearch_deepatt in bf16 needs hidden_size and embed_size to be multiples of 8 -- got %d and %d -- "
                         "(rows are loaded 16 bytes at a time); decode_dtype=float32 takes these sizes" % (H, E))
    if f32 and (H % 4 != 0 or E % 4 != 0):
        raise ValueError("rnnsearch_deepatt with decode_dtype=float32 needs hidden_size and embed_size to be multiples of 4 "
                         "-- got %d and %d -- (zk_f32_gemm reads rows 16 bytes at a time)" % (H, E))
    if H > 2048:
        raise ValueError("rnnsearch_deepatt: the additive attention kernel takes a memory width of at most 2048 (got "
                         "hidden_size %d)" % H)
    if not f32 and core.cell == "gru" and H > GRU_MAX_H:
        raise ValueError("rnnsearch_deepatt with cell=gru in bf16 takes a hidden_size of at most %d (got %d); "
                         "decode_dtype=float32 has no such limit" % (GRU_MAX_H, H))


def _ops(core, f32):
    return ops_for(core, f32, (_dec.F32_CACHES if f32 else _dec.BF16_CACHES).prefix + RN)


class Cells(object):
    """The cell of the model (core.cell) on the ops `o`: fetch() = the input projections of a whole block of rows,
    step() = one time step; for lrn / olrn also scan() = a whole scan and pair() = one step of a lower / higher pair, each
    ONE launch.  `tag` names the buffers, so that the encoder's and the step's never alias."""

    def __init__(self, core, o):
        self.c, self.o, self.e, self.H = core.cell, o, core.eng, core.H
        self.lrn, self.gated = self.c in LRN_CELLS, self.c == "olrn"

    def fetch(self, x, pre, s, tag):
        """rnns/{atr,gru,lrn,olrn}.py fetch_states of the scope pre + "fetch_state_<s>" on x: Mat [rows, in] -> the tuple of
        Mats the cell's step takes (atr: (p,); gru: (xg [rows, 2 H], xh); lrn: ([p | q | r],); olrn: ([p | q | r | s],))."""
        o, H, p = self.o, self.H, pre + "fetch_state_%s/" % s
        if self.lrn:
            return (o.project(x, p + "hide_x/W_0_0", o.mat(tag + ".pqr", x.rows, (4 if self.gated else 3) * H)),)
        if self.c == "atr":
            return (o.project(x, p + "hide_x/W_0_0", o.mat(tag + ".p", x.rows, H)),)
        return (o.project(x, p + "gate_x/W_0_0", o.mat(tag + ".xg", x.rows, 2 * H)),
                o.project(x, p + "hide_x/W_0_0", o.mat(tag + ".xh", x.rows, H)))

    def step(self, pre, s, h_prev, inp, out, out_copy=None, idx=None, mask=None, tag=""):
        """out = carry(mask, cell(h_prev[idx], inp), h_prev[idx]) with the scope pre + "cell_<s>"; the arguments of
        Engine.rnn_atr_step."""
        o, e, p = self.o, self.e, pre + "cell_%s/" % s
        if self.lrn:                  # (no variable under cell_<s>)
            e.rnn_lrn_scan(h_prev, inp[0], None, out, out_copy, idx, mask, 1, False, self.gated)
            return
        if self.c == "atr":
            e.rnn_atr_step(h_prev, o.W(p + "hide_h/W_0_0"), o.b(p + "hide_h/b_0"), inp[0], out, out_copy, idx, mask)
            return
        z = o.mat(tag + "gru.z", out.rows, self.H, F32)
        rh = o.mat(tag + "gru.rh", out.rows, self.H)
        e.rnn_gru_step(h_prev, o.W(p + "gate_h/W_0_0"), o.b(p + "gate_h/b_0"), o.W(p + "hide_h/W_0_0"), o.b(p + "hide_h/b_0"),
                       inp[0], inp[1], z, rh, out, out_copy, idx, mask)

    def pair(self, h_prev, lo, hi, out, out_copy=None, idx=None):
        """lrn / olrn: out = higher(lower(h_prev[idx], lo), hi), one step of a one-to-one pair in ONE launch."""
        self.e.rnn_lrn_scan(h_prev, lo[0], hi[0], out, out_copy, idx, None, 1, False, self.gated)

    def scan(self, lo, hi, out, seq, mask, T, reverse):
        """lrn / olrn: a whole scan from the zero state in ONE launch -- rnn.rnn (hi None) or cond_rnn(one2one=True) -- over
        the T positions of sentence-major [R * T, .] Mats, backwards with `reverse`; seq: the state of every position in the
        storage type (may be a column slice), out: the fp32 state after the last scanned position; mask: fp32 Mat [R, T]."""
        self.e.rnn_lrn_scan(None, lo[0], hi[0] if hi is not None else None, out, seq, None, mask, T, reverse, self.gated)


def encode(core, o, batch, K):
    """-> (memory Mat [B * Ls, H], projected memory Mat [B * Ls, H]); writes h_0 into the state buffer of parity 0,
    tiled K times per sentence."""
    e, H, E, NE, c = core.eng, core.H, core.E, core.NE, core.cell
    B, Ls = batch["B"], batch["Ls"]
    T = B * Ls
    smask = batch["smask"]
    mask_at = lambda t: Mat(smask, B, 1, Ls, t)
    cells = Cells(core, o)
    x = o.mat("enc.x", T, E)
    e.rnn_embed(batch["src"], T, o.table(core.src_emb), o.b("bias"), x)
    enc = o.mat("enc", T, H)
    seq_of = lambda l: enc if l == NE else o.mat("enc.seq%d" % (l & 1), T, H)      # h^l in the storage type
    hs = [Mat(e.buf(o.pre + "enc.h%d" % i, (B, H), F32), B, H) for i in (0, 1)]
    at = lambda inp, t: tuple(_at(m, B, t, Ls) for m in inp)
    whole = Mat(smask, B, Ls, Ls)       # the mask of a whole scan: lrn / olrn issue ONE launch per scan, whatever Ls
    pre = "encoder/layer_0/"
    inp = cells.fetch(x, pre, c, "enc.lo")
    if cells.lrn:
        cells.scan(inp, None, hs[0], seq_of(0), whole, Ls, False)
    else:
        prev = None
        for t in range(Ls):
            cells.step(pre, c, prev, at(inp, t), hs[t & 1], _at(seq_of(0), B, t, Ls), mask=mask_at(t), tag="enc.")
            prev = hs[t & 1]
    for l in range(1, NE + 1):          # cond_rnn(one2one=True): the lower cell on x_t, the higher on h^{l-1}_t
        pre = "encoder/layer_%d/" % l
        lo = cells.fetch(x, pre, c + "_lower", "enc.lo")
        hi = cells.fetch(seq_of(l - 1), pre, c + "_higher", "enc.hi")
        g, s = hs
        if cells.lrn:
            cells.scan(lo, hi, g, seq_of(l), whole, Ls, l % 2 == 1)
            continue
        order = range(Ls - 1, -1, -1) if l % 2 == 1 else range(Ls)
        for n, t in enumerate(order):
            cells.step(pre, c + "_lower", None if n == 0 else g, at(lo, t), s, mask=mask_at(t), tag="enc.")
            cells.step(pre, c + "_higher", s, at(hi, t), g, _at(seq_of(l), B, t, Ls), mask=mask_at(t), tag="enc.")
    feature = _at(enc, B, 0 if NE % 2 == 1 else Ls - 1, Ls)       # the state after the last scanned position
    i = "decoder_initializer/dec_init_state_init/"
    h0 = o.project(feature, i + "W_0_0", o.mat("enc.h0", B, H, F32), bias=o.b(i + "b_0"))
    rep = e.buf(o.pre + "enc.rep", (B * K,), torch.int32)
    e.h2d(rep, np.repeat(np.arange(B, dtype=np.int32), K))
    state0 = e.buf(o.pre + "hs.0", (B * K, H), F32)
    e.buf(o.pre + "hs.1", (B * K, H), F32)
    e.lib.call("zk_gather_rows", h0.ptr, H * 4, rep.data_ptr(), state0.data_ptr(), H * 4, B * K, H * 4, e.stream)
    pm = o.project(enc, "decoder/context_att/W_0_0", o.mat("pm", T, H))
    return enc, pm


def step(state, target, time, time_dev, hp):
    """One cached decoder step -> (logits Mat fp32 [BK, Vpad], state)."""
    core = state["_core"]
    o = _ops(core, state["f32"])
    f32 = o.storage.dtype == F32
    e, H, E, D, c = core.eng, core.H, core.E, core.D, core.cell
    BK, K, Ls = state["BK"], state["K"], state["Ls"]
    if time_dev is None and time >= state["Tmax"]:
        raise RuntimeError("decode step %d exceeds the allocated cache length %d" % (time, state["Tmax"]))
    cells = Cells(core, o)
    dst = state["decoder"]["state"]
    src, idx = state.pop("_gather", (dst, None))      # (no reorder since the last step: the state in place, rows as they are)
    cat = o.mat("cat", BK, H + D * H + E)             # [h' | c_0 .. c_{D-1} | y]: the operand of ff
    y = cat.cols_slice(H + D * H, H + D * H + E)
    d = "decoder/"
    e.rnn_embed(target, BK, o.table(core.tgt_emb), o.b("bias"), y, pad=hp.tgt_vocab.pad())
    ss = [o.mat("s.%d" % i, BK, H, F32) for i in (0, 1)]
    sc = o.mat("sc", BK, H)
    s = ss[0]
    cells.step(d, c + "_lower", src, cells.fetch(y, d, c + "_lower", "lo"), s, sc, idx=idx)
    for l in range(D):                                # (D >= 1: the last higher cell writes the new state and cat[:, :H])
        last = l == D - 1
        a = d + "deep_attention_%d/" % l
        qa = o.project(sc, a + "feed_query/W_0_0", o.mat("qa", BK, H), bias=o.b(a + "feed_query/b_0"))
        v = o.b(a + "feed_logits/W_0_0")
        cl = cat.cols_slice(H + l * H, H + (l + 1) * H)
        if f32:       # the fp32 context is of the storage type already: no separate fp32 buffer
            e.add_attn(qa, state["pm"], state["encodes"], v, state["mask"], cl, None, K, Ls)
        else:
            e.add_attn(qa, state["pm"], state["encodes"], v, state["mask"], o.mat("ctx", BK, H, F32), cl, K, Ls)
        nxt = dst if last else ss[(l + 1) & 1]
        name = "%s_higher_%d" % (c, l)
        cells.step(d, name, s, cells.fetch(cl, d, name, "hi"), nxt, cat.cols_slice(0, H) if last else sc)
        s = nxt
    pre = o.project(cat, "ff/W_0_0", o.mat("pre", BK, E, F32))
    feat = o.mat("feat", BK, E)
    e.rnn_bias_tanh(pre, o.b("ff/b_0"), out_copy=feat, f32=f32)
    logits = o.mat("logits", BK, core.Vpad, F32)
    o.gemm(feat, o.W(core.soft_emb), logits, BK, core.V, E, 1)
    if time_dev is None:
        state["time_filled"] = time + 1
    return logits, state


def build_state(core, hp, source, K, max_steps):
    """encoding_fn: source batch -> RnnState, as models/_rnnsearch.py:build_state (source padding and the rounding of the
    step count follow models/_decode.py: a padded position has mask 0, so every scan carries the state over it and the
    attentions give it the weight 0)."""
    f32 = _f32.wanted(hp)
    check_shape(core, f32)
    o = _ops(core, f32)
    e = core.eng
    batch, max_steps = _dec.shape_batch(core, hp, source, max_steps)
    B, Ls = batch["B"], batch["Ls"]
    enc, pm = encode(core, o, batch, K)
    mask_keep = e.buf(o.pre + "smask", (B, Ls), F32)
    mask_keep.copy_(batch["smask"])
    state = RnnState()
    state.storage = o.storage
    state.update({"_core": core, "B": B, "K": K, "BK": B * K, "Ls": Ls, "Tmax": max_steps, "encodes": enc, "pm": pm,
                  "mask": mask_keep, "time_filled": 0, "decoder": {}, "f32": f32, "_pp": 0})
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
