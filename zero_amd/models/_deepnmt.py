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
With lrn / olrn (n_p = n_c = 1, no recurrent product: models/_rnn.py Cells) a one-to-one layer is 2 projections + ONE paired
launch + 1, and every scan of the encoder -- plain or one-to-one pair -- is one launch whatever Ls.

The state is one fp32 ping-pong pair [BK, H] per decoder layer (models/_rnn.py RnnState); the beam reorder is the row index of every
layer's first cell launch.  A step that follows no reorder (time 0 of the host-side search, an eager decoding_fn call) reads
the current half with rows as they are and writes the other: a plain-form layer is ONE cell launch, and the cell launches
refuse an output that overlaps the state they read.
"""

import torch

from zero_amd.models import _rnn as R
from zero_amd.utils import dtype as zdtype

F32 = torch.float32


class DeepNmtCore(R.RnnCore):
    """RnnCore with this model's sizes: the memory is H wide, NE encoder and ND decoder layers, one state pair per decoder
    layer."""

    def __init__(self, params, model_name, store=None, device=None):
        R.RnnCore.__init__(self, params, model_name, store, device)
        self.NE, self.ND = int(params.num_encoder_layer), int(params.num_decoder_layer)
        self.layers = self.ND
        self.deep_att, self.redict = bool(params.use_deep_att), bool(params.dl4mt_redict)

    def form(self, l):
        """The form of decoder layer l: "att", "one2one" or "plain" (models/deepnmt.py:140-162)."""
        if l == 0 or self.deep_att:
            return "att"
        return "one2one" if self.ca else "plain"


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
    e, H, E, NE, ca = core.eng, core.H, core.E, core.NE, core.ca
    f32 = o.storage.dtype == F32
    B, Ls = batch["B"], batch["Ls"]
    T = B * Ls
    scans = R.Scans(core, o, batch)
    xc = o.mat("enc.x", T, E)
    xs = xc if f32 else o.mat("enc.xs", T, E, F32)
    embed(core, o, batch["src"], T, core.src_emb, xs, xc)
    hf = o.mat("enc.hf", T, H)
    y2 = None if ca else o.mat("enc.y2", T, 2 * H)           # [forward | backward] of layer 0
    for l in range(NE):
        pre = "encoder/layer_%d/" % l
        first = l == 0
        y = y2.cols_slice(0, H) if first and not ca else hf
        scans.plain(pre + "forward/", xc, False, y)
        if first and ca:              # on the reversed sequence: the lower cell on x_t, the higher on f_t
            y = o.mat("enc.g", T, H)
            scans.pair(pre + "backward/", xc, hf, True, y)
        elif first:
            scans.plain(pre + "backward/", xc, True, y2.cols_slice(H, 2 * H))
            y = y2
        if l == NE - 1:               # z: the state after the last scanned position, before y's buffer is used again
            if first and not ca:
                z = scans.ends(y2, "enc.z")
            else:
                z = R._at(y, B, 0 if first else Ls - 1, Ls)
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
    rep = R.rep_index(o, B, K)
    pms = []
    for l in range(core.ND):
        i = "layer_%d_init/" % l          # (at model scope: models/deepnmt.py:91-98 runs outside `decoder_initializer`)
        R.tile_state(o, o.project(z, i + "W_0_0", o.mat("enc.init", B, H, F32), bias=o.b(i + "b_0")), rep, l)
        pms.append(o.project(enc, "decoder/layer_%d/context_att/W_0_0" % l, o.mat("pm.l%d" % l, T, H))
                   if core.form(l) == "att" else None)
    return enc, pms


def step(core, o, state, target, srcs, dsts, idx, hp):
    """The layers of one cached decoder step (models/_rnn.py:step) -> logits Mat fp32 [BK, Vpad].  A plain-form layer is ONE
    cell launch from srcs[l] to dsts[l]."""
    H, E, c, BK = core.H, core.E, core.cell, state["BK"]
    cells = R.Cells(core, o)
    xcc = o.mat("xc", BK, E + H)                      # [x | c]: the operand of a plain-form cell and of the dl4mt ff
    xc, cc = xcc.cols_slice(0, E), xcc.cols_slice(E, E + H)
    xs = xc if o.storage.dtype == F32 else o.mat("xs", BK, E, F32)
    embed(core, o, target, BK, core.tgt_emb, xs, xc, pad=hp.tgt_vocab.pad())
    s = o.mat("s", BK, H, F32)
    sc = o.mat("sc", BK, H)
    hc = o.mat("hc", BK, H)                           # a layer's new state in the storage type: the operand of its ff
    for l in range(core.ND):
        pre = "decoder/layer_%d/" % l
        src, dst = srcs[l], dsts[l]
        form = core.form(l)
        if form == "plain":
            cells.step(pre, c, src, cells.fetch(xcc, pre, c, "lo"), dst, hc, idx=idx)
        elif form == "one2one" and cells.lrn:         # no attention between the two cells: ONE paired launch
            cells.pair(src, cells.fetch(xc, pre, c + "_lower", "lo"), cells.fetch(cc, pre, c + "_higher", "hi"), dst, hc, idx)
        else:
            att = form == "att"
            cells.step(pre, c + "_lower", src, cells.fetch(xc, pre, c + "_lower", "lo"), s, sc if att else None, idx=idx)
            if att:
                R.attend(o, state, pre + "attention/", sc, state["pms"][l], cc)
            cells.step(pre, c + "_higher", s, cells.fetch(cc, pre, c + "_higher", "hi"), dst, hc)
        ff_residual(o, pre, hc, xs, xc)
    return R.logits_tail(o, xcc, "ff") if core.redict else R.logits_tail(o, xc, None)
