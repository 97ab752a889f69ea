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
`Cells` (models/_rnn.py) is that dispatch, shared by encode() and step().  Launches of a captured decoder step (without the search's own):
  atr, lrn, olrn   embed, 1 projection, lower cell, D x (feed_query, attention, 1 projection, higher cell), ff, tanh, logits
        = 6 + 4 D
  gru   embed, 2 projections, 2 cell launches, D x (feed_query, attention, 2 projections, 2 cell launches), ff, tanh, logits
        = 8 + 6 D
and of the encoder: 1 embed + (1 + 2 NE) x n_p projections + (1 + 2 NE) x Ls x n_c cell launches (n_p = n_c = 1 for atr, 2 for
gru) + the initial state (1 product, 1 row gather) + the projected memory.  With lrn / olrn the cell launches of the encoder
are 1 + NE scans, whatever Ls: 1 embed + (1 + 2 NE) projections + (1 + NE) scans + the same tail.

The state is a ping-pong pair of fp32 [BK, H] buffers (models/_rnn.py RnnState), the beam reorder is the row index
of the step's first cell launch.  The attention contexts and the final state are written straight into column slices of one
[BK, H + D H + E] buffer in the order [h' | c_0 .. c_{D-1} | y], so ff is one product.
"""

import torch

from zero_amd.models import _rnn as R

F32 = torch.float32


class DeepAttCore(R.RnnCore):
    """RnnCore with this model's sizes: the memory is H wide, NE conditional encoder layers, D attention layers."""

    def __init__(self, params, model_name, store=None, device=None):
        R.RnnCore.__init__(self, params, model_name, store, device)
        self.ca = True
        self.NE, self.D = int(params.num_encoder_layer), int(params.num_decoder_layer)


def encode(core, o, batch, K):
    """-> (memory Mat [B * Ls, H], [projected memory Mat [B * Ls, H]]); writes h_0 into the state buffer of parity 0,
    tiled K times per sentence."""
    e, H, E, NE = core.eng, core.H, core.E, core.NE
    B, Ls = batch["B"], batch["Ls"]
    T = B * Ls
    scans = R.Scans(core, o, batch)
    x = o.mat("enc.x", T, E)
    e.rnn_embed(batch["src"], T, o.table(core.src_emb), o.b("bias"), x)
    enc = o.mat("enc", T, H)
    seq_of = lambda l: enc if l == NE else o.mat("enc.seq%d" % (l & 1), T, H)      # h^l in the storage type
    scans.plain("encoder/layer_0/", x, False, seq_of(0))
    for l in range(1, NE + 1):          # the lower cell on x_t, the higher on h^{l-1}_t; odd layers run backwards
        scans.pair("encoder/layer_%d/" % l, x, seq_of(l - 1), l % 2 == 1, seq_of(l))
    feature = R._at(enc, B, 0 if NE % 2 == 1 else Ls - 1, Ls)       # the state after the last scanned position
    i = "decoder_initializer/dec_init_state_init/"
    h0 = o.project(feature, i + "W_0_0", o.mat("enc.h0", B, H, F32), bias=o.b(i + "b_0"))
    R.tile_state(o, h0, R.rep_index(o, B, K))
    return enc, [o.project(enc, "decoder/context_att/W_0_0", o.mat("pm", T, H))]


def step(core, o, state, target, srcs, dsts, idx, hp):
    """The layers of one cached decoder step (models/_rnn.py:step) -> logits Mat fp32 [BK, Vpad]."""
    H, E, D, c, BK = core.H, core.E, core.D, core.cell, state["BK"]
    cells = R.Cells(core, o)
    cat = o.mat("cat", BK, H + D * H + E)             # [h' | c_0 .. c_{D-1} | y]: the operand of ff
    y = cat.cols_slice(H + D * H, H + D * H + E)
    d = "decoder/"
    core.eng.rnn_embed(target, BK, o.table(core.tgt_emb), o.b("bias"), y, pad=hp.tgt_vocab.pad())
    ss = [o.mat("s.%d" % i, BK, H, F32) for i in (0, 1)]
    sc = o.mat("sc", BK, H)
    s = ss[0]
    cells.step(d, c + "_lower", srcs[0], cells.fetch(y, d, c + "_lower", "lo"), s, sc, idx=idx)
    for l in range(D):                                # (D >= 1: the last higher cell writes the new state and cat[:, :H])
        last = l == D - 1
        cl = cat.cols_slice(H + l * H, H + (l + 1) * H)
        R.attend(o, state, d + "deep_attention_%d/" % l, sc, state["pm"], cl)
        nxt = dsts[0] if last else ss[(l + 1) & 1]
        name = "%s_higher_%d" % (c, l)
        cells.step(d, name, s, cells.fetch(cl, d, name, "hi"), nxt, cat.cols_slice(0, H) if last else sc)
        s = nxt
    return R.logits_tail(o, cat, "ff")
