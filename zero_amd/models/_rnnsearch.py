# coding: utf-8
"""``rnnsearch`` at inference: the encoder schedule and the cached decoder step on the kernels of zero_amd/csrc/zk_rnn.hip,
in the bf16 mode (bf16 GEMM operands, ``zk_gemm``) and in ``decode_dtype=float32`` (``zk_f32_gemm``).

Reference: models/rnnsearch.py:16-133, rnns/rnn.py (rnn, cond_rnn), rnns/atr.py, func.py:107-161.  With
carry(m, a, b) = m a + (1 - m) b and ATR(h, p) = sigmoid(p + q) p + sigmoid(p - q) h, q = h U + b:

  encoder   x_t = src_emb[source_t] + bias                       (no sqrt(H) scale, no timing signal)
            hf_t = carry(m_t, ATR_f(hf_{t-1}, x_t Wf), hf_{t-1})                                   t = 0 .. Ls-1
            caencoder:  s_t = carry(m_t, ATR_lo(g_{t+1}, x_t Wlo), g_{t+1});  g_t = carry(m_t, ATR_hi(s_t, hf_t Whi), s_t)
                        memory = g (width M = H), feature = g_0                                     t = Ls-1 .. 0
            else:       hb the plain backward scan; memory = [hf, hb] (M = 2H), feature = [hf_{Ls-1}, hb_0]
            h_0 = tanh(feature W_init + b_init);   pm = memory W_ca   (once per batch: the reference recomputes the same
            values every step)
  step      y = tgt_emb[tok] + bias (zeros when every token is pad);  s = ATR_lo(h, y Wlo);  qa = s Wq + bq
            a = softmax_j(v . tanh(qa + pm_j) + (1 - mask_j) * -inf);  c = sum_j a_j memory_j;  h' = ATR_hi(s, c Whi)
            logits = tanh([h', c, y] W_pre + b_pre) E^T

A scan is ONE launch per time step and cell (zk_rnn_atr_step): the input projections of the whole sequence are one GEMM
in front of it (models/_rnn.py: Cells with cell = atr, Scans).  The recurrent state is fp32 in both modes; each cell launch
also writes the state in the storage type where the next GEMM reads it.  The cell, attention and embedding launches of a step
write into column slices of one [BK, H + M + E] buffer, so pre_logits is one product.  The per-beam state is a ping-pong pair
of fp32 [BK, H] buffers (RnnState); the beam reorder is the row index of the step's first cell launch (no gather launch).
Memory, projected memory and mask are stored once per sentence (kv_group = K).
"""

import torch

from zero_amd.models import _rnn as R

F32 = torch.float32


class RnnSearchCore(R.RnnCore):
    """RnnCore with this model's sizes: the memory is H wide with caencoder, else [forward | backward]; the one cell that
    models/rnnsearch.py admits; the step serves a lexical shortlist."""

    shortlist = True

    def __init__(self, params, model_name, store=None, device=None):
        R.RnnCore.__init__(self, params, model_name, store, device)
        self.M = self.H if self.ca else 2 * self.H
        self.cell = "atr"


def encode(core, o, batch, K):
    """-> (memory Mat [B * Ls, M], [projected memory Mat [B * Ls, M]]); writes h_0 into the state buffer of parity 0,
    tiled K times per sentence."""
    e, H, E, M = core.eng, core.H, core.E, core.M
    B, Ls = batch["B"], batch["Ls"]
    T = B * Ls
    scans = R.Scans(core, o, batch)
    x = o.mat("enc.x", T, E)
    e.rnn_embed(batch["src"], T, o.table(core.src_emb), o.b("bias"), x)
    enc = o.mat("enc", T, M)
    f, b = "encoder/forward/", "encoder/backward/"
    if core.ca:
        hf = o.mat("enc.hf", T, H)
        scans.plain(f, x, False, hf)
        scans.pair(b, x, hf, True, enc)
        feature = R._at(enc, B, 0, Ls)
    else:
        scans.plain(f, x, False, enc.cols_slice(0, H))
        scans.plain(b, x, True, enc.cols_slice(H, 2 * H))
        feature = scans.ends(enc, "enc.feat")
    i = "decoder_initializer/atr_init/"
    h0 = o.project(feature, i + "W_0_0", o.mat("enc.h0", B, H, F32))
    e.rnn_bias_tanh(h0, o.b(i + "b_0"), out_f32=R.state_pair(o, 0, B * K, H), rep=K, f32=o.storage.dtype == F32)
    return enc, [o.project(enc, "decoder/context_att/W_0_0", o.mat("pm", T, M))]


def step(core, o, state, target, srcs, dsts, idx, hp):
    """The layers of one cached decoder step (models/_rnn.py:step) -> logits Mat fp32 [BK, Vpad]."""
    H, E, M, c, BK = core.H, core.E, core.M, core.cell, state["BK"]
    cells = R.Cells(core, o)
    cat = o.mat("cat", BK, H + M + E)                 # [h | c | y]: the operand of pre_logits
    y = cat.cols_slice(H + M, H + M + E)
    ctx = cat.cols_slice(H, H + M)
    d = "decoder/"
    core.eng.rnn_embed(target, BK, o.table(core.tgt_emb), o.b("bias"), y, pad=hp.tgt_vocab.pad())
    s = o.mat("s", BK, H, F32)
    sc = o.mat("sc", BK, H)
    cells.step(d, c + "_lower", srcs[0], cells.fetch(y, d, c + "_lower", "lo"), s, sc, idx=idx)
    R.attend(o, state, d + "attention/", sc, state["pm"], ctx)
    cells.step(d, c + "_higher", s, cells.fetch(ctx, d, c + "_higher", "hi"), dsts[0], cat.cols_slice(0, H))
    return R.logits_tail(o, cat, "pre_logits")
