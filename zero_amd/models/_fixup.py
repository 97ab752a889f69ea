# coding: utf-8
"""``transformer_fixup`` (models/transformer_fixup.py + modules/fixup.py of the reference): the layer schedule of the
Transformer with every LayerNorm replaced by learned scalar shifts and scales, no bias in any linear map.

One class issues the schedule for the three places that run it, one launch per op:

  * the encoder pass (``encode``: B * Ls rows) of decoding and scoring,
  * the training-path decoder of ``score_fn`` (``decode_train``: shifted inputs, causal self-attention),
  * the cached decode step (``step``: B * K rows, per-beam key / value caches),

in the bf16 mode (bf16 GEMM operands, ``zk_gemm`` / ``zk_attn_fwd``) and in ``decode_dtype=float32`` (``zk_f32_gemm`` /
``zk_f32_attn``).  The residual stream is fp32 in BOTH modes: nothing re-normalises it and the branches are small against
it by construction, so a bf16 stream would drop every update below half an ulp of x.  Only the GEMM operands -- the
shifted rows a boundary writes next to the stream -- are of the storage type.

A sub-layer boundary is ONE launch of ``zk_fixup_residual``:  x += scale * y;  xs = scale2 * (x - offset of the NEXT
sub-layer)  (fixup.py:15-26; transformer_fixup.py:59-60, 73, 154-155, 189).  The scalars are fp32 masters read on the
device, so captured step graphs stay valid across a weight reload.
"""

import torch

from zero_amd.func import Mat
from zero_amd.models._ops import ops_for

F32 = torch.float32


def fixup_ops(core, f32):
    """The op layer of a fixup pass (models/_ops.py) over the pass's own buffers: ``fx.*`` in bf16, ``dq.fx.*`` in fp32
    (`dq.*`: a bf16 and an fp32 decode of one engine never alias)."""
    return ops_for(core, f32, "dq.fx." if f32 else "fx.")


class Fixup(object):
    """ops: fixup_ops(core, f32).  No relative positions anywhere: every attention runs with a clipping distance of 0."""

    def __init__(self, core, ops):
        self.core, self.e, self.o = core, core.eng, ops
        self.H, self.F = core.H, core.F

    def stream(self, name, rows):
        """The fp32 residual stream of one pass."""
        return self.o.mat(name, rows, self.H, F32)

    def s(self, name):
        """fp32 master of a scalar [1] (or None: the neutral value)."""
        return None if name is None else self.o.b(name)

    def boundary(self, x, y, scale, offset, scale2, x_out, xs_out):
        self.e.fixup_residual(x, y, self.s(scale), self.s(offset), self.s(scale2), x_out, xs_out)

    def relu_shift(self, h, offset):
        self.e.fixup_relu_shift(h, self.s(offset), h)

    # ---- the schedule
    def _layers(self, side, tag, n_layers, x0, X, XS, rows, self_attn, cross_attn, final, last_out):
        """x0: the embedded input rows (storage type).  X: the fp32 stream, XS: the shifted operand rows.  self_attn(l, p,
        XS) / cross_attn(l, p, XS) -> the attention output rows (before o_map).  final = (offset, scale2) of the form behind
        the last layer; its operand rows go to last_out.  tag: prefix of the pass's own scratch buffers."""
        o = self.o
        subs = []                                        # (scope of the shift / scale pair, kind)
        for l in range(n_layers):
            pre = "%s/layer_%d" % (side, l)
            subs.append((pre + "/self_attention", "sa", l))
            if cross_attn is not None:
                subs.append((pre + "/cross_attention", "ca", l))
            subs.append((pre + "/feed_forward/ffn_layer", "ff", l))
        f_off, f_scale2 = final
        if not subs:
            self.boundary(None, x0, None, f_off, f_scale2, None, last_out)
            return last_out
        # the embedding enters the stream and is shifted for the first sub-layer (x NULL, the embedding row as y)
        self.boundary(None, x0, None, subs[0][0] + "/shift/offset", None, X, XS)
        for i, (scope, kind, l) in enumerate(subs):
            if kind == "ff":
                h = o.mat(tag + "h", rows, self.F)
                o.linear(XS, scope + "/enlarge", h)
                self.relu_shift(h, scope + "/shift/offset")             # the SAME offset as in front of `enlarge`
                y = o.linear(h, scope + "/output", o.mat(tag + "y", rows, self.H))
            else:
                p = scope + "/dot_attention/"
                att = self_attn(l, p, XS) if kind == "sa" else cross_attn(l, p, XS)
                y = o.linear(att, p + "o_map", o.mat(tag + "y", rows, self.H))
            if i + 1 < len(subs):
                self.boundary(X, y, scope + "/scale/scale", subs[i + 1][0] + "/shift/offset", None, X, XS)
            else:
                self.boundary(X, y, scope + "/scale/scale", f_off, f_scale2, None, last_out)
        return last_out

    def encode(self, batch, x0, smask):
        """transformer_fixup.py:16-88 on the embedded source rows x0 -> (the cross-attention memory [B*Ls, H] of the
        storage type, source mask)."""
        o, H = self.o, self.H
        B, Ls = batch["B"], batch["Ls"]
        T = B * Ls

        def self_attn(l, p, XS):
            qkv = o.linear(XS, p + "qkv_map", o.mat("enc.qkv", T, 3 * H))
            att = o.mat("enc.att", T, H)
            o.attn(qkv.cols_slice(0, H), qkv.cols_slice(H, 2 * H), qkv.cols_slice(2 * H, 3 * H), att, B, Ls, Ls,
                   0, 0, 0, kmask=smask, ldmask=Ls, max_rel=0)
            return att
        out = self._layers("encoder", "enc.", self.core.hp.num_encoder_layer, x0, self.stream("enc.x", T),
                           o.mat("enc.xs", T, H), T, self_attn, None, ("encoder/shift/offset", "encoder/scale/scale"),
                           o.mat("enc.out", T, H))
        return out, smask

    def decode_train(self, batch, x0, enc, smask):
        """transformer_fixup.py:91-189 on the training path (score_fn) on the embedded, shifted target rows x0: causal
        self-attention.  -> the decoder's shifted output rows [B*Lt, H] in front of the logits GEMM."""
        o, H = self.o, self.H
        B, Ls, Lt = batch["B"], batch["Ls"], batch["Lt"]
        T = B * Lt

        def self_attn(l, p, XS):
            qkv = o.linear(XS, p + "qkv_map", o.mat("dec.qkv", T, 3 * H))
            att = o.mat("dec.att", T, H)
            o.attn(qkv.cols_slice(0, H), qkv.cols_slice(H, 2 * H), qkv.cols_slice(2 * H, 3 * H), att, B, Lt, Lt, 0, 0, 0,
                   max_rel=0, causal=True)
            return att

        def cross_attn(l, p, XS):
            q = o.linear(XS, p + "q_map", o.mat("dec.q", T, H))
            kv = o.mat("dec.kv", enc.rows, 2 * H)
            o.linear(enc, p + "k_map", kv.cols_slice(0, H))
            o.linear(enc, p + "v_map", kv.cols_slice(H, 2 * H))
            att = o.mat("dec.att", T, H)
            o.attn(q, kv.cols_slice(0, H), kv.cols_slice(H, 2 * H), att, B, Lt, Ls, 0, 0, 0, kmask=smask, ldmask=Ls, max_rel=0)
            return att
        return self._layers("decoder", "dec.", self.core.hp.num_decoder_layer, x0, self.stream("dec.x", T),
                            o.mat("dec.xs", T, H), T, self_attn, cross_attn, ("decoder/shift/offset", None),
                            o.mat("dec.out", T, H))

    def step(self, target, state, time, time_dev, hp):
        """One cached decoder step (transformer_fixup.py:91-203 with state['decoder']) -> (logits Mat fp32 [B*K, Vpad],
        state).  time_dev: the step counter lives in device memory (hipGraph replay)."""
        from zero_amd.models._decode import append_kv
        core, e, o, H = self.core, self.e, self.o, self.H
        BK, K, Ls, Tmax = state["BK"], state["K"], state["Ls"], state["Tmax"]
        tdev = time_dev.data_ptr() if time_dev is not None else None
        t_host = 0 if time_dev is not None else time
        # the first-step zero embedding and the timing signal: the launches of the other models
        x0 = o.embed_step(target, BK, o.mat("dc.x0", BK, H), Tmax, t_host, tdev, hp.tgt_vocab.pad())
        layers = state["decoder"]["state"]

        def self_attn(l, p, XS):
            lay = layers["layer_%d" % l]
            qkv = o.linear(XS, p + "qkv_map", o.mat("dc.qkv", BK, 3 * H))
            append_kv(e, qkv, lay, BK, H, Tmax, o.storage.esz, time, time_dev)
            att = o.mat("dc.att", BK, H)
            # the keys 0 .. time (or *time_dev) of every row's cache of Tmax slots
            o.attn(qkv.cols_slice(0, H), Mat(lay["k"], BK * Tmax, H), Mat(lay["v"], BK * Tmax, H), att, BK, 1,
                   Tmax if time_dev is not None else time + 1, 3 * H, Tmax * H, Tmax * H, nkeys_dev=time_dev, q_pos0=t_host,
                   q_pos_dev=time_dev, max_rel=0, cached=True)
            return att

        def cross_attn(l, p, XS):
            lay = layers["layer_%d" % l]
            q = o.linear(XS, p + "q_map", o.mat("dc.q", BK, H))
            att = o.mat("dc.att", BK, H)
            # the memory was shifted and scaled once, by the encoder's last boundary (transformer_fixup.py:73, 160)
            o.attn(q, lay["mk"], lay["mv"], att, BK, 1, Ls, H, Ls * 2 * H, Ls * 2 * H, kmask=state["mask"], ldmask=Ls,
                   kv_group=K, q_pos0=t_host, q_pos_dev=time_dev, max_rel=0)
            return att
        feat = self._layers("decoder", "dc.", hp.num_decoder_layer, x0, self.stream("dc.x", BK), o.mat("dc.xs", BK, H), BK,
                            self_attn, cross_attn, ("decoder/shift/offset", None), o.mat("dc.out", BK, H))
        logits = o.logits_mat(BK)
        o.gemm(feat, o.W(core.soft_emb), logits, BK, core.V, H, 1)
        if time_dev is None:
            state["time_filled"] = time + 1
        return logits, state
