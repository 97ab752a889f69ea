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
from zero_amd.models import _decode_f32 as _f32

F32 = torch.float32
BF16 = torch.bfloat16


class Fixup(object):
    def __init__(self, core, f32):
        self.core, self.e, self.f32 = core, core.eng, bool(f32)
        self.lib = core.eng.lib
        self.H, self.F, self.nh, self.d = core.H, core.F, core.nh, core.d
        self.st = F32 if f32 else BF16
        self.esz = 4 if f32 else 2
        self.pre = "dq.fx." if f32 else "fx."          # (`dq.*`: a bf16 and an fp32 decode of one engine never alias)
        self.ops = _f32._Ops(core) if f32 else None    # the zk_f32_* launches of the fp32 mode

    # ---- buffers and operands
    def mat(self, name, rows, cols):
        """Named persistent matrix of the storage type."""
        return Mat(self.e.buf(self.pre + name, (rows, cols), self.st), rows, cols)

    def stream(self, name, rows):
        """The fp32 residual stream of one pass."""
        return Mat(self.e.buf(self.pre + name, (rows, self.H), F32), rows, self.H)

    def s(self, name):
        """fp32 master of a scalar [1] (or None: the neutral value)."""
        return None if name is None else self.core.store.w(name)

    def W(self, name):
        t = self.core.store.w(name) if self.f32 else self.core.store.s(name)
        return Mat(t, t.shape[0], t.shape[1])

    # ---- ops
    def linear(self, x, scope, out):
        """func.linear(..., bias=False) (fixup.py:43, 51, 97, 109-117, 184)."""
        W = self.W(scope + "/W_0_0")
        self.gemm(x, W, out, x.rows, W.cols, W.rows, 0)
        return out

    def gemm(self, A, B, C, M, N, K, tb):
        if self.f32:
            self.ops.gemm(A, B, C, M, N, K, tb)
        else:
            self.e.gemm(A, B, C, M, N, K, 0, tb)

    def boundary(self, x, y, scale, offset, scale2, x_out, xs_out):
        self.e.fixup_residual(x, y, self.s(scale), self.s(offset), self.s(scale2), x_out, xs_out)

    def relu_shift(self, h, offset):
        self.e.fixup_relu_shift(h, self.s(offset), h)

    def attn(self, q, k, v, out, B, Lq, Lk, bsq, bsk, bsv, kmask=None, causal=False, kv_group=1, time=0, time_dev=None,
             cached=False):
        """func.dot_attention's core on the existing softmax kernels.  cached: the keys 0 .. time (or *time_dev) of a
        per-row cache of Lk slots."""
        e, nh, d = self.e, self.nh, self.d
        if self.f32:
            if causal:
                raise NotImplementedError("transformer_fixup: the fp32 mode has no causal attention (it decodes from caches)")
            # (no relative positions: no tables, a clipping distance of 0, the query at position 0)
            self.ops.attn(q, k, v, out, B, Lq, Lk, bsq, bsk, bsv, kmask=kmask, ldmask=Lk if kmask is not None else 0,
                          kv_group=kv_group, nkeys_dev=time_dev if cached else None, max_rel=0)
            return
        if cached:
            e.attn_fwd(q, k, v, out, None, B, nh, 1, Lk, d, kmask=None, causal=False, q_pos0=0 if time_dev is not None else time,
                       bsq=bsq, bsk=bsk, bsv=bsv, pos_dev=time_dev, pos_flags=3)
        elif kv_group > 1 or bsq:
            e.attn_fwd(q, k, v, out, None, B, nh, Lq, Lk, d, kmask=kmask, causal=False, q_pos0=0 if time_dev is not None else time,
                       bsq=bsq, bsk=bsk, bsv=bsv, kv_group=kv_group, pos_dev=time_dev, pos_flags=1)
        else:
            e.attn_fwd(q, k, v, out, None, B, nh, Lq, Lk, d, kmask=kmask, causal=causal)

    # ---- the schedule
    def _layers(self, side, tag, n_layers, x0, X, XS, rows, self_attn, cross_attn, final, last_out):
        """x0: the embedded input rows (storage type).  X: the fp32 stream, XS: the shifted operand rows.  self_attn(l, p,
        XS) / cross_attn(l, p, XS) -> the attention output rows (before o_map).  final = (offset, scale2) of the form behind
        the last layer; its operand rows go to last_out.  tag: prefix of the pass's own scratch buffers."""
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
                h = self.mat(tag + "h", rows, self.F)
                self.linear(XS, scope + "/enlarge", h)
                self.relu_shift(h, scope + "/shift/offset")             # the SAME offset as in front of `enlarge`
                y = self.linear(h, scope + "/output", self.mat(tag + "y", rows, self.H))
            else:
                p = scope + "/dot_attention/"
                att = self_attn(l, p, XS) if kind == "sa" else cross_attn(l, p, XS)
                y = self.linear(att, p + "o_map", self.mat(tag + "y", rows, self.H))
            if i + 1 < len(subs):
                self.boundary(X, y, scope + "/scale/scale", subs[i + 1][0] + "/shift/offset", None, X, XS)
            else:
                self.boundary(X, y, scope + "/scale/scale", f_off, f_scale2, None, last_out)
        return last_out

    def encode(self, batch):
        """transformer_fixup.py:16-88 -> (the cross-attention memory [B*Ls, H] of the storage type, source mask)."""
        core, e, H = self.core, self.e, self.H
        hp = core.hp
        B, Ls = batch["B"], batch["Ls"]
        T = B * Ls
        smask = batch.get("smask")
        if smask is None:
            smask = e.buf("smask", (B, Ls), F32)
            e.make_mask(batch["src"], smask, T)
        if self.f32:
            x0 = self.ops.embed(batch["src"], T, Ls, core.src_emb, self.mat("enc.x0", T, H), Ls)
        else:
            x0 = e.mat("enc.x0", T, H)
            if not core.__dict__.get("_embeds_done"):      # (forward(): both embeddings went out as one launch)
                e.embed_fwd(batch["src"], core.store.s(core.src_emb), core.b("bias"), x0, B, Ls, H, drop_p=0.0, sid=9001)

        def self_attn(l, p, XS):
            qkv = self.linear(XS, p + "qkv_map", self.mat("enc.qkv", T, 3 * H))
            att = self.mat("enc.att", T, H)
            self.attn(qkv.cols_slice(0, H), qkv.cols_slice(H, 2 * H), qkv.cols_slice(2 * H, 3 * H), att, B, Ls, Ls,
                      Ls * 3 * H if self.f32 else 0, Ls * 3 * H if self.f32 else 0, Ls * 3 * H if self.f32 else 0, kmask=smask)
            return att
        out = self._layers("encoder", "enc.", hp.num_encoder_layer, x0, self.stream("enc.x", T), self.mat("enc.xs", T, H), T,
                           self_attn, None, ("encoder/shift/offset", "encoder/scale/scale"), self.mat("enc.out", T, H))
        return out, smask

    def decode_train(self, batch, enc, smask):
        """transformer_fixup.py:91-189 on the training path (score_fn): shifted inputs, causal self-attention.  bf16 mode.
        -> the decoder's shifted output rows [B*Lt, H] in front of the logits GEMM."""
        core, e, H = self.core, self.e, self.H
        hp = core.hp
        B, Ls, Lt = batch["B"], batch["Ls"], batch["Lt"]
        T = B * Lt
        x0 = e.mat("dec.x0", T, H)
        if not core.__dict__.get("_embeds_done"):
            e.embed_fwd(batch["tgt"], core.store.s(core.tgt_emb), core.b("bias"), x0, B, Lt, H, shift=True, drop_p=0.0, sid=9002)

        def self_attn(l, p, XS):
            qkv = self.linear(XS, p + "qkv_map", self.mat("dec.qkv", T, 3 * H))
            att = self.mat("dec.att", T, H)
            self.attn(qkv.cols_slice(0, H), qkv.cols_slice(H, 2 * H), qkv.cols_slice(2 * H, 3 * H), att, B, Lt, Lt, 0, 0, 0,
                      causal=True)
            return att

        def cross_attn(l, p, XS):
            q = self.linear(XS, p + "q_map", self.mat("dec.q", T, H))
            kv = self.mat("dec.kv", enc.rows, 2 * H)
            self.linear(enc, p + "k_map", kv.cols_slice(0, H))
            self.linear(enc, p + "v_map", kv.cols_slice(H, 2 * H))
            att = self.mat("dec.att", T, H)
            self.attn(q, kv.cols_slice(0, H), kv.cols_slice(H, 2 * H), att, B, Lt, Ls, 0, 0, 0, kmask=smask)
            return att
        return self._layers("decoder", "dec.", hp.num_decoder_layer, x0, self.stream("dec.x", T), self.mat("dec.xs", T, H), T,
                            self_attn, cross_attn, ("decoder/shift/offset", None), self.mat("dec.out", T, H))

    def step(self, target, state, time, time_dev, hp):
        """One cached decoder step (transformer_fixup.py:91-203 with state['decoder']) -> (logits Mat fp32 [B*K, Vpad],
        state).  time_dev: the step counter lives in device memory (hipGraph replay)."""
        from zero_amd.models._decode import append_kv
        core, e, H = self.core, self.e, self.H
        BK, K, Ls, Tmax = state["BK"], state["K"], state["Ls"], state["Tmax"]
        tdev = time_dev.data_ptr() if time_dev is not None else None
        t_host = 0 if time_dev is not None else time
        x0 = self.mat("dc.x0", BK, H)
        # the first-step zero embedding and the timing signal: the launches of the other models
        if self.f32:
            self.ops.embed_step(target, BK, x0, Tmax, t_host, tdev, hp.tgt_vocab.pad())
        else:
            tim = e.timing(Tmax + 1, H)
            self.lib.call("zk_dec_embed", target.data_ptr(), hp.tgt_vocab.pad(), core.store.s(core.tgt_emb).data_ptr(),
                          core.b("bias").data_ptr(), tim.data_ptr(), x0.ptr, BK, H, float(H) ** 0.5, t_host, tdev, None, None,
                          1.0, None, None, 0, e.stream)
        layers = state["decoder"]["state"]

        def self_attn(l, p, XS):
            lay = layers["layer_%d" % l]
            qkv = self.linear(XS, p + "qkv_map", self.mat("dc.qkv", BK, 3 * H))
            append_kv(e, qkv, lay, BK, H, Tmax, self.esz, time, time_dev)
            att = self.mat("dc.att", BK, H)
            self.attn(qkv.cols_slice(0, H), Mat(lay["k"], BK * Tmax, H), Mat(lay["v"], BK * Tmax, H), att, BK, 1,
                      Tmax if time_dev is not None else time + 1, 3 * H, Tmax * H, Tmax * H, time=time, time_dev=time_dev,
                      cached=True)
            return att

        def cross_attn(l, p, XS):
            lay = layers["layer_%d" % l]
            q = self.linear(XS, p + "q_map", self.mat("dc.q", BK, H))
            att = self.mat("dc.att", BK, H)
            # the memory was shifted and scaled once, by the encoder's last boundary (transformer_fixup.py:73, 160)
            self.attn(q, lay["mk"], lay["mv"], att, BK, 1, Ls, H, Ls * 2 * H, Ls * 2 * H, kmask=state["mask"], kv_group=K,
                      time=time, time_dev=time_dev)
            return att
        feat = self._layers("decoder", "dc.", hp.num_decoder_layer, x0, self.stream("dc.x", BK), self.mat("dc.xs", BK, H), BK,
                            self_attn, cross_attn, ("decoder/shift/offset", None), self.mat("dc.out", BK, H))
        if self.f32:
            logits = Mat(e.buf("dq.logits", (BK, core.Vpad), F32), BK, core.Vpad)
        else:
            logits = e.mat("dc.logits", BK, core.Vpad, F32)
        self.gemm(feat, self.W(core.soft_emb), logits, BK, core.V, H, 1)
        if time_dev is None:
            state["time_filled"] = time + 1
        return logits, state
