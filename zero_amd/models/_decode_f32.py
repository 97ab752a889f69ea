# coding: utf-8
"""The fp32 decode mode (round 5; ``decode_dtype="float32"``): encoder pass + cached decoder step on fp32 master
weights, fp32 activations and fp32 accumulation -- the reference's own default dtype (utils/dtype.py:12-15; run.py
``default_dtype="float32"``).

Why it exists: the north star asks for token-id exact greedy decode against the fp32 reference.  The bf16 product path
cannot deliver that (round 4: the fp32 and the bf16-storage ORACLES disagree with each other on 3 % of 256 sentences);
a path that rounds where the reference rounds can.  It is the same search (zero_amd/search.py: device-resident
bookkeeping, step graphs, fused top-2K on fp32 logits) over a different step: one launch per op of
models/transformer.py:15-84 (encoder), 120-196 (decoder step) and transformer_aan.py:92-117, 165-192 on the kernels of
zero_amd/csrc/zk_f32.hip.  All four registered models: ``transformer``, ``transformer_aan`` (incl. ``use_ffn``),
``transformer_rpr`` (relative positions inside zk_f32_attn: modules/rpr.py:10-75) and ``transformer_fuse`` (merged attention,
func.py:258-275).

The state nest, caches and reorder follow models/_decode.py (beam-invariant tensors stored once per sentence, per-beam
caches double-buffered and reordered by one row gather); buffers are named ``dq.*`` so that a bf16 and an fp32 decode of
the same engine never alias.
"""

import os

import torch

from zero_amd.func import Mat
from zero_amd.utils import dtype as zdtype

F32 = torch.float32


def wanted(hp):
    return str(getattr(hp, "decode_dtype", "bfloat16")).lower() in ("float32", "fp32", "f32")


def check_model(core):
    if core.d % 4 != 0:
        from zero_amd.hip import ZeroHipError
        raise ZeroHipError("decode_dtype=float32 needs a head size that is a multiple of 4 (got %d)" % core.d)


class _Ops(object):
    """The op layer of the fp32 step: thin wrappers over the zk_f32_* entry points (include/zero_hip.h)."""

    def __init__(self, core):
        self.core, self.e = core, core.eng
        self.lib = core.eng.lib
        self.H, self.nh, self.d = core.H, core.nh, core.d
        # round 6: row-local launches folded into their neighbours (ZERO_HIP_F32_FUSE=0: one launch per op, as in round 5 --
        # the two forms are compared in tests/test_gpu_decode_f32.py)
        self.fold = os.environ.get("ZERO_HIP_F32_FUSE", "1") != "0"

    def mat(self, name, rows, cols):
        return Mat(self.e.buf("dq." + name, (rows, cols), F32), rows, cols)

    def w(self, name):
        t = self.core.store.w(name)              # fp32 master (physical shape)
        return Mat(t, t.shape[0], t.shape[1])

    def embed(self, ids, rows, L, table, out, max_pos, pos0=0, pos_dev=None, zero_flag=None):
        """func.py:341-369: out = table[ids] * sqrt(H) + bias + timing signal of the row's position (row % L + pos0, or
        + *pos_dev); rows of a step whose ids are all pad (*zero_flag) are zero embeddings."""
        st = self.core.store
        tim = self.e.timing(max_pos + 1, self.H)
        self.lib.call("zk_f32_embed", ids.data_ptr(), rows, L, st.w(table).data_ptr(), st.w("bias").data_ptr(),
                      tim.data_ptr(), int(tim.shape[0]), out.ptr, self.H, float(self.H) ** 0.5, pos0, pos_dev,
                      zero_flag.data_ptr() if zero_flag is not None else None, self.e.stream)
        return out

    def embed_step(self, ids, rows, out, max_pos, pos0, pos_dev, pad, aan=None, cat=None):
        """embed() of one decode position with the all-pad test inside the launch; aan / cat: the first layer's average
        attention from the embedded row (cache tensor, cat Mat) in the same launch."""
        st = self.core.store
        tim = self.e.timing(max_pos + 1, self.H)
        self.lib.call("zk_f32_embed_step", ids.data_ptr(), rows, st.w(self.core.tgt_emb).data_ptr(), st.w("bias").data_ptr(),
                      tim.data_ptr(), int(tim.shape[0]), out.ptr, self.H, float(self.H) ** 0.5, pos0, pos_dev, pad,
                      aan.data_ptr() if aan is not None else None, cat.ptr if cat is not None else None, self.e.stream)
        return out

    def gemm(self, A, B, C, M, N, K, tb=0, bias=None, act=0):
        self.lib.call("zk_f32_gemm", A.ptr, B.ptr, C.ptr, M, N, K, A.ld, B.ld, C.ld, tb,
                      bias.data_ptr() if bias is not None else None, act, self.e.stream)

    def linear(self, x, scope, out, act=0):
        """func.py:14-65: out = x W + b (act 1: ReLU)."""
        W = self.w(scope + "/W_0_0")
        bias = None if self.core.fixup else self.core.store.w(scope + "/b_0")      # (fixup.py: every linear map is bias=False)
        self.gemm(x, W, out, x.rows, W.cols, W.rows, 0, bias, act)
        return out

    def add_ln(self, x, y, scope, out):
        """func.py:321-324 + 289-303: LN(x + y) with the scope's scale / offset."""
        st = self.core.store
        if self.fold and self.H % 4 == 0 and self.H <= 2048:
            # the 16-byte-load form (round 6: 4.8 us against 7.2 for a decode step's 128 rows)
            return self.ln_fused(x, y, scope, out)
        self.lib.call("zk_f32_add_ln", x.ptr, y.ptr if y is not None else None, st.w(scope + "/layer_norm/scale").data_ptr(),
                      st.w(scope + "/layer_norm/offset").data_ptr(), out.ptr, x.rows, self.H, zdtype.epsilon(), self.e.stream)
        return out

    def attn(self, q, k, v, out, B, Lq, Lk, bsq, bsk, bsv, kmask=None, ldmask=0, kv_group=1, nkeys_dev=None, rpr=None,
             q_pos0=0, q_pos_dev=None, kbias=None, max_rel=None):
        """rpr: attention scope prefix (".../dot_attention/") whose rpr_keys / rpr_values tables take part, or None.
        kbias: fp32 [.., ldmask] added to the scores (transformer_l0drop's log counts: zk_f32_attn_kb), or None.
        max_rel: the clipping distance handed to the kernel (default: the model's max_relative_position)."""
        rk = rv = None
        if rpr is not None:
            rk = self.core.store.w(rpr + "rpr_keys/embeddings").data_ptr()
            rv = self.core.store.w(rpr + "rpr_values/embeddings").data_ptr()
        head = (q.ptr, k.ptr, v.ptr, out.ptr, B, self.nh, Lq, Lk, self.d, q.ld, k.ld, v.ld, out.ld, int(bsq), int(bsk), int(bsv),
                int(Lq * out.ld), kmask.data_ptr() if kmask is not None else None, int(ldmask))
        tail = (int(kv_group), float(self.d) ** -0.5, zdtype.inf(), nkeys_dev.data_ptr() if nkeys_dev is not None else None,
                rk, rv, int(self.core.hp.max_relative_position if max_rel is None else max_rel), int(q_pos0),
                q_pos_dev.data_ptr() if q_pos_dev is not None else None, self.e.stream)
        if kbias is not None:
            self.lib.call("zk_f32_attn_kb", *head, kbias.data_ptr(), *tail)
        else:
            self.lib.call("zk_f32_attn", *head, *tail)
        return out

    def rela_attn(self, q, k, v, out, B, Lq, Lk, bsq, bsk, bsv, scope, kmask=None, ldmask=0, kv_group=1, nkeys_dev=None):
        """modules/rela.py:56-81 (zk_f32_rela_attn).  scope: the attention scope prefix (".../dot_attention/") whose
        post/{scale, gate} normalise the combined heads; the other arguments as attn()."""
        st = self.core.store
        self.lib.call("zk_f32_rela_attn", q.ptr, k.ptr, v.ptr, out.ptr, B, self.nh, Lq, Lk, self.d, q.ld, k.ld, v.ld, out.ld,
                      int(bsq), int(bsk), int(bsv), int(Lq * out.ld), kmask.data_ptr() if kmask is not None else None,
                      int(ldmask), int(kv_group), float(self.d) ** -0.5,
                      nkeys_dev.data_ptr() if nkeys_dev is not None else None, st.w(scope + "post/scale").data_ptr(),
                      st.w(scope + "post/gate").data_ptr(), float(zdtype.epsilon()), self.e.stream)
        return out

    def ln_fused(self, x, y, scope, out, gate=None, aan_next=None, time=0, time_dev=None):
        """zk_f32_ln_fused (round 6): LN(x + y) with row-local neighbours in the same launch.  gate = (z, cat): y is the
        average-attention gate of transformer_aan.py:186-189 and the residual is cat[:, :H] (x, y = None);
        aan_next = (cache tensor, cat Mat): the next layer's average attention from the normalised row."""
        st = self.core.store
        z, cat = gate if gate is not None else (None, None)
        cache, cat_out = aan_next if aan_next is not None else (None, None)
        self.lib.call("zk_f32_ln_fused", x.ptr if x is not None else None, y.ptr if y is not None else None,
                      z.ptr if z is not None else None, cat.ptr if cat is not None else None,
                      st.w(scope + "/layer_norm/scale").data_ptr(), st.w(scope + "/layer_norm/offset").data_ptr(), out.ptr,
                      out.rows, self.H, zdtype.epsilon(), cache.data_ptr() if cache is not None else None,
                      cat_out.ptr if cat_out is not None else None, int(time), time_dev, self.e.stream)
        return out

    def ffn(self, x, scope, tag, aan_next=None, time=0, time_dev=None):
        """func.py:327-338 + residual + LayerNorm (transformer.py:62-69)."""
        h = self.mat(tag + ".h", x.rows, self.core.F)
        self.linear(x, scope + "/ffn_layer/enlarge", h, act=1)
        y = self.mat("y", x.rows, self.H)
        self.linear(h, scope + "/ffn_layer/output", y)
        if aan_next is not None:
            return self.ln_fused(x, y, scope, self.mat(tag + ".o", x.rows, self.H), aan_next=aan_next, time=time,
                                 time_dev=time_dev)
        return self.add_ln(x, y, scope, self.mat(tag + ".o", x.rows, self.H))


def encode(core, hp, batch):
    """transformer.py:15-84 in fp32: -> (encoder output Mat [B*Ls, H], source mask fp32 [B, Ls])."""
    if core.fixup:
        from zero_amd.models._fixup import Fixup
        return Fixup(core, True).encode(batch)
    o = _Ops(core)
    H = core.H
    B, Ls = batch["B"], batch["Ls"]
    T = B * Ls
    smask = batch["smask"]
    x = o.embed(batch["src"], T, Ls, core.src_emb, o.mat("enc.x0", T, H), Ls)
    for l in range(hp.num_encoder_layer):
        pre = "encoder/layer_%d" % l
        p = pre + "/self_attention/dot_attention/"
        qkv = o.mat("enc.qkv", T, 3 * H)
        o.linear(x, p + "qkv_map", qkv)
        att = o.mat("enc.att", T, H)
        if core.rela:
            o.rela_attn(qkv.cols_slice(0, H), qkv.cols_slice(H, 2 * H), qkv.cols_slice(2 * H, 3 * H), att, B, Ls, Ls,
                        Ls * 3 * H, Ls * 3 * H, Ls * 3 * H, p, kmask=smask, ldmask=Ls)
        else:
            o.attn(qkv.cols_slice(0, H), qkv.cols_slice(H, 2 * H), qkv.cols_slice(2 * H, 3 * H), att, B, Ls, Ls,
                   Ls * 3 * H, Ls * 3 * H, Ls * 3 * H, kmask=smask, ldmask=Ls, rpr=p if core.rpr else None)
        y = o.mat("y", T, H)
        o.linear(att, p + "o_map", y)
        x = o.add_ln(x, y, pre + "/self_attention", o.mat("e%d.sa.o" % l, T, H))
        x = o.ffn(x, pre + "/feed_forward", "e%d.ff" % l)
    return x, smask


def step_cache(target, state, time, time_dev, hp):
    """One cached decoder step in fp32 (transformer.py:88-196 with cache / transformer_aan.py:165-260): -> logits Mat
    fp32 [B*K, Vpad].  time_dev: the step counter lives in device memory (hipGraph replay)."""
    from zero_amd.models._decode import append_kv
    core = state["_core"]
    o = _Ops(core)
    e, H = core.eng, core.H
    BK, K, B, Ls, Tmax = state["BK"], state["K"], state["B"], state["Ls"], state["Tmax"]
    if time_dev is None and time >= Tmax:
        raise RuntimeError("decode step %d exceeds the allocated cache length %d" % (time, Tmax))
    if core.fixup:
        from zero_amd.models._fixup import Fixup
        return Fixup(core, True).step(target, state, time, time_dev, hp)
    tdev = time_dev.data_ptr() if time_dev is not None else None
    t_host = 0 if time_dev is not None else time
    fold = o.fold
    x = o.mat("x", BK, H)
    nl = hp.num_decoder_layer
    cat = o.mat("cat", BK, 2 * H) if core.aan else None
    aan_in_ln = fold and core.aan           # a layer's average attention is computed by the launch that produces its input
    if fold:
        lay0 = state["decoder"]["state"]["layer_0"]
        o.embed_step(target, BK, x, Tmax, t_host, tdev, hp.tgt_vocab.pad(), lay0["aan"] if aan_in_ln else None,
                     cat if aan_in_ln else None)
    else:
        zf = state["zero_flag"]
        e.lib.call("zk_all_equal", target.data_ptr(), BK, hp.tgt_vocab.pad(), zf.data_ptr(), e.stream)
        o.embed(target, BK, 1, core.tgt_emb, x, Tmax, t_host, tdev, zf)
    for l in range(nl):
        pre = "decoder/layer_%d" % l
        lay = state["decoder"]["state"]["layer_%d" % l]
        nxt = state["decoder"]["state"].get("layer_%d" % (l + 1))
        aan_next = (nxt["aan"], cat) if (aan_in_ln and nxt is not None) else None
        if core.aan:
            a = pre + "/average_attention"
            if not aan_in_ln:
                e.lib.call("zk_f32_aan_step", x.ptr, lay["aan"].data_ptr(), cat.ptr, BK, H, t_host, tdev, e.stream)
            if hp.use_ffn:           # transformer_aan.py:176-183: the averaged half goes through its own feed-forward
                hh = o.mat("aah", BK, core.F)
                o.linear(cat.cols_slice(H, 2 * H), a + "/ffn_layer/enlarge", hh, act=1)
                ya = o.mat("ya", BK, H)
                o.linear(hh, a + "/ffn_layer/output", ya)
                e.lib.call("zk_gather_rows", ya.ptr, H * 4, None, cat.ptr + H * 4, 2 * H * 4, BK, H * 4, e.stream)
            z = o.mat("z", BK, 2 * H)
            o.linear(cat, a + "/z_project", z)
            if fold:
                x = o.ln_fused(None, None, a, o.mat("d%d.aa.o" % l, BK, H), gate=(z, cat))
            else:
                g = o.mat("y", BK, H)
                e.lib.call("zk_f32_gate", z.ptr, cat.ptr, g.ptr, BK, H, e.stream)
                x = o.add_ln(x, g, a, o.mat("d%d.aa.o" % l, BK, H))
        elif not core.fuse:
            p = pre + "/self_attention/dot_attention/"
            qkv = o.mat("qkv", BK, 3 * H)
            o.linear(x, p + "qkv_map", qkv)
            append_kv(e, qkv, lay, BK, H, Tmax, 4, time, time_dev)
            att = o.mat("att", BK, H)
            kc, vc = Mat(lay["k"], BK * Tmax, H), Mat(lay["v"], BK * Tmax, H)
            # one query per beam row over the positions 0 .. time of ITS cache (no padding mask on the target side,
            # transformer.py:136; causality is the cache's length)
            if core.rela:      # (rela.py:66-68: a single query's causal bias is all zeros -- no mask, the cache's length)
                o.rela_attn(qkv.cols_slice(0, H), kc, vc, att, BK, 1, Tmax if time_dev is not None else time + 1, 3 * H,
                            Tmax * H, Tmax * H, p, nkeys_dev=time_dev)
            else:
                o.attn(qkv.cols_slice(0, H), kc, vc, att, BK, 1, Tmax if time_dev is not None else time + 1, 3 * H, Tmax * H,
                       Tmax * H, nkeys_dev=time_dev, rpr=p if core.rpr else None, q_pos0=t_host, q_pos_dev=time_dev)
            y = o.mat("y", BK, H)
            o.linear(att, p + "o_map", y)
            x = o.add_ln(x, y, pre + "/self_attention", o.mat("d%d.sa.o" % l, BK, H))
        # encoder-decoder attention over the sentence's keys / values (stored once per sentence: kv_group = K)
        p = pre + "/" + core.cross + "/dot_attention/"
        qm = o.mat("q", BK, H)
        o.linear(x, p + "q_map", qm)
        att = o.mat("att", BK, H)
        # (relative positions, transformer_rpr.py:167-169: the query sits at position `time` against the SOURCE positions)
        if core.rela:
            o.rela_attn(qm, lay["mk"], lay["mv"], att, BK, 1, Ls, H, Ls * 2 * H, Ls * 2 * H, p, kmask=state["mask"], ldmask=Ls,
                        kv_group=K)
        else:
            o.attn(qm, lay["mk"], lay["mv"], att, BK, 1, Ls, H, Ls * 2 * H, Ls * 2 * H, kmask=state["mask"], ldmask=Ls,
                   kv_group=K, rpr=p if core.rpr else None, q_pos0=t_host, q_pos_dev=time_dev, kbias=state.get("kbias"))
        if core.fuse:
            # func.py:258-275: v_q = v_map(query); aan_o = (v_q + cache) / (time + 1); cache += v_q; o += aan_o
            vq = o.mat("vq", BK, H)
            o.linear(x, p + "v_map", vq)
            cat = o.mat("cat", BK, 2 * H)
            e.lib.call("zk_f32_aan_step", vq.ptr, lay["aan"].data_ptr(), cat.ptr, BK, H, t_host, tdev, e.stream)
            e.lib.call("zk_f32_add_rows", att.ptr, att.ld, cat.ptr + H * 4, 2 * H, att.ptr, att.ld, BK, H, e.stream)
        y = o.mat("y", BK, H)
        o.linear(att, p + "o_map", y)
        x = o.add_ln(x, y, pre + "/" + core.cross, o.mat("d%d.ca.o" % l, BK, H))
        x = o.ffn(x, pre + "/feed_forward", "d%d.ff" % l, aan_next=aan_next, time=t_host, time_dev=tdev)
    logits = Mat(e.buf("dq.logits", (BK, core.Vpad), F32), BK, core.Vpad)
    o.gemm(x, o.w(core.soft_emb), logits, BK, core.V, H, tb=1)
    if time_dev is None:
        state["time_filled"] = time + 1
    return logits, state
