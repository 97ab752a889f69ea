# coding: utf-8
"""The fp32 scorer (``score_dtype="float32"``): the training-path forward of models/transformer.py:15-216 on fp32 master
weights, fp32 activations and fp32 accumulation -- the scoring twin of the fp32 decode mode (models/_decode_f32.py).

Why it exists: ``decode_dtype=float32`` decodes token-exact against the fp32 reference with beam scores to 1e-5, but
``score_fn`` ran the bf16 training-path forward only, whose sentence scores are off by up to 5e-3 relative -- as much as the
near-tie gaps that part a bf16 from an fp32 search.  An n-best list of the fp32 decoder could not be re-ranked or
force-decoded without re-introducing that noise, and the scorer could not reproduce the scores the search printed.

One launch per op of the reference, on the kernels of zero_amd/csrc/zk_f32.hip and zk_f32_seq.hip:

  encoder    transformer.py:15-84 as ``_decode_f32.encode`` runs it, its attention through zk_f32_attn_seq (one workgroup
             per block of query rows, keys and values staged once per block) instead of the per-row zk_f32_attn
  decoder    transformer.py:87-181: zk_f32_embed_shift (row i embeds token i - 1), causal self-attention
             (zk_f32_attn_seq, causal = 1) or the cumulative average + gate of transformer_aan.py:92-108, 165-192
             (zk_f32_cumavg, zk_f32_gate), cross-attention over the source mask through the same kernel, the merged
             attention's averaged v_map(query) (func.py:258-275: zk_f32_cumavg with the attention output as addend), FFN
  loss head  transformer.py:182-216: zk_f32_gemm (tb = 1) into fp32 logits, zk_ce_fused with label smoothing 0,
             zk_loss_reduce into the per-sentence scores

for ``transformer``, ``transformer_aan`` (incl. ``use_ffn`` and both ``aan_mask`` forms), ``transformer_rpr`` and
``transformer_fuse``.  Buffers are named ``sq.*``: a decode and a scoring pass of one engine never alias.
"""

import torch

from zero_amd.models import _decode_f32
from zero_amd.models._ops import ops_for

F32 = torch.float32


def wanted(hp):
    """score_dtype takes the spellings of decode_dtype (``_decode_f32.wanted``); decode_dtype itself does not select it."""
    return str(getattr(hp, "score_dtype", "bfloat16")).lower() in ("float32", "fp32", "f32")


def check_model(core):
    if core.fixup or core.rela or core.l0drop:
        raise NotImplementedError("%s has no score_dtype=float32 path" % core.model)
    if core.d % 4 != 0 or core.d > 128:
        from zero_amd.hip import ZeroHipError
        raise ZeroHipError("score_dtype=float32 needs a head size that is a multiple of 4 and at most 128 (got %d): "
                           "zk_f32_attn_seq reads keys 16 bytes at a time and holds two channels per lane" % core.d)


def decode_train(core, hp, batch, enc, smask, o, align=None):
    """transformer.py:87-181 / transformer_aan.py:120-192 / transformer_fuse.py:131-160, training path, in fp32:
    -> decoder output Mat [B*Lt, H].  align = (layer, hook): the alignment pass (models/_align.py) -- hook(q, k) runs
    behind that layer's cross-attention and the layers end there (-> None)."""
    e, H = core.eng, core.H
    B, Ls, Lt = batch["B"], batch["Ls"], batch["Lt"]
    T = B * Lt
    tmask = batch["tmask"]
    x = o.embed_shift(batch["tgt"], T, Lt, o.mat("dec.x0", T, H))
    for l in range(hp.num_decoder_layer):
        pre = "decoder/layer_%d" % l
        if core.aan:
            a = pre + "/average_attention"
            cat = o.mat("cat", T, 2 * H)
            e.lib.call("zk_gather_rows", x.ptr, H * 4, None, cat.ptr, 2 * H * 4, T, H * 4, e.stream)      # cat[:, :H] = x
            if hp.use_ffn:           # transformer_aan.py:176-183: the average goes through its own feed-forward
                avg = o.cumavg(x, tmask, o.mat("avg", T, H), B, Lt, hp.aan_mask)
                hh = o.mat("aah", T, core.F)
                o.linear(avg, a + "/ffn_layer/enlarge", hh, act=1)
                o.linear(hh, a + "/ffn_layer/output", cat.cols_slice(H, 2 * H))
            else:
                o.cumavg(x, tmask, cat.cols_slice(H, 2 * H), B, Lt, hp.aan_mask)
            z = o.mat("z", T, 2 * H)
            o.linear(cat, a + "/z_project", z)
            g = o.mat("y", T, H)
            e.lib.call("zk_f32_gate", z.ptr, cat.ptr, g.ptr, T, H, e.stream)
            x = o.add_ln(x, g, a, o.mat("d%d.aa.o" % l, T, H))
        elif not core.fuse:
            p = pre + "/self_attention/dot_attention/"
            qkv = o.mat("qkv", T, 3 * H)
            o.linear(x, p + "qkv_map", qkv)
            att = o.mat("att", T, H)
            # no padding mask on the target side (transformer.py:136): causality alone
            o.attn_seq(qkv.cols_slice(0, H), qkv.cols_slice(H, 2 * H), qkv.cols_slice(2 * H, 3 * H), att, B, Lt, Lt,
                       Lt * 3 * H, Lt * 3 * H, Lt * 3 * H, rpr=p if core.rpr else None, causal=True)
            y = o.mat("y", T, H)
            o.linear(att, p + "o_map", y)
            x = o.add_ln(x, y, pre + "/self_attention", o.mat("d%d.sa.o" % l, T, H))
        p = pre + "/" + core.cross + "/dot_attention/"
        qm = o.mat("q", T, H)
        o.linear(x, p + "q_map", qm)
        mk, mv = o.mat("mk", B * Ls, H), o.mat("mv", B * Ls, H)
        o.linear(enc, p + "k_map", mk)
        o.linear(enc, p + "v_map", mv)
        att = o.mat("att", T, H)
        o.attn_seq(qm, mk, mv, att, B, Lt, Ls, Lt * H, Ls * H, Ls * H, kmask=smask, ldmask=Ls, rpr=p if core.rpr else None)
        if align is not None and l == align[0]:
            align[1](qm, mk)
            return None
        if core.fuse:
            # func.py:258-275: v_q = v_map(query); o += aan_weights x v_q (the masked cumulative average)
            vq = o.mat("vq", T, H)
            o.linear(x, p + "v_map", vq)
            o.cumavg(vq, tmask, att, B, Lt, True, add=att)
        y = o.mat("y", T, H)
        o.linear(att, p + "o_map", y)
        x = o.add_ln(x, y, pre + "/" + core.cross, o.mat("d%d.ca.o" % l, T, H))
        x = o.ffn(x, pre + "/feed_forward", "d%d.ff" % l)
    return x


def score(core, hp, batch):
    """transformer.py:235-249 in fp32: the batch of ``core.upload`` -> per-sentence scores fp32 [B]."""
    check_model(core)
    o = ops_for(core, True, prefix="sq.")
    e = core.eng
    B, Lt = batch["B"], batch["Lt"]
    T = B * Lt
    if "smask" not in batch or "tmask" not in batch:
        batch = dict(batch)
        batch["smask"] = e.buf("smask", (B, batch["Ls"]), F32)
        e.make_mask(batch["src"], batch["smask"], B * batch["Ls"])
        batch["tmask"] = e.buf("tmask", (B, Lt), F32)
        e.make_mask(batch["tgt"], batch["tmask"], T)
    enc, smask = _decode_f32.encode(core, hp, batch, o, o.attn_seq)
    feat = decode_train(core, hp, batch, enc, smask, o)
    logits = o.mat("logits", T, core.Vpad)
    o.gemm(feat, o.W(core.soft_emb), logits, T, core.V, core.H, tb=1)
    ce = e.buf("sq.ce", (T,), F32)
    e.ce_fused(logits, batch["tgt"], None, ce, None, T, core.V, 0.0)
    per_sample = e.buf("sq.per_sample", (B,), F32)
    loss = e.buf("sq.loss", (1,), F32)
    e.loss_reduce(ce, batch["tgt"], per_sample, loss, B, Lt)
    return per_sample
