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

from zero_amd.func import Mat
from zero_amd.models._fixup import Fixup, fixup_ops
from zero_amd.models._ops import ops_for


def wanted(hp):
    return str(getattr(hp, "decode_dtype", "bfloat16")).lower() in ("float32", "fp32", "f32")


def check_model(core):
    if core.d % 4 != 0:
        from zero_amd.hip import ZeroHipError
        raise ZeroHipError("decode_dtype=float32 needs a head size that is a multiple of 4 (got %d)" % core.d)


def encode(core, hp, batch, o=None, attn=None):
    """transformer.py:15-84 in fp32: -> (encoder output Mat [B*Ls, H], source mask fp32 [B, Ls]).  o: the ops object (default:
    the decode mode's own, over ``dq.*``); attn: the softmax attention launch (default o.attn, one wave per query row; the
    scorer passes o.attn_seq)."""
    H = core.H
    B, Ls = batch["B"], batch["Ls"]
    T = B * Ls
    smask = batch["smask"]
    if core.fixup:
        o = fixup_ops(core, True)
        return Fixup(core, o).encode(batch, o.embed(batch["src"], T, Ls, core.src_emb, o.mat("enc.x0", T, H), Ls), smask)
    o = o or ops_for(core, True)
    attn = attn or o.attn
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
            attn(qkv.cols_slice(0, H), qkv.cols_slice(H, 2 * H), qkv.cols_slice(2 * H, 3 * H), att, B, Ls, Ls,
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
    o = ops_for(core, True, shortlist=state.get("shortlist"))
    e, H = core.eng, core.H
    BK, K, B, Ls, Tmax = state["BK"], state["K"], state["B"], state["Ls"], state["Tmax"]
    if time_dev is None and time >= Tmax:
        raise RuntimeError("decode step %d exceeds the allocated cache length %d" % (time, Tmax))
    if core.fixup:
        return Fixup(core, fixup_ops(core, True)).step(target, state, time, time_dev, hp)
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
    logits = o.logits_mat(BK)
    o.gemm(x, o.W(core.soft_emb), logits, BK, o.V, H, tb=1)
    if time_dev is None:
        state["time_filled"] = time + 1
    return logits, state
