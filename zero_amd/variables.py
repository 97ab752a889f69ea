# coding: utf-8
"""Variable store of one model scope -- the HBM layout of the parameters.

The reference keeps parameters in TF's variable store under ``{scope_name}/…``
(transformer.py:222; names from func.py:48,58,196,207-212,278,297-298 and
modules/rpr.py:56), stored fp32 and cast to the compute dtype on read
(utils/dtype.py:55-69).  Here every trainable variable of the scope lives in
ONE flat fp32 buffer (master weights) with three same-shaped companions:

    master fp32 | grad fp32 | adam m fp32 | adam v fp32 | shadow bf16

so that gradient all-reduce, global-norm, clipping and Adam are each a single
pass over contiguous HBM (utils/cycle.py:94-101 semantics), and the bf16
shadow the MFMA GEMMs read is refreshed by the Adam kernel itself.  Variable
names and logical shapes equal the reference's, so checkpoints can be
exchanged by name (``export`` / ``load``).

Embedding tables are physically padded to a multiple of 8 rows (zero rows,
zero gradients) so that vocabulary-sized GEMM dimensions stay 16-byte aligned.
"""

import math
from collections import OrderedDict

import numpy as np
import torch

ALIGN = 64  # elements; keeps every variable 256-byte (fp32) / 128-byte (bf16) aligned


def _attn_specs(prefix, H, self_att, rpr, nrel, d, rela=False):
    p = prefix + "/dot_attention/"
    v = []
    if self_att:
        v += [(p + "qkv_map/W_0_0", (H, 3 * H), "w"), (p + "qkv_map/b_0", (3 * H,), "zeros")]
    else:
        for m in ("q_map", "k_map", "v_map"):
            v += [(p + m + "/W_0_0", (H, H), "w"), (p + m + "/b_0", (H,), "zeros")]
    if rpr:
        v += [(p + "rpr_keys/embeddings", (nrel, d), "w"),
              (p + "rpr_values/embeddings", (nrel, d), "w")]
    if rela:
        # modules/rela.py:81, 95-109: gated_rms_norm(scope="post") runs after the projections that feed the attention and
        # before o_map; scale is ones-initialised, gate is drawn from the scope initialiser like any weight
        v += [(p + "post/scale", (H,), "ones"), (p + "post/gate", (H,), "w")]
    v += [(p + "o_map/W_0_0", (H, H), "w"), (p + "o_map/b_0", (H,), "zeros"),
          (prefix + "/layer_norm/scale", (H,), "ones"), (prefix + "/layer_norm/offset", (H,), "zeros")]
    return v


def _ffn_specs(prefix, H, F, with_ln=True):
    p = prefix + "/ffn_layer/"
    v = [(p + "enlarge/W_0_0", (H, F), "w"), (p + "enlarge/b_0", (F,), "zeros"),
         (p + "output/W_0_0", (F, H), "w"), (p + "output/b_0", (H,), "zeros")]
    if with_ln:
        v += [(prefix + "/layer_norm/scale", (H,), "ones"), (prefix + "/layer_norm/offset", (H,), "zeros")]
    return v


def _fixup_specs(params):
    """transformer_fixup.py:16-88, 91-203 + modules/fixup.py in creation order.  No LayerNorm and no bias of a linear map
    anywhere; per sub-layer a shift/offset [1] in front and a scale/scale [1] behind.  Kinds: "fx6" / "fx2" = the scope
    initialiser times L^(-1/6) / L^(-1/2), L = 2 NE + 3 ND (fixup.py:39-40, 91-93); o_map, the FFN output and a separate
    softmax_embedding start at zero (fixup.py:52, 185; transformer_fixup.py:199-201): "w_zeros" / "embed_zeros", which
    initial_values draws like their non-zero kind and discards, so that every drawn matrix of this model is the matrix
    `transformer` draws from the same seed times its factor."""
    H, E, F = params.hidden_size, params.embed_size, params.filter_size
    Vs, Vt = params.src_vocab.size(), params.tgt_vocab.size()
    shared = params.shared_source_target_embedding

    def att(prefix, maps, l):
        p = prefix + "/dot_attention/"
        return [(prefix + "/shift/offset", (1,), "zeros", l)] + \
            [(p + m + "/W_0_0", (H, w), "fx6", l) for m, w in maps] + \
            [(p + "o_map/W_0_0", (H, H), "w_zeros", l), (prefix + "/scale/scale", (1,), "ones", l)]

    def ffn(prefix, l):
        p = prefix + "/ffn_layer/"
        return [(p + "shift/offset", (1,), "zeros", l), (p + "enlarge/W_0_0", (H, F), "fx2", l),
                (p + "output/W_0_0", (F, H), "w_zeros", l), (p + "scale/scale", (1,), "ones", l)]
    specs = [("embedding" if shared else "src_embedding", (Vs, E), "embed", None), ("bias", (E,), "w", None)]
    for l in range(params.num_encoder_layer):
        pre = "encoder/layer_%d" % l
        specs += att(pre + "/self_attention", [("qkv_map", 3 * H)], l) + ffn(pre + "/feed_forward", l)
    specs += [("encoder/shift/offset", (1,), "zeros", None), ("encoder/scale/scale", (1,), "ones", None)]
    if not shared:
        specs.append(("tgt_embedding", (Vt, E), "embed", None))
    for l in range(params.num_decoder_layer):
        pre = "decoder/layer_%d" % l
        specs += att(pre + "/self_attention", [("qkv_map", 3 * H)], l)
        specs += att(pre + "/cross_attention", [("q_map", H), ("k_map", H), ("v_map", H)], l)
        specs += ffn(pre + "/feed_forward", l)
    specs.append(("decoder/shift/offset", (1,), "zeros", None))
    if not shared and not params.shared_target_softmax_embedding:
        specs.append(("softmax_embedding", (Vt, E), "embed_zeros", None))
    return specs


def _rnnsearch_specs(params):
    """models/rnnsearch.py:16-133 + rnns/rnn.py + rnns/atr.py + func.py:107-161 in creation order (cell "atr",
    layer_norm off).  An ATR cell `s` owns fetch_state_<s>/hide_x/W_0_0 (the input projection, no bias) and
    cell_<s>/hide_h/{W_0_0, b_0} (the recurrent map); a cond_rnn creates both input projections in front of its scan and
    the recurrent maps inside it.  M: the width of the memory (H for the context-aware encoder, else [forward, backward]).
    Embeddings are plain tf.get_variable calls under the scope: the scope initialiser draws them ("embed_w": padded rows
    like "embed"), and `bias` is ONE variable shared by both embedding lookups."""
    H, E = params.hidden_size, params.embed_size
    Vs, Vt = params.src_vocab.size(), params.tgt_vocab.size()
    shared = params.shared_source_target_embedding
    M = H if params.caencoder else 2 * H

    def fetch(pre, s, width):
        return [(pre + "fetch_state_%s/hide_x/W_0_0" % s, (width, H), "w")]

    def cell(pre, s):
        return [(pre + "cell_%s/hide_h/W_0_0" % s, (H, H), "w"), (pre + "cell_%s/hide_h/b_0" % s, (H,), "zeros")]
    v = [("embedding" if shared else "src_embedding", (Vs, E), "embed_w"), ("bias", (E,), "w")]
    v += fetch("encoder/forward/", "atr", E) + cell("encoder/forward/", "atr")
    b = "encoder/backward/"
    if params.caencoder:
        v += fetch(b, "atr_lower", E) + fetch(b, "atr_higher", H) + cell(b, "atr_lower") + cell(b, "atr_higher")
    else:
        v += fetch(b, "atr", E) + cell(b, "atr")
    v += [("decoder_initializer/atr_init/W_0_0", (M, H), "w"), ("decoder_initializer/atr_init/b_0", (H,), "zeros")]
    if not shared:
        v.append(("tgt_embedding", (Vt, E), "embed_w"))
    d = "decoder/"
    v += fetch(d, "atr_lower", E) + [(d + "context_att/W_0_0", (M, M), "w")] + cell(d, "atr_lower")
    v += [(d + "attention/feed_query/W_0_0", (H, M), "w"), (d + "attention/feed_query/b_0", (M,), "zeros"),
          (d + "attention/feed_logits/W_0_0", (M, 1), "w"), (d + "attention/feed_logits/b_0", (1,), "zeros")]
    v += fetch(d, "atr_higher", M) + cell(d, "atr_higher")
    v += [("pre_logits/W_0_0", (H + M + E, E), "w"), ("pre_logits/b_0", (E,), "zeros")]
    if not shared and not params.shared_target_softmax_embedding:
        v.append(("softmax_embedding", (Vt, E), "embed_w"))
    return [(n, s, k, None) for n, s, k in v]


def _deepatt_specs(params):
    """models/rnnsearch_deepatt.py:68-128, 132-236, 240-303 + rnns/rnn.py + rnns/{atr,gru,cell}.py + func.py:107-161 in
    creation order (cell "atr", "gru", "lrn" or "olrn", layer_norm off).  A cell `s` owns its input projections fetch_state_<s>/... (no
    bias) and its recurrent maps cell_<s>/... :
        atr   fetch: hide_x/W_0_0 [in, H]                            cell: hide_h/{W_0_0 [H, H], b_0}
        gru   fetch: gate_x/W_0_0 [in, 2 H], hide_x/W_0_0 [in, H]    cell: gate_h/{W_0_0 [H, 2 H], b_0}, hide_h/{W_0_0 [H, H], b_0}
        lrn   fetch: hide_x/W_0_0 [in, 3 H]                          cell: nothing (rnns/lrn.py: no recurrent map)
        olrn  fetch: hide_x/W_0_0 [in, 4 H]                          cell: nothing (rnns/olrn.py)
    Every scan creates the input projections of its cells (and, in the decoder, context_att) IN FRONT of tf.scan and the
    recurrent maps -- in the decoder also each deep_attention_l and fetch_state_<c>_higher_l, which act on values computed
    inside the step -- INSIDE it, in the order the step body runs.  The memory is H wide.  Embeddings and `bias` as
    _rnnsearch_specs."""
    H, E = params.hidden_size, params.embed_size
    Vs, Vt = params.src_vocab.size(), params.tgt_vocab.size()
    shared = params.shared_source_target_embedding
    c = str(params.cell).lower()
    if c not in ("atr", "gru", "lrn", "olrn"):
        raise NotImplementedError("rnnsearch_deepatt: the variables of cell=%s are not laid out (atr, gru, lrn and olrn are)" % c)
    XW = {"lrn": 3 * H, "olrn": 4 * H}.get(c, H)       # the width of hide_x: [p | q | r (| s)] for lrn / olrn

    def fetch(pre, s, width):
        p = pre + "fetch_state_%s/" % s
        gate = [(p + "gate_x/W_0_0", (width, 2 * H), "w")] if c == "gru" else []
        return gate + [(p + "hide_x/W_0_0", (width, XW), "w")]

    def cell(pre, s):
        if c in ("lrn", "olrn"):      # (rnns/lrn.py:44-51, rnns/olrn.py:46-56: the scope is opened, no variable is created)
            return []
        p = pre + "cell_%s/" % s
        gate = [(p + "gate_h/W_0_0", (H, 2 * H), "w"), (p + "gate_h/b_0", (2 * H,), "zeros")] if c == "gru" else []
        return gate + [(p + "hide_h/W_0_0", (H, H), "w"), (p + "hide_h/b_0", (H,), "zeros")]
    v = [("embedding" if shared else "src_embedding", (Vs, E), "embed_w"), ("bias", (E,), "w")]
    v += fetch("encoder/layer_0/", c, E) + cell("encoder/layer_0/", c)
    for l in range(1, params.num_encoder_layer + 1):
        pre = "encoder/layer_%d/" % l
        v += fetch(pre, c + "_lower", E) + fetch(pre, c + "_higher", H) + cell(pre, c + "_lower") + cell(pre, c + "_higher")
    i = "decoder_initializer/dec_init_state_init/"
    v += [(i + "W_0_0", (H, H), "w"), (i + "b_0", (H,), "zeros")]
    if not shared:
        v.append(("tgt_embedding", (Vt, E), "embed_w"))
    d = "decoder/"
    v += fetch(d, c + "_lower", E) + [(d + "context_att/W_0_0", (H, H), "w")] + cell(d, c + "_lower")
    D = params.num_decoder_layer
    for l in range(D):
        a = d + "deep_attention_%d/" % l
        v += [(a + "feed_query/W_0_0", (H, H), "w"), (a + "feed_query/b_0", (H,), "zeros"),
              (a + "feed_logits/W_0_0", (H, 1), "w"), (a + "feed_logits/b_0", (1,), "zeros")]
        v += fetch(d, "%s_higher_%d" % (c, l), H) + cell(d, "%s_higher_%d" % (c, l))
    v += [("ff/W_0_0", (H + D * H + E, E), "w"), ("ff/b_0", (E,), "zeros")]
    if not shared and not params.shared_target_softmax_embedding:
        v.append(("softmax_embedding", (Vt, E), "embed_w"))
    return [(n, s, k, None) for n, s, k in v]


def _deepnmt_specs(params):
    """models/deepnmt.py:16-100, 103-194 + rnns/rnn.py + rnns/{atr,gru,cell}.py + func.py:14-65, 107-161, 289-303 in creation
    order (cell "atr", "gru", "lrn" or "olrn", layer_norm off).  Cells own their variables as in _deepatt_specs; a plain rnn.rnn creates its
    input projections in front of tf.scan and its recurrent maps inside it, a cond_rnn both input projections (one2one) or
    the lower one and context_att (attention) in front and the rest inside, in the order the step body runs.  Every layer
    ends with ff (func.linear to embed_size).  x_map and its layer_norm are created after the `encoder` scope is left
    (deepnmt.py:83-84), and so are the initial-state maps layer_l_init: the `decoder_initializer` scope holds only the
    construction of the cell (deepnmt.py:86-89), get_init_state(x=z, scope="layer_l") runs in the return statement behind it
    (deepnmt.py:91-98; rnns/cell.py:35-38), at model scope.  The dl4mt_redict ff comes after the `decoder` scope
    (deepnmt.py:176-177).  Embeddings and `bias` as
    _rnnsearch_specs."""
    H, E = params.hidden_size, params.embed_size
    Vs, Vt = params.src_vocab.size(), params.tgt_vocab.size()
    shared = params.shared_source_target_embedding
    ca, NE, ND = bool(params.caencoder), int(params.num_encoder_layer), int(params.num_decoder_layer)
    c = str(params.cell).lower()
    if c not in ("atr", "gru", "lrn", "olrn"):
        raise NotImplementedError("deepnmt: the variables of cell=%s are not laid out (atr, gru, lrn and olrn are)" % c)
    XW = {"lrn": 3 * H, "olrn": 4 * H}.get(c, H)       # the width of hide_x: [p | q | r (| s)] for lrn / olrn

    def fetch(pre, s, width):
        p = pre + "fetch_state_%s/" % s
        gate = [(p + "gate_x/W_0_0", (width, 2 * H), "w")] if c == "gru" else []
        return gate + [(p + "hide_x/W_0_0", (width, XW), "w")]

    def cell(pre, s):
        if c in ("lrn", "olrn"):      # (rnns/lrn.py:44-51, rnns/olrn.py:46-56: the scope is opened, no variable is created)
            return []
        p = pre + "cell_%s/" % s
        gate = [(p + "gate_h/W_0_0", (H, 2 * H), "w"), (p + "gate_h/b_0", (2 * H,), "zeros")] if c == "gru" else []
        return gate + [(p + "hide_h/W_0_0", (H, H), "w"), (p + "hide_h/b_0", (H,), "zeros")]

    def one2one(pre, low_in, high_in):
        return fetch(pre, c + "_lower", low_in) + fetch(pre, c + "_higher", high_in) + cell(pre, c + "_lower") + \
            cell(pre, c + "_higher")

    def ff(pre, width):
        return [(pre + "ff/W_0_0", (width, E), "w"), (pre + "ff/b_0", (E,), "zeros")]
    v = [("embedding" if shared else "src_embedding", (Vs, E), "embed_w"), ("bias", (E,), "w")]
    for l in range(NE):
        pre = "encoder/layer_%d/" % l
        v += fetch(pre + "forward/", c, E) + cell(pre + "forward/", c)
        if l == 0:
            v += one2one(pre + "backward/", E, H) if ca else fetch(pre + "backward/", c, E) + cell(pre + "backward/", c)
        v += ff(pre, 2 * H if l == 0 and not ca else H)
    if E != H:
        v += [("x_map/W_0_0", (E, H), "w"), ("x_map/b_0", (H,), "zeros"),
              ("layer_norm/scale", (H,), "ones"), ("layer_norm/offset", (H,), "zeros")]
    Z = 2 * H if NE == 1 and not ca else H
    for l in range(ND):
        i = "layer_%d_init/" % l      # (model scope: the `decoder_initializer` scope only builds the cell, deepnmt.py:86-98)
        v += [(i + "W_0_0", (Z, H), "w"), (i + "b_0", (H,), "zeros")]
    if not shared:
        v.append(("tgt_embedding", (Vt, E), "embed_w"))
    for l in range(ND):
        pre = "decoder/layer_%d/" % l
        if l == 0 or params.use_deep_att:
            v += fetch(pre, c + "_lower", E) + [(pre + "context_att/W_0_0", (H, H), "w")] + cell(pre, c + "_lower")
            v += [(pre + "attention/feed_query/W_0_0", (H, H), "w"), (pre + "attention/feed_query/b_0", (H,), "zeros"),
                  (pre + "attention/feed_logits/W_0_0", (H, 1), "w"), (pre + "attention/feed_logits/b_0", (1,), "zeros")]
            v += fetch(pre, c + "_higher", H) + cell(pre, c + "_higher")
        elif ca:
            v += one2one(pre, E, H)
        else:
            v += fetch(pre, c, E + H) + cell(pre, c)
        v += ff(pre, H)
    if params.dl4mt_redict:
        v += ff("", E + H)
    if not shared and not params.shared_target_softmax_embedding:
        v.append(("softmax_embedding", (Vt, E), "embed_w"))
    return [(n, s, k, None) for n, s, k in v]


def variable_specs(params, model_name):
    """[(name, logical_shape, kind, layer)] in the reference's creation order
    (transformer.py:16-33,88-102,184-192; transformer_aan.py:165-192;
    transformer_rpr.py:54-55,144-146,167-169; transformer_fuse.py:131-160; transformer_l0drop.py:250: the
    source_pruning pair is created by the decoder after its embedding lookup and before its first layer;
    transformer_rela.py:48,134,154 + modules/rela.py:34-84: `transformer` plus post/{scale,gate} per attention scope)."""
    if model_name == "rnnsearch":       # (the one family whose embeddings are not H wide: before the H == E test)
        return _rnnsearch_specs(params)
    if model_name == "rnnsearch_deepatt":
        return _deepatt_specs(params)
    if model_name == "deepnmt":
        return _deepnmt_specs(params)
    H, E, F = params.hidden_size, params.embed_size, params.filter_size
    if H != E:
        raise ValueError("hidden_size must equal embed_size for the Transformer models "
                         "(embeddings are added to H-wide layers, transformer.py:29-31)")
    if model_name == "transformer_fixup":
        return _fixup_specs(params)
    d = H // params.num_heads
    rpr = model_name == "transformer_rpr"
    aan = model_name == "transformer_aan"
    fuse = model_name == "transformer_fuse"
    rela = model_name == "transformer_rela"
    nrel = 2 * params.max_relative_position + 1
    Vs, Vt = params.src_vocab.size(), params.tgt_vocab.size()
    shared = params.shared_source_target_embedding
    specs = [("embedding" if shared else "src_embedding", (Vs, E), "embed", None),
             ("bias", (E,), "w", None)]
    for l in range(params.num_encoder_layer):
        pre = "encoder/layer_%d" % l
        specs += [(n, s, k, l) for n, s, k in _attn_specs(pre + "/self_attention", H, True, rpr, nrel, d, rela)]
        specs += [(n, s, k, l) for n, s, k in _ffn_specs(pre + "/feed_forward", H, F)]
    if not shared:
        specs.append(("tgt_embedding", (Vt, E), "embed", None))
    if model_name == "transformer_l0drop":
        # log alpha_j = encodes[j] . W + b (func.linear(source_memory, 1, scope="source_pruning")); otherwise `transformer`
        specs += [("source_pruning/W_0_0", (H, 1), "w", None), ("source_pruning/b_0", (1,), "zeros", None)]
    for l in range(params.num_decoder_layer):
        pre = "decoder/layer_%d" % l
        if fuse:      # transformer_fuse.py:131-160: merged attention sub-layer + FFN
            specs += [(n, s, k, l) for n, s, k in _attn_specs(pre + "/fuse_attention", H, False, False, nrel, d)]
            specs += [(n, s, k, l) for n, s, k in _ffn_specs(pre + "/feed_forward", H, F)]
            continue
        if aan:
            a = pre + "/average_attention"
            if params.use_ffn:
                specs += [(n, s, k, l) for n, s, k in _ffn_specs(a, H, F, with_ln=False)]
            specs += [(a + "/z_project/W_0_0", (2 * H, 2 * H), "w", l),
                      (a + "/z_project/b_0", (2 * H,), "zeros", l),
                      (a + "/layer_norm/scale", (H,), "ones", l),
                      (a + "/layer_norm/offset", (H,), "zeros", l)]
        else:
            specs += [(n, s, k, l) for n, s, k in _attn_specs(pre + "/self_attention", H, True, rpr, nrel, d, rela)]
        specs += [(n, s, k, l) for n, s, k in _attn_specs(pre + "/cross_attention", H, False, rpr, nrel, d, rela)]
        specs += [(n, s, k, l) for n, s, k in _ffn_specs(pre + "/feed_forward", H, F)]
    if not shared and not params.shared_target_softmax_embedding:
        specs.append(("softmax_embedding", (Vt, E), "embed", None))
    return specs


def _scope_init(rng, shape, kind, gain):
    """modules/initializer.py:11-32 with TF1 fan rules."""
    fi, fo = (shape[0], shape[0]) if len(shape) == 1 else (shape[0], shape[1])
    if kind == "uniform":
        return rng.uniform(-gain, gain, size=shape)
    if kind == "normal":
        return rng.normal(0.0, gain, size=shape)
    if kind == "uniform_unit_scaling":
        lim = math.sqrt(3.0 * gain / ((fi + fo) / 2.0))
        return rng.uniform(-lim, lim, size=shape)
    if kind == "normal_unit_scaling":
        std = math.sqrt(gain / ((fi + fo) / 2.0))
        return np.clip(rng.normal(0.0, std, size=shape), -2 * std, 2 * std)
    lim = math.sqrt(6.0 / (fi + fo))
    return rng.uniform(-lim, lim, size=shape)


def initial_values(params, model_name, seed):
    """Host-side draw from the reference's initial distribution
    (transformer.py:18,90 embeddings N(0,H^-0.5); main.py:26 scope initializer;
    transformer.py:38-44 deep_transformer_init)."""
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    # transformer_fixup: the depth-dependent factor of the input maps (modules/initializer.py:35-45 scale_initializer)
    depth = 2 * params.num_encoder_layer + 3 * params.num_decoder_layer
    fx = {"fx6": depth ** (-1.0 / 6.0) if depth else 1.0, "fx2": depth ** (-1.0 / 2.0) if depth else 1.0}
    for name, shape, kind, layer in variable_specs(params, model_name):
        if kind in ("embed", "embed_zeros"):
            v = rng.normal(0.0, params.hidden_size ** -0.5, size=shape)
        elif kind == "embed_w":           # rnnsearch.py:24-25, 89-90, 130-131: the scope initialiser
            v = _scope_init(rng, shape, params.initializer, params.initializer_gain)
        elif kind == "zeros":
            v = np.zeros(shape)
        elif kind == "ones":
            v = np.ones(shape)
        elif layer is not None and params.deep_transformer_init:
            v = _scope_init(rng, shape, "uniform_unit_scaling",
                            params.initializer_gain * (layer + 1) ** -0.5)
        else:
            v = _scope_init(rng, shape, params.initializer, params.initializer_gain)
        out[name] = (v * (0.0 if kind.endswith("_zeros") else fx.get(kind, 1.0))).astype(np.float32)
    return out


class VariableStore(object):
    """Flat parameter / gradient / optimiser-state buffers of one scope."""

    def __init__(self, params, model_name, device):
        self.model_name = model_name
        self.device = torch.device(device)
        self.specs = variable_specs(params, model_name)
        self.offsets, self.lshape, self.pshape = OrderedDict(), {}, {}
        off = 0
        for name, shape, kind, _ in self.specs:
            pshape = tuple(shape)
            if kind in ("embed", "embed_zeros", "embed_w") or name.endswith("/embeddings"):
                # (relative-position tables too: their zero rows make them GEMM operands with an 8-aligned
                # contraction length as they are -- no padded copy per attention call)
                pshape = ((shape[0] + 7) // 8 * 8, shape[1])
            n = int(np.prod(pshape))
            self.offsets[name] = off
            self.lshape[name] = tuple(shape)
            self.pshape[name] = pshape
            off += (n + ALIGN - 1) // ALIGN * ALIGN
        self.numel = off
        self.logical_numel = sum(int(np.prod(s)) for s in self.lshape.values())
        dev = self.device
        self.master = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(off, dtype=torch.float32, device=dev)
        self.m = torch.zeros(off, dtype=torch.float32, device=dev)
        self.v = torch.zeros(off, dtype=torch.float32, device=dev)
        self.shadow = torch.zeros(off, dtype=torch.bfloat16, device=dev)
        self.accum = None     # update_cycle slots (utils/cycle.py:27-36), created on demand
        self.step = 0         # number of applied updates (Adam's t)
        self.shadow_loads = 0  # refresh_shadow() calls; (shadow_loads, step) identifies the bf16 weights ("weight version")

    # -- views --------------------------------------------------------------
    def _view(self, flat, name):
        o = self.offsets[name]
        ps = self.pshape[name]
        return flat[o:o + int(np.prod(ps))].view(*ps)

    def w(self, name):
        """fp32 master view (physical shape)."""
        return self._view(self.master, name)

    def s(self, name):
        """bf16 shadow view (physical shape) -- what the GEMMs read."""
        return self._view(self.shadow, name)

    def g(self, name):
        """fp32 gradient view (physical shape)."""
        return self._view(self.grad, name)

    def names(self):
        return list(self.offsets.keys())

    # -- host <-> device -----------------------------------------------------
    def load(self, values):
        """values: {name: array (logical shape)}; refreshes the bf16 shadow."""
        for name in self.offsets:
            if name not in values:
                raise KeyError("missing variable %s" % name)
            v = torch.as_tensor(np.asarray(values[name], dtype=np.float32))
            if tuple(v.shape) != self.lshape[name]:
                raise ValueError("shape mismatch for %s: %s vs %s" % (name, tuple(v.shape), self.lshape[name]))
            dst = self.w(name)
            dst.zero_()
            if v.dim() == 2:
                dst[:v.shape[0], :v.shape[1]].copy_(v)
            else:
                dst.copy_(v)
        self.refresh_shadow()

    @property
    def weight_version(self):
        """Changes whenever the bf16 weights the kernels read may have changed: a load / EMA swap (refresh_shadow) or an
        optimiser update (utils/cycle.py advances ``step``).  Derived copies of weights are cached against it."""
        return (self.shadow_loads, self.step)

    def refresh_shadow(self):
        self.shadow_loads += 1
        if self.device.type == "cuda":
            from zero_amd import hip
            hip.lib().call("zk_cast_f32_bf16", self.master.data_ptr(), self.shadow.data_ptr(), self.numel,
                           torch.cuda.current_stream().cuda_stream)
        else:  # layout / bookkeeping tests on CPU only -- never on the compute path
            self.shadow.copy_(self.master.to(torch.bfloat16))

    def export(self, which="master"):
        """{name: np.ndarray (logical shape)} of master / grad / m / v (or of any flat buffer laid out
        like them, e.g. the EMA shadows)."""
        flat = getattr(self, which) if isinstance(which, str) else which
        out = OrderedDict()
        for name in self.offsets:
            t = self._view(flat, name)
            ls = self.lshape[name]
            if len(ls) == 2:
                t = t[:ls[0], :ls[1]]
            out[name] = t.detach().float().cpu().numpy().copy()
        return out


_STORES = {}


def get_store(params, model_name, device=None, initializer_seed=None, create=True):
    """The variable store of ``params.scope_name`` (tf.variable_scope(...,
    reuse=AUTO_REUSE) of transformer.py:222-226: first use creates, later uses share)."""
    scope = params.scope_name or "model"
    key = (scope, model_name)
    if key not in _STORES:
        if not create:
            raise KeyError("no variables for scope %s" % scope)
        if device is None:
            device = "cuda:%d" % torch.cuda.current_device() if torch.cuda.is_available() else "cpu"
        st = VariableStore(params, model_name, device)
        seed = params.random_seed if initializer_seed is None else initializer_seed
        st.load(initial_values(params, model_name, seed))
        _STORES[key] = st
    return _STORES[key]


def reset_stores():
    _STORES.clear()
