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
in front of it.  The recurrent state is fp32 in both modes; each cell launch also writes the state in the storage type
where the next GEMM reads it.  The cell, attention and embedding launches of a step write into column slices of one
[BK, H + M + E] buffer, so pre_logits is one product.  The per-beam state is a ping-pong pair of fp32 [BK, H] buffers; the
beam reorder is the row index of the step's first cell launch (no gather launch).  Memory, projected memory and mask are
stored once per sentence (kv_group = K).
"""

import numpy as np
import torch

from zero_amd import shortlist as _shortlist
from zero_amd.func import Engine, Mat
from zero_amd.models import _decode as _dec
from zero_amd.models import _decode_f32 as _f32
from zero_amd.models._core import trim_columns
from zero_amd.models._ops import ops_for
from zero_amd.variables import get_store

F32 = torch.float32


class RnnSearchCore(object):
    """What the search and the step-graph driver read from ``state["_core"]`` (eng, store, hp, V, Vpad, H) plus the
    sizes and variable names of this model."""

    def __init__(self, params, model_name, store=None, device=None):
        self.hp = params
        self.model = model_name
        if device is None:
            device = "cuda:%d" % torch.cuda.current_device() if torch.cuda.is_available() else "cpu"
        self.eng = Engine(device)
        self.store = store if store is not None else get_store(params, model_name, device)
        self.H, self.E = params.hidden_size, params.embed_size
        self.ca = bool(params.caencoder)
        self.M = self.H if self.ca else 2 * self.H
        shared = params.shared_source_target_embedding
        self.src_emb = "embedding" if shared else "src_embedding"
        self.tgt_emb = "embedding" if shared else "tgt_embedding"
        if shared:
            self.soft_emb = "embedding"
        else:
            self.soft_emb = "tgt_embedding" if params.shared_target_softmax_embedding else "softmax_embedding"
        self.V = params.tgt_vocab.size()
        self.Vpad = self.store.pshape[self.soft_emb][0]

    def upload(self, source, trim=True):
        """Host source ids -> device int32 + the source mask (zk_batch_prep), as TransformerCore.upload does it."""
        e = self.eng
        src = np.asarray(source.cpu() if torch.is_tensor(source) else source)
        if trim:
            src = trim_columns(src)
        B, Ls = src.shape
        ids = e.buf("ids.src", (B, Ls), torch.int32)
        e.h2d(ids, src)
        out = {"B": B, "Ls": Ls, "src": ids, "suffix": "", "max_id": max(self.hp.src_vocab.size(), self.hp.tgt_vocab.size())}
        if B > 0:
            out["smask"] = e.buf("smask", (B, Ls), F32)
            e.batch_prep(out)
        return out


def check_shape(core, f32):
    """The sizes the kernels take; nothing here depends on the data, so encoding_fn refuses before the encoder pass."""
    H, E, M = core.H, core.E, core.M
    if not f32 and (H % 8 != 0 or E % 8 != 0):
        raise ValueError("rnnsearch in bf16 needs hidden_size and embed_size to be multiples of 8 -- got %d and %d -- "
                         "(rows are loaded 16 bytes at a time); decode_dtype=float32 takes these sizes" % (H, E))
    if f32 and (H % 4 != 0 or E % 4 != 0):
        raise ValueError("rnnsearch with decode_dtype=float32 needs hidden_size and embed_size to be multiples of 4 -- got "
                         "%d and %d -- (zk_f32_gemm reads rows 16 bytes at a time)" % (H, E))
    if M > 2048:
        raise ValueError("rnnsearch: the additive attention kernel takes a memory width of at most 2048 (got %d = %s "
                         "hidden_size)" % (M, "1 x" if core.ca else "2 x"))


RN = "rn."        # this model's buffers: the decode mode's prefix + "rn." (RnnState.graph_pointers selects them by it)


def _ops(core, f32, shortlist=None):
    return ops_for(core, f32, (_dec.F32_CACHES if f32 else _dec.BF16_CACHES).prefix + RN, shortlist)


def cell(o, scope, h_prev, p, out, out_copy=None, idx=None, mask=None):
    o.e.rnn_atr_step(h_prev, o.W(scope + "/hide_h/W_0_0"), o.b(scope + "/hide_h/b_0"), p, out, out_copy, idx, mask)


def _at(m, B, t, L, c0=0, cols=None):
    """Position t of a [B, L, width] Mat: the [B, cols] view with the row stride L * width."""
    cols = m.cols if cols is None else cols
    return Mat(m.t, B, cols, L * m.ld, m.off + t * m.ld + c0)


def encode(core, o, batch, K):
    """-> (memory Mat [B * Ls, M], projected memory Mat [B * Ls, M]); writes h_0 into the state buffer of parity 0,
    tiled K times per sentence."""
    e, H, E, M = core.eng, core.H, core.E, core.M
    esz, f32 = o.storage.esz, o.storage.dtype == F32
    B, Ls = batch["B"], batch["Ls"]
    T = B * Ls
    smask = batch["smask"]
    mask_at = lambda t: Mat(smask, B, 1, Ls, t)
    x = o.mat("enc.x", T, E)
    e.rnn_embed(batch["src"], T, o.table(core.src_emb), o.b("bias"), x)
    enc = o.mat("enc", T, M)
    hs = [Mat(e.buf(o.pre + "enc.h%d" % i, (B, H), F32), B, H) for i in (0, 1)]

    def scan(scope, p, order, copy_of):
        """A plain rnn.rnn scan over the positions in `order`; copy_of(t): where position t's state goes."""
        prev = None
        for n, t in enumerate(order):
            cell(o, scope, prev, _at(p, B, t, Ls), hs[n & 1], copy_of(t), mask=mask_at(t))
            prev = hs[n & 1]
    f = "encoder/forward/"
    pf = o.project(x, f + "fetch_state_atr/hide_x/W_0_0", o.mat("enc.pf", T, H))
    b = "encoder/backward/"
    if core.ca:
        hf = o.mat("enc.hf", T, H)
        scan(f + "cell_atr", pf, range(Ls), lambda t: _at(hf, B, t, Ls))
        plo = o.project(x, b + "fetch_state_atr_lower/hide_x/W_0_0", o.mat("enc.plo", T, H))
        phi = o.project(hf, b + "fetch_state_atr_higher/hide_x/W_0_0", o.mat("enc.phi", T, H))
        g, s = hs[0], hs[1]
        for t in range(Ls - 1, -1, -1):        # cond_rnn(one2one=True) on the reversed sequence
            first = t == Ls - 1
            cell(o, b + "cell_atr_lower", None if first else g, _at(plo, B, t, Ls), s, mask=mask_at(t))
            cell(o, b + "cell_atr_higher", s, _at(phi, B, t, Ls), g, _at(enc, B, t, Ls), mask=mask_at(t))
        feature = _at(enc, B, 0, Ls)
    else:
        scan(f + "cell_atr", pf, range(Ls), lambda t: _at(enc, B, t, Ls, 0, H))
        pb = o.project(x, b + "fetch_state_atr/hide_x/W_0_0", o.mat("enc.pb", T, H))
        scan(b + "cell_atr", pb, range(Ls - 1, -1, -1), lambda t: _at(enc, B, t, Ls, H, H))
        feature = o.mat("enc.feat", B, M)
        for t, c0 in ((Ls - 1, 0), (0, H)):    # [hf_{Ls-1}, hb_0]
            src = _at(enc, B, t, Ls, c0, H)
            e.lib.call("zk_gather_rows", src.ptr, src.ld * esz, None, feature.ptr + c0 * esz, M * esz, B, H * esz,
                       e.stream)
    i = "decoder_initializer/atr_init/"
    h0 = o.project(feature, i + "W_0_0", o.mat("enc.h0", B, H, F32))
    state0 = Mat(e.buf(o.pre + "hs.0", (B * K, H), F32), B * K, H)
    e.buf(o.pre + "hs.1", (B * K, H), F32)
    e.rnn_bias_tanh(h0, o.b(i + "b_0"), out_f32=state0, rep=K, f32=f32)
    pm = o.project(enc, "decoder/context_att/W_0_0", o.mat("pm", T, M))
    return enc, pm


class RnnState(_dec.DecodeState):
    """The decode state of rnnsearch: the per-beam cache is the fp32 [BK, H] hidden state, kept as a ping-pong pair.
    reorder() hands the row index to the next step's first cell launch, which reads the old half through it and whose step
    writes the new half."""

    def _half(self, pp):
        core = self["_core"]
        return Mat(core.eng.buf(self.storage.prefix + RN + "hs.%d" % pp, (self["BK"], core.H), F32), self["BK"], core.H)

    def reorder(self, index_dev, time_dev=None, defer_aan=False):
        pp = self["_pp"]
        self["_gather"] = (self._half(pp), index_dev)
        self["_pp"] = 1 - pp
        self.bind_caches()

    def bind_caches(self):
        self["decoder"]["state"] = self._half(self["_pp"])

    def graph_pointers(self):
        """Every address a captured step holds (models/_decode.py adopt_graphs / retire_graphs)."""
        core = self["_core"]
        e = core.eng
        pre = self.storage.prefix + RN
        ptrs = [self["pack_dev"].data_ptr(), self["out_dev"].data_ptr(), self["mask"].data_ptr(), self["encodes"].ptr,
                self["pm"].ptr, e.seed.data_ptr(), core.store.shadow.data_ptr(), core.store.master.data_ptr()]
        ptrs += [b.data_ptr() for nm, b in sorted(e.bufs.items()) if nm.startswith(pre)]
        return ptrs


def step(state, target, time, time_dev, hp):
    """One cached decoder step -> (logits Mat fp32 [BK, Vpad], state)."""
    core = state["_core"]
    o = _ops(core, state["f32"], state.get("shortlist"))
    f32 = o.storage.dtype == F32
    e, H, E, M = core.eng, core.H, core.E, core.M
    BK, K, Ls = state["BK"], state["K"], state["Ls"]
    if time_dev is None and time >= state["Tmax"]:
        raise RuntimeError("decode step %d exceeds the allocated cache length %d" % (time, state["Tmax"]))
    dst = state["decoder"]["state"]
    src, idx = state.pop("_gather", (dst, None))      # (no reorder since the last step: the state in place, rows as they are)
    cat = o.mat("cat", BK, H + M + E)                 # [h | c | y]: the operand of pre_logits
    y = cat.cols_slice(H + M, H + M + E)
    c = cat.cols_slice(H, H + M)
    d = "decoder/"
    e.rnn_embed(target, BK, o.table(core.tgt_emb), o.b("bias"), y, pad=hp.tgt_vocab.pad())
    plo = o.project(y, d + "fetch_state_atr_lower/hide_x/W_0_0", o.mat("plo", BK, H))
    s = o.mat("s", BK, H, F32)
    sc = o.mat("sc", BK, H)
    cell(o, d + "cell_atr_lower", src, plo, s, sc, idx=idx)
    qa = o.project(sc, d + "attention/feed_query/W_0_0", o.mat("qa", BK, M), bias=o.b(d + "attention/feed_query/b_0"))
    v = o.b(d + "attention/feed_logits/W_0_0")
    if f32:       # the fp32 context is of the storage type already: no separate fp32 buffer
        e.add_attn(qa, state["pm"], state["encodes"], v, state["mask"], c, None, K, Ls)
    else:
        e.add_attn(qa, state["pm"], state["encodes"], v, state["mask"], o.mat("ctx", BK, M, F32), c, K, Ls)
    phi = o.project(c, d + "fetch_state_atr_higher/hide_x/W_0_0", o.mat("phi", BK, H))
    cell(o, d + "cell_atr_higher", s, phi, dst, cat.cols_slice(0, H))
    pre = o.project(cat, "pre_logits/W_0_0", o.mat("pre", BK, E, F32))
    feat = o.mat("feat", BK, E)
    e.rnn_bias_tanh(pre, o.b("pre_logits/b_0"), out_copy=feat, f32=f32)
    logits = o.logits_view(o.mat("logits", BK, core.Vpad, F32).t, BK)
    o.gemm(feat, o.W(core.soft_emb), logits, BK, o.V, E, 1)
    if time_dev is None:
        state["time_filled"] = time + 1
    return logits, state


def build_state(core, hp, source, K, max_steps):
    """encoding_fn: source batch -> RnnState.  Source padding and the rounding of the step count follow
    models/_decode.py:build_state (shape buckets for the step-graph cache): a padded position has mask 0, so both scans
    carry the state over it and the attention gives it the weight 0."""
    f32 = _f32.wanted(hp)
    check_shape(core, f32)
    o = _ops(core, f32)
    e = core.eng
    batch, max_steps = _dec.shape_batch(core, hp, source, max_steps)
    B, Ls = batch["B"], batch["Ls"]
    # the batch's output vocabulary is built from the source ids while the encoder runs (zero_amd/shortlist.py)
    sl = _shortlist.launch(core, hp, batch["src"], B, Ls, Ls, o.pre) if _shortlist.wanted(hp) else None
    enc, pm = encode(core, o, batch, K)
    mask_keep = e.buf(o.pre + "smask", (B, Ls), F32)
    mask_keep.copy_(batch["smask"])
    state = RnnState()
    state.storage = o.storage
    state.update({"_core": core, "B": B, "K": K, "BK": B * K, "Ls": Ls, "Tmax": max_steps, "encodes": enc, "pm": pm,
                  "mask": mask_keep, "time_filled": 0, "decoder": {}, "f32": f32, "_pp": 0})
    if sl is not None:
        state["shortlist"] = _shortlist.finish(core, hp, sl, o)
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
