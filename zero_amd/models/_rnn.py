# coding: utf-8
"""What the recurrent models share at inference: rnnsearch (models/_rnnsearch.py), rnnsearch_deepatt (_deepatt.py) and deepnmt
(_deepnmt.py) state their encoder and their decoder step -- ``encode`` and ``step`` under a header that is the model's
specification -- in the vocabulary of this module, which belongs to none of them:

  RnnCore       what the search and the step-graph driver read from ``state["_core"]``; each model subclasses it with its sizes
  check_shape   the sizes the kernels take
  Cells         the cell dispatch atr / gru / lrn / olrn: fetch (input projections), step, pair, scan
  Scans         the two scans of an encoder on top of Cells -- plain (rnn.rnn) and one-to-one pair (cond_rnn(one2one=True)) --
                ONE launch for lrn / olrn, one (gru: two) per position and cell otherwise; and the [last forward | first
                backward] feature gather
  state_pair / rep_index / tile_state / attend / logits_tail     the initial state, the additive attention, the output layer
  RnnState      one fp32 ping-pong pair [BK, H] per state layer; the beam reorder is the row index of a step's first cell launches
  step / build_state / make_infer_fns     the driver around a model's ``step`` and ``encode`` (SCHEDULES names their modules)

The recurrent state is fp32 in both decode modes; each cell launch also writes the state in the storage type where the next
product reads it.  Memory, projected memory and mask are stored once per sentence (kv_group = K).
"""

import importlib

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
RN = "rn."        # these models' buffers: the decode mode's prefix + "rn." (RnnState.graph_pointers selects them by it)
GRU_MAX_H = 2048        # zk_rnn_gru_gates: the LDS image of its columns of the gate matrix (include/zero_hip.h)
LRN_CELLS = ("lrn", "olrn")      # the cells without a recurrent product: a whole scan is one launch
SCHEDULES = {"rnnsearch": "_rnnsearch", "rnnsearch_deepatt": "_deepatt", "deepnmt": "_deepnmt"}      # model -> encode, step


class RnnCore(object):
    """What the search and the step-graph driver read from ``state["_core"]`` (eng, store, hp, V, Vpad, H) plus the sizes and
    variable names of a recurrent model.  A subclass sets what differs: M (the memory's width), ca, layers, shortlist."""

    layers = None          # the decoder state: one [BK, H] pair (None), or one pair per decoder layer (their number)
    shortlist = False      # zero_amd/shortlist.py serves the step of this model (the others refuse shortlist_file up front)

    def __init__(self, params, model_name, store=None, device=None):
        self.hp = params
        self.model = model_name
        if device is None:
            device = "cuda:%d" % torch.cuda.current_device() if torch.cuda.is_available() else "cpu"
        self.eng = Engine(device)
        self.store = store if store is not None else get_store(params, model_name, device)
        self.H, self.E = params.hidden_size, params.embed_size
        self.M = self.H
        self.ca = bool(params.caencoder)
        self.cell = str(params.cell).lower()
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
    name, H, E, M = core.model, core.H, core.E, core.M
    if not f32 and (H % 8 != 0 or E % 8 != 0):
        raise ValueError("%s in bf16 needs hidden_size and embed_size to be multiples of 8 -- got %d and %d -- (rows are "
                         "loaded 16 bytes at a time); decode_dtype=float32 takes these sizes" % (name, H, E))
    if f32 and (H % 4 != 0 or E % 4 != 0):
        raise ValueError("%s with decode_dtype=float32 needs hidden_size and embed_size to be multiples of 4 -- got %d and "
                         "%d -- (zk_f32_gemm reads rows 16 bytes at a time)" % (name, H, E))
    if M > 2048:        # (H <= 2048 also keeps the [forward | backward] input of deepnmt's bf16 ff within its 4096)
        raise ValueError("%s: the additive attention kernel takes a memory width of at most 2048 (got %d = %d x hidden_size "
                         "%d)" % (name, M, M // H, H))
    if not f32 and core.cell == "gru" and H > GRU_MAX_H:
        raise ValueError("%s with cell=gru in bf16 takes a hidden_size of at most %d (got %d); decode_dtype=float32 has no "
                         "such limit" % (name, GRU_MAX_H, H))


def _ops(core, f32, shortlist=None):
    return ops_for(core, f32, (_dec.F32_CACHES if f32 else _dec.BF16_CACHES).prefix + RN, shortlist)


def _at(m, B, t, L, c0=0, cols=None):
    """Position t of a [B, L, width] Mat: the [B, cols] view with the row stride L * width."""
    cols = m.cols if cols is None else cols
    return Mat(m.t, B, cols, L * m.ld, m.off + t * m.ld + c0)


class Cells(object):
    """The cell of the model (core.cell) on the ops `o`: fetch() = the input projections of a whole block of rows,
    step() = one time step; for lrn / olrn also scan() = a whole scan and pair() = one step of a lower / higher pair, each
    ONE launch.  `tag` names the buffers, so that the encoder's and the step's never alias.
      atr   p = x Wp;                      one launch  (zk_rnn_atr_step)
      gru   xg = x Wg [., 2 H], xh = x Wh;  two launches (zk_rnn_gru_gates, zk_rnn_gru_out: Engine.rnn_gru_step)
      lrn   [p | q | r] = x W [., 3 H];  olrn  [p | q | r | s] = x W [., 4 H]      (rnns/lrn.py, rnns/olrn.py: NO recurrent product)
            one launch for a WHOLE scan, single or lower / higher pair (zk_rnn_lrn_scan: Engine.rnn_lrn_scan); a step is T = 1"""

    def __init__(self, core, o):
        self.c, self.o, self.e, self.H = core.cell, o, core.eng, core.H
        self.lrn, self.gated = self.c in LRN_CELLS, self.c == "olrn"

    def fetch(self, x, pre, s, tag):
        """rnns/{atr,gru,lrn,olrn}.py fetch_states of the scope pre + "fetch_state_<s>" on x: Mat [rows, in] -> the tuple of
        Mats the cell's step takes (atr: (p,); gru: (xg [rows, 2 H], xh); lrn: ([p | q | r],); olrn: ([p | q | r | s],))."""
        o, H, p = self.o, self.H, pre + "fetch_state_%s/" % s
        if self.lrn:
            return (o.project(x, p + "hide_x/W_0_0", o.mat(tag + ".pqr", x.rows, (4 if self.gated else 3) * H)),)
        if self.c == "atr":
            return (o.project(x, p + "hide_x/W_0_0", o.mat(tag + ".p", x.rows, H)),)
        return (o.project(x, p + "gate_x/W_0_0", o.mat(tag + ".xg", x.rows, 2 * H)),
                o.project(x, p + "hide_x/W_0_0", o.mat(tag + ".xh", x.rows, H)))

    def stepper(self, pre, s, tag=""):
        """-> step(h_prev, inp, out, out_copy=None, idx=None, mask=None): out = carry(mask, cell(h_prev[idx], inp), h_prev[idx])
        with the scope pre + "cell_<s>", the arguments of Engine.rnn_atr_step.  The scope's variables are looked up here,
        once: a scan calls the step Ls times."""
        o, e, H, gated, p = self.o, self.e, self.H, self.gated, pre + "cell_%s/" % s
        if self.lrn:                  # (no variable under cell_<s>)
            return lambda h_prev, inp, out, out_copy=None, idx=None, mask=None: \
                e.rnn_lrn_scan(h_prev, inp[0], None, out, out_copy, idx, mask, 1, False, gated)
        U, b = o.W(p + "hide_h/W_0_0"), o.b(p + "hide_h/b_0")
        if self.c == "atr":
            return lambda h_prev, inp, out, out_copy=None, idx=None, mask=None: \
                e.rnn_atr_step(h_prev, U, b, inp[0], out, out_copy, idx, mask)
        Ug, bg = o.W(p + "gate_h/W_0_0"), o.b(p + "gate_h/b_0")

        def step(h_prev, inp, out, out_copy=None, idx=None, mask=None):
            z = o.mat(tag + "gru.z", out.rows, H, F32)
            rh = o.mat(tag + "gru.rh", out.rows, H)
            e.rnn_gru_step(h_prev, Ug, bg, U, b, inp[0], inp[1], z, rh, out, out_copy, idx, mask)
        return step

    def step(self, pre, s, h_prev, inp, out, out_copy=None, idx=None, mask=None, tag=""):
        """One time step: stepper(pre, s, tag) called once."""
        self.stepper(pre, s, tag)(h_prev, inp, out, out_copy, idx, mask)

    def pair(self, h_prev, lo, hi, out, out_copy=None, idx=None):
        """lrn / olrn: out = higher(lower(h_prev[idx], lo), hi), one step of a one-to-one pair in ONE launch."""
        self.e.rnn_lrn_scan(h_prev, lo[0], hi[0], out, out_copy, idx, None, 1, False, self.gated)

    def scan(self, lo, hi, out, seq, mask, T, reverse):
        """lrn / olrn: a whole scan from the zero state in ONE launch -- rnn.rnn (hi None) or cond_rnn(one2one=True) -- over
        the T positions of sentence-major [R * T, .] Mats, backwards with `reverse`; seq: the state of every position in the
        storage type (may be a column slice), out: the fp32 state after the last scanned position; mask: fp32 Mat [R, T]."""
        self.e.rnn_lrn_scan(None, lo[0], hi[0] if hi is not None else None, out, seq, None, mask, T, reverse, self.gated)


class Scans(object):
    """The scans of an encoder over the Ls positions of a batch, from the zero state, with the source mask (a padded position
    carries the state): t = Ls-1 .. 0 with `reverse`; dest: the [B * Ls, H] Mat (maybe a column slice) that takes every
    position's state in the storage type, positions un-reversed.  The fp32 state lives in one ping-pong pair [B, H] that
    every scan uses again, and so do the input projections ("enc.lo", "enc.hi"): a scan has ended before the next begins."""

    def __init__(self, core, o, batch):
        self.cells, self.o, self.c = Cells(core, o), o, core.cell
        self.B, self.Ls, self.H, self.smask = batch["B"], batch["Ls"], core.H, batch["smask"]
        self.hs = [Mat(core.eng.buf(o.pre + "enc.h%d" % i, (self.B, core.H), F32), self.B, core.H) for i in (0, 1)]
        self.whole = Mat(self.smask, self.B, self.Ls, self.Ls)       # the mask of a one-launch scan

    def _order(self, reverse):
        return range(self.Ls - 1, -1, -1) if reverse else range(self.Ls)

    def _at(self, inp, t):
        return [_at(m, self.B, t, self.Ls) for m in inp]

    def _mask(self, t):
        return Mat(self.smask, self.B, 1, self.Ls, t)

    def plain(self, pre, x, reverse, dest):
        """rnn.rnn of the cell under `pre` over x [B * Ls, in]."""
        cells, hs = self.cells, self.hs
        inp = cells.fetch(x, pre, self.c, "enc.lo")
        if cells.lrn:
            cells.scan(inp, None, hs[0], dest, self.whole, self.Ls, reverse)
            return
        step, prev = cells.stepper(pre, self.c, "enc."), None
        for n, t in enumerate(self._order(reverse)):
            step(prev, self._at(inp, t), hs[n & 1], _at(dest, self.B, t, self.Ls), None, self._mask(t))
            prev = hs[n & 1]

    def pair(self, pre, x, below, reverse, dest):
        """cond_rnn(one2one=True) under `pre`: the lower cell on x_t, the higher on below_t (the states of the scan below)."""
        cells, (g, s) = self.cells, self.hs
        lo = cells.fetch(x, pre, self.c + "_lower", "enc.lo")
        hi = cells.fetch(below, pre, self.c + "_higher", "enc.hi")
        if cells.lrn:
            cells.scan(lo, hi, g, dest, self.whole, self.Ls, reverse)
            return
        lower, higher = cells.stepper(pre, self.c + "_lower", "enc."), cells.stepper(pre, self.c + "_higher", "enc.")
        for n, t in enumerate(self._order(reverse)):
            mask = self._mask(t)
            lower(None if n == 0 else g, self._at(lo, t), s, None, None, mask)
            higher(s, self._at(hi, t), g, _at(dest, self.B, t, self.Ls), None, mask)

    def ends(self, y2, name):
        """[f_{Ls-1} | b_0] of y2 = [forward | backward] [B * Ls, 2 H]: the state after the last scanned position of either
        scan -> the Mat [B, 2 H] `name`."""
        e, esz, H = self.o.e, self.o.storage.esz, self.H
        z = self.o.mat(name, self.B, 2 * H)
        for t, c0 in ((self.Ls - 1, 0), (0, H)):
            src = _at(y2, self.B, t, self.Ls, c0, H)
            e.lib.call("zk_gather_rows", src.ptr, src.ld * esz, None, z.ptr + c0 * esz, 2 * H * esz, self.B, H * esz, e.stream)
        return z


def _half(o_pre, l, pp):
    return o_pre + "hs.l%d.%d" % (l, pp)


def state_pair(o, l, rows, H):
    """Allocates the ping-pong pair of state layer l -> the half of parity 0, which takes the initial state."""
    first = o.e.buf(_half(o.pre, l, 0), (rows, H), F32)
    o.e.buf(_half(o.pre, l, 1), (rows, H), F32)
    return Mat(first, rows, H)


def rep_index(o, B, K):
    """-> int32 [B * K]: row r of a beam batch belongs to sentence r // K."""
    rep = o.e.buf(o.pre + "enc.rep", (B * K,), torch.int32)
    o.e.h2d(rep, np.repeat(np.arange(B, dtype=np.int32), K))
    return rep


def tile_state(o, h0, rep, l=0):
    """h0 fp32 [B, H], one row per sentence -> the initial state of layer l, K rows per sentence (rep: rep_index)."""
    H, rows = h0.cols, rep.numel()
    o.e.lib.call("zk_gather_rows", h0.ptr, H * 4, rep.data_ptr(), state_pair(o, l, rows, H).ptr, H * 4, rows, H * 4, o.e.stream)


def attend(o, state, a, sc, pm, c):
    """func.py:107-161 under the scope `a`: qa = sc Wq + bq;  c = sum_j softmax_j(v . tanh(qa + pm_j) + (1 - mask_j) * -inf)
    memory_j, written into c (a Mat of the storage type, maybe a column slice)."""
    qa = o.project(sc, a + "feed_query/W_0_0", o.mat("qa", c.rows, c.cols), bias=o.b(a + "feed_query/b_0"))
    # the kernel writes an fp32 context and a copy: the fp32 mode's context is of the storage type already, no copy
    ctx, copy = (c, None) if o.storage.dtype == F32 else (o.mat("ctx", c.rows, c.cols, F32), c)
    o.e.add_attn(qa, pm, state["encodes"], o.b(a + "feed_logits/W_0_0"), state["mask"], ctx, copy, state["K"], state["Ls"])


def logits_tail(o, x, scope):
    """-> logits Mat fp32 [rows, Vpad] = tanh(x W + b) E^T with the linear map `scope`, or x E^T (scope None); E and the
    columns are the shortlist's where the step has one (o.V, o.logits_view)."""
    core, rows = o.core, x.rows
    if scope is not None:
        pre = o.project(x, scope + "/W_0_0", o.mat("pre", rows, core.E, F32))
        x = o.mat("feat", rows, core.E)
        o.e.rnn_bias_tanh(pre, o.b(scope + "/b_0"), out_copy=x, f32=o.storage.dtype == F32)
    logits = o.logits_view(o.mat("logits", rows, core.Vpad, F32).t, rows)
    o.gemm(x, o.W(core.soft_emb), logits, rows, o.V, core.E, 1)
    return logits


class RnnState(_dec.DecodeState):
    """The decode state of a recurrent model: the per-beam cache is the fp32 [BK, H] hidden state of every state layer, each
    kept as a ping-pong pair.  reorder() hands the row index to the next step's first cell launches, which read the old
    halves through it and whose step writes the new ones.  state["decoder"]["state"]: the current half (core.layers None), or
    {"layer_l": the current half of layer l}."""

    def halves(self, pp):
        core, BK = self["_core"], self["BK"]
        return [Mat(core.eng.buf(_half(self.storage.prefix + RN, l, pp), (BK, core.H), F32), BK, core.H)
                for l in range(core.layers or 1)]

    def reorder(self, index_dev, time_dev=None, defer_aan=False):
        pp = self["_pp"]
        self["_gather"] = (self.halves(pp), index_dev)
        self["_pp"] = 1 - pp
        self.bind_caches()

    def bind_caches(self):
        hs = self.halves(self["_pp"])
        self["decoder"]["state"] = hs[0] if self["_core"].layers is None else {"layer_%d" % l: h for l, h in enumerate(hs)}

    def graph_pointers(self):
        """Every address a captured step holds (models/_decode.py adopt_graphs / retire_graphs)."""
        core = self["_core"]
        e = core.eng
        pre = self.storage.prefix + RN
        ptrs = [self["pack_dev"].data_ptr(), self["out_dev"].data_ptr(), self["mask"].data_ptr(), self["encodes"].ptr,
                self["pm"].ptr, e.seed.data_ptr(), core.store.shadow.data_ptr(), core.store.master.data_ptr()]
        ptrs += [b.data_ptr() for nm, b in sorted(e.bufs.items()) if nm.startswith(pre)]
        return ptrs


def _schedule(core):
    return importlib.import_module("zero_amd.models." + SCHEDULES[core.model])


def step(state, target, time, time_dev, hp):
    """One cached decoder step -> (logits Mat fp32 [BK, Vpad], state): the model's step(core, o, state, target, srcs, dsts,
    idx, hp) reads layer l's state from srcs[l] through the row index idx (None: rows as they are) and writes dsts[l].  A step
    that follows no reorder (time 0 of the host-side search, an eager decoding_fn call) reads the current halves with rows as
    they are and writes the others: the cell launches refuse an output that overlaps the state they read."""
    core = state["_core"]
    if time_dev is None and time >= state["Tmax"]:
        raise RuntimeError("decode step %d exceeds the allocated cache length %d" % (time, state["Tmax"]))
    if "_gather" not in state:
        state.reorder(None)
    srcs, idx = state.pop("_gather")
    o = _ops(core, state["f32"], state.get("shortlist"))
    logits = _schedule(core).step(core, o, state, target, srcs, state.halves(state["_pp"]), idx, hp)
    if time_dev is None:
        state["time_filled"] = time + 1
    return logits, state


def build_state(core, hp, source, K, max_steps):
    """encoding_fn: source batch -> RnnState, through the model's encode(core, o, batch, K) -> (memory Mat [B * Ls, M],
    [projected memory Mat [B * Ls, M] or None per attention]), which also writes the initial state, tiled K times per sentence,
    into the halves of parity 0.  Source padding and the rounding of the step count follow models/_decode.py:build_state (shape
    buckets for the step-graph cache): a padded position has mask 0, so every scan carries the state over it and the
    attentions give it the weight 0."""
    f32 = _f32.wanted(hp)
    check_shape(core, f32)
    o = _ops(core, f32)
    e = core.eng
    batch, max_steps = _dec.shape_batch(core, hp, source, max_steps)
    B, Ls = batch["B"], batch["Ls"]
    # the batch's output vocabulary is built from the source ids while the encoder runs (zero_amd/shortlist.py)
    sl = _shortlist.launch(core, hp, batch["src"], B, Ls, Ls, o.pre) if core.shortlist and _shortlist.wanted(hp) else None
    enc, pms = _schedule(core).encode(core, o, batch, K)
    mask_keep = e.buf(o.pre + "smask", (B, Ls), F32)
    mask_keep.copy_(batch["smask"])
    state = RnnState()
    state.storage = o.storage
    state.update({"_core": core, "B": B, "K": K, "BK": B * K, "Ls": Ls, "Tmax": max_steps, "encodes": enc, "pm": pms[0],
                  "pms": pms, "mask": mask_keep, "time_filled": 0, "decoder": {}, "f32": f32, "_pp": 0})
    if sl is not None:
        state["shortlist"] = _shortlist.finish(core, hp, sl, o)
    _dec.check_ngram(hp, _dec.vocab_size(state), max_steps, K)
    _dec.check_sampling(hp, _dec.vocab_size(state), max_steps, K)
    state.bind_caches()
    return _dec.finish_state(state)


def make_infer_fns(params, model_name):
    hp = params
    from zero_amd.models._factory import get_core
    _dec.ngram_size(hp)
    _dec.sampling_opts(hp)
    _dec.diverse_opts(hp)
    _dec.check_prefix_opts(hp)

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
