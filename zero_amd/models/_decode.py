# coding: utf-8
"""Incremental (cached) and full-recompute decoding steps on HIP kernels.

``infer_fn`` of the reference (models/transformer.py:252-285, transformer_aan.py:294-327)
returns two closures; so does :func:`make_infer_fns`:

  encoding_fn(source)                -> state
  decoding_fn(target, state, time)   -> (logits fp32 [B*K, ld>=V], state)

MI355X layout of ``state`` (instead of the reference's beam-tiled nest, search.py:36-39):
  * beam-invariant tensors -- encoder output, source mask and the cross-attention keys /
    values ``mk`` / ``mv`` of every layer (func.py:206-216) -- are stored ONCE per sentence
    and never tiled or reordered; the attention kernel maps query row b*K+k to sentence b
    (``kv_group=K``);
  * per-beam caches -- self-attention ``k`` / ``v`` (func.py:199-205) as preallocated
    [B*K, Tmax, H] bf16 buffers written in place at position ``time`` (no concat), the AAN
    running sum (transformer_aan.py:110-112) as fp32 [B*K, H] -- are double-buffered and
    reordered by a row gather (search.py:206-209).
``cache_init``'s dummy step (search.py:56-77) is unnecessary: mk/mv are computed by
``encoding_fn``; the values are the same.

search_mode="dev" (transformer.py:277-281) recomputes the encoder and the whole prefix
through the training-path decoder each step.
"""

import collections
import ctypes
import os
import struct
import threading

import numpy as np
import torch

from zero_amd import shortlist as _shortlist
from zero_amd.func import Mat
from zero_amd.hip import ZeroHipError
from zero_amd.models._core import trim_columns
from zero_amd.models._factory import get_core
from zero_amd.models import _decode_f32 as _f32
from zero_amd.models import _l0drop as _l0
from zero_amd.models._fixup import Fixup, fixup_ops
from zero_amd.models._ops import BF16_CACHES, F32_CACHES, Storage, ops_for  # noqa: F401  (the storages are named here too)
from zero_amd.utils import dtype as zdtype

F32 = torch.float32

# Start-up of a decode batch = the part that allocates (engine buffers, pinned staging) and captures the two step
# graphs.  With several batches in flight on execution lanes (evalu.decode_many, one host thread per lane) the
# start-ups are serialised by this lock: an allocation or a host-memory pin in one thread while another thread is
# inside a stream capture invalidated that capture on ROCm 7.x ("operation failed due to a previous error during
# capture"), whereas a thread that only replays graphs beside a capturing one is fine.  The replay loop -- ~95 % of a
# batch's time -- runs unlocked; a single-threaded caller never waits.
STARTUP_LOCK = threading.RLock()


def startup_begin():
    STARTUP_LOCK.acquire()


def startup_end(state):
    """Release the start-up lock of this batch (idempotent)."""
    if state is not None and state.get("_startup_held"):
        state["_startup_held"] = False
        STARTUP_LOCK.release()


def _startup_settled(state):
    g = state.get("graphs")
    return bool(g) and len(g) >= 2 and all(not isinstance(v, str) for v in g.values())


# ---- decode-step graphs live across batches ----------------------------------------------------------------------
# Every launch argument of a step graph is either a per-step value read from device memory or a property of the batch
# SHAPE (beam rows, padded source length, cache length) and of named engine buffers, whose addresses are stable once
# they have reached their largest size.  So the two parity graphs of a batch are kept per shape (per core, i.e. per
# execution lane) and a later batch of the same shape replays them instead of capturing its own: ~2.5 ms of the
# ~4.7 ms a batch spends before its first replayed step.  An entry is only reused if the engine has not replaced a
# buffer since (realloc_gen) AND the data pointers the graph was captured with are the ones the new batch uses.
STEP_GRAPH_CACHE = 24        # shapes per core; least recently used goes first


def _graph_pointers(state, book):
    own = getattr(state, "graph_pointers", None)      # a state that is not a Transformer layer stack names its own
    if state.get("ngram_hist") is not None:           # the history the n-gram ban reads (the book's seq, or ngram_history)
        book = (tuple(book) if book is not None else ()) + tuple(state["ngram_hist"])
    if state.get("prefix") is not None:               # the table of forced target prefixes (prefix_table) and its row stride
        book = (tuple(book) if book is not None else ()) + tuple(state["prefix"])
    if own is not None:
        return tuple(own()) + (tuple(book) if book is not None else ())
    core = state["_core"]
    e = core.eng
    ptrs = [state["pack_dev"].data_ptr(), state["out_dev"].data_ptr(), state["mask"].data_ptr(),
            state["encodes"].ptr, e.seed.data_ptr(), core.store.shadow.data_ptr()]
    for l in range(core.hp.num_decoder_layer):
        lay = state["decoder"]["state"]["layer_%d" % l]
        ptrs += [lay["mk"].ptr, lay["mv"].ptr]
    ptrs.append(core.store.master.data_ptr())
    for nm in ("aan.0", "aan.1", "k.0", "k.1", "v.0", "v.1", "logits"):
        b = e.bufs.get(state.storage.prefix + nm)
        ptrs.append(b.data_ptr() if b is not None else 0)
    ptrs += [m.ptr for _, m in sorted(state.get("wt", {}).items())]
    if state.get("kbias") is not None:          # transformer_l0drop: the log-count bias of the cross-attention keys
        ptrs.append(state["kbias"].data_ptr())
    if state.get("shortlist") is not None:      # the compact target-side tables (zero_amd/shortlist.py)
        ptrs += state["shortlist"].pointers()
    return tuple(ptrs) + (tuple(book) if book is not None else ())


def _destroy_graphs(core, graphs):
    for g in graphs.values():
        if not isinstance(g, str):
            core.eng.lib.call("zk_graph_destroy", g)
    graphs.clear()


def _f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def graph_key(state, book, temperature, forbid_value, noise, dec_group, ngram=0, sample=None, diverse=None):
    """What tells the step graphs of one batch from those of another: the shape, the search's constants and the option set
    (ngram: the n-gram size of the step's ban node, 0 = none; sample: sampling_opts' pair when the step truncates; diverse:
    diverse_opts' pair when the step selects per beam group; state["prefix"], prefix_table's: the step forces a prefix)."""
    key = (state["B"], state["K"], state["Ls"], state["Tmax"], book is not None, float(temperature),
           float(forbid_value), bool(noise), int(dec_group), bool(state.get("f32")))
    if state.get("shortlist") is not None:      # the size of the output vocabulary is part of a step's shape
        key += (("shortlist", state["shortlist"].Vs),)
    if ngram > 0:                               # a step with the ban node, and its n, is a launch sequence of its own
        key += (("ngram", int(ngram)),)
    if sampling_on(sample):                     # so is one with the truncation node, per (k, p): both are launch arguments
        key += (("sample", int(sample[0]), _f32_bits(sample[1])),)
    if diverse_on(diverse):                     # and one with the group selection, per (G, lambda): launch arguments too
        key += (("diverse", int(diverse[0]), _f32_bits(diverse[1])),)
    if state.get("prefix") is not None:         # and one with the forced-prefix node (a batch of empty prefixes has none)
        key += (("prefix",),)
    return key


def adopt_graphs(state, book, temperature, forbid_value, noise, ngram=0, sample=None, diverse=None):
    """First step of a batch: take over the cached parity graphs of its shape, if they are still valid.  ngram: the
    n-gram size of the step's ban node (0: the step has none); sample: sampling_opts(hp) (None / (0, 0.0): no truncation);
    diverse: diverse_opts(hp) (None / G = 1: the fused tail)."""
    core = state["_core"]
    e = core.eng
    # (zk_dec_group(-1) = the rows-per-workgroup geometry in force: graphs captured with several batches in flight --
    # 16 rows per workgroup -- must not be adopted by a single-stream decode, nor the reverse)
    key = graph_key(state, book, temperature, forbid_value, noise, e.lib.raw("zk_dec_group")(-1), ngram, sample, diverse)
    state["_gkey"] = key
    if os.environ.get("ZERO_HIP_DECODE_GRAPH_CACHE", "1") == "0":
        return
    cache = core.__dict__.setdefault("_step_graph_cache", collections.OrderedDict())
    ent = cache.pop(key, None)
    if ent is None:
        return
    if ent["gen"] != e.realloc_gen or ent["ptrs"] != _graph_pointers(state, book):
        torch.cuda.current_stream(e.device).synchronize()
        _destroy_graphs(core, ent["graphs"])
        return
    state["graphs"] = ent["graphs"]
    core._graph_adoptions = core.__dict__.get("_graph_adoptions", 0) + 1


def retire_graphs(state):
    """End of a batch: complete parity graphs go to the shape cache of their core, everything else is destroyed."""
    graphs = state.get("graphs") if hasattr(state, "get") else None
    if not graphs:
        return
    core = state["_core"]
    e = core.eng
    complete = len(graphs) >= 2 and all(not isinstance(g, str) for g in graphs.values())
    if complete:
        # a whole batch ran from captured graphs: the step's scratch exists for this many beam rows
        core._decode_warm_rows = max(core.__dict__.get("_decode_warm_rows", 0), state["BK"])
    key = state.get("_gkey")
    torch.cuda.current_stream(e.device).synchronize()
    if complete and key is not None and os.environ.get("ZERO_HIP_DECODE_GRAPH_CACHE", "1") != "0":
        cache = core.__dict__.setdefault("_step_graph_cache", collections.OrderedDict())
        old = cache.pop(key, None)
        if old is not None and old["graphs"] is not graphs:
            _destroy_graphs(core, old["graphs"])
        cache[key] = {"gen": e.realloc_gen, "ptrs": _graph_pointers(state, state.get("book")), "graphs": dict(graphs)}
        while len(cache) > STEP_GRAPH_CACHE:
            _, ev = cache.popitem(last=False)
            _destroy_graphs(core, ev["graphs"])
        state["graphs"] = {}
        return
    _destroy_graphs(core, graphs)


class lanes_mode(object):
    """Kernel geometry for ``n`` decode batches in flight (evalu.decode_many).  Alone, the fused attention launch is
    fastest with one sentence (4 beam rows) per workgroup: 256 workgroups of 121 KB LDS, i.e. the whole chip, 12.7 us
    against 16.5 us with 16 rows per workgroup.  With several batches in flight that launch is the one kernel of a step
    the lanes cannot overlap (it owns every CU's LDS); at 16 rows per workgroup it covers a quarter of the chip and the
    lanes' launches run side by side (measured: 4 lanes 1.5-1.6 k -> 1.9-2.2 k sentences/s)."""

    def __init__(self, n):
        self.n = int(n)

    def __enter__(self):
        from zero_amd import hip
        rows = 16 if self.n > 1 else 0
        self.prev = hip.lib().raw("zk_dec_group")(rows)
        return self

    def __exit__(self, *a):
        from zero_amd import hip
        hip.lib().raw("zk_dec_group")(self.prev)


class DecodeState(dict):
    """Nested-dict state with the cache plumbing the search needs."""

    storage = BF16_CACHES

    def reorder(self, index_dev, time_dev=None, defer_aan=False):
        """Gather every per-beam cache by flat beam index [B*K] (device int32).  time_dev: the
        number of filled cache slots lives in device memory (hipGraph replay).  The caches of all
        layers are slabs of one buffer, so each kind (aan / k / v) is ONE launch.  defer_aan: leave the gather
        of the average-attention sums to the step's input launch, where the storage has one (Storage.defer_aan)."""
        core = self["_core"]
        e, st = core.eng, self.storage
        BK, H, t = self["BK"], core.H, self["time_filled"]
        nl = core.hp.num_decoder_layer
        pp = self["_pp"]
        lay0 = self["decoder"]["state"]["layer_0"]
        if "aan" in lay0:
            src = e.buf(st.prefix + "aan.%d" % pp, (nl, BK, H), F32)
            dst = e.buf(st.prefix + "aan.%d" % (1 - pp), (nl, BK, H), F32)
            if defer_aan and st.defer_aan:
                self["_aan_gather"] = (src, index_dev)
            else:
                e.lib.call("zk_gather_rows_ex", src.data_ptr(), H * 4, index_dev.data_ptr(), dst.data_ptr(), H * 4,
                           nl * BK, H * 4, BK, e.stream)
        if "k" in lay0:
            Tmax = self["Tmax"]
            row = Tmax * H * st.esz
            for nm in ("k", "v"):
                src = e.buf("%s%s.%d" % (st.prefix, nm, pp), (nl, BK, Tmax, H), st.dtype)
                dst = e.buf("%s%s.%d" % (st.prefix, nm, 1 - pp), (nl, BK, Tmax, H), st.dtype)
                if time_dev is not None:
                    e.lib.call("zk_cache_rows", src.data_ptr(), row, index_dev.data_ptr(), dst.data_ptr(), row, nl * BK,
                               H * st.esz, Tmax, time_dev.data_ptr(), 1, BK, e.stream)
                else:
                    e.lib.call("zk_gather_rows_ex", src.data_ptr(), row, index_dev.data_ptr(), dst.data_ptr(), row,
                               nl * BK, t * H * st.esz, BK, e.stream)
        self["_pp"] = 1 - pp
        self.bind_caches()

    def bind_caches(self):
        """Point every layer's cache entries at the current ping-pong half."""
        core = self["_core"]
        e, st = core.eng, self.storage
        BK, H, nl, pp = self["BK"], core.H, core.hp.num_decoder_layer, self["_pp"]
        for l in range(nl):
            lay = self["decoder"]["state"]["layer_%d" % l]
            if "aan" in lay:
                lay["aan"] = e.buf(st.prefix + "aan.%d" % pp, (nl, BK, H), F32)[l]
            if "k" in lay:
                for nm in ("k", "v"):
                    lay[nm] = e.buf("%s%s.%d" % (st.prefix, nm, pp), (nl, BK, self["Tmax"], H), st.dtype)[l]


def append_kv(e, qkv, lay, rows, H, Tmax, esz, time, time_dev):
    """This step's keys and values (columns H .. 3H of the qkv rows) go to slot ``time`` of every row's k / v cache; with
    time_dev the slot is read from device memory (hipGraph replay).  esz: bytes per element of qkv and of the caches."""
    for nm, c0 in (("k", H), ("v", 2 * H)):
        if time_dev is not None:
            e.lib.call("zk_cache_rows", qkv.ptr + c0 * esz, 3 * H * esz, None, lay[nm].data_ptr(), Tmax * H * esz, rows,
                       H * esz, Tmax, time_dev.data_ptr(), 0, 0, e.stream)
        else:
            e.lib.call("zk_gather_rows", qkv.ptr + c0 * esz, 3 * H * esz, None, lay[nm].data_ptr() + time * H * esz,
                       Tmax * H * esz, rows, H * esz, e.stream)


def _fuse_att_ok(core, hp, K):
    """The attention sub-layers of a cached decode step as one launch per (sentence, head) (zk_dec_cross / zk_dec_self)."""
    return (os.environ.get("ZERO_HIP_DECODE_FUSE_ATT", "1") != "0" and core.d == 64
            and core.H in (128, 256, 512, 1024, 2048) and not core.fuse and not core.rela and not core.fixup
            and (not core.rpr or hp.max_relative_position <= 31)
            and (not core.aan or os.environ.get("ZERO_HIP_DECODE_FUSE_LN", "1") != "0") and not hp.use_ffn)


def vocab_size(state):
    """The number of candidates per beam row of a step: the target vocabulary, or the state's shortlist."""
    sl = state.get("shortlist")
    return state["_core"].V if sl is None else sl.Vs


NGRAM_MAX = 16      # zk_ngram_ban compares at most 15 suffix tokens


def ngram_size(hp):
    """hp.no_repeat_ngram_size as an int: 0 = off; ValueError outside 0 .. NGRAM_MAX."""
    n = getattr(hp, "no_repeat_ngram_size", 0)
    n = 0 if n is None else int(n)
    if not 0 <= n <= NGRAM_MAX:
        raise ValueError("no_repeat_ngram_size=%d: the n-gram ban takes n in 1 .. %d (0 = off)" % (n, NGRAM_MAX))
    return n


def check_ngram(hp, V_eff, Tmax, K):
    """A banned token must never be among the 2K survivors of a step: a row bans at most one token per generated
    position, Tmax of them, so V_eff - Tmax candidates are always left.  V_eff: the shortlist size where there is one."""
    if ngram_size(hp) > 0 and int(V_eff) - int(Tmax) < 2 * int(K):
        raise ValueError("no_repeat_ngram_size=%d: up to %d tokens of a row can be banned (the cache length), which leaves "
                         "fewer than 2 * beam_size = %d of the %d candidates per row for the top-2K of a step"
                         % (ngram_size(hp), Tmax, 2 * K, V_eff))


def ngram_history(state, rows, cols):
    """The n-gram ban's history of a search that keeps its books on the host: an int32 [rows, cols] device buffer under the
    decode mode's prefix plus a pinned host mirror (search.py refreshes the mirror from its sequences and uploads it next to
    the step's other inputs).  state["ngram_hist"] = (device address, row stride) is what search_tail launches with and what
    _graph_pointers compares.  -> (device tensor, pinned host tensor)"""
    core = state["_core"]
    st = getattr(state, "storage", BF16_CACHES)
    own = getattr(state, "graph_pointers", None)
    name = st.prefix + ("rn." if own is not None else "") + "ngram.hist"
    dev = core.eng.buf(name, (rows, cols), torch.int32)
    pins = core.__dict__.setdefault("_decode_pins", {})
    n = rows * cols
    host = pins.get("ngram")
    if host is None or host.numel() < n:
        host = pins["ngram"] = torch.zeros(n + n // 4, dtype=torch.int32).pin_memory()
    host = host[:n].view(rows, cols)
    host.zero_()
    state["ngram_hist"] = (dev.data_ptr(), cols)
    return dev, host


def ngram_ban(e, logits, rows, V, hist, n, forbid_value, time=0, time_dev=None):
    """zk_ngram_ban on the step's logits Mat; hist = (device address of the int32 history, its row stride).  forbid_value is
    the search tail's, dtype.inf() = +1e8 (the tail subtracts it): the ban writes -forbid_value."""
    e.lib.call("zk_ngram_ban", logits.ptr, logits.ld, rows, V, hist[0], hist[1], int(time),
               time_dev.data_ptr() if time_dev is not None else None, n, -float(forbid_value), e.stream)


def sampling_opts(hp):
    """(hp.sampling_topk, hp.sampling_topp) as (int, float): 0 / 0.0 = off; ValueError for a negative k and for p outside
    [0, 1].  p = 1.0 is an active setting that keeps everything."""
    k = getattr(hp, "sampling_topk", 0)
    p = getattr(hp, "sampling_topp", 0.0)
    k = 0 if k is None else int(k)
    p = 0.0 if p is None else float(p)
    if k < 0:
        raise ValueError("sampling_topk=%d: top-k truncation takes k >= 1 (0 = off)" % k)
    if not 0.0 <= p <= 1.0:      # (a NaN fails both comparisons)
        raise ValueError("sampling_topp=%r: nucleus truncation takes p in (0, 1] (0 = off)" % p)
    return k, p


def sampling_on(sample):
    return sample is not None and (sample[0] > 0 or sample[1] > 0.0)


def sampling_min_keep(K):
    """The entries of a row the truncation always leaves: the top-2K of a step must never have to take an overwritten
    entry, and at step 0 the tail bans EOS on top."""
    return 2 * int(K) + 1


def check_sampling(hp, V_eff, Tmax, K):
    """The truncation keeps at least min_keep = 2 * beam_size + 1 entries per row, so a row must have that many -- after the
    n-gram ban, which takes up to Tmax of them (check_ngram), where both are on.  V_eff: the shortlist size where there is
    one."""
    sample = sampling_opts(hp)
    if not sampling_on(sample):
        return
    mk = sampling_min_keep(K)
    what = "sampling_topk=%d, sampling_topp=%g" % sample
    if int(V_eff) < mk:
        raise ValueError("%s: the truncation keeps at least 2 * beam_size + 1 = %d candidates per row for the top-2K of a "
                         "step, a row has only %d" % (what, mk, V_eff))
    if ngram_size(hp) > 0 and int(V_eff) - int(Tmax) < mk:
        raise ValueError("%s with no_repeat_ngram_size=%d: up to %d tokens of a row can be banned (the cache length), which "
                         "leaves fewer than 2 * beam_size + 1 = %d of the %d candidates per row for the truncation to keep"
                         % (what, ngram_size(hp), Tmax, mk, V_eff))


def sample_truncate(e, logits, rows, V, topk, topp, min_keep, forbid_value):
    """zk_sample_truncate on the step's logits Mat.  forbid_value is the search tail's, dtype.inf() = +1e8 (the tail subtracts
    it): the truncation writes -forbid_value, as the n-gram ban does.  With both settings off there is no call."""
    if int(topk) == 0 and float(topp) == 0.0:
        return
    e.lib.call("zk_sample_truncate", logits.ptr, logits.ld, rows, V, int(topk), float(topp), int(min_keep),
               -float(forbid_value), e.stream)


def prefix_file(hp):
    """hp.tgt_prefix_file as a string: "" = off."""
    return getattr(hp, "tgt_prefix_file", "") or ""


def check_prefix_opts(hp):
    """What tgt_prefix_file does not go together with; nothing here depends on the data, so infer_fn refuses before a core is
    built."""
    if prefix_file(hp) and _shortlist.wanted(hp):
        raise NotImplementedError("tgt_prefix_file=%s with shortlist_file=%s: a forced token must be a candidate of its batch, "
                                  "i.e. the prefix ids would have to be forced into the batch's shortlist inside "
                                  "zk_shortlist_build, which is not built" % (hp.tgt_prefix_file, hp.shortlist_file))


def check_prefix(prefix, B, V, eos_id, src_len, decode_length):
    """features["prefix"] of a batch of B sentences -> (int32 [B, P] right-padded with 0, the lengths n_b [B]), or (None,
    None) for None.  ValueError, naming the sentence and the numbers: a row count other than B; an id outside [1, V); EOS; a
    0 followed by a non-zero; n_b >= src_len_b + decode_length (the search stops a sentence at that length: the hypothesis
    could not end).  Nothing here touches the device: the search calls it before the encoder pass."""
    if prefix is None:
        return None, None
    p = np.asarray(prefix.cpu() if torch.is_tensor(prefix) else prefix)
    if p.ndim != 2 or p.shape[0] != int(B):
        raise ValueError("features['prefix'] has shape %s: one row of target ids per sentence of the batch, [%d, P], is "
                         "expected" % (tuple(p.shape), B))
    if p.dtype.kind not in "iu":
        raise ValueError("features['prefix'] holds %s values: target ids are integers" % p.dtype)
    p = p.astype(np.int64)
    n = (p != 0).sum(1)
    for b in range(int(B)):
        row = p[b]
        if (row[:n[b]] == 0).any():
            t = int(np.argmax(row == 0))
            raise ValueError("prefix of sentence %d: position %d is 0 (padding) and position %d holds id %d; a prefix is "
                             "right-padded" % (b, t, int(np.nonzero(row)[0][-1]), int(row[np.nonzero(row)[0][-1]])))
        bad = np.nonzero((row[:n[b]] < 1) | (row[:n[b]] >= int(V)))[0]
        if bad.size:
            raise ValueError("prefix of sentence %d: id %d at position %d is outside [1, %d), the target vocabulary"
                             % (b, int(row[bad[0]]), int(bad[0]), V))
        if (row[:n[b]] == int(eos_id)).any():
            raise ValueError("prefix of sentence %d: position %d holds the end-of-sentence id %d; a hypothesis cannot go on "
                             "behind it" % (b, int(np.argmax(row == int(eos_id))), eos_id))
        limit = int(src_len[b]) + int(decode_length)
        if n[b] >= limit:
            raise ValueError("prefix of sentence %d: %d tokens, but the search ends a hypothesis of this sentence at source "
                             "length + decode_length = %d + %d = %d tokens: it could not end" %
                             (b, int(n[b]), int(src_len[b]), int(decode_length), limit))
    return np.ascontiguousarray(p[:, :max(1, int(n.max()) if n.size else 1)].astype(np.int32)), n.astype(np.int64)


def check_prefix_ngram(prefix, n):
    """tgt_prefix_file with no_repeat_ngram_size = n: a prefix that holds an n-gram twice is refused (ValueError naming the
    sentence, the position and the n-gram).  The ban runs ahead of the force and the force leaves the forced entry as it
    finds it, so where the ban has taken the forced token itself -- the second occurrence of the n-gram -- that entry holds
    the same forbid value as the fillers around it, ties with them, and the lowest index wins: the hypothesis would leave its
    prefix.  During a prefix the row's history IS the prefix, so this is the only case in which a ban meets a forced token,
    and it is known before the encoder pass."""
    if prefix is None or n <= 0:
        return
    for b, row in enumerate(np.asarray(prefix)):
        toks = [int(v) for v in row if int(v) != 0]
        seen = {}
        for i in range(len(toks) - n + 1):
            g = tuple(toks[i:i + n])
            if g in seen:
                raise ValueError("prefix of sentence %d with no_repeat_ngram_size=%d: the %d-gram %s at position %d is already "
                                 "at position %d; the ban would take the forced token %d and the hypothesis would leave its "
                                 "prefix" % (b, n, n, g, i, seen[g], g[-1]))
            seen[g] = i


def prefix_table(state, prefix, eos_id):
    """Upload a batch's checked prefixes (check_prefix's array, or None) for the step's force node: a persistent int32 [B,
    Tmax] device buffer under the decode mode's prefix -- the same address for every batch of a shape, so a later batch can
    adopt the captured step graphs -- filled through a pinned staging copy on the current stream.  state["prefix"] = (device
    address, row stride) is what search_tail launches with and what graph_key / _graph_pointers see; None, and no buffer is
    touched, when every prefix of the batch is empty: such a batch issues no launch.  -> state["prefix"]"""
    state["prefix"] = None
    if prefix is None or not np.asarray(prefix).any():
        return None
    core = state["_core"]
    st = getattr(state, "storage", BF16_CACHES)
    own = getattr(state, "graph_pointers", None)
    B, cols = int(state["B"]), int(state["Tmax"])
    prefix = np.asarray(prefix)
    if prefix.shape[0] != B or prefix.shape[1] > cols:
        raise ValueError("prefix table of shape %s for a batch of %d sentences and %d cache positions" %
                         (tuple(prefix.shape), B, cols))
    dev = core.eng.buf(st.prefix + ("rn." if own is not None else "") + "prefix.tbl", (B, cols), torch.int32)
    pins = core.__dict__.setdefault("_decode_pins", {})
    n = B * cols
    host = pins.get("prefix")
    if host is None or host.numel() < n:
        host = pins["prefix"] = torch.zeros(n + n // 4, dtype=torch.int32).pin_memory()
    host = host[:n].view(B, cols)
    host.zero_()
    host.numpy()[:, :prefix.shape[1]] = prefix
    dev.copy_(host, non_blocking=True)
    state["prefix"] = (dev.data_ptr(), cols)
    state["prefix_eos"] = int(eos_id)
    return state["prefix"]


def prefix_force(e, logits, rows, V, table, K, eos_id, forbid_value, time=0, time_dev=None):
    """zk_prefix_force on the step's logits Mat; table = (device address of the int32 prefix table, its row stride), K = the
    beam rows per sentence (the model's beam_size: the groups of a diverse beam share the sentence's prefix).  forbid_value is
    the search tail's, dtype.inf() = +1e8: a forced row holds -forbid_value everywhere but at its token, -2 * forbid_value
    at eos_id."""
    e.lib.call("zk_prefix_force", logits.ptr, logits.ld, rows, V, table[0], table[1], int(K), int(time),
               time_dev.data_ptr() if time_dev is not None else None, int(eos_id), -float(forbid_value), e.stream)


DIVERSE_DEPTH_MAX = 16      # the deepest candidate list zk_beam_topk returns per row (TOPK_MAX of zk_decode.hip)


def diverse_opts(hp, K=None):
    """(hp.diverse_beam_groups, hp.diverse_beam_strength) as (int G, float lambda) for beam size K (default hp.beam_size);
    G = 1 = off, and the strength is then ignored: (1, 0.0).  ValueError, in this order, for G < 1, a beam size that is no
    multiple of G, a negative or non-finite strength, and beam_size + beam_size / G > DIVERSE_DEPTH_MAX (the depth of the
    per-row candidate lists from which a group's selection is exact, see search_tail)."""
    G = getattr(hp, "diverse_beam_groups", 1)
    lam = getattr(hp, "diverse_beam_strength", 0.5)
    G = 1 if G is None else int(G)
    lam = 0.5 if lam is None else float(lam)
    K = int(hp.beam_size if K is None else K)
    if G < 1:
        raise ValueError("diverse_beam_groups=%d: diverse beam search takes G >= 2 groups (1 = off)" % G)
    if G == 1:
        return 1, 0.0
    if K % G != 0:
        raise ValueError("diverse_beam_groups=%d: beam_size=%d is no multiple of the number of groups" % (G, K))
    if not 0.0 <= lam < float("inf"):      # (a NaN fails both comparisons)
        raise ValueError("diverse_beam_strength=%r: the Hamming penalty takes a finite strength >= 0" % lam)
    if K + K // G > DIVERSE_DEPTH_MAX:
        raise ValueError("diverse_beam_groups=%d with beam_size=%d: the step needs beam_size + beam_size / G = %d + %d = %d "
                         "candidates per beam row, the per-row top-k returns at most %d"
                         % (G, K, K, K // G, K + K // G, DIVERSE_DEPTH_MAX))
    return G, lam


def diverse_on(diverse):
    return diverse is not None and diverse[0] > 1


def search_tail(state, core, logits, noise, temperature, forbid_value, ngram=0, sample=None, diverse=None):
    """search.py:143-176 (+ 198-228 with the device-resident bookkeeping) on the step's fp32 ``logits`` Mat [B*K, ld]:
    optional Gumbel noise, the n-gram ban (ngram > 0: no_repeat_ngram_size), then temperature, log-softmax, EOS ban, length
    penalty and top-2K in the fused tail.  With sample = sampling_opts' pair active (sampling_topk / sampling_topp) the order
    is n-gram ban, truncation, noise, tail: the noise then draws from the truncated distribution, and banned tokens -- at the
    forbid value, with mass 0 and the lowest rank -- stay out of the counts and the mass.  With diverse = (G, lambda, eos_id),
    G > 1 (diverse_opts + the EOS id: diverse_beam_groups / diverse_beam_strength), the fused tail is replaced by the per-row
    top-k, zk_diverse_select and the bookkeeping on B*G pseudo-sentences (below).  With state["prefix"] set (prefix_table:
    tgt_prefix_file) zk_prefix_force runs directly ahead of either tail, and ahead of the truncation where there is one.  Launches on the current stream with
    the scratch of ``core``'s engine; shared by the single-model step and the ensemble step (models/_ensemble.py)."""
    e = core.eng
    book = state.get("book")
    sb = state["stepbuf"]
    V = vocab_size(state)
    if sampling_on(sample):
        if ngram > 0:
            ngram_ban(e, logits, state["BK"], V, state["ngram_hist"], ngram, forbid_value, time_dev=sb[0:1])
            ngram = 0
        if state.get("prefix") is not None:
            # a forced token outside the kept set would be truncated to the forbid value, which the force below -- it leaves
            # the forced entry as it finds it -- could not undo: force ahead of the truncation too.  The forced entry is then
            # the row's only real one and survives; the truncation lifts EOS from twice the forbid value back to it, which
            # the force ahead of the tail puts right again.  (This combination has two force launches per step.)
            prefix_force(e, logits, state["BK"], V, state["prefix"], state["K"], state["prefix_eos"], forbid_value,
                         time_dev=sb[0:1])
        sample_truncate(e, logits, state["BK"], V, sample[0], sample[1], sampling_min_keep(state["K"]), forbid_value)
    if noise:      # search.py:143-145; a fresh stream position every step
        e.lib.call("zk_add_gumbel", logits.ptr, state["BK"], V, logits.ld, float(zdtype.epsilon()),
                   e.seed.data_ptr(), 7001, e.stream)
        e.lib.call("zk_seed_advance", e.seed.data_ptr(), 1, e.stream)
    if ngram > 0:
        # the rows' histories are the search's sequences, in the row order of the logits: the device-resident book's seq
        # (the previous step's advance wrote the alive rows in the order flat_idx reorders the caches to), or the buffer
        # the host refreshes (ngram_history); the step's time word is read on the device
        ngram_ban(e, logits, state["BK"], V, state["ngram_hist"], ngram, forbid_value, time_dev=sb[0:1])
    if state.get("prefix") is not None:
        # tgt_prefix_file: the last launch ahead of the tail, so a forced token wins over a ban, a truncation and the noise;
        # the rows of a sentence are the model's beam (all groups of a diverse beam), the time word is read on the device
        prefix_force(e, logits, state["BK"], V, state["prefix"], state["K"], state["prefix_eos"], forbid_value,
                     time_dev=sb[0:1])
    if diverse_on(diverse):
        # Diverse beam search: three launches instead of the fused tail.  (1) zk_beam_topk with B*K "sentences" of beam 1:
        # every row's k2 = K + K/G best (score, token).  That depth is exact: a kept candidate with an unpenalised token has
        # fewer than 2K/G unpenalised and at most (G-1) K/G penalised entries of its row above it, and a penalised one below
        # the row's top k2 has at least 2K/G + 1 unpenalised ones above it.  (2) zk_diverse_select: per group, in order, the
        # 2K/G best under the Hamming penalty.  (3) the unchanged bookkeeping on (B*G, K/G): the book was built with these
        # sizes (search.py), and the flat row indices of the pseudo-sentences are the model's.
        G, lam, eos_id = diverse
        K, BK = state["K"], state["BK"]
        k2 = K + K // G
        assert k2 <= 2 * K        # check_ngram / check_sampling leave 2K (2K + 1) candidates per row: enough for the lists
        cs = e.buf("bs.dv.s", (BK, k2), F32)
        ci = e.buf("bs.dv.i", (BK, k2), torch.int32)
        e.beam_topk(logits, state["prev"], cs, ci, BK, 1, V, k2, temperature, 1.0, -1, forbid_value, scal_dev=sb[1:3])
        e.diverse_select(cs, ci, state["ts"], state["ti"], state["B"], K, G, k2, V, lam, 1.0, eos_id, penalty_dev=sb[1:2])
        if book is not None:
            e.lib.call("zk_beam_dev_advance", *book, e.stream)
        return
    fused_tail = False
    if book is not None:
        # merge of the chunked top-2K and the alive / finished bookkeeping in one launch
        ws = e.workspace(e.lib.query("zk_beam_topk_workspace", state["B"], state["K"], 2 * state["K"]))
        e.lib.ncalls += 1
        rc = e.lib.raw("zk_beam_topk_advance")(logits.ptr, logits.ld, float(temperature), float(forbid_value),
                                               ws.data_ptr(), ws.numel(), *book, e.stream)
        if rc not in (0, -2):
            e.lib.call("zk_beam_topk_advance", logits.ptr, logits.ld, float(temperature), float(forbid_value),
                       ws.data_ptr(), ws.numel(), *book, e.stream)      # raises with the library's message
        fused_tail = rc == 0
    if not fused_tail:
        e.beam_topk(logits, state["prev"], state["ts"], state["ti"], state["B"], state["K"], V,
                    2 * state["K"], temperature, 1.0, -1, forbid_value, scal_dev=sb[1:3])
        if book is not None:
            e.lib.call("zk_beam_dev_advance", *book, e.stream)


def _transposed(core, name):
    """bf16 copy of a projection weight with the input dimension contiguous (row = output channel): the operand layout of
    the fused decode kernels' matrix-core fragments.  Made by zk_transpose_bf16 once per WEIGHT VERSION (an optimiser
    update, a checkpoint load or an EMA swap makes a new one: variables.VariableStore.weight_version), not per
    encoded batch."""
    W = core.store.s(name)
    cache = core.__dict__.setdefault("_wt_cache", {})
    ver = core.store.weight_version
    ent = cache.get(name)
    if ent is None or ent[0] != ver or ent[2] != core.eng.realloc_gen:
        buf = core.eng.buf("dc.wt." + name, (W.shape[1], W.shape[0]), W.dtype)
        core.eng.lib.call("zk_transpose_bf16", W.data_ptr(), W.shape[1], buf.data_ptr(), W.shape[0], W.shape[0],
                          W.shape[1], core.eng.stream)
        ent = cache[name] = (ver, Mat(buf, W.shape[1], W.shape[0]), core.eng.realloc_gen)
    return ent[1]


def _cross_unfused(core, e, hp, state, lay, x, p, pre, l, time, time_dev):
    """Encoder-decoder attention sub-layer of a decode step, one launch per op."""
    H, nh, d = core.H, core.nh, core.d
    BK, K, Ls = state["BK"], state["K"], state["Ls"]
    q = e.mat("dc.q", BK, H)
    core._linear(x, p + "q_map", q)
    att = e.mat("dc.att", BK, H)
    rk = core.store.s(p + "rpr_keys/embeddings") if core.rpr else None
    rv = core.store.s(p + "rpr_values/embeddings") if core.rpr else None
    if core.rela:
        # rela.py:44-81: the K beam rows of a sentence share one pass over its keys / values; the source mask multiplies
        core._rela_attn(q, lay["mk"], lay["mv"], att, BK, 1, Ls, p, state["mask"], bsq=H, bsk=Ls * 2 * H, bsv=Ls * 2 * H,
                        kv_group=K)
    else:
        e.attn_fwd(q, lay["mk"], lay["mv"], att, None, BK, nh, 1, Ls, d, kmask=state["mask"], causal=False,
                   q_pos0=time if time is not None else 0, rpr_k=rk, rpr_v=rv, max_rel=hp.max_relative_position, bsq=H,
                   bsk=Ls * 2 * H, bsv=Ls * 2 * H, kv_group=K, pos_dev=time_dev, pos_flags=1)
    if core.fuse:
        # func.py:258-272: v_q = v_map(query); cache += v_q; o += cache / (time + 1)
        vq = e.mat("dc.vq", BK, H)
        core._linear(x, p + "v_map", vq)
        e.lib.call("zk_fuse_decode", vq.ptr, lay["aan"].data_ptr(), att.ptr, BK, H,
                   1.0 if time_dev is not None else 1.0 / float(time + 1),
                   time_dev.data_ptr() if time_dev is not None else None, e.stream)
    y = e.mat("dc.y", BK, H)
    core._linear(att, p + "o_map", y)
    x = core._ln_fwd(x, y, pre + "/" + core.cross, "dc%d.ca" % l, False, 0.0, 0)
    return x


# ---- what a model variant refuses ----------------------------------------------------------------------------------
def _l0drop_bf16_shape(core, hp, K):
    if not _fuse_att_ok(core, hp, K):
        return ("transformer_l0drop in bf16 decodes through the fused attention launch only "
                "(ZERO_HIP_DECODE_FUSE_ATT not 0, a head size of 64 -- got %d -- and a hidden size that is a "
                "power of two in 128 .. 2048 -- got %d); decode_dtype=float32 has none of these limits" % (core.d, core.H))


def _rela_bf16_shape(core, hp, K):
    if core.d % 8 != 0 or core.d > 128 or core.H > 2048:
        return ("transformer_rela in bf16 needs a head size that is a multiple of 8 and at most 128 -- got %d -- "
                "and a hidden size of at most 2048 -- got %d (zk_rela_attn reads keys 16 bytes at a time and "
                "keeps four rows of H floats in LDS); decode_dtype=float32 takes any head size" % (core.d, core.H))


# Per model name, what the variant does not do (a name that is not listed has no limit of its own):
#   cache_only   the NotImplementedError text of a search_mode other than "cache"
#   bf16_shape   (core, hp, K) -> the ValueError text of a shape its bf16 kernels do not take, or None
#   member       (exception type, text with the member's index) of its refusal as an ensemble member
VARIANT_LIMITS = {
    "transformer_l0drop": dict(
        cache_only="transformer_l0drop decodes with search_mode=cache only (the other mode re-runs the "
                   "training-path decoder, which this model does not have here)",
        bf16_shape=_l0drop_bf16_shape,
        member=(ZeroHipError, "ensemble member %d is a transformer_l0drop: its pruned memory has a length of its own per "
                              "batch, the members of an ensemble step share one shape")),
    "transformer_rela": dict(
        cache_only="transformer_rela decodes with search_mode=cache only: search_mode=dev re-runs the "
                   "training-path decoder, which this model does not have here",
        bf16_shape=_rela_bf16_shape,
        member=(NotImplementedError, "ensemble member %d is a transformer_rela: the ensemble step is built from the fused "
                                     "softmax attention launches, which this model does not use; composing it is not built")),
    "transformer_fixup": dict(
        cache_only="transformer_fixup decodes with search_mode=cache only: the re-encoding decode mode "
                   "(search_mode=dev re-runs the encoder and the whole prefix each step) is not built for it",
        member=(NotImplementedError, "ensemble member %d is a transformer_fixup: an untested member type (its step takes "
                                     "the launch-per-op path, the ensemble step is built from the fused launches)")),
    "rnnsearch": dict(
        cache_only="rnnsearch decodes with search_mode=cache only: search_mode=dev re-runs the encoder and the "
                   "training-path decoder over the whole prefix each step, which is not built for it",
        member=(NotImplementedError, "ensemble member %d is a rnnsearch: the ensemble step is built from the Transformer's "
                                     "fused attention launches and shares per-layer caches between members; composing a "
                                     "recurrent member is not built")),
    "rnnsearch_deepatt": dict(
        cache_only="rnnsearch_deepatt decodes with search_mode=cache only: search_mode=dev re-runs the encoder stack and "
                   "the training-path decoder over the whole prefix each step, which is not built for it",
        member=(NotImplementedError, "ensemble member %d is a rnnsearch_deepatt: the ensemble step is built from the "
                                     "Transformer's fused attention launches and shares per-layer caches between members; "
                                     "composing a recurrent member is not built")),
    "deepnmt": dict(
        cache_only="deepnmt decodes with search_mode=cache only: search_mode=dev re-runs the encoder stack and the "
                   "training-path decoder over the whole prefix each step, which is not built for it",
        member=(NotImplementedError, "ensemble member %d is a deepnmt: the ensemble step is built from the Transformer's "
                                     "fused attention launches and shares per-layer caches between members; composing a "
                                     "recurrent member is not built")),
}


def check_search_mode(model_name, hp):
    text = VARIANT_LIMITS.get(model_name, {}).get("cache_only")
    if text is not None and hp.search_mode != "cache":
        raise NotImplementedError(text)


def check_bf16_shape(model_name, core, hp, K):
    shape = VARIANT_LIMITS.get(model_name, {}).get("bf16_shape")
    text = shape(core, hp, K) if shape is not None else None
    if text is not None:
        raise ValueError(text)


def check_member(model_name, i):
    exc, text = VARIANT_LIMITS.get(model_name, {}).get("member", (None, None))
    if exc is not None:
        raise exc(text % i)


# ---- start-up of a batch -------------------------------------------------------------------------------------------
def pad_len():
    """ZERO_HIP_DECODE_PAD_LEN: the multiple that source lengths and step counts are rounded up to."""
    return max(1, int(os.environ.get("ZERO_HIP_DECODE_PAD_LEN", "8")))


def shape_batch(core, hp, source, max_steps):
    """Upload ``source`` in its shape bucket -> (the batch of core.upload, the step count).  Shape bucketing for the
    step-graph cache: the source is padded (id 0 = pad: masked in the encoder and in every cross-attention,
    func.py:372-387) and the cache length rounded up to a multiple of pad_len(), so that length-sorted batches fall into few
    shapes.  Masked keys contribute exact zeros to the softmax sums: hypotheses and scores are unchanged
    (tests/test_gpu_model.py).  max_steps None: the longest source + decode_length + 2."""
    pad = pad_len()
    src = np.asarray(source.cpu() if torch.is_tensor(source) else source)
    if pad > 1:
        trimmed = trim_columns(src)
        batch = core.upload(np.pad(trimmed, ((0, 0), (0, -trimmed.shape[1] % pad))), trim=False)
    else:
        batch = core.upload(src)
    if max_steps is None:
        max_steps = int((src != 0).sum(1).max()) + hp.decode_length + 2
    return batch, -(-int(max_steps) // pad) * pad


def _fused_weights(state, core, hp):
    """bf16 only: state['wt'], the transposed projection weights of the fused attention launches -- left empty where they
    do not apply, and the step then takes the launch-per-op path (_cross_unfused) instead of failing mid-decode.  The
    fused launches keep a sentence's scores in LDS (64 bytes per key for 16 rows), and the whole workgroup state must
    fit the 160 KiB of a CU."""
    e, H, K = core.eng, core.H, state["K"]
    keys = max(state["Ls"], state["Tmax"])
    if _fuse_att_ok(core, hp, K) and keys <= 1024 and \
            e.lib.query("zk_dec_attn_lds", H, keys, hp.max_relative_position if core.rpr else -1) <= 160 * 1024:
        for l in range(hp.num_decoder_layer):
            blocks = [(core.cross, ("q_map", "o_map"))]
            if not core.aan:
                blocks.append(("self_attention", ("qkv_map", "o_map")))
            for blk, maps in blocks:
                for m in maps:
                    nm = "decoder/layer_%d/%s/dot_attention/%s/W_0_0" % (l, blk, m)
                    state["wt"][nm] = _transposed(core, nm)
    if core.l0drop and not state["wt"]:
        raise ValueError("transformer_l0drop in bf16 decodes through the fused attention launch only: its workgroup "
                         "keeps the scores of max(memory slots, cache positions) = %d keys in LDS, at most 1024 of them "
                         "and within the 160 KiB of a CU at hidden size %d; decode_dtype=float32 has no such limit"
                         % (keys, H))


def _encode_bf16(core, hp, batch, o):
    return core.encode(batch, False, False)


def build_state(core, hp, model_name, source, K, max_steps):
    """encoding_fn of both decode modes: source batch -> DecodeState."""
    e, H = core.eng, core.H
    f32 = _f32.wanted(hp)
    # nothing here depends on the data: refuse before the encoder pass
    if f32:
        _f32.check_model(core)
    else:
        check_bf16_shape(model_name, core, hp, K)
    # the ops of the mode and its encoder: fp32 masters, activations and caches through zk_f32_* (models/_decode_f32.py), or
    # the training path's bf16 forward
    o = ops_for(core, f32)
    encode = _f32.encode if f32 else _encode_bf16
    st = o.storage
    batch, max_steps = shape_batch(core, hp, source, max_steps)
    B, Ls = batch["B"], batch["Ls"]
    if not _shortlist.wanted(hp):      # (a shortlist's size is known once it is built: checked below)
        check_ngram(hp, core.V, max_steps, K)
        check_sampling(hp, core.V, max_steps, K)
    # the batch's output vocabulary is built from the source ids while the encoder runs (zero_amd/shortlist.py)
    sl = _shortlist.launch(core, hp, batch["src"], B, Ls, Ls, o.pre) if _shortlist.wanted(hp) else None
    enc, smask = encode(core, hp, batch, o)
    kbias = None
    if core.l0drop:
        # the pruned memory, its mask and its length stand in for the encoder output from here on (models/_l0drop.py)
        enc_keep, mask_keep, Ls, kbias = _l0.prune(core, enc, smask, B, Ls, pad_len(), o)
    else:
        enc_keep = o.mat("enc", B * Ls, H)
        enc_keep.t.copy_(enc.t)
        mask_keep = e.buf(st.prefix + "smask", (B, Ls), F32)
        mask_keep.copy_(smask)
    BK = B * K
    nl = hp.num_decoder_layer
    state = DecodeState()
    state.storage = st
    state.update({"_core": core, "B": B, "K": K, "BK": BK, "Ls": Ls, "Tmax": max_steps, "encodes": enc_keep,
                  "mask": mask_keep, "time_filled": 0, "decoder": {"state": {}}, "f32": f32, "wt": {}, "_pp": 0})
    if kbias is not None:
        state["kbias"] = kbias
    if sl is not None:
        state["shortlist"] = _shortlist.finish(core, hp, sl, o)
        check_ngram(hp, state["shortlist"].Vs, max_steps, K)
        check_sampling(hp, state["shortlist"].Vs, max_steps, K)
    for l in range(nl):
        p = "decoder/layer_%d/%s/dot_attention/" % (l, core.cross)
        kv = o.mat("%d.kv" % l, B * Ls, 2 * H)
        o.linear(enc_keep, p + "k_map", kv.cols_slice(0, H))
        o.linear(enc_keep, p + "v_map", kv.cols_slice(H, 2 * H))
        lay = {"mk": kv.cols_slice(0, H), "mv": kv.cols_slice(H, 2 * H)}
        if core.aan or core.fuse:
            lay["aan"] = None
        else:
            lay["k"] = lay["v"] = None
        state["decoder"]["state"]["layer_%d" % l] = lay
    if not f32:
        _fused_weights(state, core, hp)
    if core.aan or core.fuse:
        e.zero(e.buf(st.prefix + "aan.0", (nl, BK, H), F32))
        e.buf(st.prefix + "aan.1", (nl, BK, H), F32)
    else:
        for nm in ("k", "v"):
            for half in (0, 1):
                e.buf("%s%s.%d" % (st.prefix, nm, half), (nl, BK, max_steps, H), st.dtype)
    state.bind_caches()
    if f32:      # the launch-per-op form of the fp32 step (ZERO_HIP_F32_FUSE=0) tests for an all-pad input on its own
        state["zero_flag"] = e.buf("dq.zflag", (1,), torch.int32)
    return finish_state(state)


def finish_state(state):
    """The part of a batch's state that does not depend on the step's dtype: the packed host <-> device buffers of
    the search and the graph table."""
    core = state["_core"]
    e = core.eng
    B, K, BK = state["B"], state["K"], state["BK"]
    # per-step scalars live in device memory ({time, float bits of the length penalty, EOS-ban id}):
    # a captured decode-step graph reads the current values at replay time
    # what the host hands to a (replayed) step -- last tokens, previous log-probs, beam reorder index and
    # the per-step scalars {time, float bits of the length penalty, EOS-ban id} -- is ONE pinned buffer
    # and one async copy; what comes back (top-2K scores and flat indices) is one copy as well
    pack = e.buf("bs.pack", (3 * BK + 4,), torch.int32)
    state["pack_dev"] = pack
    pins = core.__dict__.setdefault("_decode_pins", {})       # pinned staging survives the batch (pinning ~0.2 ms)

    def pinned(name, n):
        t = pins.get(name)
        if t is None or t.numel() < n:
            t = pins[name] = torch.zeros(n + n // 4, dtype=torch.int32).pin_memory()
        t[:n].zero_()
        return t[:n]
    state["pack_host"] = pinned("pack", 3 * BK + 4)
    state["tok"] = pack[0:BK]
    state["prev"] = pack[BK:2 * BK].view(torch.float32)
    state["idx"] = pack[2 * BK:3 * BK]
    state["stepbuf"] = pack[3 * BK:3 * BK + 4]
    out = e.buf("bs.out", (2, B, 2 * K), torch.int32)
    state["out_dev"] = out
    state["out_host"] = pinned("out", 2 * B * 2 * K).view(2, B, 2 * K)
    state["ts"] = out[0].view(torch.float32)
    state["ti"] = out[1]
    state["graphs"] = {}
    # every launch argument of a step is static: the time step (cache slot, number of valid keys,
    # relative-position origin) is read from device memory by the kernels
    state["static_ok"] = True
    return state


# ---- the step-graph driver -----------------------------------------------------------------------------------------
def _capture(state, core, body, check_realloc):
    """body() captured into a hipGraph -> its executable, or None.  The python-side ping-pong bookkeeping runs during a
    capture exactly as in an eager call.  A capture that fails (an allocation met it: a workspace grew, or another
    thread allocated -- ROCm 7 invalidates captures across threads) must not cost the evaluation, and the training run
    with it: the python-side flip of the aborted pass is undone and the caller runs the step eagerly."""
    e = core.eng
    pp0, gen0 = state["_pp"], e.realloc_gen
    try:
        gexec = e.graph_capture(body)
        core._decode_step_launches = e.last_graph_nodes
        if check_realloc and e.realloc_gen != gen0:
            e.lib.call("zk_graph_destroy", gexec)
            raise RuntimeError("buffer replaced during capture")
        return gexec
    except Exception:
        torch.cuda.synchronize(e.device)
        state["_pp"] = pp0
        state.bind_caches()
        return None


def run_step(state, core, body, fast_capture):
    """One decode step whose launch sequence ``body()`` is identical every step (per ping-pong parity): the first call
    of a parity runs it eagerly (that sizes the scratch), the second captures it into a hipGraph, later calls redo the
    python-side pointer flip and replay; a failed capture costs one eager step and the next step of the parity tries
    again.  fast_capture: where a batch of at least this many beam rows has already been decoded from graphs on this
    engine (core._decode_warm_rows), the step's scratch buffers exist, so capture straight away instead of spending an
    eager pass first; if that capture does hit an allocation after all (a larger source length can grow a workspace),
    take the eager route.  Releases the batch's start-up lock once both parity graphs exist."""
    e = core.eng
    graphs, parity = state["graphs"], state["_pp"]
    g = graphs.get(parity)
    if g is None and fast_capture and core.__dict__.get("_decode_warm_rows", 0) >= state["BK"]:
        g = _capture(state, core, body, True)
        if g is None:
            core._decode_warm_rows = 0
        else:
            graphs[parity] = g
            e.graph_launch(g)
    elif g == "warm":
        g = _capture(state, core, body, False)
        if g is not None:
            graphs[parity] = g
            e.graph_launch(g)
    elif g is not None:
        state["_pp"] = 1 - state["_pp"]           # replay: redo the python-side pointer flip
        state.bind_caches()
        e.graph_launch(g)
    if g is None:
        graphs.setdefault(parity, "warm")
        body()
    if state.get("_startup_held") and _startup_settled(state):
        startup_end(state)


def static_step(state, hp, logits_of, fast_capture, temperature, forbid_value, defer_aan=False, sample=None):
    """One whole decode step with every per-step value read from device memory: the bookkeeping head, the beam reorder of
    the caches (indices chosen by the previous step), the step itself -- logits_of(state, time_dev) -> fp32 logits Mat --
    and the fused log-softmax + length penalty + top-2K, through run_step.  A batch whose state carries no "_gkey" yet
    first asks the cross-batch cache for the graphs of its shape.  sample: the truncation's (topk, topp); None = hp's."""
    core = state["_core"]
    e = core.eng
    book = state.get("book")          # device-resident search bookkeeping (search._beam_search_device)
    noise = hp.enable_noise_beam_search
    ngram = ngram_size(hp)
    if sample is None:
        sample = sampling_opts(hp)
    diverse = diverse_opts(hp, state["K"])
    if "_gkey" not in state:
        adopt_graphs(state, book, temperature, forbid_value, noise, ngram, sample, diverse)
    if diverse_on(diverse):
        diverse = diverse + (hp.tgt_vocab.eos(),)

    def body():
        time_dev = state["stepbuf"][0:1]
        if book is not None:
            e.lib.call("zk_beam_dev_prepare", *book, e.stream)
        state.reorder(state["idx"], time_dev=time_dev, defer_aan=defer_aan)
        search_tail(state, core, logits_of(state, time_dev), noise, temperature, forbid_value, ngram, sample, diverse)
    run_step(state, core, body, fast_capture)


def make_infer_fns(params, model_name):
    hp = params
    _shortlist.check(hp, model_name)
    check_search_mode(model_name, hp)
    ngram_size(hp)
    sampling_opts(hp)
    diverse_opts(hp)
    check_prefix_opts(hp)

    def encoding_fn(source, beam_size=None, max_steps=None):
        core = get_core(hp, model_name)
        return build_state(core, hp, model_name, source, hp.beam_size if beam_size is None else beam_size, max_steps)

    def step_static(state, temperature, forbid_value):
        static_step(state, hp, lambda st, time_dev: _step_cache(st["tok"], st, None, time_dev=time_dev)[0], True,
                    temperature, forbid_value, defer_aan=state["_core"].aan)

    def _step_cache(target, state, time, time_dev=None):
        core = state["_core"]
        e, H, nh, d = core.eng, core.H, core.nh, core.d
        BK, K, B, Ls, Tmax = state["BK"], state["K"], state["B"], state["Ls"], state["Tmax"]
        if time_dev is None and time >= Tmax:
            raise RuntimeError("decode step %d exceeds the allocated cache length %d" % (time, Tmax))
        if state.get("f32"):
            return _f32.step_cache(target, state, time, time_dev, hp)
        if core.fixup:
            # launch-per-op: projection, the softmax attention kernels, o_map, zk_fixup_residual (models/_fixup.py)
            return Fixup(core, fixup_ops(core, False)).step(target, state, time, time_dev, hp)
        fuse_ln = core.aan and os.environ.get("ZERO_HIP_DECODE_FUSE_LN", "1") != "0"
        # an attention sub-layer (projection, attention, the head's share of the output projection) as ONE launch per
        # (sentence, head) with the previous LayerNorm as its prologue (zk_dec_cross / zk_dec_self)
        fuse_att = bool(state.get("wt")) and _fuse_att_ok(core, hp, K)
        eps = zdtype.epsilon()
        tdev = time_dev.data_ptr() if time_dev is not None else None

        def ln_args(pro):
            """(x, ybuf, gamma, beta, xout, H, eps, z, cat_in, parts, nparts, part_stride, bias, cache, cat_out,
            inv_count, time_dev) of zk_dec_* / zk_ln_decode's row-local LayerNorm; pro None: no prologue."""
            if pro is None:
                return None
            g = lambda k: pro.get(k)
            return (g("x"), g("ybuf"), g("gamma"), g("beta"), g("out"), H, eps, g("z"), g("cat"), g("parts"),
                    g("nparts") or 0, g("stride") or 0, g("bias"), None, None, 1.0, None)

        def ln_scope(scope):
            return dict(gamma=core.b(scope + "/layer_norm/scale").data_ptr(),
                        beta=core.b(scope + "/layer_norm/offset").data_ptr())

        def rpr_tabs(p):
            """(rpr_k, rpr_v, max_rel) of the attention scope p: relative positions inside the fused launch (round 4)."""
            if not core.rpr:
                return (None, None, 0)
            return (core.store.s(p + "rpr_keys/embeddings").data_ptr(), core.store.s(p + "rpr_values/embeddings").data_ptr(),
                    hp.max_relative_position)

        def dec_cross(x_in, pro, p, lay, parts):
            la = ln_args(pro) or (x_in.ptr, None, None, None, None, H, eps, None, None, None, 0, 0, None, None, None,
                                  1.0, None)
            Wq, Wo = state["wt"][p + "q_map/W_0_0"], state["wt"][p + "o_map/W_0_0"]
            tail = (Wo.ptr, Wo.ld, parts.data_ptr(), B, K, nh, Ls, float(d) ** -0.5, zdtype.inf()) + rpr_tabs(p) + \
                (0 if time_dev is not None else time, tdev, e.stream)
            head = la + (Wq.ptr, Wq.ld, core.b(p + "q_map/b_0").data_ptr(), lay["mk"].ptr, lay["mv"].ptr, lay["mk"].ld,
                         lay["mv"].ld, Ls * 2 * H, Ls * 2 * H, state["mask"].data_ptr(), Ls)
            if core.l0drop:       # the counting slot's weight (zk_dec_cross_kb)
                e.lib.call("zk_dec_cross_kb", *head, state["kbias"].data_ptr(), *tail)
            else:
                e.lib.call("zk_dec_cross", *head, *tail)

        def dec_self(x_in, pro, p, lay, parts):
            la = ln_args(pro) or (x_in.ptr, None, None, None, None, H, eps, None, None, None, 0, 0, None, None, None,
                                  1.0, None)
            Wq, Wo = state["wt"][p + "qkv_map/W_0_0"], state["wt"][p + "o_map/W_0_0"]
            e.lib.call("zk_dec_self", *la, Wq.ptr, Wq.ld, core.b(p + "qkv_map/b_0").data_ptr(), lay["k"].data_ptr(),
                       lay["v"].data_ptr(), Tmax, 0 if time_dev is not None else time, tdev, Wo.ptr, Wo.ld,
                       parts.data_ptr(), B, K, nh, float(d) ** -0.5, *rpr_tabs(p), e.stream)

        def ln_parts(x_in, scope, p, parts, tag):
            """x = LayerNorm(x_in + bf16(sum of the nh partial output projections + o_map bias))"""
            out = e.mat(tag + ".o", BK, H)
            ls = ln_scope(scope)
            e.lib.call("zk_ln_decode", x_in.ptr, e.mat("dc.y", BK, H).ptr, ls["gamma"], ls["beta"], out.ptr, BK, H, eps,
                       None, None, parts.data_ptr(), nh, BK * H, core.b(p + "o_map/b_0").data_ptr(), None, None, 1.0,
                       None, e.stream)
            return out

        def ffn_parts(x_in, f, l):
            """feed-forward sub-layer up to the output projection, left as split-K partial products (zk_gemm_parts: 64
            workgroups instead of 16 on 128 rows); the LayerNorm that follows adds them and the bias.  Returns the
            arguments of the row-local LayerNorm form (ln_args / zk_ln_decode)."""
            ffn_split = 4
            hh = e.mat("dc%d.ff.h" % l, BK, core.F)
            W2 = core.W(f + "/ffn_layer/output/W_0_0")
            parts = e.buf("dc.ff.parts.%d" % (l & 1), (ffn_split, BK, H), F32)
            core._linear(x_in, f + "/ffn_layer/enlarge", hh, act=1)
            n = ctypes.c_int(0)
            e.lib.call("zk_gemm_parts", hh.ptr, W2.ptr, parts.data_ptr(), BK, H, core.F, hh.ld, W2.ld, 0, 0, ffn_split,
                       ctypes.byref(n), e.stream)
            return dict(x=x_in.ptr, parts=parts.data_ptr(), nparts=n.value, stride=BK * H,
                        bias=core.b(f + "/ffn_layer/output/b_0").data_ptr(), **ln_scope(f))
        pend = None          # base model: the feed-forward LayerNorm of the previous layer, left to the next prologue
        x = e.mat("dc.x", BK, H)
        # all-pad test + embedding + timing (+ the first layer's average-attention update) in one launch
        lay0 = state["decoder"]["state"]["layer_0"]
        aan0 = core.aan
        gat = state.pop("_aan_gather", None)       # the beam reorder of the running sums, deferred to this launch
        sl = state.get("shortlist")
        tgt_table = core.store.s(core.tgt_emb) if sl is None else sl.table(core.tgt_emb)
        e.lib.call("zk_dec_embed", target.data_ptr(), hp.tgt_vocab.pad(), tgt_table.data_ptr(),
                   core.b("bias").data_ptr(), e.timing(Tmax + 1, H).data_ptr(), x.ptr, BK, H, float(H) ** 0.5,
                   0 if time_dev is not None else time, time_dev.data_ptr() if time_dev is not None else None,
                   lay0["aan"].data_ptr() if aan0 else None, e.mat("dc.cat", BK, 2 * H).ptr if aan0 else None,
                   1.0 if time_dev is not None else 1.0 / float(time + 1),
                   gat[0].data_ptr() if gat else None, gat[1].data_ptr() if gat else None,
                   hp.num_decoder_layer if gat else 0, e.stream)
        for l in range(hp.num_decoder_layer):
            pre = "decoder/layer_%d" % l
            lay = state["decoder"]["state"]["layer_%d" % l]
            if core.aan:
                a = pre + "/average_attention"
                cat = e.mat("dc.cat", BK, 2 * H)
                inv = 1.0 if time_dev is not None else 1.0 / float(time + 1)
                tdev = time_dev.data_ptr() if time_dev is not None else None
                if not (fuse_ln and l > 0 and not hp.use_ffn) and l != 0:
                    # else the previous layer's last LayerNorm (or the input launch) did it
                    e.lib.call("zk_aan_decode", x.ptr, lay["aan"].data_ptr(), cat.ptr, BK, H, inv, tdev, e.stream)
                if hp.use_ffn:           # transformer_aan.py:176-183
                    ya = e.mat("dc.ya", BK, H)
                    e.lib.call("zk_gather_rows", cat.ptr + H * 2, 2 * H * 2, None, ya.ptr, H * 2, BK, H * 2, e.stream)
                    hh = e.mat("dc.aah", BK, core.F)
                    core._linear(ya, a + "/ffn_layer/enlarge", hh, act=1)
                    core._linear(hh, a + "/ffn_layer/output", cat.cols_slice(H, 2 * H))
                z = e.mat("dc.z", BK, 2 * H)
                core._linear(cat, a + "/z_project", z)
                g = e.mat("dc.y", BK, H)
                if fuse_att:
                    # gate + residual + LayerNorm ride as the prologue of the encoder-decoder attention launch
                    xo = e.mat("dc%d.aa.o" % l, BK, H)
                    pend = dict(x=x.ptr, ybuf=g.ptr, out=xo.ptr, z=z.ptr, cat=cat.ptr, **ln_scope(a))
                    x = xo
                elif fuse_ln:
                    # gate + residual + LayerNorm in one launch (zk_ln_decode)
                    xo = e.mat("dc%d.aa.o" % l, BK, H)
                    e.lib.call("zk_ln_decode", x.ptr, g.ptr, core.b(a + "/layer_norm/scale").data_ptr(),
                               core.b(a + "/layer_norm/offset").data_ptr(), xo.ptr, BK, H, zdtype.epsilon(),
                               z.ptr, cat.ptr, None, 0, 0, None, None, None, 1.0, None, e.stream)
                    x = xo
                else:
                    e.aan_gate_fwd(z, cat, g, BK, H)
                    x = core._ln_fwd(x, g, a, "dc%d.aa" % l, False, 0.0, 0)
            elif fuse_att:
                p = pre + "/self_attention/dot_attention/"
                parts_s = e.buf("dc.parts.s", (nh, BK, H), F32)
                dec_self(x, pend, p, lay, parts_s)
                if pend is not None:
                    x = pend["xmat"]
                xo = e.mat("dc%d.sa.o" % l, BK, H)
                pend = dict(x=x.ptr, ybuf=e.mat("dc.y", BK, H).ptr, out=xo.ptr, parts=parts_s.data_ptr(), nparts=nh,
                            stride=BK * H, bias=core.b(p + "o_map/b_0").data_ptr(),
                            **ln_scope(pre + "/self_attention"))
                x = xo
            elif not core.fuse:
                p = pre + "/self_attention/dot_attention/"
                qkv = e.mat("dc.qkv", BK, 3 * H)
                core._linear(x, p + "qkv_map", qkv)
                append_kv(e, qkv, lay, BK, H, Tmax, 2, time, time_dev)
                att = e.mat("dc.att", BK, H)
                rk = core.store.s(p + "rpr_keys/embeddings") if core.rpr else None
                rv = core.store.s(p + "rpr_values/embeddings") if core.rpr else None
                if core.rela:
                    # rela.py:37-43, 66-68: the causal bias of a single query is all zeros, so every cached key 0 .. time
                    # counts and there is no mask; the key count comes from the device at a captured step
                    core._rela_attn(qkv.cols_slice(0, H), Mat(lay["k"], BK * Tmax, H), Mat(lay["v"], BK * Tmax, H), att, BK,
                                    1, Tmax if time_dev is not None else time + 1, p, None, bsq=3 * H, bsk=Tmax * H,
                                    bsv=Tmax * H, nkeys_dev=time_dev)
                else:
                    e.attn_fwd(qkv.cols_slice(0, H), Mat(lay["k"], BK * Tmax, H), Mat(lay["v"], BK * Tmax, H), att,
                               None, BK, nh, 1, Tmax if time_dev is not None else time + 1, d, kmask=None, causal=False,
                               q_pos0=0 if time_dev is not None else time, rpr_k=rk,
                               rpr_v=rv, max_rel=hp.max_relative_position, bsq=3 * H, bsk=Tmax * H, bsv=Tmax * H,
                               pos_dev=time_dev, pos_flags=3)
                y = e.mat("dc.y", BK, H)
                core._linear(att, p + "o_map", y)
                x = core._ln_fwd(x, y, pre + "/self_attention", "dc%d.sa" % l, False, 0.0, 0)
            p = pre + "/" + core.cross + "/dot_attention/"
            if fuse_att:
                parts_c = e.buf("dc.parts.c", (nh, BK, H), F32)
                dec_cross(x, pend, p, lay, parts_c)        # x is already the prologue's output buffer
                pend = None
                x = ln_parts(x, pre + "/" + core.cross, p, parts_c, "dc%d.ca" % l)
            else:
                x = _cross_unfused(core, e, hp, state, lay, x, p, pre, l, time, time_dev)
            nxt = state["decoder"]["state"].get("layer_%d" % (l + 1))
            if fuse_att and not core.aan:
                # feed-forward sub-layer; its residual + LayerNorm is the prologue of the next layer's self-attention
                f = pre + "/feed_forward"
                xo = e.mat("dc%d.ff.o" % l, BK, H)
                la = ffn_parts(x, f, l)
                la.update(out=xo.ptr, xmat=xo)
                if nxt is not None:
                    pend = la
                else:
                    e.lib.call("zk_ln_decode", *ln_args(la)[:5], BK, *ln_args(la)[5:], e.stream)
                    x = xo
                continue
            if fuse_ln and core.aan and not hp.use_ffn and (nxt is not None or fuse_att):
                # feed-forward sub-layer whose LayerNorm also prepares the next layer's average attention
                # (cache += x; cat = [x | cache / (time + 1)]) in the same launch
                f = pre + "/feed_forward"
                xo = e.mat("dc%d.ff.o" % l, BK, H)
                if fuse_att:
                    la = ffn_parts(x, f, l)
                else:
                    hh = e.mat("dc%d.ff.h" % l, BK, core.F)
                    core._linear(x, f + "/ffn_layer/enlarge", hh, act=1)
                    y = e.mat("dc.y", BK, H)
                    core._linear(hh, f + "/ffn_layer/output", y)
                    la = dict(x=x.ptr, ybuf=y.ptr, **ln_scope(f))
                g = lambda k: la.get(k)
                e.lib.call("zk_ln_decode", la["x"], g("ybuf"), la["gamma"], la["beta"], xo.ptr, BK, H, eps, None, None,
                           g("parts"), g("nparts") or 0, g("stride") or 0, g("bias"),
                           nxt["aan"].data_ptr() if nxt is not None else None,
                           e.mat("dc.cat", BK, 2 * H).ptr if nxt is not None else None,
                           1.0 if time_dev is not None else 1.0 / float(time + 1),
                           (time_dev.data_ptr() if time_dev is not None else None) if nxt is not None else None, e.stream)
                x = xo
            else:
                x = core._ffn_fwd(x, pre + "/feed_forward", "dc%d.ff" % l, False, 0, False)
        logits = e.mat("dc.logits", BK, core.Vpad, F32)
        if sl is None:
            e.gemm(x, core.W(core.soft_emb), logits, BK, core.V, H, 0, 1)
        else:      # the same buffer as [BK, Vs] against the compact softmax table
            logits = sl.logits(logits.t, BK)
            soft = sl.table(core.soft_emb)
            e.gemm(x, Mat(soft, soft.shape[0], soft.shape[1]), logits, BK, sl.Vs, H, 0, 1)
        if time_dev is None:
            state["time_filled"] = time + 1
        return logits, state

    def _step_dev(target, source, time):
        """transformer.py:277-281: encoder + training-path decoder on the whole prefix."""
        core = get_core(hp, model_name)
        e = core.eng
        batch = core.upload(source, target)
        enc, smask = core.encode(batch, False, False)
        feat, _, _ = core.decode_train(batch, enc, smask, False, False)
        BK, Lt = batch["B"], batch["Lt"]
        last = Mat(feat.t, BK, core.H, Lt * core.H, (Lt - 1) * core.H)
        logits = e.mat("dc.logits", BK, core.Vpad, F32)
        e.gemm(last, core.W(core.soft_emb), logits, BK, core.V, core.H, 0, 1)
        return logits, source

    def decoding_fn(target, state, time):
        if hp.search_mode == "cache":
            return _step_cache(target, state, time)
        if _f32.wanted(hp):
            raise ZeroHipError("decode_dtype=float32 decodes with search_mode=cache only (the dev mode re-runs the bf16 "
                               "training-path decoder, transformer.py:277-281)")
        return _step_dev(target, state, time)

    decoding_fn.step_static = step_static
    decoding_fn.step_cache = _step_cache      # the cached step with the time in device memory (models/_ensemble.py)
    return encoding_fn, decoding_fn
