# coding: utf-8
"""Lexical shortlist decoding: a per-batch output vocabulary (vocabulary selection as in Jean et al. 2015, the
``--shortlist`` of other toolkits).

Token ids touch the model in two places only: the decoder's input embedding and the logits product.  With a compact copy
``E[S]`` of the target-side table(s) in both, the whole decode step -- model, Gumbel noise, top-2K, device-resident
bookkeeping -- runs in shortlist space with V replaced by Vs = len(S); ``search.beam_search`` maps the ids of the result
through ``S`` once, at its end.  Decoding with shortlist S IS decoding with the model whose target-side tables are
restricted to the rows S (the log-softmax runs over the shortlist), followed by that mapping.  S is ascending, so ties go
to the same token as in the full vocabulary.

``S`` of a batch (zk_shortlist_build, include/zero_hip.h): the ``shortlist_first`` lowest ids (vocabulary files are sorted by
falling frequency, zero_amd/vocab.py), plus the first ``shortlist_best`` entries of the lexical row of every source token of
the batch, filled with the lowest missing ids up to Vs = min(V, roundup(|S|, shortlist_round)).  The rounding makes step
graphs reusable: they are cached per shape and Vs is part of the shape.

The table file has one ``tgt_token src_token probability`` per line, as alignment tools write it.
"""

import threading

import numpy as np
import torch

I32 = torch.int32

# the models whose decode step reads its target-side tables through the shortlist
MODELS = ("transformer", "transformer_aan", "transformer_rpr", "transformer_fuse", "rnnsearch")


def wanted(hp):
    return bool(getattr(hp, "shortlist_file", ""))


def check(hp, model_name=None, ensemble=False):
    """What shortlist decoding refuses, before a core is built; nothing when shortlist_file is empty."""
    if not wanted(hp):
        return
    if ensemble:
        raise NotImplementedError("shortlist_file is set: shortlist decoding of an ensemble is not built (its members "
                                  "would have to share one shortlist)")
    if model_name not in MODELS:
        raise NotImplementedError("shortlist_file is set: shortlist decoding is built for %s, not for %s"
                                  % (", ".join(MODELS), model_name))
    if hp.search_mode != "cache":
        raise NotImplementedError("shortlist_file is set: shortlist decoding runs with search_mode=cache only (got %s)"
                                  % hp.search_mode)
    if int(hp.shortlist_first) < 3:
        raise ValueError("shortlist_first must be at least 3 (pad / unk / eos keep the ids 0, 1, 2), got %d"
                         % hp.shortlist_first)
    if int(hp.shortlist_round) < 8 or int(hp.shortlist_round) % 8 != 0:
        raise ValueError("shortlist_round must be a positive multiple of 8, got %d" % hp.shortlist_round)
    if int(hp.shortlist_best) < 0:
        raise ValueError("shortlist_best must not be negative, got %d" % hp.shortlist_best)


# ---- the lexical table -------------------------------------------------------------------------------------------
class LexTable(object):
    """CSR over source ids: row s = ids[off[s] : off[s + 1]], the target ids of source id s by falling probability."""

    def __init__(self, off, ids):
        self.off = np.ascontiguousarray(off, dtype=np.int32)
        self.ids = np.ascontiguousarray(ids, dtype=np.int32)

    def row(self, s):
        return self.ids[self.off[s]:self.off[s + 1]]


def parse_table(lines, src_vocab, tgt_vocab):
    """Lines of ``tgt_token src_token probability`` -> LexTable.  Lines whose tokens are missing from either vocabulary
    (and lines that are not three fields) are dropped; a source row is sorted by falling probability, equal probabilities
    keep the order of the file."""
    src, tgt, prob = [], [], []
    for line in lines:
        f = line.split()
        if len(f) != 3:
            continue
        t, s = tgt_vocab.find(f[0]), src_vocab.find(f[1])
        if t is None or s is None:
            continue
        try:
            p = float(f[2])
        except ValueError:
            continue
        src.append(s); tgt.append(t); prob.append(p)
    src, tgt = np.asarray(src, dtype=np.int64), np.asarray(tgt, dtype=np.int32)
    by_prob = np.argsort(-np.asarray(prob, dtype=np.float64), kind="stable")
    order = by_prob[np.argsort(src[by_prob], kind="stable")]
    off = np.zeros(src_vocab.size() + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=src_vocab.size()), out=off[1:])
    return LexTable(off, tgt[order])


_TABLES = {}
_TABLES_LOCK = threading.Lock()


def load_table(path, src_vocab, tgt_vocab):
    """parse_table of a file, cached per (path, vocabularies)."""
    key = (path, id(src_vocab), id(tgt_vocab))
    with _TABLES_LOCK:
        ent = _TABLES.get(key)
        if ent is None or ent[0] is not src_vocab or ent[1] is not tgt_vocab:
            with open(path, "r") as reader:
                ent = _TABLES[key] = (src_vocab, tgt_vocab, parse_table(reader, src_vocab, tgt_vocab))
        return ent[2]


# ---- the per-batch driver ----------------------------------------------------------------------------------------
class Shortlist(object):
    """What a decode state carries: Vs, the leading dimension of the logits, the compact tables and S (host int64)."""

    def __init__(self, core, Vs, ld, tables, S, bufs):
        self.core, self.Vs, self.ld, self.tables, self.S, self.bufs = core, Vs, ld, tables, S, bufs

    def table(self, name):
        """The compact table standing in for the variable ``name`` in a decode step, or None."""
        return self.tables.get(name)

    def pointers(self):
        """The addresses a captured step holds (models/_decode.py _graph_pointers)."""
        return [b.data_ptr() for b in self.bufs]

    def logits(self, buf, rows):
        """The step's logits buffer (sized for the whole vocabulary) viewed as [rows, ld]."""
        from zero_amd.func import Mat
        return Mat(buf.reshape(-1)[:rows * self.ld].view(rows, self.ld), rows, self.ld)

    def map_back(self, seq):
        return self.S[np.asarray(seq)]


def _lex_on_device(core, hp):
    """The table of hp.shortlist_file on this core's engine: uploaded once per engine."""
    lex = load_table(hp.shortlist_file, hp.src_vocab, hp.tgt_vocab)
    ent = core.__dict__.get("_shortlist_lex")
    if ent is None or ent[0] is not lex:
        dev = core.eng.device
        ids = lex.ids if lex.ids.size else np.zeros(1, dtype=np.int32)        # (never a NULL pointer)
        ent = core._shortlist_lex = (lex, torch.from_numpy(lex.off).to(dev), torch.from_numpy(ids).to(dev))
    return ent[1], ent[2]


def launch(core, hp, src_dev, rows, ld_src, Ls, pre):
    """First half of the per-batch driver, right after the source ids reached the device: the build kernel and the
    asynchronous copy of its result into pinned staging.  -> the handle ``finish`` takes.  pre: the prefix of the decode
    mode's engine buffers of this model."""
    e = core.eng
    V = core.V
    # one buffer [ids cap = V | count 2], sized by the vocabulary alone: it never grows, so it never invalidates a graph
    out = e.buf(pre + "sl.ids", (V + 2,), I32)
    off, ids = _lex_on_device(core, hp)
    e.shortlist_build(src_dev, rows, ld_src, Ls, off, ids, hp.shortlist_best, hp.shortlist_first, V, hp.shortlist_round,
                      out[:V], out[V:])
    pins = core.__dict__.setdefault("_decode_pins", {})
    host = pins.get("sl.ids")
    if host is None or host.numel() != V + 2:
        host = pins["sl.ids"] = torch.zeros(V + 2, dtype=I32).pin_memory()
    host.copy_(out, non_blocking=True)
    return out, host


def finish(core, hp, handle, o):
    """Second half: read Vs back (the one stream synchronisation of the batch) and gather the compact tables with
    zk_gather_rows_ex -- rows of the storage type of the ops object ``o`` (bf16 shadow / fp32 master), two tables when the
    softmax embedding is separate.  -> Shortlist."""
    e = core.eng
    out, host = handle
    V, Vpad = core.V, core.Vpad
    torch.cuda.current_stream(e.device).synchronize()
    h = host.numpy()
    n, Vs = int(h[V]), int(h[V + 1])
    if not 3 <= n <= Vs <= V:
        raise RuntimeError("zk_shortlist_build reported a shortlist of %d, %d ids for a vocabulary of %d" % (n, Vs, V))
    S = h[:Vs].astype(np.int64)
    ld = (Vs + 7) // 8 * 8                   # the physical row count of a table of Vs rows (variables.VariableStore)
    st = o.storage
    tables, bufs = {}, [out]
    for name in dict.fromkeys((core.tgt_emb, core.soft_emb)):
        full = core.store.w(name) if st.dtype == torch.float32 else core.store.s(name)
        width = int(full.shape[1])
        if (width * st.esz) % 16 != 0:
            raise ValueError("shortlist decoding gathers table rows 16 bytes at a time: the row of %s has %d bytes"
                             % (name, width * st.esz))
        # sized for the whole vocabulary once: a larger shortlist never reallocates
        buf = e.buf(o.pre + "sl." + name, (Vpad, width), st.dtype)
        t = buf[:ld]
        e.lib.call("zk_gather_rows_ex", full.data_ptr(), width * st.esz, out.data_ptr(), t.data_ptr(), width * st.esz, Vs,
                   width * st.esz, 0, e.stream)
        if ld > Vs:
            e.zero(t[Vs:])
        tables[name] = t
        bufs.append(buf)
    return Shortlist(core, Vs, ld, tables, S, bufs)
