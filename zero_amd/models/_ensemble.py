# coding: utf-8
"""Ensemble decoding: M models per beam-search step, their distributions combined on the device.

Counterpart of the reference's ``tower_ensemble_graph`` (main.py:65-115).  Per decode step every member's
``decoding_fn`` runs on the same last tokens with its own cache; the search continues on

    combined = log( (1/M) * sum_m softmax(logits_m) )                      (main.py:101-103)

which ``zk_ensemble_logprob`` (csrc/zk_ensemble.hip) evaluates in the stable form
``logsumexp_m(logits_m - logsumexp(logits_m)) - log M``; ``combined`` then takes the unchanged path of
search.py:141-176 (noise, temperature, log-softmax again, EOS ban, length penalty, top-2K) with the search parameters
of member 0, and the chosen beams reorder the cache of every member.  Member i lives in the scope
``<scope_name>_ensembler_<i>`` (main.py:73), so members may be of different model types and sizes; they share the
vocabularies (main.py:629).

State sharing.  ``search.beam_search`` drives ONE (encoding_fn, decoding_fn) pair and one ``DecodeState``.  The composed
state (:class:`EnsembleState`) holds the members' own states and lends member 0's packed step buffers -- last tokens,
previous log-probs, reorder index, step scalars, top-2K output -- to everybody: every member's kernels read the same
``tok`` / ``idx`` / ``stepbuf`` device tensors, ``reorder`` and ``bind_caches`` are forwarded to every member, and the
ping-pong parity is kept in lockstep.  Every member has its own core, hence its own engine buffers (nothing aliases);
all launches of a step go to the one current stream (``Engine.stream`` is the current stream, and the search has entered
member 0's work stream), so the whole step -- M cache reorders, M decoder steps, the combine, the tail -- is captured
and replayed as ONE hipGraph with the device-resident bookkeeping, like a single model's.

Step graphs are captured per batch and destroyed at its end (the ``ZERO_HIP_DECODE_GRAPH_CACHE=0`` behaviour): the
cross-batch graph cache keys graphs per core and per shape, which does not identify a member SET, and a graph captured
for one member set must never be replayed for another.

One batch at a time: the ensemble step runs on execution lane 0 only (``zero_amd.main.ensemble`` decodes its batches
one after the other); a call from another lane raises instead of running on buffers that were never exercised there.
"""

import copy
import ctypes

import torch

from zero_amd.hip import ZeroHipError
from zero_amd.models import _decode as _dec
from zero_amd.models import _decode_f32 as _f32
from zero_amd.models._factory import current_lane, get_core

F32 = torch.float32


def member_scope(params, midx):
    """main.py:73: the variable scope of member ``midx``."""
    return "%s_ensembler_%d" % (params.scope_name or "model", midx)


def member_params(params, midx):
    """A copy of ``params`` that lives in the member's scope."""
    hp = copy.copy(params)
    hp.scope_name = member_scope(params, midx)
    return hp


def member_tensors(tensors, midx, ema=False):
    """main.py:660-714 on a restored checkpoint ``{name: array}``: every ``<scope>/<rest>`` entry is renamed to
    ``<scope>_ensembler_<midx>/<rest>``; with ``ema`` the ExponentialMovingAverage shadows replace the plain values
    they shadow (main.py:675-683).  Entries without a scope (``global_step``, the beta powers) keep their names."""
    tensors = dict(tensors)
    if ema:
        for key in list(tensors):
            ema_key = key + "/ExponentialMovingAverage"
            if ema_key in tensors:
                tensors[key] = tensors[ema_key]
    out = {}
    for name, value in tensors.items():
        cut = name.find("/")
        if cut < 0:
            out[name] = value
        else:
            out["%s_ensembler_%d/%s" % (name[:cut], midx, name[cut + 1:])] = value
    return out


def max_members():
    from zero_amd import hip
    return int(hip.lib().raw("zk_ensemble_max")())


def check_members(total_params):
    """Everything that can be refused from the parameters alone, before any device work."""
    M = len(total_params)
    if M == 0:
        raise ZeroHipError("ensemble decoding needs at least one member (got none)")
    for i, p in enumerate(total_params):
        _dec.check_member(str(p.model_name).lower(), i)
    if M > max_members():
        raise ZeroHipError("ensemble decoding combines at most %d members per step (zk_ensemble_logprob); got %d"
                           % (max_members(), M))
    sizes = [int(p.tgt_vocab.size()) for p in total_params]
    if len(set(sizes)) != 1:
        raise ZeroHipError("ensemble members must share the target vocabulary (main.py:629); sizes per member: %s"
                           % ", ".join("%d: %d" % (i, s) for i, s in enumerate(sizes)))
    modes = [bool(_f32.wanted(p)) for p in total_params]
    if len(set(modes)) != 1:
        raise ZeroHipError("ensemble members disagree on decode_dtype (member 0 decides): %s"
                           % ", ".join("%d: %s" % (i, getattr(p, "decode_dtype", "bfloat16"))
                                       for i, p in enumerate(total_params)))
    if len(set(p.search_mode for p in total_params)) != 1:
        raise ZeroHipError("ensemble members disagree on search_mode: %s"
                           % ", ".join("%d: %s" % (i, p.search_mode) for i, p in enumerate(total_params)))
    K = int(total_params[0].beam_size)
    if 2 * K > 16:
        raise ZeroHipError("beam_size=%d: the fused search tail keeps at most 16 candidates per sentence (2 * beam_size), "
                           "and the device-resident bookkeeping at most 16 beams" % K)
    if current_lane() != 0:
        raise ZeroHipError("ensemble decoding runs one batch at a time on execution lane 0 (called on lane %d)"
                           % current_lane())


class EnsembleState(_dec.DecodeState):
    """What search.py asks of a DecodeState, for M members: ``self["members"]`` are their states; the packed step buffers
    are member 0's; cache plumbing is forwarded and the ping-pong parity of all members follows ``self["_pp"]``."""

    def reorder(self, index_dev, time_dev=None, defer_aan=False):
        for m in self["members"]:
            m.reorder(index_dev, time_dev=time_dev, defer_aan=defer_aan and m["_core"].aan)
        self["_pp"] = 1 - self["_pp"]

    def bind_caches(self):
        for m in self["members"]:
            m["_pp"] = self["_pp"]
            m.bind_caches()


def combine(core, logits, rows):
    """zk_ensemble_logprob on the members' fp32 logits Mats -> Mat [rows, Vpad] in a buffer of ``core``'s engine."""
    e = core.eng
    M = len(logits)
    out = e.mat("ens.logprob", rows, core.Vpad, F32)
    ws = e.workspace(e.lib.query("zk_ensemble_logprob_workspace", rows, M, core.V))
    e.lib.call("zk_ensemble_logprob", (ctypes.c_void_p * M)(*[l.ptr for l in logits]),
               (ctypes.c_int * M)(*[int(l.ld) for l in logits]), M, rows, core.V, out.ptr, out.ld, ws.data_ptr(),
               ws.numel(), e.stream)
    return out


def make_infer_fns(total_graphs, total_params):
    """-> (encoding_fn, decoding_fn, search params): one pair for ``search.beam_search`` over all members.  The search
    parameters are member 0's (main.py:66) in member 0's scope, so that the search finds member 0's core and stream."""
    from zero_amd import shortlist
    for p in total_params:
        shortlist.check(p, ensemble=True)
    check_members(total_params)
    hps = [member_params(p, i) for i, p in enumerate(total_params)]
    names = [p.model_name for p in total_params]
    pairs = [g.infer_fn(hp) for g, hp in zip(total_graphs, hps)]
    encs, decs = [p[0] for p in pairs], [p[1] for p in pairs]
    hp0 = hps[0]

    def encoding_fn(source, beam_size=None, max_steps=None):
        members = [enc(source, beam_size=beam_size, max_steps=max_steps) for enc in encs]
        m0 = members[0]
        for i, m in enumerate(members):
            for k in ("B", "K", "BK", "Ls", "Tmax"):
                if m[k] != m0[k]:
                    raise ZeroHipError("ensemble member %d has %s=%s, member 0 has %s (decode_length and the padding of "
                                       "all members must agree)" % (i, k, m[k], m0[k]))
        state = EnsembleState()
        for k in ("_core", "B", "K", "BK", "Ls", "Tmax", "pack_dev", "pack_host", "tok", "prev", "idx", "stepbuf",
                  "out_dev", "out_host", "ts", "ti", "static_ok"):
            state[k] = m0[k]
        # "_gkey" present: the cross-batch graph cache neither hands graphs to this batch nor takes them at its end
        state.update({"members": members, "graphs": {}, "_pp": 0, "time_filled": 0, "_gkey": None,
                      "f32": bool(m0.get("f32"))})
        return state

    def decoding_fn(target, state, time):
        """The composed step outside a captured graph (main.py:85-103): cache mode on the members' states, dev mode
        (every member re-runs its training-path decoder on the whole prefix) on the tiled source."""
        if hp0.search_mode == "cache":
            logits = [dec(target, m, time)[0] for dec, m in zip(decs, state["members"])]
            state["time_filled"] = time + 1
            return combine(state["_core"], logits, state["BK"]), state
        logits = [dec(target, state, time)[0] for dec in decs]
        return combine(get_core(hp0, names[0]), logits, logits[0].rows), state

    def step_logits(state, time_dev):
        logits = [dec.step_cache(state["tok"], m, None, time_dev=time_dev)[0] for dec, m in zip(decs, state["members"])]
        return combine(state["_core"], logits, state["BK"])

    def step_static(state, temperature, forbid_value):
        """One whole ensemble step with every per-step value read from device memory (models/_decode.py static_step):
        bookkeeping head, every member's cache reorder, every member's decoder step, the combine, the search tail.  One
        eager pass per ping-pong parity sizes every member's scratch, the second is captured, the rest are replays."""
        _dec.static_step(state, hp0, step_logits, False, temperature, forbid_value, defer_aan=True)

    decoding_fn.step_static = step_static
    return encoding_fn, decoding_fn, hp0


def tower_ensemble_graph(eval_features, total_graphs, total_params):
    """main.py:65-115 -> (seqs [B, K, L], scores [B, K]).  Mirrors ``tower_infer_graph``: member i's ``infer_fn`` is built
    on a copy of its params whose scope_name has ``_ensembler_<i>`` appended, and one composed pair goes to
    ``search.beam_search``.  One batch at a time (lane 0)."""
    from zero_amd.search import beam_search
    encoding_fn, decoding_fn, hp0 = make_infer_fns(total_graphs, total_params)
    out = beam_search(eval_features, encoding_fn, decoding_fn, hp0)
    return out["seq"], out["score"]
