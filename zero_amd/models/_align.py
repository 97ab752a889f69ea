# coding: utf-8
"""The alignment pass (``alignment_file``): one teacher-forced run of the training-path forward over (source, returned
hypothesis), up to and including ONE decoder layer's cross-attention, with zk_align_probs launched in line right behind
that attention -- the head-averaged softmax rows and their arg-max straight from the layer's q and k projections.

Why a pass of its own: every attention launch keeps its probabilities in registers or LDS, and the fused decode launches
and the device-resident beam book are pinned entry points.  A pass behind the search (what fairseq's --print-alignment
does) is independent of every search route and option, and with the option off nothing at all differs.

  bf16 (default)          TransformerCore.forward(..., align=(layer, hook)): encoder, decoder layers 0 .. layer; k is the first H
                          columns of the layer's [., 2 H] kv buffer (ldk = 2 H); where the attention launch formed q itself
                          (fuse_proj) the hook forms the aligned layer's q with one _linear into ``al.q``.
  score_dtype=float32     _score_f32.decode_train(..., align=(layer, hook)) on the scorer's ``q`` / ``mk`` buffers.

No later layer, no logits product, no loss.  The rule is stated once, in tests/align_ref.py.
"""
import numpy as np
import torch

from zero_amd.models import _score_f32

F32 = torch.float32
BUILT = ("transformer", "transformer_aan", "transformer_fuse")
_WHY = {
    "transformer_rpr": "its cross-attention has a relative-position term",
    "transformer_rela": "its attention is ReLU, not a softmax",
    "transformer_l0drop": "its memory is compacted",
    "transformer_fixup": "the pass is not built for its LayerNorm-free layers",
    "rnnsearch": "a recurrent model has no cross-attention heads to read",
    "rnnsearch_deepatt": "a recurrent model has no cross-attention heads to read",
    "deepnmt": "a recurrent model has no cross-attention heads to read",
}


def check_model(model_name, mode=None):
    """alignment_file is built for transformer, transformer_aan and transformer_fuse; anything else is refused by name."""
    if mode == "ensemble":
        raise NotImplementedError("alignment_file is not built for --mode ensemble (model %s)" % model_name)
    if model_name not in BUILT:
        raise NotImplementedError("alignment_file is not built for %s: %s" %
                                  (model_name, _WHY.get(model_name, "only %s are" % ", ".join(BUILT))))


def layer_index(hp):
    """alignment_layer as an index 0 .. num_decoder_layer - 1 (Python-style: -1 = the last layer)."""
    n, l = int(hp.num_decoder_layer), int(getattr(hp, "alignment_layer", -1))
    if not -n <= l < n:
        raise ValueError("alignment_layer=%d is out of range for %d decoder layers" % (l, n))
    return l % n


def max_source_len(core):
    return int(core.eng.lib.raw("zk_align_max_lk")())


def check_sizes(core, hp, Ls):
    if not _score_f32.wanted(hp) and core.d % 32 != 0:
        raise ValueError("alignment_file: the bf16 form needs a head size that is a multiple of 32 (got %d); use "
                         "score_dtype=float32" % core.d)
    if _score_f32.wanted(hp):
        _score_f32.check_model(core)
    limit = max_source_len(core)
    if Ls > limit:
        raise ValueError("alignment_file: a source of %d positions is longer than the kernel's limit of %d" % (Ls, limit))


def align(core, hp, batch, layer, want_probs):
    """batch: core.upload(source, target) (+ "amask": fp32 [B, Ls], the positions an alignment may name; default the source
    mask) -> (best int32 [B, Lt], probs fp32 [B, Lt, Ls] or None), device tensors of the core's engine."""
    e, H = core.eng, core.H
    B, Ls, Lt = batch["B"], batch["Ls"], batch["Lt"]
    check_sizes(core, hp, Ls)
    best = e.buf("al.best", (B, Lt), torch.int32)
    probs = e.buf("al.probs", (B, Lt, Ls), F32) if want_probs else None
    amask = batch.get("amask")
    if _score_f32.wanted(hp):
        from zero_amd.models import _decode_f32
        from zero_amd.models._ops import ops_for
        o = ops_for(core, True, prefix="sq.")
        if "smask" not in batch or "tmask" not in batch:
            batch = dict(batch)
            batch["smask"] = e.buf("smask", (B, Ls), F32)
            e.make_mask(batch["src"], batch["smask"], B * Ls)
            batch["tmask"] = e.buf("tmask", (B, Lt), F32)
            e.make_mask(batch["tgt"], batch["tmask"], B * Lt)
        enc, smask = _decode_f32.encode(core, hp, batch, o, o.attn_seq)

        def hook(q, k):
            e.align_probs(q, k, B, core.nh, Lt, Ls, core.d, kmask=smask, ldmask=Ls, amask=amask, probs=probs, best=best)
        _score_f32.decode_train(core, hp, batch, enc, smask, o, align=(layer, hook))
        return best, probs
    smask = batch.get("smask")
    if smask is None:
        smask = e.buf("smask", (B, Ls), F32)
        e.make_mask(batch["src"], smask, B * Ls)
        batch = dict(batch, smask=smask)

    def hook(x, q, kv, p):
        if q is None:      # the attention launch formed q in its prologue: this layer's once more, into a buffer of its own
            q = e.mat("al.q", x.rows, H)
            core._linear(x, p + "q_map", q)
        e.align_probs(q, kv.cols_slice(0, H), B, core.nh, Lt, Ls, core.d, kmask=smask, ldmask=Ls, amask=amask, probs=probs,
                      best=best)
    core.forward(batch, train=False, save=False, label_smooth=0.0, align=(layer, hook))
    return best, probs


def eligible_mask(src, eos):
    """The positions an alignment may name: the source's tokens without its EOS (source lines carry one, vocab.to_id) --
    the last non-pad position of a row is cleared when it holds ``eos``."""
    src = np.asarray(src)
    am = (src != 0).astype(np.float32)
    n = (src != 0).sum(1)
    for b in range(src.shape[0]):
        if n[b] > 0 and int(src[b, n[b] - 1]) == int(eos):
            am[b, n[b] - 1] = 0.0
    return am
