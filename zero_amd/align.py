# coding: utf-8
"""Word alignments from the decoder's cross-attention (``alignment_file``, ``alignment_layer``, ``replace_unk``).

Every hypothesis token gets the source position it attends to: after the search, one teacher-forced pass over (source,
returned hypothesis) on the training-path forward reads the head-averaged weights of one decoder layer's cross-attention
(zero_amd/models/_align.py, zk_align_probs).  Row t of that pass predicts target token t (its input is token t - 1); the
hard alignment is the arg-max over the source's words -- the source's own EOS position is not eligible -- and the row of the
hypothesis' EOS is dropped.  The rule is stated once, in tests/align_ref.py.
"""
import os

import numpy as np

from zero_amd.models import _align
from zero_amd.models._core import trim_columns


def wanted(params):
    return bool(str(getattr(params, "alignment_file", "") or ""))


def check_opts(params, mode="test"):
    """Option validation of the new code paths (evaluate(), scorer(), align_fn), before a checkpoint is read."""
    if bool(getattr(params, "replace_unk", False)) and not wanted(params):
        raise ValueError("replace_unk needs alignment_file: the replacement is read off the alignment")
    if not wanted(params):
        return False
    _align.check_model(params.model_name, mode)
    _align.layer_index(params)
    if mode == "test" and int(getattr(params, "top_beams", 1) or 1) > 1:
        raise ValueError("alignment_file aligns the best hypothesis of a line: top_beams=%d is not supported with it"
                         % int(params.top_beams))
    return True


def _padded(ids):
    """ZERO_HIP_PAD_LEN (Trainer.prepare_static): both sides padded to a multiple of it; pad columns change nothing."""
    ids = trim_columns(ids)
    pad = max(1, int(os.environ.get("ZERO_HIP_PAD_LEN", "1")))
    extra = (-ids.shape[1]) % pad
    if extra:
        ids = np.concatenate([ids, np.zeros((ids.shape[0], extra), ids.dtype)], 1)
    return np.ascontiguousarray(ids)


def align_fn(features, params, model_name, initializer=None, want_probs=False):
    """features = {"source": int [B, Ls], "target": int [B, Lt]} (0 = pad; the target with its EOS, as score_fn takes it)
    -> {"best": int32 [B, Lt], "probs": fp32 [B, Lt, Ls] or None} (device tensors): best[b, t] is the source position the row
    that predicts target token t attends to, -1 where no position is eligible.  score_dtype selects the form."""
    import copy
    import torch
    from zero_amd.models._factory import closing_dropout, get_core
    _align.check_model(model_name)
    params = closing_dropout(copy.copy(params))
    params.label_smooth = 0.0
    layer = _align.layer_index(params)
    core = get_core(params, model_name, initializer)
    src, tgt = (np.asarray(x.cpu() if torch.is_tensor(x) else x) for x in (features["source"], features["target"]))
    if src.shape[0] == 0:
        dev = core.store.device
        return {"best": torch.zeros((0, tgt.shape[1]), dtype=torch.int32, device=dev),
                "probs": torch.zeros((0, tgt.shape[1], src.shape[1]), dtype=torch.float32, device=dev) if want_probs else None}
    src, tgt = _padded(src), _padded(tgt)
    _align.check_sizes(core, params, src.shape[1])
    batch = core.upload(src, tgt, trim=False)
    am = core.eng.buf("al.amask", src.shape, torch.float32)
    core.eng.h2d(am, _align.eligible_mask(src, params.src_vocab.eos()))
    batch["amask"] = am
    best, probs = _align.align(core, params, batch, layer, want_probs)
    return {"best": best, "probs": probs}


def hard_pairs(best_row, src_len, tgt_len):
    """best_row: a sentence's row of align_fn's "best"; src_len: source words (without the EOS); tgt_len: hypothesis words
    (without its EOS: that row is dropped) -> [(s, t)], t ascending; rows without an alignment (-1) are skipped."""
    out = []
    for t in range(min(int(tgt_len), len(best_row))):
        s = int(best_row[t])
        if 0 <= s < int(src_len):
            out.append((s, t))
    return out


def format_pairs(pairs):
    """[(s, t)] -> "s-t s-t ..." (0-based, the Pharaoh format of fast_align / Marian / fairseq); no pairs: an empty line."""
    return " ".join("%d-%d" % (s, t) for s, t in pairs)


def replace_unk_tokens(hyp_tokens, pairs, raw_src_tokens, unk):
    """Every hypothesis token equal to ``unk`` becomes the raw whitespace token of the source line at its aligned position;
    without an alignment, or with a position behind the raw tokens (a truncated line), the token is left alone."""
    where = {t: s for s, t in pairs}
    out = list(hyp_tokens)
    for t, tok in enumerate(out):
        s = where.get(t)
        if tok == unk and s is not None and 0 <= s < len(raw_src_tokens):
            out[t] = raw_src_tokens[s]
    return out
