"""Shared by the ensemble tests (CPU and GPU): toy members and the ensemble oracle composed from oracle/ref_torch.py."""
import copy

import numpy as np
import torch

from oracle import ref_torch as rt
from tests.common import make_hp, make_batch, perturb


def make_member(model, seed, **kw):
    """One toy member, built like tests/test_gpu_model.py _setup: make_hp defaults, perturbed biases / LayerNorm
    parameters, target embedding x 6 (peaked distributions), cache-mode search.  -> (hp, Pn, source)."""
    rng = np.random.default_rng(seed)
    hp = make_hp(model, **kw)
    hp.search_mode = "cache"
    Pn = perturb(rt.init_params(hp, model, seed=seed + 1), rng)
    Pn["tgt_embedding"] = (Pn["tgt_embedding"] * 6.0).astype(np.float32)
    src, _ = make_batch(rng, 5, 9, 11, hp.src_vocab.size(), hp.tgt_vocab.size())
    return hp, Pn, src


def make_members(models, seeds, **kw):
    """-> (hps, Pns, source of member 0)."""
    built = [make_member(m, s, **kw) for m, s in zip(models, seeds)]
    return [b[0] for b in built], [b[1] for b in built], built[0][2]


def composed_infer_fn(hps, Pns, models):
    """The reference's ensemble pair (main.py:76-103) out of the oracle's own single-model infer_fn:
    encoding_fn(source) = {"ensembler_i": enc_i(source)}; decoding_fn runs every member on its sub-state and returns
    log(mean_m softmax(logits_m))."""
    pairs = [rt.infer_fn(hp, rt.to_torch(Pn), m) for hp, Pn, m in zip(hps, Pns, models)]
    M = len(pairs)

    def encoding_fn(source):
        return {"ensembler_%d" % i: enc(source) for i, (enc, _) in enumerate(pairs)}

    def decoding_fn(target, state, time):
        probs = []
        for i, (_, dec) in enumerate(pairs):
            key = "ensembler_%d" % i
            logits, state[key] = dec(target, state[key], time)
            probs.append(torch.softmax(logits.float(), -1))
        return torch.log(sum(probs) / M), state

    return encoding_fn, decoding_fn


def composed_oracle(hps, Pns, models, src, store_bf16=False):
    """rt.beam_search over the composed pair with member 0's hparams -> {'seq', 'score', 'steps'}."""
    enc, dec = composed_infer_fn(hps, Pns, models)
    prev = rt.Cfg.store_bf16
    rt.Cfg.store_bf16 = store_bf16
    try:
        return rt.beam_search({"source": torch.tensor(src)}, enc, dec, hps[0])
    finally:
        rt.Cfg.store_bf16 = prev


def single_oracle(hp, Pn, model, src):
    enc, dec = rt.infer_fn(hp, rt.to_torch(Pn), model)
    return rt.beam_search({"source": torch.tensor(src)}, enc, dec, hp)


def with_beam(hps, K, **over):
    out = []
    for hp in hps:
        hp = copy.copy(hp)
        hp.beam_size = K
        for k, v in over.items():
            setattr(hp, k, v)
        out.append(hp)
    return out
