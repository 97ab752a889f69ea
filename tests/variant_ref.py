"""What the references of the variant models share (a plain module, no pytest in it; CPU only): tests/rela_ref.py,
fixup_ref.py, l0drop_ref.py, rnnsearch_ref.py and score_f32_ref.py keep the arithmetic, bounds, defects, cases and fixture
constants that are their own, and take from here

``STORAGE``, ``ragged``, ``sharpen``      the storage types of the kernel forms, the padded id matrices and the sharpened model
``storage_model`` / ``search``            oracle.ref_torch's beam search over a restated (encoding_fn, decoding_fn) pair
``candidate_margin``                      the measurement that the REFERENCE ALONE is far from a tie on a fixture
``init_params`` / ``make_fixture``        the recurrent models' random weights and what the REFERENCE ALONE shows on them
``assert_within`` / ``exceeds``           the element-wise check of a kernel (or stand-in) against its float64 statement
``embed_step`` / ``embed_shifted`` / ``cached_state`` / ``empty_caches``   the Transformer decoder's inputs and caches
"""
import contextlib
import copy

import numpy as np
import torch

from oracle import ref_torch as rt

STORAGE = {"bf16": torch.bfloat16, "fp32": torch.float32}


# ---------------------------------------------------------------------------------------------- fixtures
def ragged(lengths, vocab_size, seed, width=None):
    """[len(lengths), width or max(lengths)] int64 ids: row b holds lengths[b] - 1 ids drawn from 3 .. vocab_size - 1, then
    eos = 2, then pad = 0."""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(lengths), width or max(lengths)), dtype=np.int64)
    for b, n in enumerate(lengths):
        out[b, :n - 1] = rng.integers(3, vocab_size, n - 1)
        out[b, n - 1] = 2
    return out


def sharpen(hp, Pn, factor=6.0):
    """The output distribution sharpened so that bf16 noise cannot flip near-ties of a random model."""
    Pn = dict(Pn)
    name = rt._emb_name(hp, "softmax")
    Pn[name] = (Pn[name] * factor).astype(np.float32)
    return Pn


# ---------------------------------------------------------------------------------------------- the reference's search
@contextlib.contextmanager
def storage_model(on):
    """ref_torch's own bf16 storage model (Cfg.store_bf16) for the duration of the block."""
    prev = rt.Cfg.store_bf16
    rt.Cfg.store_bf16 = bool(on)
    try:
        yield
    finally:
        rt.Cfg.store_bf16 = prev


def search(decoding_fns, hp, Pn, src, K, dtype, store_bf16=False):
    """rt.beam_search (beam K, search_mode = cache) over decoding_fns(hp, P) with the numpy parameters Pn in `dtype`.
    -> (the search's result, the per-step candidate tables of hp.search_trace)."""
    hp = copy.copy(hp)
    hp.beam_size, hp.search_mode = K, "cache"
    hp.search_trace = []
    with storage_model(store_bf16), torch.no_grad():
        enc, dec = decoding_fns(hp, rt.to_torch(Pn, dtype=dtype))
        out = rt.beam_search({"source": torch.as_tensor(src)}, enc, dec, hp)
    return out, hp.search_trace


def candidate_margin(search_fn, hp, Pn, src, beams=(1, 4), factor=4.0, tol=None, seed=None):
    """The proof that the REFERENCE ALONE is far from a tie on a fixture.  search_fn(hp, Pn, src, K, dtype) -> (result,
    trace).  Measured on the CPU, for every beam of `beams`:
      * the float64 and the fp32 run give identical hypotheses (every beam, every token) and the same candidate order at
        every step;
      * gap   the smallest difference, over all steps and sentences of the float64 run, between a candidate the search keeps
              (one of its 2K) and its runner-up (the next one in rank, kept or not);
      * err   the largest |score_fp32 - score_float64| over the candidates both runs rank (the kept 2K);
      * rel   with tol = (ATOL, RTOL): the largest |score_fp32 - score_float64| / (ATOL + RTOL |score_float64|) over the same
              candidates -- how much of that score tolerance the fp32 reference itself uses up;
    and gap > factor * err (one factor, 4, for every variant; tests/l0drop_ref.make_fixture asks the same of its margin).
    -> dict gap, err (and rel), the worst over the beams.  seed only labels the assertion messages."""
    gap, err, rel = np.inf, 0.0, 0.0
    for K in beams:
        o64, t64 = search_fn(hp, Pn, src, K, torch.float64)
        o32, t32 = search_fn(hp, Pn, src, K, torch.float32)
        assert np.array_equal(o64["seq"], o32["seq"]), ("float64 and fp32 reference disagree", K, seed)
        assert len(t64) == len(t32)
        for (s64, i64), (s32, i32) in zip(t64, t32):
            s64, s32 = np.maximum(s64.astype(np.float64), -1e35), np.maximum(s32.astype(np.float64), -1e35)
            live = s64[:, :2 * K] > -1e30                      # (the first step of a beam has K - 1 dead rows)
            g = np.where(live, s64[:, :2 * K] - s64[:, 1:2 * K + 1], np.inf)      # each kept candidate and its runner-up
            gap = min(gap, float(g.min()))
            assert np.array_equal(i64[:, :2 * K][live], i32[:, :2 * K][live]), ("candidate order differs", K, seed)
            diff = np.abs(s64[:, :2 * K] - s32[:, :2 * K])
            err = max(err, float(diff[live].max()))
            if tol is not None:
                rel = max(rel, float((diff / (tol[0] + tol[1] * np.abs(s64[:, :2 * K])))[live].max()))
    assert gap > factor * err, (gap, err, seed)
    return {"gap": gap, "err": err} if tol is None else {"gap": gap, "err": err, "rel": rel}


def init_params(hp, model, seed):
    """Every variable of zero_amd.variables.variable_specs(hp, model) from its initial distribution (weights and embeddings
    from the scope initialiser; "zeros" and "ones" draw nothing), with the biases and LayerNorm pairs perturbed so that every
    term is exercised."""
    from tests.common import perturb
    from zero_amd.variables import variable_specs
    rng = np.random.default_rng(seed)
    Pn = {}
    for name, shape, kind, _ in variable_specs(hp, model):
        if kind in ("zeros", "ones"):
            v = np.zeros(shape) if kind == "zeros" else np.ones(shape)
        else:
            v = rt._scope_init(rng, shape, hp.initializer, hp.initializer_gain)
        Pn[name] = np.asarray(v, np.float32)
    return perturb(Pn, rng)


def make_fixture(model, decoding_fns, tol, hp, src, seed, factor=4.0):
    """The tiny model of the GPU model tests with what the REFERENCE ALONE shows on it, measured on the CPU and asserted,
    for beam 1 and 4:
      * candidate_margin: the float64 and the fp32 run give identical hypotheses and candidate orders, and the smallest gap
        between a kept candidate and its runner-up exceeds factor x err, the largest fp32 - float64 score difference;  rel:
        that difference as a share of ATOL + RTOL |score_float64|, tol = (ATOL, RTOL) -- how much of the project's fp32 score
        tolerance the fp32 reference itself uses up (rnnsearch_ref.score_tol);
      * with the output embedding sharpened x 6, the bf16-storage restatement (rt.Cfg.store_bf16) keeps the best hypothesis
        of every sentence of the fp32 run.
    -> dict Pn, gap, err, rel (the worst over both beams)."""
    Pn = init_params(hp, model, seed)
    run = lambda *a, **k: search(decoding_fns, *a, **k)
    m = candidate_margin(run, hp, Pn, src, factor=factor, tol=tol, seed=seed)
    Ps = sharpen(hp, Pn)
    for K in (1, 4):
        a, _ = run(hp, Ps, src, K, torch.float32)
        b, _ = run(hp, Ps, src, K, torch.float32, store_bf16=True)
        assert rt.decode_hypothesis(a["seq"], hp) == rt.decode_hypothesis(b["seq"], hp), ("bf16 storage model", K, seed)
    return dict(m, Pn=Pn)


# ---------------------------------------------------------------------------------------------- the element-wise check
def assert_within(got, ref, bound, what):
    """Every element finite and within its bound; -> the largest |err| / bound (0 / 0 counts as 0)."""
    from tests import parity as PR
    got = np.asarray(got, np.float64)
    ref, bound = np.asarray(ref, np.float64).reshape(got.shape), np.asarray(bound, np.float64).reshape(got.shape)
    PR.assert_elementwise(torch.as_tensor(got), torch.as_tensor(ref), torch.as_tensor(bound), what)
    err = np.abs(got - ref)
    return float(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0).max())


def exceeds(got, ref, bound):
    """True when some element is outside its bound (or not finite): what a planted defect must do."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    return bool((~np.isfinite(err)).any() or (err > bound).any())


# ---------------------------------------------------------------------------------------------- Transformer decoder inputs
def _embed(target, hp, P):
    return rt._st_fwd(P[rt._emb_name(hp, "tgt")])[target] * (hp.hidden_size ** 0.5) + P["bias"]


def embed_step(target, time, hp, P):
    """The input of ONE cached decoder step: emb[target] sqrt(H) + bias, zero on the all-pad first step, plus the timing
    signal of position `time`; stored at the site "embed"."""
    inputs = _embed(target, hp, P)
    if bool((target == hp.tgt_vocab.pad()).all()):
        inputs = torch.zeros_like(inputs)
    return rt._st(inputs + rt.timing_signal(1, hp.hidden_size, P["bias"].dtype, time=time), "embed")


def embed_shifted(target, hp, P):
    """The inputs of the training-path decoder: the same embedding shifted right by one zero row, plus the timing signal."""
    inputs = torch.nn.functional.pad(_embed(target, hp, P), (0, 0, 1, 0))[:, :-1, :]
    return rt._st(inputs + rt.timing_signal(inputs.shape[1], hp.hidden_size, P["bias"].dtype), "embed")


def cached_state(encoder_state):
    """The state an encoding_fn hands to rt.beam_search under search_mode = cache."""
    encoder_state["decoder"] = {"state": encoder_state["decoder_initializer"]}
    return encoder_state


def empty_caches(B, H, n_layers, dtype):
    """The decoder_initializer of a Transformer encoder: per layer an empty self-attention cache."""
    return {"layer_%d" % l: {"k": torch.zeros(B, 0, H, dtype=dtype), "v": torch.zeros(B, 0, H, dtype=dtype)}
            for l in range(n_layers)}
