"""What the decode benchmarks of scripts/ share: the BASELINE configs[3] decode shape, its synthetic batches, the host-clock
timing of whole decodes and the runner that gives every leg a child process of its own.  The measurement method and the
output format stay with each script."""
import json
import os
import subprocess
import sys
import time

import numpy as np

V = 32000


def decode_hp(model, scope, dtype, **over):
    """Transformer-base widths, beam 4, alpha 0.6, decode_length 50, eval batch 32, synthetic vocabularies of V words,
    search_mode = cache, seed 1234; `over` replaces or adds hparams."""
    from zero_amd.config import transformer_base_params, SyntheticVocab
    hp = transformer_base_params(**dict(dict(model_name=model, scope_name=scope, beam_size=4, decode_alpha=0.6, decode_length=50,
                                             eval_batch_size=32, decode_dtype=dtype, search_mode="cache", random_seed=1234),
                                        **over))
    hp.src_vocab = SyntheticVocab(V)
    hp.tgt_vocab = SyntheticVocab(V)
    return hp


def _fill(V, lens, rng):
    src = np.zeros((len(lens), int(max(lens)) + 1), dtype=np.int64)
    for r, n in enumerate(lens):
        src[r, :n] = rng.integers(3, V, n)
        src[r, n] = 2
    return src


def one_batch(V, n=32):
    """ONE batch of n synthetic sentences of 28 +- 6 tokens (clipped to 8 .. 48) and their EOS."""
    rng = np.random.default_rng(1234)
    return _fill(V, np.clip(np.rint(rng.normal(28, 6, n)), 8, 48).astype(int), rng)


def sorted_batches(V, sentences, batch):
    """The job of bench.py --mode decode: sentences of 28 +- 14 tokens (clipped to 4 .. 100) in length-sorted batches
    (data.py:69-73)."""
    rng = np.random.default_rng(1234)
    lens = np.clip(np.rint(rng.normal(28, 14, sentences)), 4, 100).astype(int)
    order = np.argsort(lens, kind="stable")
    return [_fill(V, lens[order[b0:b0 + batch]], rng) for b0 in range(0, sentences, batch)]


def time_decodes(fn, repeats):
    """fn() -> decode steps.  Two warm-up calls (the second replays captured step graphs), then `repeats` calls under the
    host clock, each between two device synchronises.  -> dict decode_steps, repeats, ms_per_step (median), _min, _max."""
    import torch

    def once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = int(fn())
        torch.cuda.synchronize()
        return time.perf_counter() - t0, steps
    once()
    once()
    runs = [once() for _ in range(repeats)]
    per = [1e3 * t / s for t, s in runs]
    return {"decode_steps": runs[0][1], "repeats": repeats, "ms_per_step": float(np.median(per)), "ms_per_step_min": min(per),
            "ms_per_step_max": max(per)}


def run_legs(script, legs, argv, env_of, timeout):
    """`python script --leg <leg> argv...` once per leg, each in a child process of its own under `timeout` seconds and with
    env_of(leg) added to the environment (env_of None: nothing added); a leg answers with a line "LEG <json>".  The first
    failing leg ends the run.  -> ({leg: its JSON}, 0), or (None, exit code): 124 after a time-out."""
    who = os.path.basename(script)[:-3]
    out = {}
    for leg in legs:
        cmd = [sys.executable, os.path.abspath(script), "--leg", leg] + [str(a) for a in argv]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=True,
                               env=dict(os.environ, **(env_of(leg) if env_of else {})))
        except subprocess.TimeoutExpired:
            print("%s: leg %s exceeded %d s; stopping" % (who, leg, timeout), file=sys.stderr)
            return None, 124
        lines = [l for l in p.stdout.splitlines() if l.startswith("LEG ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stderr[-4000:])
            print("%s: leg %s failed (exit %d); stopping" % (who, leg, p.returncode), file=sys.stderr)
            return None, p.returncode or 1
        out[leg] = json.loads(lines[-1][4:])
    return out, 0
