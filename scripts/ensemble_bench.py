"""Ensemble decode throughput on the BASELINE configs[3] decode shape (transformer_aan, Transformer-base sizes, beam 4,
alpha 0.6, decode_length 50, eval batch 32, V = 32000; the workload of scripts/decode_bench.py): M in {1, 2, 4} members of
identical shape (different random weights) against the single model, and the combine kernel (zk_ensemble_logprob) alone.

Prints ONE JSON line:
  single / ensemble[M]: sentences/s and ms per decode step -- median over --repeats passes over the same batches, after
      one warm-up pass (buffer sizing; the ensemble captures its step graphs anew for every batch, the single model
      replays cached ones), host clock around work that ends in a device synchronise;
  ensemble[M].steps_vs_single: ms per ensemble step / (M * ms per single-model step of this run);
  kernel[M]: the combine on [128, 32000] fp32 logits per member -- median of --kernel-iters calls, each between two HIP
      events, and the bytes it must move ((M + 1) * rows * V * 4: every member's logits read once, the result written
      once) over that time.  The kernel reads the logits a second time in its combine pass, mostly from the caches.

Every leg runs in a child process of its own under its own time limit; the first failing leg ends the run.

usage: python scripts/ensemble_bench.py [--sentences 256] [--repeats 3] [--dtype bfloat16]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _benchlib as BL  # noqa: E402

V = BL.V
ROWS = 128


def leg_decode(args, M):
    """M = 0: the single model through tower_infer_graph's pair; M >= 1: M members through the ensemble pair."""
    import numpy as np
    import torch
    from zero_amd.models import model as registry, load_all
    from zero_amd.search import beam_search
    load_all()
    graph = registry.get_model("transformer_aan")
    # members of identical shape, different weights
    hps = [BL.decode_hp("transformer_aan", "ensbench%d" % i, args.dtype, random_seed=1234 + i) for i in range(max(M, 1))]
    batches = BL.sorted_batches(V, args.sentences, hps[0].eval_batch_size)

    def one_pass():
        steps = sent = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for src in batches:
            if M == 0:
                enc, dec = graph.infer_fn(hps[0])
                out = beam_search({"source": src}, enc, dec, hps[0])
            else:
                from zero_amd.models._ensemble import make_infer_fns
                enc, dec, hp0 = make_infer_fns([graph] * M, hps)
                out = beam_search({"source": src}, enc, dec, hp0)
            steps += out["steps"]
            sent += src.shape[0]
        torch.cuda.synchronize()
        return time.perf_counter() - t0, steps, sent
    one_pass()                                                  # warm-up: buffer sizing, code objects
    runs = [one_pass() for _ in range(args.repeats)]
    ms = [1e3 * t / s for t, s, _ in runs]
    sps = [n / t for t, _, n in runs]
    return {"members": M, "sentences": runs[0][2], "decode_steps": runs[0][1], "repeats": args.repeats,
            "ms_per_step": float(np.median(ms)), "ms_per_step_min": min(ms), "ms_per_step_max": max(ms),
            "sentences_per_s": float(np.median(sps))}


def leg_kernel(args):
    import numpy as np
    import torch
    from zero_amd.func import Engine, Mat
    from zero_amd.models._ensemble import combine

    class _Core(object):                 # what combine() reads of a core
        pass
    core = _Core()
    core.eng, core.V, core.Vpad = Engine("cuda:0"), V, V
    out = {}
    g = torch.Generator().manual_seed(5)
    logits = [Mat((torch.randn(ROWS, V, generator=g) * 3).cuda(), ROWS, V) for _ in range(4)]
    for M in (1, 2, 4):
        for _ in range(10):
            combine(core, logits[:M], ROWS)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.kernel_iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            combine(core, logits[:M], ROWS)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e-3)
        t = float(np.median(times))
        nbytes = (M + 1) * ROWS * V * 4
        out[str(M)] = {"us": t * 1e6, "us_min": min(times) * 1e6, "bytes_must_move": nbytes, "bytes_per_s": nbytes / t,
                       "iters": args.kernel_iters}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--dtype", default="bfloat16")
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds per leg (a child process each)")
    ap.add_argument("--leg", default="", help="internal: run one leg in this process and print its JSON")
    args = ap.parse_args()
    if args.leg:
        res = leg_kernel(args) if args.leg == "kernel" else leg_decode(args, int(args.leg))
        print("LEG " + json.dumps(res))
        return 0
    legs, rc = BL.run_legs(__file__, ("0", "1", "2", "4", "kernel"), ["--sentences", args.sentences, "--repeats", args.repeats,
                                                                      "--kernel-iters", args.kernel_iters, "--dtype", args.dtype],
                           None, args.leg_timeout)
    if rc:
        return rc
    single = legs["0"]
    ens = {}
    for M in ("1", "2", "4"):
        ens[M] = dict(legs[M], steps_vs_single=legs[M]["ms_per_step"] / (int(M) * single["ms_per_step"]))
    print(json.dumps({"workload": "BASELINE configs[3] decode shape: transformer_aan base, beam 4, batch 32, V=32000, "
                                  "%d synthetic sentences, decode_dtype=%s" % (args.sentences, args.dtype),
                      "single": single, "ensemble": ens, "kernel": legs["kernel"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
