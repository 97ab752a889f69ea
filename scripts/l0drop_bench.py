"""What does L0Drop's pruning buy on the decode step?  The BASELINE configs[3] job shape (Transformer-base sizes, beam 4,
alpha 0.6, decode_length 50, eval batch 32, V = 32000, length-sorted synthetic sentences; the workload of bench.py --mode
decode) decoded with ``transformer`` and with ``transformer_l0drop`` on the SAME weights, the latter with a random
source_pruning direction (log_alpha of std ~3 over the LayerNormed encoder outputs) and biases that keep roughly 100 %,
50 % and 25 % of the source.

Prints ONE JSON line (and writes it to --out): per leg sentences/s and ms per decode step -- median over --repeats passes
over the same batches on --lanes execution lanes (zero_amd.evalu.decode_many), after a warm-up pass by every lane; host
clock around work that ends in a device synchronise -- and, for the pruned legs, the kept fraction the device counted
(sum of kept / sum of valid source positions over the job) and the mean memory length against the mean source length.
The all-kept leg against ``transformer`` is the cost of the feature itself: one more slot and two more launches plus one
4-byte read-back per batch.

Every leg runs in a child process of its own under its own time limit; the first failing leg ends the run.

usage: python scripts/l0drop_bench.py [--sentences 3000] [--repeats 3] [--lanes 4] [--dtype bfloat16]
       [--out profiles/l0drop_bench.json]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")      # before the HIP runtime initialises: several batches in flight

import _benchlib as BL  # noqa: E402

LOG_ALPHA_0 = math.log(1.0 / 11.0)
# leg -> bias of source_pruning (None: the plain transformer); log_alpha ~ N(b0, 3): quantiles of the normal distribution
LEGS = {"transformer": None, "keep100": 20.0, "keep50": LOG_ALPHA_0, "keep25": LOG_ALPHA_0 - 0.674 * 3.0}


def leg(args, name):
    import threading
    import numpy as np
    import torch
    from zero_amd.evalu import decode_many
    from zero_amd.models import model as registry, load_all
    from zero_amd.models._factory import get_core
    from zero_amd.search import beam_search
    from zero_amd.variables import initial_values
    load_all()
    b0 = LEGS[name]
    model = "transformer" if b0 is None else "transformer_l0drop"
    hp = BL.decode_hp(model, "l0bench_" + model, args.dtype)
    # the same weights in every leg
    values = initial_values(BL.decode_hp("transformer", "l0bench_transformer", args.dtype), "transformer", 1234)
    if b0 is not None:
        H = hp.hidden_size
        values["source_pruning/W_0_0"] = (np.random.default_rng(99).normal(0.0, 3.0 / math.sqrt(H), (H, 1))).astype(np.float32)
        values["source_pruning/b_0"] = np.asarray([b0], np.float32)
    core0 = get_core(hp, model, values)
    graph = registry.get_model(model)
    batches = BL.sorted_batches(BL.V, args.sentences, hp.eval_batch_size)
    tl = threading.local()
    stats = {"kept": 0, "valid": 0, "Lm": 0, "Ls": 0, "n": 0}
    lock = threading.Lock()

    def work(src, count=False):
        if not hasattr(tl, "fns"):
            tl.fns = graph.infer_fn(hp)
        out = beam_search({"source": src}, tl.fns[0], tl.fns[1], hp)
        if count and b0 is not None:
            core = get_core(hp, model)
            pre = "dq." if args.dtype == "float32" else "dc."
            B = src.shape[0]
            torch.cuda.synchronize()
            cnt = core.eng.bufs[pre + "l0.cnt"][:2 * B].view(2, B).cpu().numpy()
            with lock:
                stats["kept"] += int(cnt[0].sum()); stats["valid"] += int(cnt.sum())
                stats["Lm"] += 1 + int(cnt[0].max()); stats["Ls"] += src.shape[1]; stats["n"] += 1
        return out["steps"]

    decode_many(batches[-2:], work, args.lanes, each_lane=True)        # warm-up on the longest batches, by every lane
    decode_many(batches, work, args.lanes)
    runs = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = sum(decode_many(batches, work, args.lanes))
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0, steps))
    decode_many(batches, lambda s: work(s, True), 1)                   # untimed: the counts the device left, batch by batch
    n = sum(b.shape[0] for b in batches)
    res = {"leg": name, "model": model, "source_pruning_b0": b0, "sentences": n, "decode_steps": runs[0][1],
           "repeats": args.repeats, "lanes": args.lanes,
           "sentences_per_s": float(np.median([n / t for t, _ in runs])),
           "ms_per_step": float(np.median([1e3 * t / s for t, s in runs])),
           "ms_per_step_min": min(1e3 * t / s for t, s in runs), "ms_per_step_max": max(1e3 * t / s for t, s in runs),
           "launches_per_step": int(core0.__dict__.get("_decode_step_launches", 0))}
    if b0 is not None:
        res.update(kept_fraction=stats["kept"] / max(stats["valid"], 1), mean_memory_slots=stats["Lm"] / max(stats["n"], 1),
                   mean_source_length=stats["Ls"] / max(stats["n"], 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=4)
    ap.add_argument("--dtype", default="bfloat16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l0drop_bench.json"), help="'' writes no file")
    ap.add_argument("--leg-timeout", type=int, default=200, help="seconds per leg (a child process each)")
    ap.add_argument("--leg", default="", help="internal: run one leg in this process and print its JSON")
    args = ap.parse_args()
    if args.leg:
        print("LEG " + json.dumps(leg(args, args.leg)))
        return 0
    legs, rc = BL.run_legs(__file__, LEGS, ["--sentences", args.sentences, "--repeats", args.repeats, "--lanes", args.lanes,
                                            "--dtype", args.dtype], None, args.leg_timeout)
    if rc:
        return rc
    base = legs["transformer"]
    for name, r in legs.items():
        r["sentences_per_s_vs_transformer"] = r["sentences_per_s"] / base["sentences_per_s"]
    text = json.dumps({"workload": "BASELINE configs[3] decode shape: Transformer-base, beam 4, batch 32, V=32000, %d synthetic "
                                   "sentences, %d lanes, decode_dtype=%s; same weights in every leg"
                                   % (args.sentences, args.lanes, args.dtype),
                       "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"), "legs": legs})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
