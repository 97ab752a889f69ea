"""What do sampling_topk / sampling_topp cost a decode step on this box?  The option adds ONE launch (zk_sample_truncate,
zero_amd/csrc/zk_sample.hip) between the step's logits and the Gumbel noise / the fused search tail: a per-row selection over
the V logits of every beam row.  Two parts, in ONE run so that a drift of the box hits every leg:

(1) ONE batch of the BASELINE configs[3] decode shape (batch 32, alpha 0.6, decode_length 50, V = 32000, H = 512, transformer,
    synthetic sentences of 28 +- 6 tokens) on one stream, beam 4 and beam 1, in bf16 and in fp32, with the option off, with
    sampling_topk = 10, with sampling_topp = 0.9, and with both.  The legs of a (dtype, beam) share ONE scope: the same weights
    and engine.  The off leg issues the launches the step had before the option existed.  Per leg: ms_per_step (search without
    the encoder pass, over the steps it took), decode_steps, launches_per_step (the nodes of the captured step).  No noise: the
    legs then decode deterministically, and random weights run to the length cap either way.
(2) zk_sample_truncate alone on logits [128, 32000] (randn * 5) with topk = 10, topp = 0.9 and both, min_keep = 9, beside
    zk_beam_topk (B 32, K 4, 2K = 8) on the same values: --iters back-to-back launches between two device events, and the same
    launch as the only node of a replayed graph.  The truncation works in place and the buffer is not restored between the
    launches: every launch makes the same passes over a row whatever it holds and stores all entries below its threshold
    again -- all but ten under top-k, which is idempotent; under top-p a truncated row's nucleus narrows from launch to launch
    (down to min_keep), which changes the number of stores by a few hundred of 32000.

Method as the sibling benches: two warm-up rounds, then --repeats rounds in which the legs ALTERNATE; median with minimum and
maximum.  No speed is asserted anywhere.  Reads nothing outside the repository.

Prints ONE JSON line and writes it to --out.

usage: python scripts/sampling_bench.py [--repeats 5] [--iters 200] [--dtypes bfloat16,float32] [--beams 4,1]
                                        [--out profiles/sampling_bench.json]"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _benchlib as BL  # noqa: E402

TAGS = {"bfloat16": "bf16", "float32": "fp32"}
LEGS = (("off", 0, 0.0), ("topk10", 10, 0.0), ("topp0.9", 0, 0.9), ("both", 10, 0.9))


def stat(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


class Leg(object):
    def __init__(self, name, dtype, K, topk, topp, src, base_hp):
        from zero_amd.models import model as registry
        from zero_amd.models._factory import get_core
        self.name, self.dtype, self.src = name, dtype, src
        self.hp = copy.copy(base_hp)
        self.hp.beam_size, self.hp.sampling_topk, self.hp.sampling_topp = K, topk, topp
        self.core = get_core(self.hp, "transformer")
        self.enc, self.dec = registry.get_model("transformer").infer_fn(self.hp)
        self.enc_ms, self.all_ms, self.steps, self.launches = [], [], 0, 0

    def once(self, record):
        import torch
        from zero_amd.search import beam_search
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        ev[0].record()
        self.enc(self.src, beam_size=self.hp.beam_size, max_steps=int(self.src.shape[1]) + self.hp.decode_length + 2)
        ev[1].record()
        torch.cuda.synchronize()
        ev[2].record()
        out = beam_search({"source": self.src}, self.enc, self.dec, self.hp)
        ev[3].record()
        torch.cuda.synchronize()
        if not self.launches:      # the first run of a leg captures its step graphs (the legs share the core, and its counter)
            self.launches = int(self.core.__dict__.get("_decode_step_launches", 0))
        if record:
            self.enc_ms.append(ev[0].elapsed_time(ev[1]))
            self.all_ms.append(ev[2].elapsed_time(ev[3]))
            self.steps = int(out["steps"])

    def result(self):
        per = [(a - e) / self.steps for a, e in zip(self.all_ms, self.enc_ms)]
        return {"leg": self.name, "decode_dtype": self.dtype, "beam_size": int(self.hp.beam_size),
                "sampling_topk": int(self.hp.sampling_topk), "sampling_topp": float(self.hp.sampling_topp),
                "sentences": int(self.src.shape[0]), "decode_steps": self.steps, "repeats": len(self.all_ms),
                "ms_per_step": stat(per), "launches_per_step": self.launches}


def kernel_part(repeats, iters):
    """zk_sample_truncate alone, beside zk_beam_topk on the same logits."""
    import torch
    from zero_amd.func import Engine, Mat
    e = Engine("cuda:%d" % torch.cuda.current_device())
    B, K, V = 32, 4, BL.V
    rows = B * K
    res = {}
    with torch.cuda.stream(e.work_stream):
        pristine = torch.randn(rows, V, device="cuda") * 5.0
        work = pristine.clone()
        prev = torch.zeros(rows, device="cuda")
        out_s = torch.zeros(B, 2 * K, device="cuda")
        out_i = torch.zeros(B, 2 * K, dtype=torch.int32, device="cuda")
        mat = Mat(pristine, rows, V)

        def truncate(topk, topp):
            return lambda: e.lib.call("zk_sample_truncate", work.data_ptr(), V, rows, V, topk, topp, 2 * K + 1, -1e8, e.stream)
        launches = {"zk_beam_topk": lambda: e.beam_topk(mat, prev, out_s, out_i, B, K, V, 2 * K, 1.0, 1.0, -1, 1e8)}
        for name, topk, topp in LEGS[1:]:
            launches["zk_sample_truncate/" + name] = truncate(topk, topp)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            return 1e3 * a.elapsed_time(b) / iters          # microseconds per call
        for name, fn in launches.items():
            work.copy_(pristine)
            fn()
            torch.cuda.synchronize()
            g = e.graph_capture(fn)
            try:
                res[name] = {"back_to_back_us": stat([timed(fn) for _ in range(2 + repeats)][2:]),
                             "graph_replay_us": stat([timed(lambda: e.graph_launch(g)) for _ in range(2 + repeats)][2:]),
                             "graph_nodes": int(e.last_graph_nodes)}
            finally:
                e.lib.call("zk_graph_destroy", g)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200, help="launches between two events in the kernel part")
    ap.add_argument("--dtypes", default=",".join(TAGS), help="comma-separated subset of: " + ", ".join(TAGS))
    ap.add_argument("--beams", default="4,1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_bench.json"), help="'' writes no file")
    args = ap.parse_args()
    import torch
    from zero_amd.models import load_all
    from zero_amd.models._factory import reset_cores
    if not torch.cuda.is_available():
        print("sampling_bench: needs a GPU (a CPU run measures nothing)", file=sys.stderr)
        return 1
    load_all()
    src = BL.one_batch(BL.V)
    legs = {}
    for dt in args.dtypes.split(","):
        for K in [int(k) for k in args.beams.split(",")]:
            reset_cores()
            base_hp = BL.decode_hp("transformer", "smbench_%s_k%d" % (TAGS[dt], K), dt)
            members = [Leg("%s/beam%d/%s" % (TAGS[dt], K, name), dt, K, topk, topp, src, base_hp) for name, topk, topp in LEGS]
            for m in members:
                m.once(False)
                m.once(False)
            for _ in range(args.repeats):
                for m in members:                    # alternating legs
                    m.once(True)
            base = None
            for m in members:
                r = legs[m.name] = m.result()
                print("sampling_bench: %s: %d steps, %.4f ms per step, %d launches per step" %
                      (m.name, r["decode_steps"], r["ms_per_step"]["median"], r["launches_per_step"]), file=sys.stderr)
                if base is None:
                    base = r
                else:
                    r["ms_per_step_vs_off"] = r["ms_per_step"]["median"] / base["ms_per_step"]["median"]
                    r["us_per_step_over_off"] = 1e3 * (r["ms_per_step"]["median"] - base["ms_per_step"]["median"])
    reset_cores()
    kern = kernel_part(args.repeats, args.iters)
    for k, r in kern.items():
        print("sampling_bench: %s: %.2f us back to back, %.2f us as a replayed graph" %
              (k, r["back_to_back_us"]["median"], r["graph_replay_us"]["median"]), file=sys.stderr)
    text = json.dumps({"workload": "ONE batch of the BASELINE configs[3] decode shape: transformer, batch 32, beam 4 and 1, "
                                   "decode_length 50, V=32000, H=512, random weights; sampling off, topk=10, topp=0.9 and both on the "
                                   "same weights; device events on one stream; alternating legs, median of %d; zk_sample_truncate "
                                   "and zk_beam_topk alone on [128, 32000] logits (randn * 5), %d launches between two events"
                                   % (args.repeats, args.iters),
                       "legs": legs, "kernel": kern})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
