"""What does tgt_prefix_file cost a decode step on this box?  The option adds ONE launch (zk_prefix_force, zero_amd/csrc/
zk_prefix.hip) directly ahead of the fused search tail.  Two parts, in ONE run so that a drift of the box hits every leg:

(1) ONE batch of the BASELINE configs[3] decode shape (batch 32, beam 4, alpha 0.6, decode_length 50, V = 32000, H = 512,
    transformer, synthetic sentences of 28 +- 6 tokens) on one stream, in bf16 and in fp32, in three legs that share ONE scope
    (the same weights and engine):
      off      no features["prefix"]: the launches the step had before the option existed
      ended    a table whose only prefix is one token of sentence 0: the launch is in every step, and from step 1 on every
               workgroup leaves after its two reads
      forced   every sentence forced for all but the last step it may take (source length + decode_length - 1 random tokens):
               every row of every step is rewritten, 128 x 32000 floats = 16 MB of stores
    Per leg: ms_per_step (search without the encoder pass, over the steps it took), decode_steps, launches_per_step (the nodes
    of the captured step).  Random weights: the off and ended legs run to the length cap; so does the forced one by construction.
(2) zk_prefix_force alone on logits [128, 32000], the time read from a device word, at a forced time (every row rewritten)
    and at a time behind the table's prefixes (every workgroup exits): --iters back-to-back launches between two device
    events, and the same launch as the only node of a replayed graph.  Its neighbour on the same shape is zk_sample_truncate,
    which reads and writes whole rows: 22 - 26 us in profiles/sampling_bench.json.

Method as the sibling benches: two warm-up rounds, then --repeats rounds in which the legs ALTERNATE; median with minimum and
maximum.  No speed is asserted anywhere.  Reads nothing outside the repository.

Prints ONE JSON line and writes it to --out.

usage: python scripts/prefix_bench.py [--repeats 5] [--iters 200] [--dtypes bfloat16,float32] [--out profiles/prefix_bench.json]"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _benchlib as BL  # noqa: E402

TAGS = {"bfloat16": "bf16", "float32": "fp32"}
LEGS = ("off", "ended", "forced")


def stat(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def tables(src, hp):
    """-> {leg: features["prefix"] or None}."""
    import numpy as np
    rng = np.random.default_rng(11)
    n = (np.asarray(src) != 0).sum(1) + hp.decode_length - 1
    forced = np.zeros((src.shape[0], int(n.max())), dtype=np.int32)
    for b, nb in enumerate(n):
        forced[b, :nb] = rng.integers(3, BL.V, int(nb))
    ended = np.zeros((src.shape[0], 1), dtype=np.int32)
    ended[0, 0] = 7
    return {"off": None, "ended": ended, "forced": forced}


class Leg(object):
    def __init__(self, name, dtype, prefix, src, base_hp):
        from zero_amd.models import model as registry
        from zero_amd.models._factory import get_core
        self.name, self.dtype, self.src, self.prefix = name, dtype, src, prefix
        self.hp = copy.copy(base_hp)
        self.core = get_core(self.hp, "transformer")
        self.enc, self.dec = registry.get_model("transformer").infer_fn(self.hp)
        self.enc_ms, self.all_ms, self.steps, self.held, self.launches = [], [], 0, 0, 0

    def once(self, record):
        import numpy as np
        import torch
        from zero_amd.search import beam_search
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        ev[0].record()
        self.enc(self.src, beam_size=self.hp.beam_size, max_steps=int(self.src.shape[1]) + self.hp.decode_length + 2)
        ev[1].record()
        torch.cuda.synchronize()
        feats = {"source": self.src}
        if self.prefix is not None:
            feats["prefix"] = self.prefix
        ev[2].record()
        out = beam_search(feats, self.enc, self.dec, self.hp)
        ev[3].record()
        torch.cuda.synchronize()
        if not self.launches:      # the leg's first search captures its step (later ones adopt the graphs of their shape)
            self.launches = int(self.core.__dict__.get("_decode_step_launches", 0))
        if record:
            self.enc_ms.append(ev[0].elapsed_time(ev[1]))
            self.all_ms.append(ev[2].elapsed_time(ev[3]))
            self.steps = int(out["steps"])
            if self.prefix is not None:
                seqs = np.asarray(out["seq"])
                self.held = sum(int(np.array_equal(seqs[b, 0, :int((p != 0).sum())], p[p != 0])) for b, p in enumerate(self.prefix))

    def result(self):
        per = [(a - e) / self.steps for a, e in zip(self.all_ms, self.enc_ms)]
        return {"leg": self.name, "decode_dtype": self.dtype, "sentences": int(self.src.shape[0]), "decode_steps": self.steps,
                "repeats": len(self.all_ms), "ms_per_step": stat(per), "launches_per_step": self.launches,
                "best_hypotheses_that_start_with_their_prefix": int(self.held)}


def kernel_part(repeats, iters):
    """zk_prefix_force alone."""
    import numpy as np
    import torch
    from zero_amd.func import Engine
    e = Engine("cuda:%d" % torch.cuda.current_device())
    rows, K, V, ldp = 128, 4, BL.V, 64
    rng = np.random.default_rng(7)
    logits = torch.randn(rows, V, device="cuda")
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    table = np.zeros((rows // K, ldp), dtype=np.int32)
    table[:, :32] = rng.integers(3, V, (rows // K, 32))
    tab = torch.from_numpy(table).cuda()
    res = {}
    with torch.cuda.stream(e.work_stream):
        launch = lambda: e.lib.call("zk_prefix_force", logits.data_ptr(), V, rows, V, tab.data_ptr(), ldp, K, 0, word.data_ptr(),
                                    2, -1e8, e.stream)
        for kind, t in (("forced/t16", 16), ("ended/t40", 40)):
            word.fill_(t)
            launch()
            torch.cuda.synchronize()
            g = e.graph_capture(launch)

            def timed(fn):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(iters):
                    fn()
                b.record()
                torch.cuda.synchronize()
                return 1e3 * a.elapsed_time(b) / iters          # microseconds per call
            try:
                res[kind] = {"back_to_back_us": stat([timed(launch) for _ in range(2 + repeats)][2:]),
                             "graph_replay_us": stat([timed(lambda: e.graph_launch(g)) for _ in range(2 + repeats)][2:])}
            finally:
                e.lib.call("zk_graph_destroy", g)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200, help="launches between two events in the kernel part")
    ap.add_argument("--dtypes", default=",".join(TAGS), help="comma-separated subset of: " + ", ".join(TAGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefix_bench.json"), help="'' writes no file")
    args = ap.parse_args()
    import torch
    from zero_amd.models import load_all
    from zero_amd.models._factory import reset_cores
    if not torch.cuda.is_available():
        print("prefix_bench: needs a GPU (a CPU run measures nothing)", file=sys.stderr)
        return 1
    load_all()
    src = BL.one_batch(BL.V)
    legs = {}
    for dt in args.dtypes.split(","):
        reset_cores()
        base_hp = BL.decode_hp("transformer", "pfbench_" + TAGS[dt], dt)
        tabs = tables(src, base_hp)
        members = [Leg("%s/%s" % (TAGS[dt], name), dt, tabs[name], src, base_hp) for name in LEGS]
        for m in members:
            m.once(False)
            m.once(False)
        for _ in range(args.repeats):
            for m in members:                    # alternating legs
                m.once(True)
        base = None
        for m in members:
            r = legs[m.name] = m.result()
            print("prefix_bench: %s: %d steps, %.4f ms per step, %d launches per step, %d of %d best hypotheses start with their prefix"
                  % (m.name, r["decode_steps"], r["ms_per_step"]["median"], r["launches_per_step"],
                     r["best_hypotheses_that_start_with_their_prefix"], r["sentences"]), file=sys.stderr)
            if base is None:
                base = r
            else:
                r["ms_per_step_vs_off"] = r["ms_per_step"]["median"] / base["ms_per_step"]["median"]
                r["us_per_step_over_off"] = 1e3 * (r["ms_per_step"]["median"] - base["ms_per_step"]["median"])
    reset_cores()
    kern = kernel_part(args.repeats, args.iters)
    for k, r in kern.items():
        print("prefix_bench: zk_prefix_force %s: %.2f us back to back, %.2f us as a replayed graph" %
              (k, r["back_to_back_us"]["median"], r["graph_replay_us"]["median"]), file=sys.stderr)
    text = json.dumps({"workload": "ONE batch of the BASELINE configs[3] decode shape: transformer, batch 32, beam 4, decode_length "
                                   "50, V=32000, H=512, random weights; legs off / ended / forced on the same weights; device "
                                   "events on one stream; alternating legs, median of %d; zk_prefix_force alone on [128, 32000] "
                                   "logits, %d launches between two events" % (args.repeats, args.iters),
                       "legs": legs, "kernel": kern})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
