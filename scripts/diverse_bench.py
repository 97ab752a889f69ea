"""What does diverse beam search (diverse_beam_groups / diverse_beam_strength) cost a decode step on this box?  With G > 1 the
step's fused tail (top-2K over the sentence's K V candidates + bookkeeping, one launch) becomes three steps: zk_beam_topk per beam
row with depth K + K/G, zk_diverse_select (zero_amd/csrc/zk_diverse.hip) and zk_beam_dev_advance.  Two parts, in ONE run so that a
drift of the box hits every leg:

(1) ONE batch of the BASELINE configs[3] decode shape (batch 32, alpha 0.6, decode_length 50, V = 32000, H = 512, transformer,
    synthetic sentences of 28 +- 6 tokens) on one stream, beam 4 and beam 8, in bf16 and in fp32, with G = 1 (off), 2 and 4,
    strength 0.5.  The legs of a (dtype, beam) share ONE scope: the same weights and engine.  The G = 1 leg issues the launches
    the step had before the option existed.  Per leg: ms_per_step (search without the encoder pass, over the steps it took),
    decode_steps, launches_per_step (the nodes of the captured step).  Random weights run to the length cap in every leg.
(2) On logits [B K, 32000] (randn * 5) for beam 4 and 8: zk_diverse_select alone (G = 2 and 4, on the lists the per-row top-k
    made), the per-row zk_beam_topk (B K sentences of beam 1, k2 = K + K/G), and the zk_beam_topk it replaces (B sentences of
    beam K, k2 = 2K): --iters back-to-back launches between two device events, and the same launch as the only node(s) of a
    replayed graph.

Method as the sibling benches: two warm-up rounds, then --repeats rounds in which the legs ALTERNATE; median with minimum and
maximum.  No speed is asserted anywhere.  Reads nothing outside the repository.

Prints ONE JSON line and writes it to --out.

usage: python scripts/diverse_bench.py [--repeats 5] [--iters 200] [--dtypes bfloat16,float32] [--beams 4,8]
                                       [--out profiles/diverse_bench.json]"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _benchlib as BL  # noqa: E402

TAGS = {"bfloat16": "bf16", "float32": "fp32"}
GROUPS = (1, 2, 4)
STRENGTH = 0.5


def stat(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


class Leg(object):
    def __init__(self, name, dtype, K, G, src, base_hp):
        from zero_amd.models import model as registry
        from zero_amd.models._factory import get_core
        self.name, self.dtype, self.src = name, dtype, src
        self.hp = copy.copy(base_hp)
        self.hp.beam_size, self.hp.diverse_beam_groups, self.hp.diverse_beam_strength = K, G, STRENGTH
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
                "diverse_beam_groups": int(self.hp.diverse_beam_groups), "diverse_beam_strength": STRENGTH,
                "sentences": int(self.src.shape[0]), "decode_steps": self.steps, "repeats": len(self.all_ms),
                "ms_per_step": stat(per), "launches_per_step": self.launches}


def kernel_part(repeats, iters, beams):
    """zk_diverse_select alone, the per-row zk_beam_topk, and the per-sentence zk_beam_topk they replace."""
    import torch
    from zero_amd.func import Engine, Mat
    e = Engine("cuda:%d" % torch.cuda.current_device())
    B, V = 32, BL.V
    res = {}
    with torch.cuda.stream(e.work_stream):
        for K in beams:
            rows = B * K
            logits = torch.randn(rows, V, device="cuda") * 5.0
            prev = -torch.rand(rows, device="cuda")
            out_s = torch.zeros(B, 2 * K, device="cuda")
            out_i = torch.zeros(B, 2 * K, dtype=torch.int32, device="cuda")
            mat = Mat(logits, rows, V)
            launches = {"beam%d/zk_beam_topk[B,K,2K]" % K:
                        lambda: e.beam_topk(mat, prev, out_s, out_i, B, K, V, 2 * K, 1.0, 1.0, -1, 1e8)}
            for G in GROUPS[1:]:
                if K % G or K + K // G > 16:
                    continue
                k2 = K + K // G
                cs = torch.zeros(rows, k2, device="cuda")
                ci = torch.zeros(rows, k2, dtype=torch.int32, device="cuda")
                launches["beam%d/G%d/zk_beam_topk[BK,1,%d]" % (K, G, k2)] = \
                    lambda cs=cs, ci=ci, k2=k2: e.beam_topk(mat, prev, cs, ci, rows, 1, V, k2, 1.0, 1.0, -1, 1e8)
                launches["beam%d/G%d/zk_diverse_select" % (K, G)] = \
                    lambda cs=cs, ci=ci, k2=k2, G=G: e.diverse_select(cs, ci, out_s, out_i, B, K, G, k2, V, STRENGTH, 1.0, 2)

            def timed(fn):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(iters):
                    fn()
                b.record()
                torch.cuda.synchronize()
                return 1e3 * a.elapsed_time(b) / iters          # microseconds per call
            for name, fn in launches.items():      # (insertion order: the select of a G runs on the lists just made)
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
    ap.add_argument("--beams", default="4,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diverse_bench.json"), help="'' writes no file")
    args = ap.parse_args()
    import torch
    from zero_amd.models import load_all
    from zero_amd.models._factory import reset_cores
    if not torch.cuda.is_available():
        print("diverse_bench: needs a GPU (a CPU run measures nothing)", file=sys.stderr)
        return 1
    load_all()
    src = BL.one_batch(BL.V)
    beams = [int(k) for k in args.beams.split(",")]
    legs = {}
    for dt in args.dtypes.split(","):
        for K in beams:
            reset_cores()
            base_hp = BL.decode_hp("transformer", "dvbench_%s_k%d" % (TAGS[dt], K), dt)
            members = [Leg("%s/beam%d/G%d" % (TAGS[dt], K, G), dt, K, G, src, base_hp) for G in GROUPS if K % G == 0]
            for m in members:
                m.once(False)
                m.once(False)
            for _ in range(args.repeats):
                for m in members:                    # alternating legs
                    m.once(True)
            base = None
            for m in members:
                r = legs[m.name] = m.result()
                print("diverse_bench: %s: %d steps, %.4f ms per step, %d launches per step" %
                      (m.name, r["decode_steps"], r["ms_per_step"]["median"], r["launches_per_step"]), file=sys.stderr)
                if base is None:
                    base = r
                else:
                    r["ms_per_step_vs_G1"] = r["ms_per_step"]["median"] / base["ms_per_step"]["median"]
                    r["us_per_step_over_G1"] = 1e3 * (r["ms_per_step"]["median"] - base["ms_per_step"]["median"])
    reset_cores()
    kern = kernel_part(args.repeats, args.iters, beams)
    for k, r in kern.items():
        print("diverse_bench: %s: %.2f us back to back, %.2f us as a replayed graph" %
              (k, r["back_to_back_us"]["median"], r["graph_replay_us"]["median"]), file=sys.stderr)
    text = json.dumps({"workload": "ONE batch of the BASELINE configs[3] decode shape: transformer, batch 32, beam 4 and 8, "
                                   "decode_length 50, V=32000, H=512, random weights; diverse_beam_groups 1 (off), 2 and 4 at "
                                   "strength 0.5 on the same weights; device events on one stream; alternating legs, median of "
                                   "%d; zk_diverse_select, the per-row zk_beam_topk and the per-sentence zk_beam_topk alone on "
                                   "[32 K, 32000] logits (randn * 5), %d launches between two events" % (args.repeats, args.iters),
                       "legs": legs, "kernel": kern})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
