"""What does no_repeat_ngram_size cost a decode step on this box?  The option adds ONE launch (zk_ngram_ban, zero_amd/csrc/
zk_ngram.hip) between the step's logits and the fused search tail.  Two parts, in ONE run so that a drift of the box hits every
leg:

(1) ONE batch of the BASELINE configs[3] decode shape (batch 32, beam 4, alpha 0.6, decode_length 50, V = 32000, H = 512,
    transformer, synthetic sentences of 28 +- 6 tokens) on one stream, in bf16 and in fp32, with no_repeat_ngram_size = 0 and
    = 3.  Both legs of a dtype share ONE scope: the same weights and engine.  The n = 0 leg issues the launches the step had
    before the option existed.  Per leg: ms_per_step (search without the encoder pass, over the steps it took), decode_steps,
    launches_per_step (the nodes of the captured step), and how many best hypotheses hold a 3-gram twice.  Random weights: the
    hypotheses run to the length cap either way, so both legs take the same number of steps.
(2) zk_ngram_ban alone on logits [128, 32000] with n = 3 at t = 32 and t = 128, the time read from a device word: histories
    over 2 symbols (every start position matches and stores) and all-distinct ones (none does); --iters back-to-back launches
    between two device events, and the same launch as the only node of a replayed graph.

Method as the sibling benches: two warm-up rounds, then --repeats rounds in which the legs ALTERNATE; median with minimum and
maximum.  No speed is asserted anywhere.  Reads nothing outside the repository.

Prints ONE JSON line and writes it to --out.

usage: python scripts/ngram_bench.py [--repeats 5] [--iters 200] [--dtypes bfloat16,float32] [--out profiles/ngram_bench.json]"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _benchlib as BL  # noqa: E402

TAGS = {"bfloat16": "bf16", "float32": "fp32"}
LEGS = (("n0", 0), ("n3", 3))


def stat(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def repeats_3gram(seqs):
    out = 0
    for row in seqs[:, 0]:
        toks = []
        for t in row:
            if int(t) in (0, 2):
                break
            toks.append(int(t))
        grams = [tuple(toks[i:i + 3]) for i in range(len(toks) - 2)]
        out += len(set(grams)) != len(grams)
    return out


class Leg(object):
    def __init__(self, name, dtype, n, src, base_hp):
        from zero_amd.models import model as registry
        from zero_amd.models._factory import get_core
        self.name, self.dtype, self.src = name, dtype, src
        self.hp = copy.copy(base_hp)
        self.hp.no_repeat_ngram_size = n
        self.core = get_core(self.hp, "transformer")
        self.enc, self.dec = registry.get_model("transformer").infer_fn(self.hp)
        self.enc_ms, self.all_ms, self.steps, self.rep = [], [], 0, 0

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
        ev[2].record()
        out = beam_search({"source": self.src}, self.enc, self.dec, self.hp)
        ev[3].record()
        torch.cuda.synchronize()
        if record:
            self.enc_ms.append(ev[0].elapsed_time(ev[1]))
            self.all_ms.append(ev[2].elapsed_time(ev[3]))
            self.steps = int(out["steps"])
            self.rep = repeats_3gram(np.asarray(out["seq"]))

    def result(self):
        per = [(a - e) / self.steps for a, e in zip(self.all_ms, self.enc_ms)]
        return {"leg": self.name, "decode_dtype": self.dtype, "no_repeat_ngram_size": int(self.hp.no_repeat_ngram_size),
                "sentences": int(self.src.shape[0]), "decode_steps": self.steps, "repeats": len(self.all_ms),
                "ms_per_step": stat(per), "best_hypotheses_with_a_repeated_3gram": int(self.rep),
                "launches_per_step": int(self.core.__dict__.get("_decode_step_launches", 0))}


def kernel_part(repeats, iters):
    """zk_ngram_ban alone."""
    import numpy as np
    import torch
    from zero_amd.func import Engine
    e = Engine("cuda:%d" % torch.cuda.current_device())
    rows, V, ldh, n = 128, BL.V, 136, 3
    rng = np.random.default_rng(7)
    logits = torch.randn(rows, V, device="cuda")
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    hists = {"two_symbols": rng.integers(3, 5, (rows, ldh)), "all_distinct": np.stack([rng.permutation(ldh) + 3 for _ in range(rows)])}
    res = {}
    with torch.cuda.stream(e.work_stream):
        for kind, h in hists.items():
            hist = torch.from_numpy(h.astype(np.int32)).cuda()
            launch = lambda: e.lib.call("zk_ngram_ban", logits.data_ptr(), V, rows, V, hist.data_ptr(), ldh, 0, word.data_ptr(),
                                        n, -1e8, e.stream)
            for t in (32, 128):
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
                    res["%s/t%d" % (kind, t)] = {
                        "back_to_back_us": stat([timed(launch) for _ in range(2 + repeats)][2:]),
                        "graph_replay_us": stat([timed(lambda: e.graph_launch(g)) for _ in range(2 + repeats)][2:])}
                finally:
                    e.lib.call("zk_graph_destroy", g)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200, help="launches between two events in the kernel part")
    ap.add_argument("--dtypes", default=",".join(TAGS), help="comma-separated subset of: " + ", ".join(TAGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ngram_bench.json"), help="'' writes no file")
    args = ap.parse_args()
    import torch
    from zero_amd.models import load_all
    from zero_amd.models._factory import reset_cores
    if not torch.cuda.is_available():
        print("ngram_bench: needs a GPU (a CPU run measures nothing)", file=sys.stderr)
        return 1
    load_all()
    src = BL.one_batch(BL.V)
    legs = {}
    for dt in args.dtypes.split(","):
        reset_cores()
        base_hp = BL.decode_hp("transformer", "ngbench_" + TAGS[dt], dt)
        members = [Leg("%s/%s" % (TAGS[dt], name), dt, n, src, base_hp) for name, n in LEGS]
        for m in members:
            m.once(False)
            m.once(False)
        for _ in range(args.repeats):
            for m in members:                    # alternating legs
                m.once(True)
        base = None
        for m in members:
            r = legs[m.name] = m.result()
            print("ngram_bench: %s: %d steps, %.4f ms per step, %d launches per step, %d of %d best hypotheses repeat a 3-gram" %
                  (m.name, r["decode_steps"], r["ms_per_step"]["median"], r["launches_per_step"],
                   r["best_hypotheses_with_a_repeated_3gram"], r["sentences"]), file=sys.stderr)
            if base is None:
                base = r
            else:
                r["ms_per_step_vs_n0"] = r["ms_per_step"]["median"] / base["ms_per_step"]["median"]
                r["us_per_step_over_n0"] = 1e3 * (r["ms_per_step"]["median"] - base["ms_per_step"]["median"])
    reset_cores()
    kern = kernel_part(args.repeats, args.iters)
    for k, r in kern.items():
        print("ngram_bench: zk_ngram_ban %s: %.2f us back to back, %.2f us as a replayed graph" %
              (k, r["back_to_back_us"]["median"], r["graph_replay_us"]["median"]), file=sys.stderr)
    text = json.dumps({"workload": "ONE batch of the BASELINE configs[3] decode shape: transformer, batch 32, beam 4, decode_length "
                                   "50, V=32000, H=512, random weights; no_repeat_ngram_size 0 and 3 on the same weights; device "
                                   "events on one stream; alternating legs, median of %d; zk_ngram_ban alone on [128, 32000] logits, "
                                   "n = 3, %d launches between two events" % (args.repeats, args.iters),
                       "legs": legs, "kernel": kern})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
