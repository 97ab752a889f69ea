"""What does a lexical shortlist (zero_amd/shortlist.py) buy a decode step on this box?  The output layer of a step multiplies
the B*K beam rows by the whole [V, H] softmax table and writes, then re-reads, fp32 logits [B*K, V]; with a shortlist V
becomes Vs.  The byte counts follow from the shapes -- this script measures the time.  Three parts, in ONE run so that a drift
of the box hits every leg:

(1) ONE batch of the BASELINE configs[3] decode shape (batch 32, beam 4, alpha 0.6, decode_length 50, V = 32000, H = 512,
    transformer, synthetic sentences of 28 +- 6 tokens) on one stream, in bf16 and in fp32, with the shortlist off and with a
    synthetic lexical table (four random translations per source word; shortlist_first 100, shortlist_round 1024) read with
    shortlist_best = 2 (Vs = 2048) and = 4 (Vs = 4096).  All legs of a dtype share ONE scope: the same weights and engine.
    Per leg: start_ms (one encoding_fn call: encoder, shortlist build + read-back + gather), ms_per_step, sentences_per_s,
    launches_per_step, Vs.  The shortlist legs carry their ratios to the leg without.
(2) Eight such batches on four lanes (zero_amd.evalu.decode_many) under the host clock: sentences per second, the same legs.
(3) The per-batch driver's two launches alone, --iters repetitions between two device events: zk_shortlist_build on the
    batch's source ids, and the zk_gather_rows_ex of Vs table rows (bf16 and fp32 rows of H = 512).

Method as the sibling benches: two warm-up rounds, then --repeats rounds in which the legs ALTERNATE; median with minimum and
maximum.  Random weights: the hypotheses run to the length cap.  No speed is asserted anywhere.

Prints ONE JSON line and writes it to --out.

usage: python scripts/shortlist_bench.py [--repeats 5] [--iters 20] [--dtypes bfloat16,float32] [--out profiles/shortlist_bench.json]"""
import argparse
import copy
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _benchlib as BL  # noqa: E402

TAGS = {"bfloat16": "bf16", "float32": "fp32"}
LEGS = (("off", None), ("Vs2048", 2), ("Vs4096", 4))        # name, shortlist_best
FIRST, ROUND, PER_WORD = 100, 1024, 4
LANE_BATCHES, LANES = 8, 4


def stat(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def write_table(path):
    """PER_WORD random translations per source id, by falling probability."""
    import numpy as np
    rng = np.random.default_rng(99)
    tgt = rng.integers(FIRST, BL.V, (BL.V, PER_WORD))
    with open(path, "w") as f:
        for s in range(3, BL.V):
            for i in range(PER_WORD):
                f.write("%d %d %.2f\n" % (tgt[s, i], s, 0.9 - 0.2 * i))


class Leg(object):
    def __init__(self, name, dtype, best, table, src, base_hp):
        from zero_amd.models import model as registry
        from zero_amd.models._factory import get_core
        self.name, self.dtype, self.src = name, dtype, src
        self.hp = copy.copy(base_hp)
        if best is not None:
            self.hp.override_from_dict(dict(shortlist_file=table, shortlist_first=FIRST, shortlist_best=best,
                                            shortlist_round=ROUND))
        self.core = get_core(self.hp, "transformer")
        self.enc, self.dec = registry.get_model("transformer").infer_fn(self.hp)
        self.enc_ms, self.all_ms, self.lanes_sps, self.steps, self.Vs = [], [], [], 0, BL.V

    def once(self, record):
        import torch
        from zero_amd.search import beam_search
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        ev[0].record()
        st = self.enc(self.src, beam_size=self.hp.beam_size, max_steps=int(self.src.shape[1]) + self.hp.decode_length + 2)
        ev[1].record()
        torch.cuda.synchronize()
        if st.get("shortlist") is not None:
            self.Vs = st["shortlist"].Vs
        ev[2].record()
        out = beam_search({"source": self.src}, self.enc, self.dec, self.hp)
        ev[3].record()
        torch.cuda.synchronize()
        if record:
            self.enc_ms.append(ev[0].elapsed_time(ev[1]))
            self.all_ms.append(ev[2].elapsed_time(ev[3]))
            self.steps = int(out["steps"])

    def lanes(self, record):
        import torch
        from zero_amd.evalu import decode_many
        from zero_amd.models import model as registry
        from zero_amd.search import beam_search
        import threading
        tl, hp = threading.local(), self.hp

        def work(src):
            if not hasattr(tl, "fns"):
                tl.fns = registry.get_model("transformer").infer_fn(hp)
            return beam_search({"source": src}, tl.fns[0], tl.fns[1], hp)["steps"]
        batches = [self.src] * LANE_BATCHES
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        decode_many(batches, work, streams=LANES)
        torch.cuda.synchronize()
        if record:
            self.lanes_sps.append(LANE_BATCHES * self.src.shape[0] / (time.perf_counter() - t0))

    def result(self):
        per = [(a - e) / self.steps for a, e in zip(self.all_ms, self.enc_ms)]
        sps = [1e3 * self.src.shape[0] / a for a in self.all_ms]
        return {"leg": self.name, "decode_dtype": self.dtype, "Vs": int(self.Vs), "sentences": int(self.src.shape[0]),
                "decode_steps": self.steps, "repeats": len(self.all_ms), "start_ms": stat(self.enc_ms), "ms_per_step": stat(per),
                "sentences_per_s": stat(sps), "four_lanes_sentences_per_s": stat(self.lanes_sps),
                "launches_per_step": int(self.core.__dict__.get("_decode_step_launches", 0))}


def driver_part(table, src, repeats, iters):
    """zk_shortlist_build and the row gather alone."""
    import numpy as np
    import torch
    from zero_amd import shortlist
    from zero_amd.config import SyntheticVocab
    from zero_amd.func import Engine
    e = Engine("cuda:%d" % torch.cuda.current_device())
    lex = shortlist.load_table(table, SyntheticVocab(BL.V), SyntheticVocab(BL.V))
    off, ids = torch.from_numpy(lex.off).cuda(), torch.from_numpy(lex.ids).cuda()
    s = torch.from_numpy(np.ascontiguousarray(src, dtype=np.int32)).cuda()
    out = torch.empty(BL.V + 2, dtype=torch.int32, device="cuda")
    H = 512

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / iters          # microseconds per call
    res = {}
    for name, best in LEGS[1:]:
        build = lambda: e.shortlist_build(s, s.shape[0], s.shape[1], s.shape[1], off, ids, best, FIRST, BL.V, ROUND,
                                          out[:BL.V], out[BL.V:])
        build()
        torch.cuda.synchronize()
        n, Vs = (int(x) for x in out[BL.V:].cpu())
        r = {"n": n, "Vs": Vs, "source_tokens": int((src != 0).sum()),
             "build_us": stat([timed(build) for _ in range(2 + repeats)][2:])}
        for dt, tag, esz in ((torch.bfloat16, "bf16", 2), (torch.float32, "fp32", 4)):
            full = torch.randn(BL.V, H, device="cuda").to(dt)
            dst = torch.empty(BL.V, H, device="cuda", dtype=dt)
            gather = lambda: e.lib.call("zk_gather_rows_ex", full.data_ptr(), H * esz, out.data_ptr(), dst.data_ptr(), H * esz,
                                        Vs, H * esz, 0, e.stream)
            r["gather_%s_us" % tag] = stat([timed(gather) for _ in range(2 + repeats)][2:])
        res[name] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="repetitions between two events in the driver part")
    ap.add_argument("--dtypes", default=",".join(TAGS), help="comma-separated subset of: " + ", ".join(TAGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shortlist_bench.json"), help="'' writes no file")
    args = ap.parse_args()
    import torch
    from zero_amd.models import load_all
    from zero_amd.models._factory import reset_cores
    if not torch.cuda.is_available():
        print("shortlist_bench: needs a GPU (a CPU run measures nothing)", file=sys.stderr)
        return 1
    load_all()
    src = BL.one_batch(BL.V)
    legs = {}
    with tempfile.TemporaryDirectory() as tmp:
        table = os.path.join(tmp, "lex.txt")
        write_table(table)
        for dt in args.dtypes.split(","):
            reset_cores()
            base_hp = BL.decode_hp("transformer", "slbench_" + TAGS[dt], dt)
            members = [Leg("%s/%s" % (TAGS[dt], name), dt, best, table, src, base_hp) for name, best in LEGS]
            for m in members:
                m.once(False)
                m.once(False)
            for _ in range(args.repeats):
                for m in members:                    # alternating legs
                    m.once(True)
            for r in range(2 + args.repeats):
                for m in members:
                    m.lanes(r >= 2)
            base = None
            for m in members:
                r = legs[m.name] = m.result()
                print("shortlist_bench: %s: Vs %d, start %.3f ms, %.4f ms per step, %.0f sentences/s on four lanes" %
                      (m.name, r["Vs"], r["start_ms"]["median"], r["ms_per_step"]["median"],
                       r["four_lanes_sentences_per_s"]["median"]), file=sys.stderr)
                if base is None:
                    base = r
                else:
                    for k in ("ms_per_step", "start_ms", "sentences_per_s", "four_lanes_sentences_per_s"):
                        r[k + "_vs_off"] = r[k]["median"] / base[k]["median"]
        reset_cores()
        driver = driver_part(table, src, args.repeats, args.iters)
    for k, r in driver.items():
        print("shortlist_bench: driver %s: n %d, build %.1f us, gather bf16 %.1f us, fp32 %.1f us" %
              (k, r["n"], r["build_us"]["median"], r["gather_bf16_us"]["median"], r["gather_fp32_us"]["median"]), file=sys.stderr)
    text = json.dumps({"workload": "ONE batch of the BASELINE configs[3] decode shape: transformer, batch 32, beam 4, "
                                   "decode_length 50, V=32000, H=512, random weights; shortlist_first %d, shortlist_round %d, a "
                                   "synthetic table of %d translations per source word; device events on one stream, host "
                                   "clock for %d batches on %d lanes; alternating legs, median of %d" %
                                   (FIRST, ROUND, PER_WORD, LANE_BATCHES, LANES, args.repeats), "legs": legs, "driver": driver})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
