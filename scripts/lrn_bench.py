"""What do the lrn / olrn cells buy ``rnnsearch_deepatt`` on this box?  Their recurrence is element-wise, so a whole scan is ONE
launch (zk_rnn_lrn_scan) after one input projection; with atr every position of every scan is a launch of its own.  Two parts,
both in ONE run so that a drift of the box hits every leg:

(1) ONE batch of the BASELINE configs[3] decode shape (batch 32, beam 4, alpha 0.6, decode_length 50, V = 32000, synthetic
    sentences of 28 +- 6 tokens) on one stream, hidden_size = embed_size = 512, num_encoder_layer = num_decoder_layer = --depth
    (default 2), in bf16 and in fp32, with cell = atr, lrn, olrn.  Per leg (scripts/rnnsearch_bench.py Leg): encoder_ms (one
    encoding_fn call), ms_per_step, sentences_per_s, launches_per_step; the lrn / olrn legs also carry their ratios to atr.
    Cell launches of an encoder pass: (1 + 2 NE) Ls for atr, 1 + NE for lrn / olrn; a step is 6 + 4 D launches for all three.
(2) The scan kernel alone, R = 32 rows, H = 512, Ls = 32 positions, bf16 and fp32, lrn single and olrn paired: ONE launch with
    T = 32 against 32 chained launches with T = 1 that hand the fp32 state on (what a launch-per-position schedule would issue).
    --iters (default 20) repetitions between two device events, per-repetition time reported.

Method as the sibling benches: device events on the calling stream, two warm-up rounds, then --repeats rounds in which the legs
ALTERNATE; median with minimum and maximum.  Random weights: the hypotheses run to the length cap.  No speed is asserted
anywhere.

Prints ONE JSON line and writes it to --out.

usage: python scripts/lrn_bench.py [--repeats 5] [--depth 2] [--iters 20] [--out profiles/lrn_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _benchlib as BL  # noqa: E402
from deepatt_bench import CellLeg  # noqa: E402

CELLS = ("atr", "lrn", "olrn")
TAGS = {"bfloat16": "bf16", "float32": "fp32"}
SCAN_R, SCAN_H, SCAN_T = 32, 512, 32


def stat(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


class ScanLeg(object):
    """One form of the scan kernel on random operands: whole() is one T-step launch, chained() T one-step launches."""

    def __init__(self, eng, dtype, gated, paired):
        import torch
        from zero_amd.func import Mat
        self.e, self.gated, self.Mat = eng, gated, Mat
        R, H, T = SCAN_R, SCAN_H, SCAN_T
        W = (4 if gated else 3) * H
        g = torch.Generator(device="cuda").manual_seed(5)
        rnd = lambda *s: torch.randn(*s, device="cuda", generator=g).to(dtype)
        self.lo = Mat(rnd(R * T, W), R * T, W)
        self.hi = Mat(rnd(R * T, W), R * T, W) if paired else None
        self.mask = Mat(torch.ones(R, T, device="cuda"), R, T)
        self.seq = Mat(torch.zeros(R * T, H, device="cuda", dtype=dtype), R * T, H)
        self.hs = [Mat(torch.zeros(R, H, device="cuda"), R, H) for _ in (0, 1)]

    def whole(self):
        self.e.rnn_lrn_scan(None, self.lo, self.hi, self.hs[0], self.seq, None, self.mask, SCAN_T, False, self.gated)

    def chained(self):
        R, T, Mat = SCAN_R, SCAN_T, self.Mat
        at = lambda m, t: None if m is None else Mat(m.t, R, m.cols, T * m.ld, t * m.ld)
        prev = None
        for t in range(T):
            self.e.rnn_lrn_scan(prev, at(self.lo, t), at(self.hi, t), self.hs[t & 1], at(self.seq, t), None,
                                (Mat(self.mask.t, R, 1, T, t), 1, T), 1, False, self.gated)
            prev = self.hs[t & 1]

    def time(self, fn, iters):
        import torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / iters                  # microseconds per repetition


def scan_part(repeats, iters):
    import torch
    from zero_amd.func import Engine
    eng = Engine("cuda:%d" % torch.cuda.current_device())
    out = {}
    for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        for name, gated, paired in (("lrn_single", False, False), ("olrn_paired", True, True)):
            leg = ScanLeg(eng, dtype, gated, paired)
            whole, chained = [], []
            for r in range(2 + repeats):
                w, c = leg.time(leg.whole, iters), leg.time(leg.chained, iters)       # alternating
                if r >= 2:
                    whole.append(w)
                    chained.append(c)
            res = {"rows": SCAN_R, "hidden_size": SCAN_H, "positions": SCAN_T, "one_launch_us": stat(whole),
                   "chained_%d_launches_us" % SCAN_T: stat(chained)}
            res["chained_over_one"] = res["chained_%d_launches_us" % SCAN_T]["median"] / res["one_launch_us"]["median"]
            res["us_per_position_in_one_launch"] = res["one_launch_us"]["median"] / SCAN_T
            out["%s/%s" % (tag, name)] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--depth", type=int, default=2, help="num_encoder_layer = num_decoder_layer")
    ap.add_argument("--iters", type=int, default=20, help="repetitions between two events in the scan part")
    ap.add_argument("--dtypes", default=",".join(TAGS), help="comma-separated subset of: " + ", ".join(TAGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lrn_bench.json"), help="'' writes no file")
    args = ap.parse_args()
    import torch
    from zero_amd.models import load_all
    from zero_amd.models._factory import reset_cores
    if not torch.cuda.is_available():
        print("lrn_bench: needs a GPU (a CPU run measures nothing)", file=sys.stderr)
        return 1
    load_all()
    src = BL.one_batch(BL.V)
    legs = {}
    for dt in args.dtypes.split(","):
        reset_cores()
        members = [CellLeg("%s/deepatt_%s" % (TAGS[dt], c), "rnnsearch_deepatt", c, dt, args.depth, src) for c in CELLS]
        for m in members:
            m.once(False)
            m.once(False)
        for _ in range(args.repeats):
            for m in members:                    # alternating legs
                m.once(True)
        base = None
        for m in members:
            r = legs[m.name] = m.result()
            Ls = r["source_width"]
            r["encoder_cell_launches"] = (1 + 2 * args.depth) * Ls if m.cell == "atr" else 1 + args.depth
            print("lrn_bench: %s: encoder %.3f ms, %.4f ms per step, %d launches per captured step" %
                  (m.name, r["encoder_ms"]["median"], r["ms_per_step"]["median"], r["launches_per_step"]), file=sys.stderr)
            if base is None:
                base = r
            else:
                r["ms_per_step_vs_atr"] = r["ms_per_step"]["median"] / base["ms_per_step"]["median"]
                r["encoder_ms_vs_atr"] = r["encoder_ms"]["median"] / base["encoder_ms"]["median"]
    reset_cores()
    scans = scan_part(args.repeats, args.iters)
    for k, r in scans.items():
        print("lrn_bench: scan %s: one launch %.1f us, %d chained %.1f us (x %.1f)" %
              (k, r["one_launch_us"]["median"], SCAN_T, r["chained_%d_launches_us" % SCAN_T]["median"], r["chained_over_one"]),
              file=sys.stderr)
    text = json.dumps({"workload": "ONE batch of the BASELINE configs[3] decode shape: batch 32, beam 4, decode_length 50, "
                                   "V=32000, hidden_size = embed_size = 512, num_encoder_layer = num_decoder_layer = %d, one "
                                   "stream, random weights; device events, alternating legs, median of %d" %
                                   (args.depth, args.repeats), "legs": legs, "scan": scans})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
