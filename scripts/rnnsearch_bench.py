"""What does decoding with ``rnnsearch`` cost next to ``transformer`` at the same sizes?  ONE batch of the BASELINE
configs[3] decode shape (batch 32, beam 4, alpha 0.6, decode_length 50, V = 32000, synthetic sentences of 28 +- 6 tokens) on
one stream, hidden_size = embed_size = 512 for both models, in bf16 and in fp32; and rnnsearch alone at the reference's
default sizes (hidden_size 1000, embed_size 620: fp32 only, 620 is no multiple of 8).

Per leg:
    encoder_ms       one encoding_fn call (rnnsearch: embedding, the input projections, one launch per time step and cell of
                     the forward and the backward scan, decoder_initializer, the projected memory)
    ms_per_step      (whole beam search - encoder_ms of the same repeat) / decode steps
    sentences_per_s  sentences / whole beam search
    launches_per_step  nodes of the captured step graph

Method: device events on the calling stream around each call (the search runs on the engine's work stream between two
stream waits); two warm-up decodes per leg (the second replays captured step graphs); then --repeats rounds in which the
legs of a pair ALTERNATE (transformer, rnnsearch, transformer, ...), so that a drift of the box hits both; median with
minimum and maximum.  Random weights: the hypotheses run to the length cap, so the step counts of the two models are
close but not equal -- ms_per_step is the comparable figure, sentences_per_s the end-to-end one of this job.  No speed is
asserted anywhere.

Prints ONE JSON line and writes it to --out.

usage: python scripts/rnnsearch_bench.py [--repeats 5] [--out profiles/rnnsearch_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _benchlib as BL  # noqa: E402

# pair -> [(leg, model, decode_dtype, hidden_size, embed_size)]
PAIRS = {
    "bf16_512": [("bf16/transformer", "transformer", "bfloat16", 512, 512), ("bf16/rnnsearch", "rnnsearch", "bfloat16", 512, 512)],
    "fp32_512": [("fp32/transformer", "transformer", "float32", 512, 512), ("fp32/rnnsearch", "rnnsearch", "float32", 512, 512)],
    "fp32_reference_sizes": [("fp32/rnnsearch_1000_620", "rnnsearch", "float32", 1000, 620)],
}


class Leg(object):
    def __init__(self, leg, model, dtype, H, E, src):
        from zero_amd.models import model as registry
        from zero_amd.models._factory import get_core
        self.name, self.model, self.dtype, self.H, self.E, self.src = leg, model, dtype, H, E, src
        self.hp = BL.decode_hp(model, "rnnbench_" + leg.replace("/", "_"), dtype, hidden_size=H, embed_size=E, cell="atr",
                               caencoder=True, layer_norm=False)
        self.core = get_core(self.hp, model)
        self.enc, self.dec = registry.get_model(model).infer_fn(self.hp)
        self.enc_ms, self.all_ms, self.steps = [], [], 0

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
        if record:
            self.enc_ms.append(ev[0].elapsed_time(ev[1]))
            self.all_ms.append(ev[2].elapsed_time(ev[3]))
            self.steps = int(out["steps"])

    def result(self):
        import numpy as np
        per = [(a - e) / self.steps for a, e in zip(self.all_ms, self.enc_ms)]
        sps = [1e3 * self.src.shape[0] / a for a in self.all_ms]
        stat = lambda xs: {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}
        return {"leg": self.name, "model": self.model, "decode_dtype": self.dtype, "hidden_size": self.H, "embed_size": self.E,
                "sentences": int(self.src.shape[0]), "source_width": int(self.src.shape[1]), "decode_steps": self.steps,
                "repeats": len(self.all_ms), "encoder_ms": stat(self.enc_ms), "ms_per_step": stat(per),
                "sentences_per_s": stat(sps), "launches_per_step": int(self.core.__dict__.get("_decode_step_launches", 0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs", default=",".join(PAIRS), help="comma-separated subset of: " + ", ".join(PAIRS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnsearch_bench.json"), help="'' writes no file")
    args = ap.parse_args()
    import torch
    from zero_amd.models import load_all
    from zero_amd.models._factory import reset_cores
    if not torch.cuda.is_available():
        print("rnnsearch_bench: needs a GPU (a CPU run measures nothing)", file=sys.stderr)
        return 1
    load_all()
    src = BL.one_batch(BL.V)
    legs = {}
    for pair in args.pairs.split(","):
        reset_cores()
        members = [Leg(*spec, src) for spec in PAIRS[pair]]
        for m in members:
            m.once(False)
            m.once(False)
        for _ in range(args.repeats):
            for m in members:                    # alternating legs
                m.once(True)
        for m in members:
            legs[m.name] = m.result()
            print("rnnsearch_bench: %s: %d launches per captured step, %d steps" % (m.name, legs[m.name]["launches_per_step"],
                                                                                  legs[m.name]["decode_steps"]), file=sys.stderr)
        if len(members) == 2:
            a, b = (legs[m.name] for m in members)
            b["ms_per_step_vs_transformer"] = b["ms_per_step"]["median"] / a["ms_per_step"]["median"]
            b["sentences_per_s_vs_transformer"] = b["sentences_per_s"]["median"] / a["sentences_per_s"]["median"]
    text = json.dumps({"workload": "ONE batch of the BASELINE configs[3] decode shape: batch 32, beam 4, decode_length 50, "
                                   "V=32000, one stream, random weights; device events, alternating legs", "legs": legs})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
