"""What does decoding with ``deepnmt`` cost, per cell and depth, next to ``rnnsearch`` at the same sizes on the same box?  ONE
batch of the BASELINE configs[3] decode shape (batch 32, beam 4, alpha 0.6, decode_length 50, V = 32000, synthetic sentences of
28 +- 6 tokens) on one stream, hidden_size = embed_size = 512, in bf16 and in fp32:

    rnnsearch              cell=atr, caencoder (2 scans; a step is 10 launches of the model's own)
    deepnmt cell=atr       the defaults' form (caencoder, dl4mt_redict, no deep attention), num_encoder_layer = num_decoder_layer
                           = each of --depth (default 2 and 4): e + 10 + 5 (D - 1) launches per step, e = 2 in bf16, 1 in fp32
    deepnmt cell=gru       the same depths: e + 14 + 9 (D - 1) launches per step

Per leg (scripts/rnnsearch_bench.py Leg): encoder_ms (one encoding_fn call), ms_per_step ((whole beam search - encoder_ms of the
same repeat) / decode steps), sentences_per_s, launches_per_step (nodes of the captured step graph).

Method as scripts/deepatt_bench.py: device events on the calling stream around each call; two warm-up decodes per leg (the
second replays captured step graphs); then --repeats rounds in which the legs of a group ALTERNATE, so that a drift of the box
hits all; median with minimum and maximum.  Random weights: the hypotheses run to the length cap.  No speed is asserted anywhere.

Prints ONE JSON line and writes it to --out.

usage: python scripts/deepnmt_bench.py [--repeats 5] [--depth 2,4] [--out profiles/deepnmt_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _benchlib as BL  # noqa: E402
from rnnsearch_bench import Leg  # noqa: E402

H = E = 512
DTYPES = {"bfloat16": "bf16", "float32": "fp32"}


class DepthLeg(Leg):
    def __init__(self, leg, model, cell, dtype, depth, src):
        from zero_amd.models import model as registry
        from zero_amd.models._factory import get_core
        self.name, self.model, self.dtype, self.H, self.E, self.src = leg, model, dtype, H, E, src
        self.cell, self.depth = cell, depth
        self.hp = BL.decode_hp(model, "nmtbench_" + leg.replace("/", "_"), dtype, hidden_size=H, embed_size=E, cell=cell,
                               caencoder=True, use_deep_att=False, dl4mt_redict=True, layer_norm=False, num_heads=1,
                               num_encoder_layer=depth, num_decoder_layer=depth)
        self.core = get_core(self.hp, model)
        self.enc, self.dec = registry.get_model(model).infer_fn(self.hp)
        self.enc_ms, self.all_ms, self.steps = [], [], 0

    def result(self):
        out = Leg.result(self)
        out["cell"] = self.cell
        if self.model == "deepnmt":
            out["num_encoder_layer"] = out["num_decoder_layer"] = self.depth
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--depth", default="2,4", help="num_encoder_layer = num_decoder_layer of the deepnmt legs, comma-separated")
    ap.add_argument("--dtypes", default=",".join(DTYPES), help="comma-separated subset of: " + ", ".join(DTYPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deepnmt_bench.json"), help="'' writes no file")
    args = ap.parse_args()
    import torch
    from zero_amd.models import load_all
    from zero_amd.models._factory import reset_cores
    if not torch.cuda.is_available():
        print("deepnmt_bench: needs a GPU (a CPU run measures nothing)", file=sys.stderr)
        return 1
    load_all()
    src = BL.one_batch(BL.V)
    depths = [int(d) for d in args.depth.split(",")]
    legs = {}
    for dt in args.dtypes.split(","):
        tag = DTYPES[dt]
        reset_cores()
        members = [DepthLeg("%s/rnnsearch" % tag, "rnnsearch", "atr", dt, 1, src)]
        members += [DepthLeg("%s/deepnmt_%s_d%d" % (tag, cell, d), "deepnmt", cell, dt, d, src)
                    for d in depths for cell in ("atr", "gru")]
        for m in members:
            m.once(False)
            m.once(False)
        for _ in range(args.repeats):
            for m in members:                    # alternating legs
                m.once(True)
        base = None
        for m in members:
            r = legs[m.name] = m.result()
            print("deepnmt_bench: %s: %d launches per captured step, %d steps" % (m.name, r["launches_per_step"],
                                                                                 r["decode_steps"]), file=sys.stderr)
            if base is None:
                base = r
            else:
                r["ms_per_step_vs_rnnsearch"] = r["ms_per_step"]["median"] / base["ms_per_step"]["median"]
                r["encoder_ms_vs_rnnsearch"] = r["encoder_ms"]["median"] / base["encoder_ms"]["median"]
    text = json.dumps({"workload": "ONE batch of the BASELINE configs[3] decode shape: batch 32, beam 4, decode_length 50, "
                                   "V=32000, hidden_size = embed_size = 512, one stream, random weights; device events, "
                                   "alternating legs", "legs": legs})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
