"""What does a decode step of ``transformer_fixup`` cost next to ``transformer``?  ONE batch of the BASELINE configs[3]
shape (Transformer-base widths, batch 32, beam 4, alpha 0.6, decode_length 50, V = 32000, synthetic sentences of
28 +- 6 tokens) decoded on one stream, in bf16 and in fp32.  Every matrix the two models share by name holds the same
values in every leg (`transformer`'s draw; the fixup legs keep their offsets at 0 and their scales at 1):

    transformer          the default bf16 step: the fused attention launches (zk_dec_cross / zk_dec_self)
    transformer_unfused  ZERO_HIP_DECODE_FUSE_ATT=0 ZERO_HIP_DECODE_FUSE_LN=0: one launch per op -- the launch structure
                         transformer_fixup runs in, so fixup against this leg is the boundary alone (residual + LayerNorm ->
                         zk_fixup_residual, the ReLU epilogue of `enlarge` -> zk_fixup_relu_shift, no bias epilogues)
    transformer_fixup    projection, zk_attn_fwd, o_map, zk_fixup_residual; enlarge, zk_fixup_relu_shift, output,
                         zk_fixup_residual
    fp32: transformer / transformer_fixup (both one launch per op)

Prints ONE JSON line (and writes it to --out): per leg the ms per decode step -- median, min and max over --repeats
decodes of the same batch after two warm-up decodes (the second replays captured step graphs); host clock around work
that ends in a device synchronise -- the number of steps and the launches per captured step.  The outputs of the legs
are different models' outputs and are not compared here (tests/test_gpu_fixup_model.py does that).

Every leg runs in a child process of its own under its own time limit; the first failing leg ends the run.

usage: python scripts/fixup_bench.py [--repeats 5] [--out profiles/fixup_bench.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V = 32000
# leg -> (model, decode_dtype, ZERO_HIP_DECODE_FUSE_ATT and ZERO_HIP_DECODE_FUSE_LN)
LEGS = {"bf16/transformer": ("transformer", "bfloat16", "1"),
        "bf16/transformer_unfused": ("transformer", "bfloat16", "0"),
        "bf16/transformer_fixup": ("transformer_fixup", "bfloat16", "1"),
        "fp32/transformer": ("transformer", "float32", "1"),
        "fp32/transformer_fixup": ("transformer_fixup", "float32", "1")}


def _params(model, dtype):
    from zero_amd.config import transformer_base_params, SyntheticVocab
    hp = transformer_base_params(model_name=model, scope_name="fixupbench_" + model, beam_size=4, decode_alpha=0.6,
                                 decode_length=50, eval_batch_size=32)
    hp.src_vocab = SyntheticVocab(V)
    hp.tgt_vocab = SyntheticVocab(V)
    hp.decode_dtype = dtype
    hp.search_mode = "cache"
    hp.random_seed = 1234
    return hp


def leg(args, name):
    import numpy as np
    import torch
    from zero_amd.models import model as registry, load_all
    from zero_amd.models._factory import get_core
    from zero_amd.search import beam_search
    from zero_amd.variables import initial_values
    load_all()
    model, dtype, _ = LEGS[name]
    hp = _params(model, dtype)
    values = initial_values(hp, model, 1234)
    # the same matrices in every leg: fixup's own draw leaves o_map and the FFN output at zero (modules/fixup.py:52, 185)
    base = initial_values(_params("transformer", dtype), "transformer", 1234)
    values.update({k: v for k, v in base.items() if k in values})
    core = get_core(hp, model, values)
    rng = np.random.default_rng(1234)
    lens = np.clip(np.rint(rng.normal(28, 6, hp.eval_batch_size)), 8, 48).astype(int)
    src = np.zeros((len(lens), int(lens.max()) + 1), dtype=np.int64)
    for r, n in enumerate(lens):
        src[r, :n] = rng.integers(3, V, n)
        src[r, n] = 2
    enc, dec = registry.get_model(model).infer_fn(hp)

    def once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = beam_search({"source": src}, enc, dec, hp)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, int(out["steps"])
    once()
    once()
    runs = [once() for _ in range(args.repeats)]
    per = [1e3 * t / s for t, s in runs]
    return {"leg": name, "model": model, "decode_dtype": dtype, "sentences": int(src.shape[0]), "source_width": int(src.shape[1]),
            "decode_steps": runs[0][1], "repeats": args.repeats, "ms_per_step": float(np.median(per)),
            "ms_per_step_min": min(per), "ms_per_step_max": max(per),
            "launches_per_step": int(core.__dict__.get("_decode_step_launches", 0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fixup_bench.json"), help="'' writes no file")
    ap.add_argument("--leg-timeout", type=int, default=150, help="seconds per leg (a child process each)")
    ap.add_argument("--leg", default="", help="internal: run one leg in this process and print its JSON")
    args = ap.parse_args()
    if args.leg:
        print("LEG " + json.dumps(leg(args, args.leg)))
        return 0
    legs = {}
    for name, (_, _, fuse) in LEGS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--repeats", str(args.repeats)]
        env = dict(os.environ, ZERO_HIP_DECODE_FUSE_ATT=fuse, ZERO_HIP_DECODE_FUSE_LN=fuse)
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.leg_timeout, text=True, env=env)
        except subprocess.TimeoutExpired:
            print("fixup_bench: leg %s exceeded %d s; stopping" % (name, args.leg_timeout), file=sys.stderr)
            return 124
        lines = [l for l in p.stdout.splitlines() if l.startswith("LEG ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stderr[-4000:])
            print("fixup_bench: leg %s failed (exit %d); stopping" % (name, p.returncode), file=sys.stderr)
            return p.returncode or 1
        legs[name] = json.loads(lines[-1][4:])
    for dt in ("bf16", "fp32"):
        r = legs[dt + "/transformer_fixup"]
        r["ms_per_step_vs_transformer"] = r["ms_per_step"] / legs[dt + "/transformer"]["ms_per_step"]
        if dt == "bf16":
            r["ms_per_step_vs_transformer_unfused"] = r["ms_per_step"] / legs["bf16/transformer_unfused"]["ms_per_step"]
    text = json.dumps({"workload": "ONE batch of the BASELINE configs[3] decode shape: Transformer-base, beam 4, batch 32, "
                                   "V=32000, one stream; same weights in every leg", "legs": legs})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
