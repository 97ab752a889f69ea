"""What does a decode step of ``transformer_rela`` or ``transformer_fixup`` cost next to ``transformer``?  ONE batch of the
BASELINE configs[3] shape (Transformer-base widths, batch 32, beam 4, alpha 0.6, decode_length 50, V = 32000, synthetic
sentences of 28 +- 6 tokens) decoded on one stream, in bf16 and in fp32, with the same weights in every leg.

--variant rela   (the rela leg adds its post/{scale, gate} vectors to `transformer`'s draw):

    transformer          the default bf16 step: the fused attention launches (zk_dec_cross / zk_dec_self)
    transformer_unfused  ZERO_HIP_DECODE_FUSE_ATT=0: one launch per op -- the launch structure transformer_rela runs in,
                         so rela against this leg is the attention kernel alone (zk_attn_fwd -> zk_rela_attn)
    transformer_rela     projection, zk_rela_attn, o_map, residual + LayerNorm
                         (rela against `transformer` = kernel + what the launch-per-op structure costs)
    fp32: transformer / transformer_rela (both one launch per op: zk_f32_attn -> zk_f32_rela_attn)

--variant fixup  (every matrix the two models share by name holds `transformer`'s draw; the fixup legs keep their offsets
                  at 0 and their scales at 1):

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
are different models' outputs and are not compared here (tests/test_gpu_rela_model.py, tests/test_gpu_fixup_model.py do
that).

Every leg runs in a child process of its own under its own time limit; the first failing leg ends the run.

usage: python scripts/variant_step_bench.py --variant {rela,fixup} [--repeats 5] [--out profiles/<variant>_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _benchlib as BL  # noqa: E402

# variant -> the environment switches a leg sets (to 0 in the unfused leg, to 1 in every other), and which of `transformer`'s
# values a leg takes: all of them (rela: the variant only ADDS vectors), or only those of names the variant has itself
# (fixup's own draw leaves o_map and the FFN output at zero, modules/fixup.py:52, 185; it has no biases or LayerNorms)
VARIANTS = {"rela": dict(env=("ZERO_HIP_DECODE_FUSE_ATT",), shared_names_only=False),
            "fixup": dict(env=("ZERO_HIP_DECODE_FUSE_ATT", "ZERO_HIP_DECODE_FUSE_LN"), shared_names_only=True)}


def legs_of(variant):
    """leg -> (model, decode_dtype, the value of the variant's environment switches)"""
    m = "transformer_" + variant
    return {"bf16/transformer": ("transformer", "bfloat16", "1"),
            "bf16/transformer_unfused": ("transformer", "bfloat16", "0"),
            "bf16/" + m: (m, "bfloat16", "1"),
            "fp32/transformer": ("transformer", "float32", "1"),
            "fp32/" + m: (m, "float32", "1")}


def leg(args, name):
    from zero_amd.models import model as registry, load_all
    from zero_amd.models._factory import get_core
    from zero_amd.search import beam_search
    from zero_amd.variables import initial_values
    load_all()
    model, dtype, _ = legs_of(args.variant)[name]
    params = lambda m: BL.decode_hp(m, "%sbench_%s" % (args.variant, m), dtype)
    hp = params(model)
    values = initial_values(hp, model, 1234)
    base = initial_values(params("transformer"), "transformer", 1234)                    # the same weights in every leg
    values.update({k: v for k, v in base.items() if k in values} if VARIANTS[args.variant]["shared_names_only"] else base)
    core = get_core(hp, model, values)
    src = BL.one_batch(BL.V, hp.eval_batch_size)
    enc, dec = registry.get_model(model).infer_fn(hp)
    res = {"leg": name, "model": model, "decode_dtype": dtype, "sentences": int(src.shape[0]), "source_width": int(src.shape[1])}
    res.update(BL.time_decodes(lambda: beam_search({"source": src}, enc, dec, hp)["steps"], args.repeats))
    res["launches_per_step"] = int(core.__dict__.get("_decode_step_launches", 0))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", required=True, choices=sorted(VARIANTS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="default profiles/<variant>_bench.json; '' writes no file")
    ap.add_argument("--leg-timeout", type=int, default=150, help="seconds per leg (a child process each)")
    ap.add_argument("--leg", default="", help="internal: run one leg in this process and print its JSON")
    args = ap.parse_args()
    if args.leg:
        print("LEG " + json.dumps(leg(args, args.leg)))
        return 0
    table = legs_of(args.variant)
    legs, rc = BL.run_legs(__file__, table, ["--variant", args.variant, "--repeats", args.repeats],
                           lambda name: dict.fromkeys(VARIANTS[args.variant]["env"], table[name][2]), args.leg_timeout)
    if rc:
        return rc
    for dt in ("bf16", "fp32"):
        r = legs["%s/transformer_%s" % (dt, args.variant)]
        r["ms_per_step_vs_transformer"] = r["ms_per_step"] / legs[dt + "/transformer"]["ms_per_step"]
        if dt == "bf16":
            r["ms_per_step_vs_transformer_unfused"] = r["ms_per_step"] / legs["bf16/transformer_unfused"]["ms_per_step"]
    text = json.dumps({"workload": "ONE batch of the BASELINE configs[3] decode shape: Transformer-base, beam 4, batch 32, "
                                   "V=32000, one stream; same weights in every leg", "legs": legs})
    print(text)
    out = os.path.join(ROOT, "profiles", args.variant + "_bench.json") if args.out is None else args.out
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
