"""What does the fp32 scorer cost, and does its attention kernel do what it was written for?

(a) kernel   zk_f32_attn_seq (one workgroup per block of 32 query rows, keys and values staged in LDS once per block)
             against the per-row zk_f32_attn (one wave per query row, every row streams the sentence's keys and values from
             memory), fed the SAME operands at B = 64, nh = 8, d = 64, Lq = Lk = 64: q / k / v as column slices of one
             [B L, 3H] projection, no mask.  Non-causal for both kernels, causal for the new kernel only (the per-row kernel
             has no causal form).  Legs alternate inside every repetition; a leg is --inner back-to-back launches between
             two device events, so that the window is the kernel and not the launch.  Outputs of the two kernels are
             compared on the way (largest absolute difference; their score chains are the same, the softmax is online in
             one and two-pass in the other).
(b) scorer   sentences/s of score_fn with score_dtype = float32 and = bfloat16 on ONE batch of 64 sentence pairs of 64
             tokens of the Transformer-base model (V = 32000), same weights, device events around a whole score_fn call
             (upload included), the two legs alternating.

Prints ONE JSON line and writes it to --out: per leg the median, min and max over --repeats, and the ratios of medians.

usage: python scripts/score_f32_bench.py [--repeats 30] [--inner 20] [--out profiles/score_f32_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, NH, D, L, V = 64, 8, 64, 64, 32000


def _stats(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "n": len(xs)}


def _timed(fn, inner):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner          # ms per call


def kernel_legs(args):
    import torch
    from zero_amd.func import Engine
    e = Engine("cuda:0")
    H = NH * D
    g = torch.Generator().manual_seed(1234)
    qkv = torch.randn(B * L, 3 * H, generator=g).cuda()
    outs = {k: torch.empty(B * L, H, device="cuda") for k in ("row", "seq", "seq_causal")}
    head = lambda o: (qkv.data_ptr(), qkv.data_ptr() + H * 4, qkv.data_ptr() + 2 * H * 4, o.data_ptr(), B, NH, L, L, D, 3 * H,
                      3 * H, 3 * H, H, L * 3 * H, L * 3 * H, L * 3 * H, L * H, None, 0)
    legs = {
        "zk_f32_attn": lambda: e.lib.call("zk_f32_attn", *head(outs["row"]), 1, D ** -0.5, 1e8, None, None, None, 0, 0, None,
                                          e.stream),
        "zk_f32_attn_seq": lambda: e.lib.call("zk_f32_attn_seq", *head(outs["seq"]), D ** -0.5, 1e8, None, None, 0, 0, 0,
                                              e.stream),
        "zk_f32_attn_seq_causal": lambda: e.lib.call("zk_f32_attn_seq", *head(outs["seq_causal"]), D ** -0.5, 1e8, None, None, 0,
                                                     0, 1, e.stream),
    }
    for fn in legs.values():                   # warm-up: code objects, the launch attribute, caches
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, fn in legs.items():
            ms[k].append(_timed(fn, args.inner))
    res = {k: dict(_stats(v), unit="ms per launch") for k, v in ms.items()}
    res["max_abs_difference_seq_vs_row"] = float((outs["seq"] - outs["row"]).abs().max())
    res["speedup_seq_over_row"] = res["zk_f32_attn"]["median"] / res["zk_f32_attn_seq"]["median"]
    res["causal_over_noncausal_seq"] = res["zk_f32_attn_seq_causal"]["median"] / res["zk_f32_attn_seq"]["median"]
    res["shape"] = {"B": B, "nh": NH, "d": D, "Lq": L, "Lk": L, "inner_launches_per_sample": args.inner}
    return res


def scorer_legs(args):
    import copy
    import numpy as np
    import torch
    from zero_amd.config import transformer_base_params, SyntheticVocab
    from zero_amd.models import model as registry, load_all
    from zero_amd.models._factory import get_core
    from zero_amd.variables import initial_values
    load_all()
    hp = transformer_base_params(model_name="transformer", scope_name="scoref32bench")
    hp.src_vocab, hp.tgt_vocab = SyntheticVocab(V), SyntheticVocab(V)
    hp.random_seed = 1234
    get_core(hp, "transformer", initial_values(hp, "transformer", 1234))
    rng = np.random.default_rng(1234)
    src, tgt = rng.integers(3, V, (B, L)), rng.integers(3, V, (B, L))
    src[:, -1], tgt[:, -1] = 2, 2
    score_fn = registry.get_model("transformer").score_fn
    hps = {}
    for dt in ("float32", "bfloat16"):
        hps[dt] = copy.copy(hp)
        hps[dt].score_dtype = dt
    legs = {dt: (lambda p=p: score_fn({"source": src, "target": tgt}, p)["score"]) for dt, p in hps.items()}
    scores = {}
    for dt, fn in legs.items():
        for _ in range(3):
            scores[dt] = fn()
    torch.cuda.synchronize()
    ms = {dt: [] for dt in legs}
    for _ in range(args.repeats):
        for dt, fn in legs.items():
            ms[dt].append(_timed(fn, 1))
    res = {}
    for dt, v in ms.items():
        res[dt] = dict(_stats(v), unit="ms per score_fn call of %d sentences" % B)
        res[dt]["sentences_per_s"] = B / (res[dt]["median"] * 1e-3)
    a, b = scores["float32"].float().cpu().numpy(), scores["bfloat16"].float().cpu().numpy()
    res["largest_relative_difference_bf16_vs_fp32_scores"] = float(np.abs(b / a - 1).max())
    res["fp32_over_bf16_time"] = res["float32"]["median"] / res["bfloat16"]["median"]
    res["shape"] = {"model": "transformer (base)", "B": B, "Ls": L, "Lt": L, "V": V}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20, help="back-to-back launches per kernel sample")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_f32_bench.json"), help="'' writes no file")
    ap.add_argument("--only", default="", choices=("", "kernel", "scorer"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("score_f32_bench: needs a GPU (a timing taken elsewhere says nothing)", file=sys.stderr)
        return 1
    out = {"method": "device events; warm-up, then --repeats samples per leg with the legs alternating; median, min, max"}
    if args.only in ("", "kernel"):
        out["kernel"] = kernel_legs(args)
    if args.only in ("", "scorer"):
        out["scorer"] = scorer_legs(args)
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
