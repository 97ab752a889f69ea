"""What the word-alignment option costs (alignment_file; zero_amd/csrc/zk_align.hip, zero_amd/models/_align.py).

  kernel   zk_align_probs (bf16) and zk_f32_align_probs alone at B = 32, nh = 8, d = 64, Lq = Lk = 64, each with and without
           the probs output, beside the plain torch composition (bmm, softmax, mean over the heads) on the same operands
  pass     the alignment pass (align_fn) on one 64 x 64 batch of 32 sentences of the base model against score_fn on the same
           batch, in both dtypes

Device events, the legs alternating, median of five samples (--repeats) of --inner back-to-back calls each.  Writes one
JSON line, also to profiles/align_bench.json.

usage: python scripts/align_bench.py [--repeats 5] [--inner 20] [--out profiles/align_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import _benchlib as BL  # noqa: E402

B, NH, D, L = 32, 8, 64, 64


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


def _alternate(legs, repeats, inner, warm=3):
    import torch
    for fn in legs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            ms[k].append(_timed(fn, inner))
    return {k: _stats(v) for k, v in ms.items()}


def kernel_legs(args):
    import torch
    from zero_amd.func import Engine, Mat
    e = Engine("cuda:0")
    H = NH * D
    g = torch.Generator().manual_seed(1234)
    q32, k32 = torch.randn(B * L, H, generator=g).cuda(), torch.randn(B * L, H, generator=g).cuda()
    kmask = torch.ones(B, L, device="cuda")
    probs = torch.empty(B, L, L, device="cuda")
    best = torch.empty(B, L, dtype=torch.int32, device="cuda")
    legs, keep = {}, {}
    for name, dt in (("zk_align_probs", torch.bfloat16), ("zk_f32_align_probs", torch.float32)):
        q, k = q32.to(dt), k32.to(dt)
        qm, km = Mat(q, B * L, H), Mat(k, B * L, H)
        legs[name] = lambda qm=qm, km=km: e.align_probs(qm, km, B, NH, L, L, D, kmask=kmask, probs=probs, best=best)
        legs[name + "_best_only"] = lambda qm=qm, km=km: e.align_probs(qm, km, B, NH, L, L, D, kmask=kmask, best=best)

        def torch_leg(q=q, k=k):
            qh = q.view(B, L, NH, D).permute(0, 2, 1, 3)
            kh = k.view(B, L, NH, D).permute(0, 2, 3, 1)
            s = torch.matmul(qh, kh).float() * D ** -0.5 + ((1.0 - kmask) * -1e8)[:, None, None, :]
            P = torch.softmax(s, -1).mean(1)
            keep["P"], keep["best"] = P, P.argmax(-1)
        legs["torch_" + ("bf16" if dt == torch.bfloat16 else "fp32")] = torch_leg
    res = {k: dict(v, unit="ms per call") for k, v in _alternate(legs, args.repeats, args.inner).items()}
    res["zk_align_probs_over_torch_bf16"] = res["zk_align_probs"]["median"] / res["torch_bf16"]["median"]
    res["zk_f32_align_probs_over_torch_fp32"] = res["zk_f32_align_probs"]["median"] / res["torch_fp32"]["median"]
    res["shape"] = {"B": B, "nh": NH, "d": D, "Lq": L, "Lk": L, "inner_calls_per_sample": args.inner}
    return res


def pass_legs(args):
    import copy
    import numpy as np
    from zero_amd import align as zalign
    from zero_amd.models import model as registry, load_all
    from zero_amd.models._factory import get_core
    from zero_amd.variables import initial_values
    load_all()
    hp = BL.decode_hp("transformer", "alignbench", "bfloat16")
    get_core(hp, "transformer", initial_values(hp, "transformer", 1234))
    rng = np.random.default_rng(1234)
    src, tgt = rng.integers(3, BL.V, (B, L)), rng.integers(3, BL.V, (B, L))
    src[:, -1], tgt[:, -1] = 2, 2
    feats = {"source": src, "target": tgt}
    score_fn = registry.get_model("transformer").score_fn
    legs = {}
    for dt in ("bfloat16", "float32"):
        p = copy.copy(hp)
        p.score_dtype = dt
        legs["align_" + dt] = lambda p=p: zalign.align_fn(feats, p, "transformer")
        legs["score_" + dt] = lambda p=p: score_fn(feats, p)
    res = {k: dict(v, unit="ms per call of %d sentences" % B) for k, v in _alternate(legs, args.repeats, 1).items()}
    for dt in ("bfloat16", "float32"):
        res["align_over_score_" + dt] = res["align_" + dt]["median"] / res["score_" + dt]["median"]
    res["shape"] = {"model": "transformer (base)", "B": B, "Ls": L, "Lt": L, "V": BL.V, "alignment_layer": -1}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="back-to-back calls per kernel sample")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"), help="'' writes no file")
    ap.add_argument("--only", default="", choices=("", "kernel", "pass"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("align_bench: needs a GPU (a timing taken elsewhere says nothing)", file=sys.stderr)
        return 1
    out = {"method": "device events; warm-up, then --repeats samples per leg with the legs alternating; median, min, max"}
    if args.only in ("", "kernel"):
        out["kernel"] = kernel_legs(args)
    if args.only in ("", "pass"):
        out["pass"] = pass_legs(args)
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
