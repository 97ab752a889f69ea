"""The cases of the single-tile attention backward (k_attn_bwd_fused64) that tests/golden/make_attn_bwd_golden.py pins and
tests/test_gpu_attn_bwd_image.py recomputes: inputs from a CPU generator with fixed seeds, lse from the fp64 logits on
the CPU (so that nothing of the forward kernels enters the pinned bytes), dq / dk / dv from zk_attn_bwd."""
import hashlib
import json
import os

import torch

from tests.util_gpu import eng, mat, rand_bf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_bwd_parent.json")
D = 64
SEED, SID = 99, 5
# name -> (B, nh, Lq, Lk, key mask: None | "tail" | "key0", causal, dropout)
SHAPES = {
    "full64": (2, 2, 64, 64, None, False, 0.0),
    "ragged_mask": (3, 2, 37, 53, "tail", False, 0.0),
    "one_query_mask": (1, 2, 1, 7, "tail", False, 0.0),
    "causal50": (2, 3, 50, 50, None, True, 0.0),
    "mask_dropout": (2, 8, 64, 64, "tail", False, 0.2),
    "only_key0": (2, 2, 64, 64, "key0", False, 0.0),
}
# 0 = dO read from memory; n = dO computed from (dY [rows, n], W_o [H, n]); 640 = one full 512-column chunk + one slab
OPROJ_N = (0, 128, 512, 640)
CASES = ["%s-%s" % (s, "plain" if n == 0 else "oproj%d" % n) for s in SHAPES for n in OPROJ_N]


def key_mask(kind, B, Lk):
    if kind is None:
        return None
    km = torch.ones(B, Lk)
    if kind == "tail":                       # sentence b keeps its first Lk - (3b + 2) % Lk keys (at least key 0)
        for b in range(B):
            km[b, max(1, Lk - (3 * b + 2) % Lk):] = 0
    else:                                    # the last sentence sees key 0 only
        km[B - 1, 1:] = 0
    return km


def inputs(name):
    """Everything a case feeds the kernel, on the device; the same bytes on every call."""
    shape, var = name.rsplit("-", 1)
    B, nh, Lq, Lk, mk, causal, drop = SHAPES[shape]
    n = 0 if var == "plain" else int(var[5:])
    H = nh * D
    seed = 1000 * (list(SHAPES).index(shape) + 1)
    q, k, v = rand_bf(B * Lq, H, seed=seed + 1), rand_bf(B * Lk, H, seed=seed + 2), rand_bf(B * Lk, H, seed=seed + 3)
    km = key_mask(mk, B, Lk)
    # lse of the masked logits in fp64 on the CPU (func.py:218-256)
    qh = q.cpu().double().view(B, Lq, nh, D).permute(0, 2, 1, 3) * D ** -0.5
    kh = k.cpu().double().view(B, Lk, nh, D).permute(0, 2, 1, 3)
    lg = qh @ kh.transpose(-1, -2)
    if km is not None:
        lg = lg + ((1 - km.double()) * -1e8)[:, None, None, :]
    if causal:
        lg = lg + (-1e8 * (1 - torch.tril(torch.ones(Lq, Lk, dtype=torch.float64))))[None, None]
    lse = torch.logsumexp(lg, -1).float().reshape(-1).cuda()
    c = dict(name=name, B=B, nh=nh, Lq=Lq, Lk=Lk, H=H, causal=causal, drop=drop, q=q, k=k, v=v, lse=lse, n=n,
             kmask=None if km is None else km.cuda())
    if n:
        c["dy"] = rand_bf(B * Lq, n, seed=seed + 9)
        c["Wo"] = rand_bf(H, n, scale=0.05, seed=seed + 10)
    else:
        c["dout"] = rand_bf(B * Lq, H, seed=seed + 9)
    return c


def run(c, dq=None, dk=None, dv=None):
    """zk_attn_bwd on the case (outputs: Mat views; fresh zeroed matrices when not given) -> (dq, dk, dv) tensors"""
    e = eng()
    own = dq is None
    if own:
        dq, dk, dv = (mat(torch.zeros_like(c[x])) for x in ("q", "k", "v"))
    out = torch.zeros_like(c["q"])           # the kernel takes D_i from P and dP, not from O
    dout = c["dout"] if c["n"] == 0 else torch.full_like(c["q"], float("nan"))
    e.set_seed(SEED)
    n0 = e.lib.ncalls
    e.attn_bwd(mat(c["q"]), mat(c["k"]), mat(c["v"]), mat(out), mat(dout), c["lse"], dq, dk, dv, c["B"], c["nh"], c["Lq"],
               c["Lk"], D, kmask=c["kmask"], causal=c["causal"], drop_p=c["drop"], sid=SID, impl=2,
               oproj=(mat(c["dy"]), mat(c["Wo"])) if c["n"] else None)
    torch.cuda.synchronize()
    assert e.lib.ncalls - n0 == 1, "the single-tile kernel must have taken the call"
    return dq.torch(), dk.torch(), dv.torch()


def digest(t):
    raw = t.contiguous().view(torch.int16).cpu().numpy().tobytes()
    return {"sha256": hashlib.sha256(raw).hexdigest(), "head": [float(x) for x in t.reshape(-1)[:8].float().cpu()]}


def record(name):
    dq, dk, dv = run(inputs(name))
    return {"dq": digest(dq), "dk": digest(dk), "dv": digest(dv)}


def load(path=GOLDEN):
    with open(path) as f:
        return json.load(f)
