"""Element-wise parity checking shared by the kernel tests (a plain module, no pytest in it).

Three tools:

``guarded``            an operand or output as a row window of a larger flat buffer.  Every element outside the
                       ``[r*ld+off, r*ld+off+cols)`` windows holds one fixed finite bit pattern, the window holds NaN
                       (an output nobody wrote yet) or the given data (an input, or a residual that aliases C).
                       ``check_guard()`` compares the outside bit for bit, ``check_intact()`` the whole buffer.
``assert_elementwise`` every element finite and within its own bound; nothing is excused.
``gemm_bound``         the float64 reference of a GEMM with its fused epilogue and the DERIVED bound per element.

The GEMM bound.  With bf16 operands every product a*b is exact in fp32, so a kernel that accumulates K products in
fp32 in any order (MFMA blocks, split-K slab sums) is off by at most (K-1) roundings of partial sums, each at most
2^-24 of the running magnitude, which never exceeds mag = |alpha| (|A| |B|) + |bias| + |res|; the epilogue (alpha,
bias, residual, aux_scale, the dropout scale) adds a handful more.  2^-23 per term is TWICE that unit:

    bound = u_out |ref| + (K + 8) 2^-23 mag          u_out = 2^-8 (bf16 out: half an ulp of 8 bits), 2^-23 (fp32 out)

The activation, aux_scale and the dropout mask are applied to ref and to mag alike, so an element the mask or the ReLU
gate zeroes has bound 0 and must be exactly 0.

The attention row check (``attn_row_ratio``) compares d-vectors: ||got_row - ref_row|| <= c_x max(||ref_row||,
rms row norm of the tensor); ``attn_math`` is both its float64 reference and -- in float32 with bf16 rounding at the
storage sites oracle/ref_torch.py Cfg.store_bf16 names (probabilities, attention output, the incoming gradients of
scores / q / k / v) -- the CPU emulation the constants c_x are measured on (tests/test_gpu_attention_elementwise.py).
"""
import itertools

import torch

from zero_amd.func import Mat

GUARD_I16 = 0x4ACE            # bf16 6.75e6; two of them side by side are the fp32 0x4ACE4ACE = 6.76e6: finite, not small
LEAD = 64                     # guard elements in front of the first row and behind the last one


class Guarded(object):
    """See ``guarded``.  ``mat`` is the Mat view the kernels get, ``t`` the flat buffer."""

    def __init__(self, rows, cols, ld, off, dtype, prefill, device):
        assert dtype in (torch.bfloat16, torch.float32)
        assert 0 <= off and off + cols <= ld, (cols, ld, off)
        self.rows, self.cols, self.ld, self.off, self.dtype = int(rows), int(cols), int(ld), int(off), dtype
        n = LEAD + self.rows * self.ld + LEAD
        words = n * (2 if dtype == torch.float32 else 1)
        raw = torch.full((words,), GUARD_I16, dtype=torch.int16)
        self.t = raw.view(dtype)
        idx = torch.arange(n)
        rel = idx - LEAD
        r, c = torch.div(rel, self.ld, rounding_mode="floor"), rel % self.ld
        inside = (rel >= 0) & (r < self.rows) & (c >= self.off) & (c < self.off + self.cols)
        self.outside = ~inside
        win = self.window(self.t)
        if prefill is None:
            win.fill_(float("nan"))
        else:
            win.copy_(prefill.detach().to("cpu").to(dtype).reshape(self.rows, self.cols))
        self._int = torch.int32 if dtype == torch.float32 else torch.int16
        self.before = self.t.view(self._int).clone()
        self.t = self.t.to(device)
        self.mat = Mat(self.t, self.rows, self.cols, self.ld, LEAD + self.off)

    def window(self, flat=None):
        flat = self.t if flat is None else flat
        return torch.as_strided(flat, (self.rows, self.cols), (self.ld, 1), LEAD + self.off)

    def value(self):
        """The window as a contiguous CPU tensor."""
        return self.window().detach().cpu().clone()

    def _where(self, i):
        rel = int(i) - LEAD - self.off
        r = rel // self.ld
        return r, rel - r * self.ld

    def check_guard(self, what="output"):
        now = self.t.detach().cpu().view(self._int)
        bad = torch.nonzero((now != self.before) & self.outside).reshape(-1)
        if bad.numel():
            r, c = self._where(bad[0])
            raise AssertionError("%s: %d element(s) outside the %d x %d window (ld %d) were written; the first at "
                                 "(row %d, col %d) relative to the window, bits %#x" %
                                 (what, bad.numel(), self.rows, self.cols, self.ld, r, c,
                                  int(now[bad[0]]) & (0xffffffff if self._int == torch.int32 else 0xffff)))

    def rebase(self):
        """From here on the present content is what check_guard / check_intact compare with (an output of one call that
        is an input of the next)."""
        self.before = self.t.detach().cpu().view(self._int).clone()

    def check_intact(self, what="input"):
        now = self.t.detach().cpu().view(self._int)
        bad = torch.nonzero(now != self.before).reshape(-1)
        if bad.numel():
            r, c = self._where(bad[0])
            raise AssertionError("%s: %d element(s) of a read-only operand changed; the first at (row %d, col %d) "
                                 "relative to its window" % (what, bad.numel(), r, c))


def guarded(rows, cols, ld=None, off=0, dtype=torch.bfloat16, prefill=None, device="cpu"):
    return Guarded(rows, cols, cols if ld is None else ld, off, dtype, prefill, device)


def assert_elementwise(got, ref64, bound64, what):
    got = got.detach().to("cpu").double()
    ref64 = ref64.detach().to("cpu").double().reshape(got.shape)
    bound64 = bound64.detach().to("cpu").double().reshape(got.shape)
    if got.dim() == 1:
        got, ref64, bound64 = got[None], ref64[None], bound64[None]
    got, ref64, bound64 = (x.reshape(-1, x.shape[-1]) for x in (got, ref64, bound64))
    err = (got - ref64).abs()
    nonfinite = ~torch.isfinite(got)
    bad = nonfinite | (err > bound64)
    n = int(bad.sum())
    if n == 0:
        return
    # worst = a non-finite element if there is one, else the largest excess over the bound
    excess = torch.where(nonfinite, torch.full_like(err, float("inf")), err / bound64.clamp_min(1e-300))
    excess = torch.where(bad, excess, torch.zeros_like(excess))
    flat = int(excess.reshape(-1).argmax())
    r, c = flat // got.shape[1], flat % got.shape[1]
    raise AssertionError(
        "%s: %d of %d elements outside their bound (%d non-finite); worst at (row %d, col %d): got %r ref %r bound %.3e "
        "(|err| / bound = %.3g); row %% 64 = %d, col %% 64 = %d, row %% 256 = %d, col %% 256 = %d" %
        (what, n, got.numel(), int(nonfinite.sum()), r, c, float(got[r, c]), float(ref64[r, c]), float(bound64[r, c]),
         float(excess[r, c]), r % 64, c % 64, r % 256, c % 256))


U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -23}
PER_TERM = 2.0 ** -23


def gemm_bound(a, b, K, out_dtype, alpha=1.0, bias=None, res=None, act=0, aux=None, aux_scale=1.0, mask=None):
    """a: op(A) [M, K], b: op(B) [K, N] (the bf16 values); bias [N]; res / aux [M, N]; mask [M, N] = the dropout scale
    per element (0 or 1 / keep).  Returns (ref, bound) in float64 on the CPU."""
    d = lambda x: x.detach().to("cpu").double()
    a, b = d(a), d(b)
    ref = alpha * (a @ b)
    mag = abs(alpha) * (a.abs() @ b.abs())
    if bias is not None:
        ref = ref + d(bias)
        mag = mag + d(bias).abs()
    if res is not None:
        ref = ref + d(res)
        mag = mag + d(res).abs()
    if act == 1:
        ref = torch.relu(ref)              # (mag >= 0: the ReLU leaves it)
    elif act == 2:
        gate = (d(aux) > 0).double() * aux_scale
        ref = ref * gate
        mag = mag * gate.abs()
    if mask is not None:
        ref = ref * d(mask)
        mag = mag * d(mask).abs()
    return ref, U_OUT[out_dtype] * ref.abs() + (K + 8) * PER_TERM * mag


def cpu_gemm_standin(a, b, out_dtype, alpha=1.0, bias=None, res=None, act=0, aux=None, aux_scale=1.0, mask=None,
                     k_limit=None):
    """What a correct kernel computes, on the CPU: fp32 product, fp32 epilogue, one rounding to the output type.
    k_limit: leave the K terms from there on out (a planted defect)."""
    a, b = a.float(), b.float()
    if k_limit is not None:
        a, b = a[:, :k_limit], b[:k_limit]
    v = alpha * (a @ b)
    if bias is not None:
        v = v + bias.float()
    if res is not None:
        v = v + res.float()
    if act == 1:
        v = torch.relu(v)
    elif act == 2:
        v = torch.where(aux.float() > 0, v * aux_scale, torch.zeros_like(v))
    if mask is not None:
        v = v * mask.float()
    return v.to(out_dtype)


def pairwise(factors, valid=lambda row: True):
    """Greedy pairwise covering: rows (dicts) over ``factors`` (name -> list of levels) such that every valid pair of
    levels of two factors appears in some row.  Deterministic."""
    names = list(factors)
    rows = [dict(zip(names, lv)) for lv in itertools.product(*(factors[n] for n in names))]
    rows = [r for r in rows if valid(r)]
    pairs = lambda r: {(n1, repr(r[n1]), n2, repr(r[n2])) for n1, n2 in itertools.combinations(names, 2)}
    todo = set().union(*(pairs(r) for r in rows))
    out = []
    while todo:
        best = max(rows, key=lambda r: len(pairs(r) & todo))
        out.append(best)
        todo -= pairs(best)
    return out


# ---------------------------------------------------------------------------------------------- attention
def _bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


class _RoundFwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _bf(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return _bf(g)


def attn_math(q, k, v, dout, B, nh, Lq, Lk, d, kmask=None, causal=False, rk=None, rv=None, max_rel=0,
              drop_mask=None, emulate=False):
    """func.py:218-256 and its gradients on [B*L, nh*d] matrices (CPU).  emulate = False: float64, nothing rounded (the
    reference).  emulate = True: float32 with bf16 rounding where the bf16 pipeline stores (Cfg.store_bf16 of
    oracle/ref_torch.py): the probabilities that feed P.V, the attention output, the gradient of the scores and the
    gradients of q / k / v.  Returns a dict out, lse, dq, dk, dv[, drk, drv]."""
    dt = torch.float32 if emulate else torch.float64
    leaf = lambda x: None if x is None else x.detach().to("cpu").to(dt).clone().requires_grad_(True)
    qf, kf, vf, rkf, rvf = leaf(q), leaf(k), leaf(v), leaf(rk), leaf(rv)
    H = nh * d
    qh = qf.view(B, Lq, nh, d).permute(0, 2, 1, 3) * d ** -0.5
    kh = kf.view(B, Lk, nh, d).permute(0, 2, 1, 3)
    vh = vf.view(B, Lk, nh, d).permute(0, 2, 1, 3)
    lg = qh @ kh.transpose(-1, -2)
    if rk is not None:
        idx = (torch.arange(Lq)[:, None] - torch.arange(Lk)[None, :]).clamp(-max_rel, max_rel) + max_rel
        lg = lg + torch.einsum("bhqd,qkd->bhqk", qh, rkf[idx])
    if kmask is not None:
        lg = lg + ((1 - kmask.detach().to("cpu").to(dt)) * -1e8)[:, None, None, :]
    if causal:
        lg = lg + (-1e8 * (1 - torch.tril(torch.ones(Lq, Lk, dtype=dt))))[None, None]
    if emulate:
        lg = _RoundBwd.apply(lg)
    w = torch.softmax(lg, -1)
    lse = torch.logsumexp(lg, -1)
    wd = w if drop_mask is None else w * drop_mask.detach().to("cpu").to(dt).view(B, nh, Lq, Lk)
    if emulate:
        wd = _RoundFwd.apply(wd)
    o = wd @ vh
    if rv is not None:
        o = o + torch.einsum("bhqk,qkd->bhqd", wd, rvf[idx])
    o = o.permute(0, 2, 1, 3).reshape(B * Lq, H)
    if emulate:
        o = _RoundFwd.apply(o)
    o.backward(dout.detach().to("cpu").to(dt))
    rnd = _bf if emulate else (lambda x: x)
    res = {"out": o.detach().double(), "lse": lse.detach().double(), "dq": rnd(qf.grad).double(),
           "dk": rnd(kf.grad).double(), "dv": rnd(vf.grad).double()}
    if rk is not None:
        res["drk"] = rkf.grad.double()
        res["drv"] = rvf.grad.double()
    return res


def attn_rows(x, d):
    """[T, nh*d] -> one row per (sentence, position, head) d-vector; a [n, d] table stays as it is."""
    return x.detach().to("cpu").double().reshape(-1, d)


def attn_row_ratio(got, ref64, d):
    """Per d-vector ||got - ref|| / max(||ref||, rms row norm of the tensor); NaN / inf rows give inf."""
    g, r = attn_rows(got, d), attn_rows(ref64, d)
    rn = r.norm(dim=1)
    scale = torch.maximum(rn, rn.pow(2).mean().sqrt()).clamp_min(1e-300)
    ratio = (g - r).norm(dim=1) / scale
    return torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))


def assert_attn_rows(got, ref64, d, c_x, what, heads=1):
    ratio = attn_row_ratio(got, ref64, d)
    bad = ratio > c_x
    n = int(bad.sum())
    if n:
        i = int(ratio.argmax())
        raise AssertionError("%s: %d of %d d-vectors beyond c = %.3g; worst ratio %.3g at vector %d (matrix row %d, "
                             "head %d); row %% 64 = %d" % (what, n, ratio.numel(), c_x, float(ratio[i]), i, i // heads,
                                                         i % heads, (i // heads) % 64))
    return float(ratio.max())


# (B, nh, Lq, Lk, mask, causal, rpr, drop); d = 64.  mask: None, "ragged" (every sentence but the first loses a few
# trailing keys), "key0" (sentence 1 keeps key 0 only), "tail" (sentence 1's last 64-key tile is masked entirely).
# The first six are ATT_CASES of tests/test_gpu_kernels.py, then dropout (one tile, and several query and key tiles: the
# dropout index of the keys behind the first 64), relative positions, and the added edges:
# one query, key counts around the 64-key tiles, the two masks.
ATTN_CASES = [
    (2, 2, 64, 64, None, False, False, 0.0), (3, 2, 37, 53, "ragged", False, False, 0.0),
    (2, 3, 50, 50, None, True, False, 0.0), (2, 2, 70, 130, "ragged", False, False, 0.0),
    (1, 2, 130, 130, None, True, False, 0.0), (2, 8, 64, 64, "ragged", False, False, 0.0),
    (2, 2, 64, 64, "ragged", False, False, 0.2), (2, 2, 70, 130, "ragged", False, False, 0.2),
    (2, 2, 20, 20, None, True, True, 0.0), (3, 2, 37, 53, "ragged", False, True, 0.0),
    (2, 2, 70, 130, "ragged", False, True, 0.0),
    (2, 2, 1, 7, "ragged", False, False, 0.0),
    (2, 2, 64, 63, None, False, False, 0.0), (2, 2, 33, 65, "ragged", False, False, 0.0),
    (2, 2, 64, 127, None, False, False, 0.0), (1, 2, 70, 129, None, False, False, 0.0),
    (2, 2, 40, 256, "ragged", False, False, 0.0),
    (2, 2, 64, 64, "key0", False, False, 0.0), (2, 2, 64, 128, "tail", False, False, 0.0),
    (2, 2, 70, 256, "tail", False, False, 0.0),
]
ATTN_D = 64
ATTN_MAX_REL = 4


def attn_inputs(case, seed=0):
    """CPU operands of one case: bf16 q / k / v / dout (and the two fp32-valued bf16 tables), the fp32 key mask."""
    B, nh, Lq, Lk, mask, causal, rpr, drop = case
    d, H = ATTN_D, nh * ATTN_D
    g = torch.Generator(device="cpu")
    g.manual_seed(1000 + seed)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(torch.bfloat16)
    x = {"q": rnd(B * Lq, H), "k": rnd(B * Lk, H), "v": rnd(B * Lk, H), "dout": rnd(B * Lq, H), "kmask": None,
         "rk": None, "rv": None}
    if rpr:
        x["rk"] = rnd(2 * ATTN_MAX_REL + 1, d, scale=0.3)
        x["rv"] = rnd(2 * ATTN_MAX_REL + 1, d, scale=0.3)
    if mask is not None:
        km = torch.ones(B, Lk)
        if mask == "ragged":
            for b in range(1, B):
                km[b, Lk - (b * 3) % max(Lk - 1, 1):] = 0
        elif mask == "key0":
            km[1, 1:] = 0
        elif mask == "tail":
            km[1, (Lk - 1) // 64 * 64:] = 0
        km[:, 0] = 1
        x["kmask"] = km
    return x


def plant_attn_defects(ref, d, nh):
    """Defective copies of a correct [T, nh*d] tensor, each wrong in ONE (row, head) d-vector: the vector zeroed, the
    vector of the neighbouring row, one 8-element chunk stale (the NaN prefill).  Each is planted twice: at the vector
    that differs most from its neighbour below (the easiest to see), and (``*_median``) at the one whose difference is
    the median -- the typical one -- among the vectors of at least rms size that differ from their neighbour at all.
    A vector equal to its neighbour (where the mask leaves one key, every query row of a sentence holds the same one)
    cannot show the neighbour defect and is not a candidate; a vector far below the rms row norm is below the scale
    of the row check by construction (parity.attn_row_ratio) and is not one either."""
    rows = attn_rows(ref, d).norm(dim=1).view(-1, nh)
    rms = rows.pow(2).mean().sqrt()
    vecs = attn_rows(ref, d).view(-1, nh, d)
    diff = (vecs[1:] - vecs[:-1]).norm(dim=2).reshape(-1)
    cand = torch.nonzero((diff > 0) & (rows[:-1] >= rms).reshape(-1)).reshape(-1)
    if cand.numel() == 0:                      # two rows, the first the smaller: it is the only place there is
        cand = torch.nonzero(diff > 0).reshape(-1)
    order = cand[diff[cand].argsort()]
    out = {}
    for tag, at in (("", int(order[-1])), ("_median", int(order[(len(order) - 1) // 2]))):
        r, h = divmod(at, nh)
        sl = slice(h * d, (h + 1) * d)
        zeroed = ref.clone(); zeroed[r, sl] = 0
        neigh = ref.clone(); neigh[r, sl] = ref[r + 1, sl]
        stale = ref.clone(); stale[r, h * d + 8:h * d + 16] = float("nan")
        out.update({"zeroed" + tag: zeroed, "neighbour" + tag: neigh, "stale" + tag: stale})
    return out
