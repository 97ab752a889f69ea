"""Element-wise parity checking shared by the kernel tests (a plain module, no pytest in it).

Three tools:

``guarded``            an operand or output as a row window of a larger flat buffer.  Every element outside the
                       ``[r*ld+off, r*ld+off+cols)`` windows holds one fixed finite bit pattern, the window holds NaN
                       (an output nobody wrote yet) or the given data (an input, or a residual that aliases C).
                       ``check_guard()`` compares the outside bit for bit, ``check_intact()`` the whole buffer.
``assert_elementwise`` every element finite and within its own bound; nothing is excused.
``gemm_bound``         the float64 reference of a GEMM with its fused epilogue and the DERIVED bound per element.

The row kernels of the training step (LayerNorm, cross entropy, column sums) have their references, derived bounds and CPU
stand-ins at the end of this file (``ln_fwd_bound``, ``ln_bwd_bound``, ``ce_bound``, ``colsum_ref``, ``assert_exact``).

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
    of = [pairs(r) for r in rows]                   # (once per row: the same rows in the same order as recomputing them)
    todo = set().union(*of)
    out = []
    while todo:
        best = max(range(len(rows)), key=lambda i: len(of[i] & todo))
        out.append(rows[best])
        todo -= of[best]
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


# ---------------------------------------------------------------------------------------------- row kernels
# References and DERIVED bounds of the row kernels of zero_amd/csrc/zk_elem.hip (LayerNorm, cross entropy, column sums)
# and, below them, what a correct kernel computes on the CPU (fp32 arithmetic, bf16 at the storage sites, torch's own
# summation order) with the planted defects of tests/test_rowkernel_checker.py.
#
# Units.  One fp32 operation is off by at most 2^-24 of its result (half an ulp); every count below is charged
# PER_TERM = 2^-23, twice that, as gemm_bound does.  A sum of n terms in ANY order (lanes, shuffles, LDS partials,
# partial rows of a workspace) has n - 1 additions, each off by at most 2^-24 of a partial sum that never exceeds the sum
# of the magnitudes: (n - 1) 2^-24 sum|terms|.  bf16 storage is off by at most 2^-8 of the stored value.
C_LN = 8         # per-row operations of the LayerNorm kernels besides the H - 1 additions (counted in ln_*_bound)
C_RED = 4        # per-term operations of a column reduction besides the rows - 1 additions (counted in ln_bwd_bound)
RSQRT_ULP = 2.0  # rsqrtf: 2 ulp, the largest figure the CUDA / HIP math tables give for it
# __expf / __logf: their error cannot be derived from this code base.  MEASURED on an MI355X over CE_CASES x ls of
# tests/test_gpu_rowkernels_elementwise.py against the float64 reference (profiles/rowkernel_parity_constants.json):
# the smallest c_exp the kernels need is C_EXP_MEASURED (the gradient at V = 70001 with label smoothing; ce alone needs
# 0.63); the constant is twice that, rounded up to a power of two.  The margin covers other seeds.
C_EXP_MEASURED = 1.33
C_EXP = 4.0


def _d(x):
    return x.detach().to("cpu").double()


def ratio(got, ref64, bound64):
    """max |err| / bound (an element off its bound-0 reference, or a non-finite one, gives inf)."""
    got, ref64, bound64 = _d(got).reshape(-1), _d(ref64).reshape(-1), _d(bound64).reshape(-1)
    err = (got - ref64).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound64.clamp_min(1e-300))
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    return float(r.max()) if r.numel() else 0.0


def assert_exact(got, ref64, what):
    """A reduction of small integers: every summation order gives the same fp32 bits, the float64 sum."""
    got, ref64 = _d(got), _d(ref64).reshape(got.shape)
    if got.dim() == 1:
        got, ref64 = got[None], ref64[None]
    bad = ~(got == ref64)                                   # (NaN != anything)
    n = int(bad.sum())
    if n:
        r, c = (int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError("%s: %d of %d elements outside their bound (0: an exact sum); first at (row %d, col %d): "
                             "got %r ref %r" % (what, n, got.numel(), r, c, float(got[r, c]), float(ref64[r, c])))


def ln_fwd_bound(x, y, scale, gamma, beta, eps, s_stored=None, e=None):
    """zk_add_ln_fwd (zk_ln_dev.h add_ln_fwd_row): s = x + y * scale (bf16 when saved), out = gamma (s - mean) rstd +
    beta.  x, y: the bf16 operands [rows, H] (y may be None), scale: what zk_dropout_mask gives for the seed and site
    (None = no dropout), s_stored: the sum the KERNEL saved (None = the inference form).  A STAGED reference: returns
    {"s", "mean", "rstd", "out"} -> (ref, bound), float64; "s" only with s_stored.

    s.  fp32: y * scale (one rounding, of |y scale|), + x (one, of at most |x| + |y scale|), then bf16:
        bound_s = 2^-8 |ref| + 2 PER_TERM (|x| + |y scale|);  without y the kernel stores x itself: bound 0.
    The statistics are the kernel's own function of v, the values it normalises: the STORED s when it saves one
    (zk_ln_dev.h:46-51), so the reference takes them from s_stored and e = 0 below; the fp32 sum otherwise, and the
    reference takes the unrounded x + y scale, from which the kernel's v is off by e = 2 PER_TERM (|x| + |y scale|).
    mean = fl(sum v) * fl(1 / H): H - 1 additions, the rounding of 1 / H, the product: H + 1 half-units of mean|v|.
        bound_mean = (H + C_LN) PER_TERM mean|v| + mean(e)
    var = sum (v - mean)^2 / H.  sum (v - m)^2 = H var + H (m - mu)^2, so the error of the mean enters squared:
    dm2 = bound_mean^2; e enters as 2 sqrt(var mean(e^2)) + mean(e^2) (Cauchy-Schwarz).  Relative to the sum of the
    (non-negative) terms: v - mean rounded (counts twice in the square), the square, H - 1 additions, 1 / H and the
    product, + eps: H + 5 half-units.  rstd = rsqrtf(var + eps): half the relative error of var + eps, and RSQRT_ULP ulps:
        rel_rstd = ((H + C_LN) PER_TERM + (dm2 + ...) / (var + eps)) / 2 + RSQRT_ULP PER_TERM;  bound_rstd = rstd rel_rstd
    out = gamma (v - mean) rstd + beta, then bf16.  v - mean is off by bound_mean + e and its own rounding, rstd by
    rel_rstd, two products and the addition of beta (of at most |gamma (v - mean) rstd| + |beta|) follow: on |v - mu|
    that is (H + 6) / 2 + RSQRT_ULP + 4 <= H + 5 units for H >= 8, on mean|v| H + 1 half-units, on |beta| one:
        bound_out = 2^-8 |ref| + (H + C_LN) PER_TERM (|gamma| rstd (|v - mu| + mean|v|) + |beta|)
                    + |gamma| rstd (mean(e) + e + |v - mu| (dm2 + ...) / (2 (var + eps)))
    (the last line is second order with a saved sum).  C_LN = 8 covers each of these counts and is not tuned.
    e (inference form only; [rows, H]): the caller's own bound on |v - (x + y scale)| in place of 2 PER_TERM (|x| + |y scale|),
    for a y that is itself a reference with an error (the product inside zk_gemm_add_ln, tests/chain_ref.py).  None: as
    above, bit for bit."""
    x = _d(x)
    H = x.shape[1]
    zero = torch.zeros_like(x)
    if y is None:
        s_ref, mag, s_bound = x, zero, zero
    else:
        ys = _d(y) * (1.0 if scale is None else _d(scale).reshape(x.shape))
        s_ref, mag = x + ys, x.abs() + ys.abs()
        s_bound = U_OUT[torch.bfloat16] * s_ref.abs() + 2 * PER_TERM * mag
    res = {}
    if s_stored is not None:
        res["s"] = (s_ref, s_bound)
        v, e = _d(s_stored), zero
    else:
        v, e = s_ref, (2 * PER_TERM * mag if e is None else _d(e).reshape(x.shape))
    g, b = _d(gamma)[None], _d(beta)[None]
    mu, ma = v.mean(1), v.abs().mean(1)
    lin = (H + C_LN) * PER_TERM
    mean_bound = lin * ma + e.mean(1)
    dv = v - mu[:, None]
    var = (dv * dv).mean(1)
    rstd = (var + eps) ** -0.5
    e2 = (e * e).mean(1)
    var_abs = mean_bound ** 2 + 2 * (var * e2).sqrt() + e2
    rel = 0.5 * (lin + var_abs / (var + eps)) + RSQRT_ULP * PER_TERM
    res["mean"] = (mu, mean_bound)
    res["rstd"] = (rstd, rstd * rel)
    out = g * dv * rstd[:, None] + b
    gr = g.abs() * rstd[:, None]
    res["out"] = (out, U_OUT[torch.bfloat16] * out.abs() + lin * (gr * (dv.abs() + ma[:, None]) + b.abs())
                  + gr * (e.mean(1)[:, None] + e + dv.abs() * (0.5 * var_abs / (var + eps))[:, None]))
    return res


def ln_bwd_bound(dout, s, mean, rstd, gamma, scale=None, ds_stored=None, dy_stored=None):
    """zk_add_ln_bwd (k_add_ln_bwd<>, k_add_ln_bwd_wide) + zk_add_ln_bwd_reduce.  mean and rstd are INPUTS: the
    reference uses their fp32 values.  xh = (s - mean) rstd, g = dout gamma,
        ds = rstd (g - mean(g) - xh mean(g xh))                                      (bf16)
        dy = ds_stored * scale (bf16; the kernel forms it from the ds it STORED; only with dropout)
        dgamma = sum_r dout xh, dbeta = sum_r dout, dbias_prev = sum_r dy_stored (ds_stored without dropout; zk_elem.hip:251-267)
    ds.  xh: two roundings, g: one, g xh: one, the row sums: H - 1 additions, 1 / H and its product: two, xh mean(g xh):
    one more, two subtractions and the product with rstd: at most H + 10 half-units on the largest of the three terms:
        bound_ds = 2^-8 |ref| + (H + C_LN) PER_TERM rstd (|g| + mean|g| + |xh| mean|g xh|)
    dy: one product, one bf16 rounding: (2^-8 + PER_TERM) |ref|; where scale is 0 the bound is 0.
    Column sums: a term costs at most three roundings (xh: two, the product: one) and there are rows - 1 additions:
        bound = (rows + C_RED) PER_TERM sum_r |term|;  a column of zero terms has bound 0."""
    do, sv, g = _d(dout), _d(s), _d(gamma)[None]
    rows, H = do.shape
    mu, rs = _d(mean).reshape(rows, 1), _d(rstd).reshape(rows, 1)
    xh, gg = (sv - mu) * rs, do * g
    kd = dict(dim=1, keepdim=True)
    ds = rs * (gg - gg.mean(**kd) - xh * (gg * xh).mean(**kd))
    mag = rs.abs() * (gg.abs() + gg.abs().mean(**kd) + xh.abs() * (gg * xh).abs().mean(**kd))
    res = {"ds": (ds, U_OUT[torch.bfloat16] * ds.abs() + (H + C_LN) * PER_TERM * mag)}
    red = lambda t: (t.sum(0), (rows + C_RED) * PER_TERM * t.abs().sum(0))
    res["dgamma"], res["dbeta"] = red(do * xh), red(do)
    if ds_stored is not None:
        src = _d(ds_stored)
        if scale is not None:
            dy = src * _d(scale).reshape(rows, H)
            res["dy"] = (dy, (U_OUT[torch.bfloat16] + PER_TERM) * dy.abs())
            src = _d(dy_stored)
        res["dbias_prev"] = red(src)
    return res


def ce_constants(V, ls):
    """p, q and the normaliser as zk_ce_fused forms them on the host, in fp32 (util.py:88-103)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    if not 0.0 < ls < 1.0:
        return 1.0, 0.0, 0.0
    n = f(float(V - 1))
    p = f(1.0) - f(ls)
    q = f(ls) / n
    norm = -(p * torch.log(p) + n * q * torch.log(q + f(1e-20)))
    return float(p), float(q), float(norm)


def ce_terms(z, ids, w, V, ld, ls):
    """zk_ce_fused in float64: ce = lse - p z_gold - q (sum z - z_gold) - normaliser per row, dlogits = w (softmax -
    soft) in [0, V), exactly 0 in the pad columns [V, ld) and in every row with w == 0.  z: the fp32 logits [T, >= V],
    w: None = forward only.  Returns the references and the pieces of the bounds (see ce_bound)."""
    z = _d(z)[:, :V]
    T = z.shape[0]
    ar, gold = torch.arange(T), ids.detach().to("cpu").long()
    p, q, norm = ce_constants(V, ls)
    lse = torch.logsumexp(z, 1)
    zg, sabs = z[ar, gold], z.abs().sum(1)
    t = {"ce": lse - p * zg - q * (z.sum(1) - zg) - norm,
         "ce_exp": lse.abs() + p * zg.abs() + q * sabs, "ce_sum": (V + C_RED) * PER_TERM * q * sabs}
    if w is not None:
        sm = torch.exp(z - lse[:, None])
        soft = torch.full_like(z, q)
        soft[ar, gold] = p
        wv = _d(w).reshape(T, 1)
        t["dl"] = torch.zeros(T, ld, dtype=torch.float64)
        t["dl_exp"] = torch.zeros(T, ld, dtype=torch.float64)
        t["dl"][:, :V] = wv * (sm - soft)
        t["dl_exp"][:, :V] = wv.abs() * (sm * (1 + (z - lse[:, None]).abs()) + soft)
    return t


def ce_bound(t, c_exp=None):
    """The bounds on ce_terms' references: {"ce", "dl"} -> (ref, bound).
        ce: c_exp PER_TERM (|lse| + p |z_gold| + q sum|z|) + (V + C_RED) PER_TERM q sum|z|
            the second term is derived (sum z: V - 1 additions of at most sum|z|, times q, the subtraction of z_gold);
        dl: 2^-8 |ref| + c_exp PER_TERM w (softmax (1 + |z - lse|) + soft)        (bf16; 0 where w or the column is 0)
            an error d of the exponent z - lse moves softmax by softmax d, and d grows with |z - lse|.
    c_exp stands for __expf, __logf and the fp32 sum of the exponentials: MEASURED (C_EXP above), not derived."""
    c = C_EXP if c_exp is None else c_exp
    res = {"ce": (t["ce"], c * PER_TERM * t["ce_exp"] + t["ce_sum"])}
    if "dl" in t:
        res["dl"] = (t["dl"], U_OUT[torch.bfloat16] * t["dl"].abs() + c * PER_TERM * t["dl_exp"])
    return res


def ce_c_exp_needed(t, ce, dl=None):
    """The smallest c_exp with which ce (and dl) are inside ce_bound: for the measurement."""
    need = lambda got, ref, fixed, shape: float(((( _d(got).reshape(ref.shape) - ref).abs() - fixed) /
                                                 (PER_TERM * shape).clamp_min(1e-300)).clamp_min(0).max())
    out = {"ce": need(ce, t["ce"], t["ce_sum"], t["ce_exp"])}
    if dl is not None:
        out["dl"] = need(dl, t["dl"], U_OUT[torch.bfloat16] * t["dl"].abs(), t["dl_exp"])
    return out


def colsum_ref(a, skip_L=0, scale=None, prev=None):
    """out[c] = sum_r a[r, c] scale[r, c] over the rows with r % skip_L != 0 (skip_L = 0: every row) (+ prev: accumulate).
    A term costs one rounding (the dropout scale), the sum rows - 1 additions, the accumulation one:
        bound = (rows + C_RED) PER_TERM (sum_r |a scale| + |prev|)"""
    t = _d(a)
    rows = t.shape[0]
    if scale is not None:
        t = t * _d(scale).reshape(t.shape)
    if skip_L > 0:
        t = t.clone()
        t[::skip_L] = 0
    ref, mag = t.sum(0), t.abs().sum(0)
    if prev is not None:
        ref, mag = ref + _d(prev), mag + _d(prev).abs()
    return ref, (rows + C_RED) * PER_TERM * mag


def check_all(got, bounds, what, exact=()):
    """Every output of ``got`` (name -> tensor or None) against ``bounds`` (name -> (ref, bound)), in the order of
    ``bounds`` (the staged order); the names in ``exact`` bit for bit.  Returns name -> worst |err| / bound."""
    worst = {}
    for key, (ref, bound) in bounds.items():
        if got.get(key) is None:
            continue
        if key in exact:
            assert_exact(got[key], ref, "%s [%s]" % (what, key))
        else:
            assert_elementwise(got[key], ref, bound, "%s [%s]" % (what, key))
        worst[key] = ratio(got[key], ref, bound)
    return worst


# ---- what a correct kernel computes (fp32, bf16 at the storage sites), and the planted defects
def _f(x):
    return x.detach().to("cpu").float()


def ln_fwd_standin(x, y, scale, gamma, beta, eps, save, defect=None, at=(0, 0)):
    """defect (at = (row, first column of an 8-column chunk)): "unbiased" (variance H / (H - 1), every row),
    "short_stats" (statistics over the first H - 8 columns, every row), "eps_outside" (1 / (sqrt(var) + eps), row at[0]),
    "neighbour" (row at[0] normalised with the statistics of the row below), "stale" (the chunk left at NaN),
    "drop_ignored" (the chunk's dropout scale taken as 1)."""
    r0, c0 = at
    a = _f(x)
    H = a.shape[1]
    if y is not None:
        sc = torch.ones_like(a) if scale is None else _f(scale).reshape(a.shape).clone()
        if defect == "drop_ignored":
            sc[r0, c0:c0 + 8] = 1.0
        a = a + _f(y) * sc
    s = a.to(torch.bfloat16) if save else None
    v = s.float() if save else a
    n = H - 8 if defect == "short_stats" else H
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    mean = v[:, :n].sum(1) * inv
    dv = v - mean[:, None]
    var = (dv[:, :n] * dv[:, :n]).sum(1) * inv
    if defect == "unbiased":
        var = var * (H / (H - 1.0))
    rstd = torch.rsqrt(var + eps)
    if defect == "eps_outside":
        rstd[r0] = 1.0 / (var[r0].sqrt() + eps)
    m_use, r_use = mean.clone(), rstd.clone()
    if defect == "neighbour":
        m_use[r0], r_use[r0] = mean[r0 + 1], rstd[r0 + 1]
    out = (_f(gamma)[None] * (v - m_use[:, None]) * r_use[:, None] + _f(beta)[None]).to(torch.bfloat16)
    if defect == "stale":
        out[r0, c0:c0 + 8] = float("nan")
    return {"s": s, "mean": mean if save else None, "rstd": rstd if save else None, "out": out}


def ln_bwd_standin(dout, s, mean, rstd, gamma, scale=None, defect=None, at=0):
    """defect: "drop_term" (xh mean(g xh) left out in row ``at``), "rows16_31" / "last_row" (those rows missing from the
    three column sums), "dbp_noscale" (dbias_prev summed from ds: the dropout scale left out)."""
    do, sv, g = _f(dout), _f(s), _f(gamma)[None]
    rows, H = do.shape
    mu, rs = _f(mean).reshape(rows, 1), _f(rstd).reshape(rows, 1)
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(H), dtype=torch.float32)
    xh, gg = (sv - mu) * rs, do * g
    mg, mgx = gg.sum(1, keepdim=True) * inv, (gg * xh).sum(1, keepdim=True) * inv
    t = xh * mgx
    if defect == "drop_term":
        t[at] = 0
    ds = (rs * (gg - mg - t)).to(torch.bfloat16)
    dy = (ds.float() * _f(scale).reshape(rows, H)).to(torch.bfloat16) if scale is not None else None
    keep = torch.ones(rows, 1)
    if defect == "rows16_31":
        keep[16:32] = 0
    if defect == "last_row":
        keep[-1] = 0
    src = ds.float() if (dy is None or defect == "dbp_noscale") else dy.float()
    return {"ds": ds, "dy": dy, "dgamma": (do * xh * keep).sum(0), "dbeta": (do * keep).sum(0),
            "dbias_prev": (src * keep).sum(0)}


def ce_standin(z, ids, w, V, ld, ls, defect=None, at=0):
    """defect: "no_q" (the smoothing mass left out off the gold column), "gold_shift" (gold + 1), "no_norm" (the
    normaliser left out of ce), "lse_tail" (the last V % 4 columns left out of the log-sum-exp), "pad" (dlogits[at, V]
    non-zero), "w0" (the rows with w == 0 get the gradient of w = 1)."""
    zf = _f(z)[:, :V]
    T = zf.shape[0]
    ar, gold = torch.arange(T), ids.detach().to("cpu").long()
    p, q, norm = ce_constants(V, ls)
    zl = zf[:, :V & ~3] if defect == "lse_tail" else zf
    if zl.shape[1] == 0:
        lse = torch.full((T,), float("-inf"))
    else:
        m = zl.max(1).values
        lse = m + torch.log(torch.exp(zl - m[:, None]).sum(1))
    if defect == "gold_shift":
        gold = (gold + 1) % V
    zg = zf[ar, gold]
    ce = lse - p * zg - q * (zf.sum(1) - zg) - (0.0 if defect == "no_norm" else norm)
    if w is None:
        return {"ce": ce, "dl": None}
    soft = torch.full_like(zf, 0.0 if defect == "no_q" else q)
    soft[ar, gold] = p
    wv = _f(w).reshape(T).clone()
    if defect == "w0":
        wv[wv == 0] = 1.0
    dl = torch.zeros(T, ld)
    dl[:, :V] = wv[:, None] * (torch.exp(zf - lse[:, None]) - soft)
    if defect == "pad":
        dl[at, V] = 2.0 ** -10
    return {"ce": ce, "dl": dl.to(torch.bfloat16)}


def colsum_standin(a, skip_L=0, scale=None, prev=None, defect=None):
    """defect: "skip_included" (the rows r % skip_L == 0 summed too), "last_chunk" (the last chunk of 32 rows missing),
    "acc_ignored" (prev not added)."""
    t = _f(a)
    rows = t.shape[0]
    if scale is not None:
        t = t * _f(scale).reshape(t.shape)
    keep = torch.ones(rows, 1)
    if skip_L > 0 and defect != "skip_included":
        keep[::skip_L] = 0
    if defect == "last_chunk":
        keep[(rows - 1) // 32 * 32:] = 0
    out = (t * keep).sum(0)
    if prev is not None and defect != "acc_ignored":
        out = out + _f(prev)
    return out
