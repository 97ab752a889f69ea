"""References, DERIVED bounds and CPU stand-ins of the element kernels of zero_amd/csrc/zk_elem.hip that the row-kernel
tests leave out: the embedding (forward, sorted and atomic backward), the average-attention scan and gate, the optimiser
pass.  A plain module (no pytest in it); the primitives (PER_TERM, U_OUT, C_EXP, C_RED, check_all, ...) are those of
tests/parity.py and none is redefined here.

Units, as in tests/parity.py: one fp32 operation is off by at most 2^-24 of its result (a half-unit); every count below
is charged PER_TERM = 2^-23, twice that, so a count of k PER_TERM covers 2 k roundings and holds whether or not the
compiler contracts a product and a sum into one FMA (contraction only removes roundings).  A bf16 store adds U_OUT =
2^-8 of the stored value.  A sum of n terms in any order is off by at most (n - 1) 2^-24 sum|terms|.

Every ``*_bound`` returns name -> (ref, bound) in float64 for parity.check_all; every ``*_standin`` computes what a
correct kernel computes (fp32, bf16 at the storage sites) and takes ``defect=`` (tests/test_elemkernel_checker.py).
"""
import torch

from tests.parity import PER_TERM, U_OUT, C_EXP, C_RED, _d, _f

BF = torch.bfloat16
SCAN_SEG = 4                      # zk_elem.hip: the scan splits L into 4 segments of ceil(L / 4) steps
FLT_MIN = 2.0 ** -126             # the smallest normal fp32 number


def f32(v):
    """The fp32 value the host hands to a kernel for the Python float v."""
    return float(torch.tensor(float(v), dtype=torch.float32))


# ---------------------------------------------------------------------------------------------- embedding
def embed_scale(H):
    return f32(float(H) ** 0.5)


def embed_row_ids(ids, shift, zero_all=False, defect=None):
    """The embedding id of every output row of ids [B, L] (-1: the row has none): the shifted input carries ids[r - 1]
    and has none at t = 0; zero_flag set leaves no row with one."""
    ids = torch.as_tensor(ids).long()
    B, L = ids.shape
    if zero_all:
        return torch.full((B * L,), -1, dtype=torch.long)
    if shift:
        src = ids if defect == "shift_reads_r" else torch.cat([ids[:, :1], ids[:, :-1]], 1)
        rid = src.clone()
        rid[:, 0] = -1
        return rid.reshape(-1)
    return ids.reshape(-1).clone()


def embed_fwd_bound(ids, table, bias, timing, scale, shift=0, pos0=0, zero_all=False, dm=None):
    """zk_embed_fwd / one side of zk_embed_fwd_pair: out = bf16((table[id] scale + bias + timing[pos0 + t]) dm); a row
    without an embedding gets timing dm only (no bias).  dm: what zk_dropout_mask gives for rows x H elements (None: 1).
    Roundings: the product with scale, + bias, + timing, the product with dm: four, each of at most the sum of the
    three magnitudes (times dm):
        bound = 2^-8 |ref| + 4 PER_TERM (|t scale| + |bias| + |timing|) dm;   dm = 0: bound 0, the element is exactly 0."""
    idt = torch.as_tensor(ids)
    B, L = idt.shape
    rid = embed_row_ids(idt, shift, zero_all)
    has = (rid >= 0).double()[:, None]
    t = _d(table)[rid.clamp_min(0)] * scale * has
    b = _d(bias)[None] * has
    tim = _d(timing)[pos0:pos0 + L].repeat(B, 1)
    m = torch.ones_like(t) if dm is None else _d(dm).reshape(t.shape)
    ref = (t + b + tim) * m
    return {"out": (ref, U_OUT[BF] * ref.abs() + 4 * PER_TERM * (t.abs() + b.abs() + tim.abs()) * m)}


def embed_fwd_standin(ids, table, bias, timing, scale, shift=0, pos0=0, zero_all=False, dm=None, defect=None):
    """defect: "bias_scaled" ((t + bias) scale), "shift_reads_r" (the shifted row reads ids[r]), "bias_on_empty" (bias on
    the rows without an embedding), "pos0_ignored", "drop_no_row" (dropout indexed by the column alone)."""
    idt = torch.as_tensor(ids)
    B, L = idt.shape
    rid = embed_row_ids(idt, shift, zero_all, defect)
    has = (rid >= 0).float()[:, None]
    t, b = _f(table)[rid.clamp_min(0)], _f(bias)[None]
    v = ((t + b) * scale if defect == "bias_scaled" else t * scale + b) * has
    if defect == "bias_on_empty":
        v = v + b * (1 - has)
    p = 0 if defect == "pos0_ignored" else pos0
    v = v + _f(timing)[p:p + L].repeat(B, 1)
    if dm is not None:
        m = _f(dm).reshape(v.shape)
        v = v * (m[:1].expand_as(v) if defect == "drop_no_row" else m)
    return {"out": v.to(BF)}


def embed_bwd_bound(ids, dout, V, scale, shift=0, dm=None, prev=None, accumulate=0, prev_bias=None):
    """zk_embed_bwd_sorted (one side of the pair) and zk_embed_bwd: dtable[id] = scale sum_{rows of id} dout dm
    (+ the prior row with accumulate; the atomic form always adds), dbias = prev_bias + sum over the rows that have an
    embedding (the atomic form only).  prev: the table before the call [V, H].  A row of the table whose id is not in the
    batch is never written: its reference is prev and its bound 0.  A term costs one rounding (dm), a run of n rows
    n - 1 additions, then the product with scale and the accumulation:
        bound = (run_length + C_RED) PER_TERM (sum|terms| + |prev|)     per element; a run of zero terms has bound 0."""
    rid = embed_row_ids(ids, shift)
    rows = torch.nonzero(rid >= 0).reshape(-1)
    g = _d(dout) * (1.0 if dm is None else _d(dm).reshape(dout.shape))
    H = g.shape[1]
    terms = g[rows] * scale
    ref = torch.zeros(V, H, dtype=torch.float64).index_add_(0, rid[rows], terms)
    mag = torch.zeros(V, H, dtype=torch.float64).index_add_(0, rid[rows], terms.abs())
    run = torch.bincount(rid[rows], minlength=V).double()[:, None]
    pv = torch.zeros(V, H, dtype=torch.float64) if prev is None else _d(prev)
    if accumulate:
        ref, mag = ref + pv, mag + pv.abs()
    here = run > 0
    res = {"dtable": (torch.where(here, ref, pv), torch.where(here, (run + C_RED) * PER_TERM * mag, torch.zeros_like(mag)))}
    if prev_bias is not None:
        pb = _d(prev_bias)
        res["dbias"] = (pb + g[rows].sum(0), (rows.numel() + C_RED) * PER_TERM * (pb.abs() + g[rows].abs().sum(0)))
    return res


def embed_bwd_standin(ids, dout, V, scale, shift=0, dm=None, prev=None, accumulate=0, prev_bias=None, defect=None):
    """defect: "drop_ignored", "no_scale", "past64" (the rows past the 64th of a run lost), "acc_ignored"."""
    rid = embed_row_ids(ids, shift)
    rows = torch.nonzero(rid >= 0).reshape(-1)
    g = _f(dout)
    if dm is not None and defect != "drop_ignored":
        g = g * _f(dm).reshape(g.shape)
    H = g.shape[1]
    key = rid[rows]
    if defect == "past64":
        order = torch.argsort(key, stable=True)
        ks = key[order]
        first = torch.searchsorted(ks, ks, right=False)
        keep = torch.zeros(rows.numel(), dtype=torch.bool)
        keep[order] = (torch.arange(rows.numel()) - first) < 64
        rows_s, key_s = rows[keep], key[keep]
    else:
        rows_s, key_s = rows, key
    acc = torch.zeros(V, H).index_add_(0, key_s, g[rows_s])
    out = acc * (1.0 if defect == "no_scale" else scale)
    pv = torch.zeros(V, H) if prev is None else _f(prev)
    if accumulate and defect != "acc_ignored":
        out = out + pv
    here = (torch.bincount(key, minlength=V) > 0)[:, None]
    res = {"dtable": torch.where(here, out, pv)}
    if prev_bias is not None:
        res["dbias"] = _f(prev_bias) + g[rows].sum(0)
    return res


# ---------------------------------------------------------------------------------------------- average-attention scan
def scan_masks(L):
    """[4, L]: a full sentence, a padded tail (the first ceil(L / 2) steps live), a hole in the middle (steps
    max(1, L // 4) .. L // 2 masked; it crosses the first segment boundary at L = 130; L = 2: step 0; L = 1: none), an
    all-zero mask."""
    m = torch.ones(4, L)
    m[1, (L + 1) // 2:] = 0
    if L >= 3:
        lo = max(1, L // 4)
        m[2, lo:max(lo, L // 2) + 1] = 0
    elif L == 2:
        m[2, 0] = 0
    m[3] = 0
    return m


def scan_masks_dyadic(L):
    """[4, L]: no live step, one and two leading live steps, one live step in the middle: every count is 0, 1 or 2, so
    without use_mask every den is 1 or 2 and every step counts: the reverse sums of small integers are exact in fp32."""
    m = torch.zeros(4, L)
    m[1, :1] = 1
    m[2, :2] = 1
    m[3, L // 2] = 1
    return m


def _scan_coef(mask, use_mask, dt, defect=None):
    m = mask.detach().to("cpu").to(dt)
    B, L = m.shape
    cnt = m.cumsum(1)
    if defect == "cnt_counts_masked":
        cnt = torch.arange(1, L + 1, dtype=dt)[None].expand(B, L)
    if defect == "cnt_early":
        cnt = cnt - m
    one = torch.ones_like(m)
    u = m if (use_mask and defect != "u1_under_mask") else one
    w = m if use_mask else one
    if defect == "den_unclamped":
        den = cnt
    else:
        den = cnt.clamp_min(1) if use_mask else torch.where(cnt <= 0, one, cnt)
    return u, w, den


def _rev(t):
    return t.flip(1).cumsum(1).flip(1)


def scan_fwd_bound(x, mask, use_mask, att=None, exact=False):
    """k_aan_fwd (the average half of cat) and k_cumavg_add_fwd (att given: out = att + avg).  With cnt_t = sum_{s<=t} m_s:
        avg_t = w_t sum_{s<=t} u_s x_s / den(cnt_t);  use_mask: u = w = m, den = max(cnt, 1); else u = w = 1, den = cnt
        (1 where cnt <= 0).
    The kernel forms a = w / den (one rounding), adds u x step by step (u is 0 or 1: the products are exact; t additions
    in whatever grouping the four segments give) and multiplies: t + 3 half-units of the summed magnitudes:
        bound = 2^-8 |ref| + (steps_t + 4) PER_TERM w_t sum u|x| / den,   steps_t = t + 1;
    w_t = 0 (a masked step under use_mask): bound 0, exactly 0.  att: one more rounding, of |att| + |avg|.
    exact (small integers: every running sum is exact): the quotient and the product remain,
        bound = 2^-8 |ref| + 3 PER_TERM |ref|   (with att: 3 PER_TERM (|att| + |avg|))."""
    B, L = mask.shape
    xv = _d(x).view(B, L, -1)
    u, w, den = _scan_coef(mask, use_mask, torch.float64)
    a = (w / den)[..., None]
    avg = a * (u[..., None] * xv).cumsum(1)
    mag = a * (u[..., None] * xv.abs()).cumsum(1)
    steps = torch.arange(1, L + 1, dtype=torch.float64)[None, :, None]
    ref, b = avg, (steps + 4) * PER_TERM * mag
    if att is not None:
        av = _d(att).view(B, L, -1)
        ref = avg + av
        b = b + PER_TERM * (av.abs() + avg.abs())
    if exact:
        b = 3 * PER_TERM * (ref.abs() if att is None else av.abs() + avg.abs())
    H = xv.shape[2]
    return ref.reshape(B * L, H), (U_OUT[BF] * ref.abs() + b).reshape(B * L, H)


def scan_segment(L):
    """(t0, t1) of the last non-empty segment behind the first (None when L = 1 has none)."""
    ln = (L + SCAN_SEG - 1) // SCAN_SEG
    segs = [(min(L, s * ln), min(L, s * ln + ln)) for s in range(SCAN_SEG)]
    live = [s for s in segs[1:] if s[1] > s[0]]
    return live[-1] if live else None


def scan_fwd_standin(x, mask, use_mask, att=None, defect=None):
    """defect: "carry_dropped" (the last non-empty segment starts from 0 instead of the earlier segments' totals),
    "exclusive" (the current step missing from the average), "cnt_counts_masked", "den_unclamped", "u1_under_mask",
    "last8" (the last 8 columns left at the NaN prefill)."""
    B, L = mask.shape
    xv = _f(x).view(B, L, -1)
    u, w, den = _scan_coef(mask, use_mask, torch.float32, defect)
    ux = u[..., None] * xv
    s = ux.cumsum(1)
    if defect == "exclusive":
        s = s - ux
    if defect == "carry_dropped":
        t0, t1 = scan_segment(L)
        s = s.clone()
        s[:, t0:t1] = s[:, t0:t1] - s[:, t0 - 1:t0]
    out = (w / den)[..., None] * s
    if att is not None:
        out = out + _f(att).view(B, L, -1)
    out = out.reshape(B * L, -1).to(BF)
    if defect == "last8":
        out[:, -8:] = float("nan")
    return out


def scan_bwd_bound(g, gmag, mask, use_mask, extra=(), exact=False):
    """k_cumavg_bwd, and k_aan_bwd with extra = (ds, dxg, dcat[:, :H]):
        dx_s = u_s sum_{t>=s} (w_t / den(cnt_t)) g_t  (+ the extra terms).
    g: the float64 gradient flowing into the average (k_aan_bwd: dyg, or dyg + dcat[:, H:] with flag bit 1 clear), gmag
    its magnitude (|dyg| + |dcat[:, H:]|: the fp32 sum is rounded relative to at most that).  Per term: a = w / den and
    the product (and the rounding of g where it is a sum), then the additions: terms_s + 3 half-units of the magnitudes:
        bound = 2^-8 |ref| + (terms_s + 4) PER_TERM u_s sum (w / den) |g|,   terms_s = L - s;
    extra: three more additions, each of at most the summed magnitudes: + 3 PER_TERM (scan magnitude + sum|extra|).
    exact (small integers, dens that are powers of two): the fp32 value is the float64 one before the bf16 store; the
    bound is that of the exact forward, 2^-8 |ref| + 3 PER_TERM |ref|."""
    B, L = mask.shape
    gv, gm = _d(g).view(B, L, -1), _d(gmag).view(B, L, -1)
    H = gv.shape[2]
    u, w, den = _scan_coef(mask, use_mask, torch.float64)
    a = (w / den)[..., None]
    ref, mag = u[..., None] * _rev(a * gv), u[..., None] * _rev(a * gm)
    terms = (L - torch.arange(L, dtype=torch.float64))[None, :, None]
    b = (terms + 4) * PER_TERM * mag
    if extra:
        ex = [_d(t).view(B, L, H) for t in extra]
        ref = ref + sum(ex)
        b = b + 3 * PER_TERM * (mag + sum(t.abs() for t in ex))
    if exact:
        b = 3 * PER_TERM * ref.abs()
    return ref.reshape(B * L, H), (U_OUT[BF] * ref.abs() + b).reshape(B * L, H)


def scan_bwd_standin(g, mask, use_mask, extra=(), defect=None):
    """defect: "cnt_early" (the count decremented before it is used), "carry_wrong_side" (a segment starts from the
    totals of the segments BEFORE it instead of those behind it)."""
    B, L = mask.shape
    gv = _f(g).view(B, L, -1)
    u, w, den = _scan_coef(mask, use_mask, torch.float32, defect)
    t = (w / den)[..., None] * gv
    r = _rev(t)
    if defect == "carry_wrong_side":
        ln = (L + SCAN_SEG - 1) // SCAN_SEG
        r = torch.zeros_like(t)
        before = torch.zeros_like(t[:, 0])
        for sg in range(SCAN_SEG):
            t0, t1 = min(L, sg * ln), min(L, sg * ln + ln)
            if t1 > t0:
                r[:, t0:t1] = _rev(t[:, t0:t1]) + before[:, None]
                before = before + t[:, t0:t1].sum(1)
    out = u[..., None] * r
    for e in extra:
        out = out + _f(e).view(B, L, -1)
    return out.reshape(B * L, -1).to(BF)


def aan_bwd_g(dyg, dcat, H, flags, dt=torch.float64, defect=None):
    """The gradient that flows into the average under zk_aan_bwd's flag bit 1 (set: dcat[:, H:] is already folded into
    dyg and must not be read) and its magnitude |dyg| (+ |dcat[:, H:]|).  defect: "dc2_added" (added although the bit is
    set), "dc2_dropped" (left out although it is clear)."""
    add = not (flags & 2)
    if defect == "dc2_added":
        add = True
    if defect == "dc2_dropped":
        add = False
    conv = lambda t: t.detach().to("cpu").to(dt)
    g = conv(dyg)
    mag = g.abs()
    if add:
        g, mag = g + conv(dcat[:, H:]), mag + conv(dcat[:, H:]).abs()
    return g, mag


# ---------------------------------------------------------------------------------------------- average-attention gate
# __expf and the division: their error cannot be derived from this code base.  It enters through ONE constant c on a shape
# term, as C_EXP does in ce_bound.  MEASURED on an MI355X over GATE_CASES of tests/test_gpu_elemkernels_elementwise.py
# against the float64 reference (profiles/elemkernel_parity_constants.json): the smallest c the gate kernels need is
# C_GATE_MEASURED; that is at most C_EXP / 2, so the gate keeps C_EXP (the rule: twice the need, rounded up to a power
# of two, only where the need is larger than C_EXP / 2).
C_GATE_MEASURED = 0.0325          # (dz at 33 x 64; the bf16 store hides most of the exponential's error)
C_GATE = C_EXP


def _sig(z):
    return torch.sigmoid(z)


def gate_terms(z, cat, dg=None):
    """k_aan_gate_fwd / k_aan_gate_bwd in float64.  z = [z_i | z_f], cat = [x | y] ([rows, 2 H]):
        o = x s_i + y s_f;   dz_i = g x s_i (1 - s_i), dz_f = g y s_f (1 - s_f), dx = g s_i, dy = g s_f   (s = sigmoid(z)).
    Returns name -> (ref, shape, floor).  The kernels form s = 1 / (1 + __expf(-z)): an error d of the exponent moves s by
    s (1 - s) d <= s d, and d grows with |z|: the shape term of o is |x| s_i (1 + |z_i|) + |y| s_f (1 + |z_f|).
    Backward: |d[s (1 - s)]| = |1 - 2 s| |ds| <= |ds|, so dz has the shape |g x| s (1 + |z|), and dx has |g| s (1 + |z|).
    The floor.  For z < -87.3 the true s = e^z is below 2^-126, the smallest normal fp32 number, and 1 + e^-z is above
    the largest: EVERY fp32 evaluation of 1 / (1 + e^-z) gives 0 there (the CPU stand-in does too), and for z > 87.3 the
    same holds for e^-z under flush-to-zero.  So s is off by up to 2^-126 absolutely, whatever the relative constant:
        floor = 2^-126 x the magnitudes s multiplies (|x| + |y|; |g x|; |g|), plus one denormal step 2^-149.
    (A floor of one denormal step alone cannot hold at z = -90: the reference there is 8.2e-40 |x| and the only
    fp32 result is 0.)"""
    zd, cd = _d(z), _d(cat)
    H = zd.shape[1] // 2
    zi, zf, x, y = zd[:, :H], zd[:, H:], cd[:, :H], cd[:, H:]
    si, sf = _sig(zi), _sig(zf)
    step = 2.0 ** -149
    t = {"out": (x * si + y * sf, x.abs() * si * (1 + zi.abs()) + y.abs() * sf * (1 + zf.abs()),
                 FLT_MIN * (x.abs() + y.abs()) + step)}
    if dg is not None:
        g = _d(dg)
        cat2 = lambda a, b: torch.cat([a, b], 1)
        # (1 - s) as sigmoid(-z): no cancellation in the reference at large z
        t["dz"] = (cat2(g * x * si * _sig(-zi), g * y * sf * _sig(-zf)),
                   cat2((g * x).abs() * si * (1 + zi.abs()), (g * y).abs() * sf * (1 + zf.abs())),
                   cat2(FLT_MIN * (g * x).abs(), FLT_MIN * (g * y).abs()) + step)
        t["dxg"] = (g * si, g.abs() * si * (1 + zi.abs()), FLT_MIN * g.abs() + step)
        t["dyg"] = (g * sf, g.abs() * sf * (1 + zf.abs()), FLT_MIN * g.abs() + step)
    return t


def gate_bound(t, c=None):
    """bound = 2^-8 |ref| + c PER_TERM shape + floor for every output of gate_terms; c = C_GATE (measured, not derived)."""
    c = C_GATE if c is None else c
    return {k: (ref, U_OUT[BF] * ref.abs() + c * PER_TERM * shape + floor) for k, (ref, shape, floor) in t.items()}


def gate_c_needed(t, got):
    """The smallest c with which every output is inside gate_bound: for the measurement."""
    out = {}
    for k, (ref, shape, floor) in t.items():
        err = (_d(got[k]).reshape(ref.shape) - ref).abs() - U_OUT[BF] * ref.abs() - floor
        out[k] = float((err / (PER_TERM * shape).clamp_min(1e-300)).clamp_min(0).max())
    return out


def gate_standin(z, cat, dg=None, defect=None):
    """defect: "swapped" (z_f gates x and z_i gates y), "no_1ms" (the factor 1 - s missing from dz)."""
    zf_, cf = _f(z), _f(cat)
    H = zf_.shape[1] // 2
    zi, zf, x, y = zf_[:, :H], zf_[:, H:], cf[:, :H], cf[:, H:]
    if defect == "swapped":
        zi, zf = zf, zi
    si, sf = 1.0 / (1.0 + torch.exp(-zi)), 1.0 / (1.0 + torch.exp(-zf))
    res = {"out": (x * si + y * sf).to(BF)}
    if dg is not None:
        g = _f(dg)
        ki, kf = (1.0, 1.0) if defect == "no_1ms" else (1.0 - si, 1.0 - sf)
        res["dz"] = torch.cat([g * x * si * ki, g * y * sf * kf], 1).to(BF)
        res["dxg"], res["dyg"] = (g * si).to(BF), (g * sf).to(BF)
    return res


# ---------------------------------------------------------------------------------------------- optimiser
N_TREE = 16      # additions on the path of one term through two block sums (6 shuffle levels + the wave partials, twice)


def adam_grid(n, key10, per_thread=4):
    """zk_adam_step's block count: flat_grid(n, 4) = ceil((n / 4) / 256) in [1, 2048], or tuning key 10 when that is
    smaller (0 or above 2048: flat_grid's)."""
    g = max(1, min(2048, (n // per_thread + 255) // 256))
    return min(g, key10) if 0 < key10 <= 2048 else g


def adam_terms_per_thread(n, grid, contig):
    """The most elements one thread of k_adam squares and adds (the vector part and one tail element)."""
    n4 = n // 4
    if contig:
        rounds = ((n4 + grid - 1) // grid + 255) // 256
    else:
        rounds = (n4 + grid * 256 - 1) // (grid * 256)
    return 4 * rounds + 1


def norm_bound(x, scale, terms_per_thread, nblocks):
    """scale ||x||_2 as the kernels form it: per thread a chain of squares (a term: the square, and the product with
    grad_scale where there is one: its relative error counts twice), a block sum, the partials of ``nblocks`` blocks
    summed by one block of 256 threads and its block sum, the root (which halves the relative error of the sum), the
    product with scale.  At most T + ceil(nblocks / 256) + N_TREE + 4 half-units on the sum of non-negative terms, so
        bound = (T + ceil(nblocks / 256) + N_TREE + C_RED) PER_TERM ref      (more than twice what was counted).
    The parts: k_adam's partials + k_norm_final2, k_adam<false>'s partials + k_norm_final, k_sumsq_partial + k_norm_final."""
    ref = scale * _d(x).norm()
    return ref.reshape(1), ((terms_per_thread + (nblocks + 255) // 256 + N_TREE + C_RED) * PER_TERM * ref.abs()).reshape(1)


def adam_factor(hyper, norm_free, gnorm=None):
    """f: grad_scale, times clip / max(gnorm, clip) on the norm_free = 0 path with clipping on (float64 of the fp32 words)."""
    f = float(hyper[4])
    if not norm_free and float(hyper[5]) > 0:
        f = f * float(hyper[5]) / max(float(gnorm), float(hyper[5]))
    return f


def adam_bound(p, g, m, v, hyper, norm_free=1, gnorm=None, m_stored=None, v_stored=None):
    """k_adam: gj = g f, m' = b1 m + (1 - b1) gj, v' = b2 v + (1 - b2) gj^2, p' = p - lr m' / (sqrt(v') + eps).
    hyper: the fp32 words the kernel reads; gnorm: the hyper[6] the kernel read (norm_free = 0).
    f costs up to two roundings (the quotient and the product of the clip), gj one: 3 half-units relative.
    m': 1 - b1, its product with gj, b1 m, the sum: at most 6 half-units on its second term, 2 on the first:
        bound_m = 4 PER_TERM (|b1 m| + |(1 - b1) gj|)
    v': gj^2 carries 6, 1 - b2 and two products 3 more, the sum 1: 10 half-units:
        bound_v = 6 PER_TERM (|b2 v| + (1 - b2) gj^2)
    p' is STAGED: its reference takes the m' and v' the kernel stored.  The update: sqrtf (2 half-units allowed), + eps,
    lr m', the quotient (up to 2.5 ulp: 5 half-units), then the subtraction, rounded relative to |p'| <= |p| + |update|:
        bound_p = 6 PER_TERM |update| + PER_TERM |p|
    Where g = m = v = 0 every bound but PER_TERM |p| is 0; that p keeps its BITS is asserted separately."""
    pd, gd, md, vd = _d(p), _d(g), _d(m), _d(v)
    lr, b1, b2, eps = (float(hyper[i]) for i in range(4))
    f = adam_factor(hyper, norm_free, gnorm)
    gj = gd * f
    m1, m2 = b1 * md, (1 - b1) * gj
    v1, v2 = b2 * vd, (1 - b2) * gj * gj
    res = {"m": (m1 + m2, 4 * PER_TERM * (m1.abs() + m2.abs())), "v": (v1 + v2, 6 * PER_TERM * (v1.abs() + v2.abs()))}
    ms = res["m"][0] if m_stored is None else _d(m_stored)
    vs = res["v"][0] if v_stored is None else _d(v_stored)
    upd = lr * ms / (vs.sqrt() + eps)
    res["p"] = (pd - upd, 6 * PER_TERM * upd.abs() + PER_TERM * pd.abs())
    return res


def adam_standin(p, g, m, v, hyper, norm_free=1, gnorm=None, defect=None):
    """fp32.  Returns p, m, v, shadow (bf16), gnorm (norm_free = 1: of the scaled gradient), pnorm.  defect: "eps_inside"
    (sqrt(v + eps)), "v_unscaled" (v from g instead of g f), "no_1mb1" (m' = b1 m + gj), "shadow_old" (the shadow of the
    parameter before the update), "tail_skipped" (the n % 4 tail left as it was), "pnorm_after", "clip_on_normfree"."""
    pf, gf, mf, vf = _f(p), _f(g), _f(m), _f(v)
    t = lambda i: torch.tensor(float(hyper[i]), dtype=torch.float32)
    lr, b1, b2, eps = t(0), t(1), t(2), t(3)
    f = adam_factor(hyper, 0 if (defect == "clip_on_normfree" and norm_free) else norm_free,
                    _d(gf * float(hyper[4])).norm() if norm_free else gnorm)
    gj = gf * f32(f)
    m2 = b1 * mf + (gj if defect == "no_1mb1" else (1 - b1) * gj)
    gv = gf if defect == "v_unscaled" else gj
    v2 = b2 * vf + (1 - b2) * gv * gv
    p2 = pf - lr * m2 / (torch.sqrt(v2 + eps) if defect == "eps_inside" else torch.sqrt(v2) + eps)
    n = pf.numel()
    if defect == "tail_skipped" and n % 4:
        k = n - n % 4
        m2[k:], v2[k:], p2[k:] = mf[k:], vf[k:], pf[k:]
    res = {"p": p2, "m": m2, "v": v2, "shadow": (pf if defect == "shadow_old" else p2).to(BF),
           "pnorm": (p2 if defect == "pnorm_after" else pf).double().norm().float().reshape(1)}
    if norm_free:
        res["gnorm"] = (gf * f32(float(hyper[4]))).double().norm().float().reshape(1)
    return res


def ema_bound(ema, p, d):
    """zk_ema: e' = e - (1 - d) (e - p): 1 - d, the difference, the product, the subtraction: four roundings, each of at
    most |e| + |p|:  bound = 4 PER_TERM (|e| + |p|)."""
    e, w = _d(ema), _d(p)
    return e - (1 - d) * (e - w), 4 * PER_TERM * (e.abs() + w.abs())


def axpby_bound(y, x, a, b):
    """zk_axpby_f32: y' = b y + a x: two products and a sum: three roundings:  bound = 3 PER_TERM (|b y| + |a x|)."""
    yd, xd = _d(y), _d(x)
    return b * yd + a * xd, 3 * PER_TERM * ((b * yd).abs() + (a * xd).abs())
