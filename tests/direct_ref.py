"""References of the small kernels that only whole-model runs reached (a plain module, no pytest in it), in the manner of
tests/rnnsearch_ref.py: per family a numpy statement with ``defect=`` (ONE planted defect, each something a kernel could
do), the check a kernel is held to -- a derived element-wise bound, or bit-equality -- and a torch-fp32 stand-in of what a
correct kernel computes.  tests/test_direct_checker.py (CPU) shows on the cases below that every stand-in passes and every
defect fails; tests/test_gpu_direct_kernels.py runs the same cases through the entry points.

    embed        zk_rnn_embed / zk_f32_rnn_embed      out[r] = table[clip(ids[r], 0, V - 1)] + bias; all zeros when pad >= 0
                                                      and EVERY id of the launch equals pad.  One fp32 add (and one RNE
                                                      rounding to bf16): bit-equal to the stand-in.
    bias_tanh    zk_rnn_bias_tanh / zk_f32_...        y = tanh(x + bias); input row r -> output rows r rep .. r rep + rep - 1.
                                                      Bound with the one MEASURED constant C_TANH (below).
    aan_decode   zk_aan_decode                        cache += x; cat = [x | cache * inv], inv = 1 / (time_dev + 1) or the argument.
    add_rows     zk_f32_add_rows                      out = a + b, three row strides: bit-equal.
    transpose    zk_transpose_bf16                    dst = src^T: bit-equal.
    rows         zk_rows_pack / zk_rows_scatter_add   the row-sparse payload [ids int32 x R][rows R x H]: bit-equal.
    seed         zk_seed_advance                      seed = (seed + inc) mod 2^64.

The layout defects (add_rows, transpose) are stated on FLAT buffers with guard elements, as the kernels see them: a wrong
stride then shows as a wrong element or as a write outside the window, which is what parity.guarded catches on the device.
"""
import numpy as np
import torch

BF, F32 = torch.bfloat16, torch.float32
ST = {"bf16": BF, "fp32": F32}
U24, U23, U8 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -8
LEAD = 64                        # guard elements of the flat statements (tests/parity.py LEAD)


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def st(a, form):
    """float64 values rounded to the storage type of `form` (so that they are exact where a kernel reads them)."""
    return _t(a).float().to(ST[form]).double().numpy()


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def bf(a):
    return st(a, "bf16")


def not_bf16(a):
    """The fp32 values of `a` with mantissa bit 11 set (one of the sixteen that bf16 drops): none is bf16-representable."""
    a = np.ascontiguousarray(np.where(np.asarray(a) == 0, 0.5, a), np.float32)
    a = (a.view(np.int32) | 0x800).view(np.float32).astype(np.float64)
    assert (bf(a) != a).all()
    return a


def bits(a, form="fp32"):
    """The storage bits of float64-held values: int32 (fp32) / int16 (bf16) arrays, for bit-for-bit comparisons."""
    t = _t(a).float()
    return (t.view(torch.int32) if form == "fp32" else t.to(BF).view(torch.int16)).numpy()


def same_bits(got, ref, form="fp32"):
    return np.array_equal(bits(got, form), bits(ref, form))


def exceeds(got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    return bool((~np.isfinite(err)).any() or (err > bound).any())


# ---------------------------------------------------------------------------------------------- embed
EMBED_DEFECTS = ("no_bias", "bias_bf16", "zero_if_any_pad", "zero_per_row", "pad_scan_256", "pad_rule_without_pad")
EMBED_V = 11
PAD = 2


def embed_ref(ids, table, bias, pad, defect=None):
    """ids [rows] int; table [V, E] (values of the storage type); bias [E] (fp32 values) -> out [rows, E] float64.

    defect:  no_bias;  bias_bf16 (the bias rounded to bf16 before the add);  zero_if_any_pad (zeros when ANY id is pad);
    zero_per_row (the rows whose id is pad are zeroed, each on its own);  pad_scan_256 (only the first 256 ids are looked
    at);  pad_rule_without_pad (the rule applied without the pad >= 0 condition)."""
    ids, table, bias = np.asarray(ids), np.asarray(table, np.float64), np.asarray(bias, np.float64)
    V = table.shape[0]
    b = {"no_bias": np.zeros_like(bias), "bias_bf16": bf(bias)}.get(defect, bias)
    out = table[np.clip(ids, 0, V - 1)] + b[None, :]
    if defect == "zero_per_row":
        out[(ids == pad) & (pad >= 0)] = 0.0
        return out
    seen = ids[:256] if defect == "pad_scan_256" else ids
    hit = (seen == pad).any() if defect == "zero_if_any_pad" else (seen == pad).all()
    if hit and (pad >= 0 or defect == "pad_rule_without_pad"):
        out[:] = 0.0
    return out


def embed_bound(ref, form):
    """Kept only to show the stand-in right against float64 (the kernels are held to bit-equality with the stand-in): one
    fp32 add, 2^-24 |t + b|, and one rounding to bf16, 2^-8 |t + b|."""
    return (U24 + (U8 if form == "bf16" else 0.0)) * np.abs(ref)


def embed_standin(ids, table, bias, pad, form):
    ids_t = torch.as_tensor(np.asarray(ids)).long()
    out = (_t(table).float()[ids_t.clamp(0, table.shape[0] - 1)] + _t(bias).float()[None, :]).to(ST[form])
    if pad >= 0 and bool((ids_t == pad).all()):
        out = torch.zeros_like(out)
    return out.double().numpy()


def embed_cases(form):
    """name -> dict(ids, table, bias, pad).  V = 11; the widths 5 / 8, 72, 300 (the second trip of the column loop), 520;
    rows = 300: the second trip of the pad scan.  The ids hold 0, V - 1, repeats, -3 and V + 5 (clamped to rows 0, V - 1)."""
    V = EMBED_V
    g = np.random.default_rng(11)
    cases = {}

    def add(name, ids, E, pad):
        cases[name] = dict(ids=np.asarray(ids, np.int64), table=st(g.normal(0, 1, (V, E)), form),
                           bias=not_bf16(g.normal(0, 0.3, E)), pad=pad)

    add("r1", [V - 1], 5 if form == "fp32" else 8, -1)
    add("r5_pad0", [0, V - 1, 3, -3, V + 5], 72, 0)              # (id 0 IS the pad here, but not every id: nothing zeroed)
    ids = g.integers(0, V, 300)
    ids[:6] = (0, V - 1, 4, 4, -3, V + 5)
    add("r300", ids, 300, -1)
    add("r3", [V + 5, 3, 3], 520, -1)
    allpad = np.full(300, PAD)
    add("all_pad", allpad, 300, PAD)
    for name, at in (("all_pad_but_last", 299), ("all_pad_but_first", 0)):
        ids = allpad.copy()
        ids[at] = 7
        add(name, ids, 300, PAD)
    add("no_pad_all_equal", np.full(300, -1), 300, -1)          # every id equals "pad" = -1: pad < 0 means no rule at all
    return cases


# ---------------------------------------------------------------------------------------------- bias_tanh
TANH_DEFECTS = ("no_bias", "rep_interleaved", "f32_out_rounded", "tanh_naive", "copy_from_x")
TANH_SHAPES = [(1, 5, 1), (5, 72, 3), (33, 300, 4)]
TANH_SPECIALS = (2.0 ** -12, 60.0, -3e38, -0.0, 9.0, -2.0 ** -12, -60.0, 3e38, 0.0, -9.0)
# tanhf: its error cannot be derived from this code base.  MEASURED: the smallest constant with which the torch-fp32
# stand-in is inside tanh_bound against the float64 statement over tanh_cases (tanh_need; tests/test_direct_checker.py
# re-measures it on every run); C_TANH is twice that, rounded up to a power of two, with the project's C_EXP = 4 as the floor
# (the factor 2 is for another tanhf, the device's).  profiles/elemkernel_parity_constants.json "direct_kernels" records
# both and, beside them, what the MI355X's tanhf needs (it does not set the constant).
C_TANH_MEASURED = 0.5201
C_TANH = 4.0


def c_tanh_rule(measured):
    return max(4.0, 2.0 ** np.ceil(np.log2(max(2.0 * measured, 1e-30))))


def _naive_tanh(z):
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp((np.float32(2.0) * z.astype(np.float32)).astype(np.float32)).astype(np.float32)
        return ((e - np.float32(1.0)) / (e + np.float32(1.0))).astype(np.float64)


def bias_tanh_ref(x, bias, rep, form="fp32", defect=None):
    """x [rows, cols] (fp32 values); bias [cols] (fp32 values) or None -> dict of float64 arrays [rows rep, cols]: out (the
    fp32 output), copy (the storage-type output; the statement is the same y), z, y.

    defect:  no_bias;  rep_interleaved (input row r goes to the rows k rows + r);  f32_out_rounded (the fp32 output carries
    bf16 precision);  tanh_naive ((e^2z - 1) / (e^2z + 1) in fp32: no relative accuracy near 0, inf / inf beyond z = 44);
    copy_from_x (the copy is taken before the tanh)."""
    x = np.asarray(x, np.float64)
    rows = x.shape[0]
    z = x + (0.0 if (bias is None or defect == "no_bias") else np.asarray(bias, np.float64)[None, :])
    y = _naive_tanh(z) if defect == "tanh_naive" else np.tanh(z)
    src = np.tile(np.arange(rows), rep) if defect == "rep_interleaved" else np.repeat(np.arange(rows), rep)
    out, cp = y[src], (z if defect == "copy_from_x" else y)[src]
    if defect == "f32_out_rounded":
        out = bf(out)
    return {"out": out, "copy": cp, "z": z[src], "y": y[src]}


def tanh_bound(ref, form, copy=False, c_tanh=None):
    """|dy| <= 2^-24 |z| (1 - y^2)   the rounding of the sum z = x + bias, through the slope of tanh
             + C_TANH 2^-23 |y|      tanhf itself: RELATIVE, so tanh(2^-12) is held to a few ulps of 2^-12
             + 2^-126                the smallest normal (flushed subnormals)
             + 2^-8 |y|              the copy in bf16 (the fp32 form's copy is the fp32 value)."""
    c = C_TANH if c_tanh is None else c_tanh
    y = ref["y"]
    return U24 * np.abs(ref["z"]) * (1 - y * y) + c * U23 * np.abs(y) + 2.0 ** -126 + (U8 * np.abs(y) if (copy and form == "bf16") else 0.0)


def tanh_need(got, ref, where=False):
    """The smallest c_tanh with which the fp32 output `got` is inside tanh_bound (inf where y = 0 is missed); where: (need, the
    z that needs it)."""
    err = np.abs(np.asarray(got, np.float64) - ref["y"])
    over = np.maximum(err - U24 * np.abs(ref["z"]) * (1 - ref["y"] ** 2) - 2.0 ** -126, 0.0)
    ay = np.abs(ref["y"])
    need = np.where(over > 0, over / np.where(ay > 0, U23 * ay, 1e-300), 0.0)
    need = np.where(np.isfinite(np.asarray(got, np.float64)), need, np.inf)
    return (float(need.max()), float(ref["z"].reshape(-1)[need.argmax()])) if where else float(need.max())


def bias_tanh_standin(x, bias, rep, form):
    z = _t(x).float() if bias is None else _t(x).float() + _t(bias).float()[None, :]
    y = torch.tanh(z).repeat_interleave(rep, 0)
    return {"out": y.double().numpy(), "copy": y.to(ST[form]).double().numpy()}


def tanh_cases():
    """(rows, cols, rep, with_bias) -> dict(x, bias, rep).  Normal draws and, from element 0 on, the arguments of
    TANH_SPECIALS IN z: x = fl(special - bias), so that z = x + bias is the special value (to an ulp) with and without a
    bias.  (1, 5, 1) has room for the first five."""
    cases = {}
    for rows, cols, rep in TANH_SHAPES:
        for wb in (True, False):
            g = np.random.default_rng(rows * 1000 + cols + wb)
            bias = not_bf16(g.normal(0, 0.3, cols)) if wb else None
            x = g.normal(0, 1.5, (rows, cols))
            n = min(len(TANH_SPECIALS), x.size)
            x.reshape(-1)[:n] = np.asarray(TANH_SPECIALS[:n]) - (np.tile(bias, rows)[:n] if wb else 0.0)
            cases[(rows, cols, rep, wb)] = dict(x=f32(x), bias=bias, rep=rep)
    return cases


# ---------------------------------------------------------------------------------------------- aan_decode
AAN_DEFECTS = ("cache_holds_mean", "inv_from_argument", "count_off_by_one", "halves_swapped", "cache_bf16")
AAN_SHAPES = [(3, 8), (5, 72), (33, 128)]                 # (33, 128): 528 groups of 8 = three blocks, the last one partial
# name -> (time_dev or None, the inv_count ARGUMENT).  time6: the argument is wrong on purpose, the device value must win.
AAN_TIMES = {"time0": (0, 1.0), "time6_wrong_arg": (6, 0.5), "arg_only": (None, float(np.float32(1.0 / 7.0)))}


def aan_decode_ref(x, cache, inv_count, time_dev=None, defect=None):
    """x [rows, H] (bf16 values); cache [rows, H] (fp32 values); inv_count: the argument (an fp32 value); time_dev: int or
    None -> dict cache (the new running sum), cat [rows, 2 H], s, avg.

    defect:  cache_holds_mean (the cache keeps s inv);  inv_from_argument (time_dev ignored);  count_off_by_one
    (1 / (time_dev + 2));  halves_swapped (cat = [avg | x]);  cache_bf16 (the running sum stored with bf16 precision)."""
    x, cache = np.asarray(x, np.float64), np.asarray(cache, np.float64)
    inv = float(inv_count)
    if time_dev is not None and defect != "inv_from_argument":
        inv = 1.0 / (time_dev + (2 if defect == "count_off_by_one" else 1))
    s = cache + x
    avg = s * inv
    new = {"cache_holds_mean": avg, "cache_bf16": bf(s)}.get(defect, s)
    cat = np.concatenate([avg, x] if defect == "halves_swapped" else [x, avg], 1)
    return {"cache": new, "cat": cat, "s": s, "avg": avg}


def aan_bound(ref):
    """cache: one fp32 add, 2^-24 |s|.  cat: the left half is x bit for bit (bound 0); the right half is the rounded s
    times the rounded inv (1 / (t + 1) formed in fp32), the product rounded, then bf16: (2^-8 + 4 2^-23) |s inv|."""
    H = ref["s"].shape[1]
    cat = np.concatenate([np.zeros_like(ref["s"]), (U8 + 4 * U23) * np.abs(ref["avg"])], 1)
    assert cat.shape[1] == 2 * H
    return {"cache": U24 * np.abs(ref["s"]), "cat": cat}


def aan_decode_standin(x, cache, inv_count, time_dev=None):
    xs, c = _t(x).float(), _t(cache).float()
    inv = torch.tensor(inv_count, dtype=F32) if time_dev is None else torch.tensor(1.0, dtype=F32) / torch.tensor(float(time_dev + 1), dtype=F32)
    s = c + xs
    return {"cache": s.double().numpy(), "cat": torch.cat([xs, (s * inv).to(BF).float()], 1).double().numpy()}


def aan_inputs(rows, H, call=0):
    g = np.random.default_rng(rows * 100 + H + 7 * call)
    return dict(x=bf(g.normal(0, 1, (rows, H))), cache=not_bf16(g.normal(0, 2, (rows, H))))


# ---------------------------------------------------------------------------------------------- flat buffers
GUARD_VALUE = 6.75e6             # what the guard elements of a flat statement hold (finite, not small)


def flat(rows, ld, fill=np.nan):
    """A flat float64 buffer of LEAD + rows ld + LEAD elements: guards outside, `fill` in the rows."""
    b = np.full(LEAD + rows * ld + LEAD, GUARD_VALUE)
    b[LEAD:LEAD + rows * ld] = fill
    return b


def window(buf, rows, cols, ld, off=0):
    return np.lib.stride_tricks.as_strided(buf[LEAD + off:], (rows, cols), (ld * buf.itemsize, buf.itemsize))


def _put(buf, idx, val):
    ok = (idx >= 0) & (idx < buf.size)            # (a defective index past the buffer: the statement drops the access)
    buf[idx[ok]] = val[ok]


def _get(buf, idx):
    return np.where((idx >= 0) & (idx < buf.size), buf[np.clip(idx, 0, buf.size - 1)], np.nan)


# ---------------------------------------------------------------------------------------------- add_rows
ADD_ROWS_DEFECTS = ("b_stride_from_out", "cols_from_ld")
ADD_ROWS_SHAPES = [(1, 1), (5, 20), (33, 300)]


def add_rows_flat(abuf, a0, lda, bbuf, b0, ldb, obuf, o0, ldo, rows, cols, defect=None):
    """out[r, c] = a[r, c] + b[r, c] on flat buffers (element offsets a0 / b0 / o0 of the first element, row strides); obuf
    may BE abuf (in place).  Returns the new obuf (a copy).  fp32 arithmetic.

    defect:  b_stride_from_out (b read with ldo);  cols_from_ld (ldo columns per row instead of cols)."""
    n = ldo if defect == "cols_from_ld" else cols
    r, c = (v.reshape(-1) for v in np.meshgrid(np.arange(rows), np.arange(n), indexing="ij"))
    va = _get(abuf, a0 + r * lda + c).astype(np.float32)
    vb = _get(bbuf, b0 + r * (ldo if defect == "b_stride_from_out" else ldb) + c).astype(np.float32)
    out = obuf.copy()
    _put(out, o0 + r * ldo + c, (va + vb).astype(np.float64))
    return out


def add_rows_case(rows, cols, in_place):
    """The operands as flat guarded buffers: b is the right half of a [rows, 2 cols] buffer (ldb = 2 cols + 4); in place:
    out IS a (lda = ldo, the product's own call), else three distinct strides.  -> dict of the add_rows_flat arguments."""
    g = np.random.default_rng(rows + cols)
    lda, ldb = cols + 3, 2 * cols + 4
    ldo = lda if in_place else cols + 6
    a, b = flat(rows, lda, 1.0), flat(rows, ldb, 2.0)
    window(a, rows, cols, lda, 1)[:] = f32(g.normal(0, 1, (rows, cols)))
    window(b, rows, 2 * cols, ldb, 2)[:] = f32(g.normal(0, 1, (rows, 2 * cols)))
    o = a if in_place else flat(rows, ldo)
    return dict(abuf=a, a0=LEAD + 1, lda=lda, bbuf=b, b0=LEAD + 2 + cols, ldb=ldb, obuf=o, o0=LEAD + (1 if in_place else 2),
                ldo=ldo, rows=rows, cols=cols)


def add_rows_standin(x):
    r, c = x["rows"], x["cols"]
    a = torch.as_tensor(window(x["abuf"], r, c, x["lda"], x["a0"] - LEAD).copy()).float()
    b = torch.as_tensor(window(x["bbuf"], r, c, x["ldb"], x["b0"] - LEAD).copy()).float()
    return (a + b).double().numpy()


# ---------------------------------------------------------------------------------------------- transpose
TRANSPOSE_DEFECTS = ("copy", "tiles_not_swapped", "ld_swapped")
# (rows, cols, ld_src, ld_dst): one element; a partial tile with both strides padded; one exact tile; 2 x 3 and 3 x 2 tiles with
# partial edges; four row tiles of a narrow matrix
TRANSPOSE_SHAPES = [(1, 1, 1, 1), (5, 72, 80, 8), (64, 64, 64, 64), (65, 130, 136, 72), (130, 65, 72, 136), (200, 8, 8, 208)]


def transpose_flat(src, ld_src, dst, ld_dst, rows, cols, defect=None):
    """dst[c, r] = src[r, c] on flat buffers whose first elements sit at LEAD.  Returns the new dst (a copy).

    defect:  copy (element k of the window lands at element k: nothing is transposed);  tiles_not_swapped (each 64 x 64 tile
    is transposed where it stands: tile (i, j) lands at tile (i, j) of dst);  ld_swapped (each stride taken from the other
    operand)."""
    r, c = (v.reshape(-1) for v in np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij"))
    ls, ld = (ld_dst, ld_src) if defect == "ld_swapped" else (ld_src, ld_dst)
    val = _get(src, LEAD + r * ls + c)
    if defect == "copy":
        k = r * cols + c
        dr, dc = k // rows, k % rows
    elif defect == "tiles_not_swapped":
        dr, dc = r // 64 * 64 + c % 64, c // 64 * 64 + r % 64
    else:
        dr, dc = c, r
    inside = (dr < cols) & (dc < rows) if defect == "tiles_not_swapped" else np.ones_like(dr, bool)
    out = dst.copy()
    _put(out, (LEAD + dr * ld + dc)[inside], val[inside])
    return out


def transpose_case(rows, cols, ld_src, ld_dst):
    """Values distinct per element and exact in bf16: element k holds the bf16 with the bits 0x3000 + k (positive normals)."""
    assert rows * cols < 0x4000
    v = (torch.arange(rows * cols) + 0x3000).to(torch.int16).view(BF).double().numpy().reshape(rows, cols)
    assert len(np.unique(v)) == v.size and np.isfinite(v).all()
    src = flat(rows, ld_src, 3.0)
    window(src, rows, cols, ld_src)[:] = v
    return dict(src=src, ld_src=ld_src, dst=flat(cols, ld_dst), ld_dst=ld_dst, rows=rows, cols=cols)


# ---------------------------------------------------------------------------------------------- rows pack / scatter
ROWS_DEFECTS = ("stale_uid_packed", "ids_not_minus_one", "no_clear", "clear_every_slot", "no_poison", "scatter_overwrites",
                "scatter_ignores_vocab_rows", "bf16_halves_swapped", "second_column_trip_dropped")
PACK_ONLY = ("stale_uid_packed", "ids_not_minus_one", "no_clear", "clear_every_slot", "no_poison")
# name -> (R, H, V, n): n < R;  n == R and a second trip of the column loop (H > 256);  n = 0 (every slot -1 / zero, the table
# untouched);  n > R (overflow: slot 0 poisoned);  R > 8192 (the grid-stride trip: 2048 blocks x 4 waves take 8192 slots)
ROWS_CASES = {"n3_of_4": (4, 4, 9, 3), "full_H260": (8, 260, 20, 8), "empty_H512": (12, 512, 40, 0),
              "overflow": (8, 8, 30, 11), "grid_stride": (8196, 4, 9000, 8196)}
TABLE_EXTRA = 8                  # the table allocation is this many rows larger than vocab_rows
NAN_WORD = 0x7fc00000


def payload_words(R, H, bf16):
    return R + R * H // (2 if bf16 else 1)


def _rows_to_words(rows, bf16):
    t = torch.as_tensor(np.ascontiguousarray(rows, np.float32))
    return (t.to(BF) if bf16 else t).reshape(-1).view(torch.int32).numpy().copy()


def payload_rows(words, R, H, bf16):
    """The row block of a payload (int32 words) as float32 [R, H]."""
    t = torch.as_tensor(np.ascontiguousarray(words[R:], np.int32))
    return (t.view(BF).float() if bf16 else t.view(F32)).reshape(R, H).numpy().copy()


def rows_pack_ref(table, uid, n, R, H, bf16, clear_rows, defect=None):
    """table float32 [rows, H] (NOT modified); uid int [>= min(n, R)]; n = *n_uniq_dev -> (payload int32 words, new table).

    Payload = [ids int32 x R][rows R x H]: slot u < min(n, R) carries uid[u] and table[uid[u]] (one RNE rounding in the bf16
    form); every other slot id -1 and a zero row; clear_rows != 0 zeroes the packed table rows.  n > R (overflow): slot 0
    carries at least one NaN (here, as the kernel does, in every fourth column), every other slot is unchanged.

    defect:  stale_uid_packed (the slots >= n are filled from uid);  ids_not_minus_one (their ids are 0);  no_clear;
    clear_every_slot (the rows uid[u] of ALL R slots are cleared);  no_poison;  second_column_trip_dropped (columns >= 256
    are neither written -- they keep the NaN prefill -- nor cleared)."""
    table = np.array(table, np.float32)
    uid = np.asarray(uid)
    nu = R if defect == "stale_uid_packed" else min(n, R)
    ids = np.full(R, 0 if defect == "ids_not_minus_one" else -1, np.int32)
    rows = np.zeros((R, H), np.float32)
    for u in range(nu):                            # (slot by slot, as the statement reads; the stand-in is vectorised)
        ids[u] = uid[u]
        rows[u] = table[uid[u]]
    if n > R and defect != "no_poison":
        rows[0, 0::4] = np.nan
    hi = 256 if defect == "second_column_trip_dropped" else H
    rows[:, hi:] = np.nan
    if clear_rows and defect != "no_clear":
        for u in range(R if defect == "clear_every_slot" else nu):
            table[uid[u], :hi] = 0.0
    return np.concatenate([ids, _rows_to_words(rows, bf16)]), table


def rows_scatter_ref(table, words, R, H, bf16, vocab_rows, defect=None):
    """table[ids[u]] += rows[u] for every slot with 0 <= ids[u] < vocab_rows (one fp32 add per element) -> new table.

    defect:  scatter_overwrites;  scatter_ignores_vocab_rows (every id >= 0 is taken);  bf16_halves_swapped (the two bf16 of
    a 32-bit word unpacked in the wrong order);  second_column_trip_dropped."""
    table = np.array(table, np.float32)
    ids, rows = np.asarray(words[:R]), payload_rows(words, R, H, bf16)
    if defect == "bf16_halves_swapped" and bf16:
        rows = rows.reshape(R, H // 2, 2)[:, :, ::-1].reshape(R, H)
    hi = 256 if defect == "second_column_trip_dropped" else H
    for u in range(R):
        if ids[u] < 0 or (ids[u] >= vocab_rows and defect != "scatter_ignores_vocab_rows"):
            continue
        if defect == "scatter_overwrites":
            table[ids[u], :hi] = rows[u, :hi]
        else:
            table[ids[u], :hi] += rows[u, :hi]
    return table


def rows_pack_standin(table, uid, n, R, H, bf16, clear_rows):
    """torch, vectorised.  -> (payload words, new table)"""
    t = torch.as_tensor(np.array(table, np.float32))
    nu = min(n, R)
    u = torch.as_tensor(np.asarray(uid[:nu], np.int64))
    ids = torch.full((R,), -1, dtype=torch.int32)
    ids[:nu] = u.to(torch.int32)
    rows = torch.zeros(R, H)
    rows[:nu] = t[u]
    if n > R:
        rows[0, 0::4] = float("nan")
    if clear_rows:
        t[u] = 0.0
    body = (rows.to(BF) if bf16 else rows).reshape(-1).view(torch.int32)
    return torch.cat([ids, body]).numpy(), t.numpy()


def rows_scatter_standin(table, words, R, H, bf16, vocab_rows):
    t = torch.as_tensor(np.array(table, np.float32))
    w = torch.as_tensor(np.ascontiguousarray(words, np.int32))
    ids = w[:R].long()
    rows = w[R:].view(BF if bf16 else F32).view(R, H).float()
    ok = (ids >= 0) & (ids < vocab_rows)
    t.index_put_((ids[ok],), rows[ok], accumulate=True)      # (ids are unique inside a payload: one add per element)
    return t.numpy()


def rows_case(name):
    """-> dict table float32 [V + TABLE_EXTRA, H] (no value bf16-representable, row r distinctive: about r + 1), uid int32 [max(R, n)]
    (uid[n:R]: STALE but valid ids of other rows), n, R, H, V."""
    R, H, V, n = ROWS_CASES[name]
    g = np.random.default_rng(R + H)
    table = not_bf16((np.arange(V + TABLE_EXTRA)[:, None] + 1.0) * (1.0 + 0.25 * g.random((V + TABLE_EXTRA, H)))).astype(np.float32)
    uid = g.permutation(V)[:max(R, n)].astype(np.int32)
    return dict(table=table, uid=uid, n=n, R=R, H=H, V=V)


def scatter_case(name, bf16):
    """A payload of its own for the scatter: unique valid ids, and three slots with -1, vocab_rows and vocab_rows + 3 whose
    rows are NOT zero (a kernel that takes them writes); the target table prefilled non-zero.  -> dict table, words, R, H, V."""
    R, H, V, _ = ROWS_CASES[name]
    g = np.random.default_rng(R * 3 + H)
    table = not_bf16(g.normal(0, 3, (V + TABLE_EXTRA, H))).astype(np.float32)
    ids = g.permutation(V)[:R].astype(np.int32)
    ids[[R // 2, R - 1, 0]] = (-1, V, V + 3)
    rows = not_bf16(g.normal(0, 1, (R, H))).astype(np.float32)
    return dict(table=table, words=np.concatenate([ids, _rows_to_words(rows, bf16)]), R=R, H=H, V=V)


def two_rank_inputs():
    R, H, V = 8, 260, 20
    g = np.random.default_rng(5)
    uid = [np.asarray(u, np.int32) for u in ((3, 17, 0, 9, 12, 5), (9, 4, 17, 19, 1, 0, 8, 13))]
    t = []
    for k in (0, 1):
        tab = np.zeros((V + TABLE_EXTRA, H), np.float32)
        tab[uid[k]] = not_bf16(g.normal(0, 1, (len(uid[k]), H))).astype(np.float32)
        t.append(tab)
    return t, uid, R, H, V


def two_rank_expect(t, bf16):
    rnd = (lambda a: torch.as_tensor(a).to(BF).float().numpy()) if bf16 else (lambda a: a)
    return (np.zeros_like(t[0]) + rnd(t[0])) + rnd(t[1])


# ---------------------------------------------------------------------------------------------- seed
def seed_advance_ref(seed, inc):
    return (int(seed) + int(inc)) % (1 << 64)
