// zk_sample.hip -- sampling_topk / sampling_topp: the truncation of a decode step's logits (zero_amd/models/_decode.py
// search_tail; the rule is stated in tests/sampling_ref.py).
//
// For one beam row with logits x, s = softmax(x), c(v) = #{u : x_u > x_v} and M(v) = sum of s_u over x_u > x_v, token v is
// kept iff   c(v) < min_keep   or   ((topk == 0 or c(v) < topk) and (topp == 0 or M(v) < topp)).
// Whether v is kept depends on x_v alone and the predicate only turns false as x_v falls, so the kept set is {v : x_v >= tau}
// for one threshold per row.  The kernel finds tau and overwrites everything below it with `value` (the finite forbid value of
// the search tail), BEFORE the Gumbel noise and the log-softmax of the tail.
//
// One workgroup of ZS_THREADS = 1024 threads per row, one launch, no workspace, no global atomics, no floating-point atomics:
//   1. the row is fetched once into LDS (raw fp32 bits) and its maximum found (integer max of the order-preserving keys);
//   2. a radix descent over the 32-bit key, 4 x 8 bits.  Each level histograms the next byte of the keys that match the prefix
//      found so far: a count (u32) and a mass (u64) per bucket, the mass being the fixed-point llrint(expf(x - max) * 2^S).
//      Integer addition is associative, so the sums do not depend on the order the LDS atomics arrive in: two runs are
//      bit-identical.  S = min(40, 62 - ceil(log2 V)): V terms of at most 2^S never overflow 63 bits.
//      The top byte of real logits takes a handful of values, so one histogram would serialise every wave on two or three
//      addresses.  There are ZS_COPIES = 8 histograms, laid out [bucket][copy] so that the copies of a bucket sit on different
//      banks, and lane l adds to copy l & 7: a wave's worst case is 8 lanes per address instead of 64.
//      After a level 256 threads fold the copies (one bucket each), and wave 0 scans the buckets from the top (4 per lane, a
//      shuffle scan over the lanes): bucket b with c_b keys and m_b mass strictly above it still holds a kept key iff the
//      predicate holds at (c_b, m_b); the lowest such bucket is descended into.  The mass test is the integer
//      m < ceil(topp * total) with the product rounded once, in double; topp >= 1 keeps every token (M(v) < 1 for finite
//      logits), so the mass test is then off rather than left to the quantised masses;
//   3. a last pass stores `value` at the entries whose key is below tau, with plain vector stores (16 bytes where four
//      neighbours all go).  Nothing else is written: not the kept entries, not the columns V .. ld-1.
// Every pass reads the row 16 bytes per lane where the rows start on 16-byte boundaries (ld a multiple of 4 and an aligned
// base; the decode step's logits are), one word per lane otherwise, eight loads in flight per thread either way: the
// workgroup is alone on its CU (the LDS), so nothing else hides a load's latency.  For the same reason the workgroup is as
// large as it can be: a row is one CU's work whatever its thread count, and with 16 waves the LDS atomics and reads of one
// wave run under the arithmetic of the others.  Measured on 128 x 32000 logits, top-p 0.9, back to back: 47 us with 256
// threads, 31 us with 512, 26 us with 1024 (scripts/sampling_bench.py; zk_beam_topk on the same logits: 20 us).
//
// On chip: a row of V <= ZS_LDS_MAX_V = 32768 floats (128 KiB) plus 27 KiB of histograms fits the 160 KiB of a CU, so each
// logit is read from memory once.  A longer row is not staged: every pass re-reads it (from L2, a row is written by the GEMM
// just before) -- the same code with the fetch pointed at global memory.
#include "zk_common.h"

#define ZS_THREADS 1024
#define ZS_COPIES 8
#define ZS_LDS_MAX_V 32768
#define ZS_BATCH 8

typedef unsigned long long zs_u64;

__device__ __forceinline__ unsigned zs_key(unsigned bits) {       // order-preserving: x < y  <=>  key(x) < key(y)
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ unsigned zs_unkey(unsigned key) {
  return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
}

struct alignas(16) ZsShared {      // (the staged row behind it is read and written 16 bytes at a time)
  unsigned cnt[256 * ZS_COPIES];
  zs_u64 mass[256 * ZS_COPIES];
  unsigned rcnt[256];
  zs_u64 rmass[256];
  unsigned wmax[ZS_THREADS / 64];
  unsigned prefix;       // the key bits fixed so far (right-aligned)
  unsigned above_c;      // keys strictly above the prefix's range
  zs_u64 above_m;        // their mass
  zs_u64 thr;            // ceil(topp * total)
};

// One pass over a row of n words at src (the LDS copy, or global memory): f4(words, i) on four consecutive words where W = 4
// (rows whose start and stride are 16-byte aligned), f1(word, i) on single words (W = 1, and the tail of a row).  The loads of
// ZS_BATCH trips are issued before the first word is used: a workgroup is alone on its CU, so what hides a load's latency is
// the loads of the same thread behind it.
template <int W, class F4, class F1>
__device__ __forceinline__ void zs_scan(const unsigned* __restrict__ src, unsigned n, unsigned tid, F4 f4, F1 f1) {
  const unsigned nq = n / W;
  for (unsigned q0 = tid; q0 < nq; q0 += ZS_THREADS * ZS_BATCH) {
    uint4 v[ZS_BATCH];
#pragma unroll
    for (int u = 0; u < ZS_BATCH; ++u) {
      const unsigned q = q0 + ZS_THREADS * u;
      if (q < nq) {
        if (W == 4) v[u] = reinterpret_cast<const uint4*>(src)[q];
        else v[u].x = src[q];
      }
    }
#pragma unroll
    for (int u = 0; u < ZS_BATCH; ++u) {
      const unsigned q = q0 + ZS_THREADS * u;
      if (q < nq) {
        if (W == 4) f4(v[u], q * 4);
        else f1(v[u].x, q);
      }
    }
  }
  for (unsigned i = nq * W + tid; i < n; i += ZS_THREADS) f1(src[i], i);
}

template <bool STAGED, int W>
__global__ void __launch_bounds__(ZS_THREADS) k_sample_truncate(float* __restrict__ logits, int ld, int V, int topk,
                                                                float topp, int min_keep, float value, float scale) {
  extern __shared__ __align__(16) unsigned char zs_smem[];
  ZsShared& sh = *reinterpret_cast<ZsShared*>(zs_smem);
  unsigned* staged = reinterpret_cast<unsigned*>(zs_smem + sizeof(ZsShared));
  const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* row = logits + (size_t)blockIdx.x * ld;
  const unsigned* grow = reinterpret_cast<const unsigned*>(row);
  const unsigned n = (unsigned)V;
  const unsigned* src = STAGED ? staged : grow;      // what the passes after the first read

  // ---- 1. the row, once; its maximum
  unsigned kmax = 0;
  {
    auto f1 = [&](unsigned bits, unsigned i) {
      if (STAGED) staged[i] = bits;
      kmax = max(kmax, zs_key(bits));
    };
    auto f4 = [&](uint4 v, unsigned i) {
      if (STAGED) *reinterpret_cast<uint4*>(staged + i) = v;
      kmax = max(max(kmax, zs_key(v.x)), max(zs_key(v.y), max(zs_key(v.z), zs_key(v.w))));
    };
    zs_scan<W>(grow, n, tid, f4, f1);
  }
  for (int d = 32; d >= 1; d >>= 1) kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, d));
  if (lane == 0) sh.wmax[wave] = kmax;
  if (tid == 0) { sh.prefix = 0; sh.above_c = 0; sh.above_m = 0; sh.thr = 0; }
  __syncthreads();
  for (int w = 0; w < ZS_THREADS / 64; ++w) kmax = max(kmax, sh.wmax[w]);
  const float xmax = __uint_as_float(zs_unkey(kmax));
  const bool use_mass = topp > 0.f && topp < 1.f;
  const unsigned copy = lane & (ZS_COPIES - 1);

  // ---- 2. the descent
  for (int level = 0; level < 4; ++level) {
    const int shift = 24 - 8 * level;
    for (unsigned i = tid; i < 256 * ZS_COPIES; i += ZS_THREADS) { sh.cnt[i] = 0; sh.mass[i] = 0; }
    __syncthreads();
    const unsigned prefix = sh.prefix;
    {
      auto f1 = [&](unsigned bits, unsigned) {
        const unsigned key = zs_key(bits);
        if (level > 0 && (key >> (shift + 8)) != prefix) return;
        const unsigned slot = ((key >> shift) & 255u) * ZS_COPIES + copy;
        atomicAdd(&sh.cnt[slot], 1u);
        if (use_mass) {
          const zs_u64 w = (zs_u64)__builtin_rintf(expf(__uint_as_float(bits) - xmax) * scale);
          atomicAdd(&sh.mass[slot], w);
        }
      };
      auto f4 = [&](uint4 v, unsigned i) { f1(v.x, i); f1(v.y, i); f1(v.z, i); f1(v.w, i); };
      zs_scan<W>(src, n, tid, f4, f1);
    }
    __syncthreads();
    if (tid < 256) {
      unsigned c = 0;
      zs_u64 m = 0;
      for (int k = 0; k < ZS_COPIES; ++k) { c += sh.cnt[tid * ZS_COPIES + k]; m += sh.mass[tid * ZS_COPIES + k]; }
      sh.rcnt[tid] = c;
      sh.rmass[tid] = m;
    }
    __syncthreads();
    if (wave == 0) {
      // lane l owns the buckets 255 - 4l .. 252 - 4l, in the order of the walk (from the top)
      unsigned c[4], cs = 0;
      zs_u64 m[4], ms = 0;
      for (int j = 0; j < 4; ++j) {
        const int b = 255 - (int)(4 * lane + j);
        c[j] = sh.rcnt[b]; m[j] = sh.rmass[b];
        cs += c[j]; ms += m[j];
      }
      unsigned ci = cs;
      zs_u64 mi = ms;
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned tc = (unsigned)__shfl_up((int)ci, d);
        const zs_u64 tm = (zs_u64)__shfl_up((long long)mi, d);
        if ((int)lane >= d) { ci += tc; mi += tm; }
      }
      zs_u64 thr = sh.thr;
      if (level == 0 && use_mass) {
        const zs_u64 total = (zs_u64)__shfl((long long)mi, 63);
        thr = (zs_u64)ceil((double)topp * (double)total);
      }
      unsigned ce = sh.above_c + (ci - cs);      // strictly above this lane's first bucket
      zs_u64 me = sh.above_m + (mi - ms);
      unsigned pc[4];
      zs_u64 pm[4];
      int ntrue = 0;
      for (int j = 0; j < 4; ++j) {
        pc[j] = ce; pm[j] = me;
        const bool p = ce < (unsigned)min_keep || ((topk == 0 || ce < (unsigned)topk) && (!use_mass || me < thr));
        ntrue += __popcll(__ballot(p));
        ce += c[j]; me += m[j];
      }
      // the predicate holds on a prefix of the walk -- at its first bucket always (at the top level nothing is above it and
      // min_keep >= 1; deeper down the level above chose a bucket at which it held): the last such bucket is the one
      const int tstar = ntrue - 1;
      if ((int)lane == (tstar >> 2)) {
        const int j = tstar & 3;
        sh.prefix = (prefix << 8) | (unsigned)(255 - tstar);
        sh.above_c = pc[j];
        sh.above_m = pm[j];
        sh.thr = thr;
      }
    }
    __syncthreads();
  }

  // ---- 3. everything below the threshold (four at a time where all four go)
  const unsigned tau = sh.prefix;
  if (tau == 0) return;
  auto f1 = [&](unsigned bits, unsigned i) {
    if (zs_key(bits) < tau) row[i] = value;
  };
  auto f4 = [&](uint4 v, unsigned i) {
    const bool a = zs_key(v.x) < tau, b = zs_key(v.y) < tau, c = zs_key(v.z) < tau, d = zs_key(v.w) < tau;
    if (a && b && c && d) {
      *reinterpret_cast<float4*>(row + i) = make_float4(value, value, value, value);
    } else {
      if (a) row[i] = value;
      if (b) row[i + 1] = value;
      if (c) row[i + 2] = value;
      if (d) row[i + 3] = value;
    }
  };
  zs_scan<W>(src, n, tid, f4, f1);
}

extern "C" {
int zk_sample_truncate(float* logits, int ld, int rows, int V, int topk, float topp, int min_keep, float value,
                       hipStream_t stream) {
  ZK_CHECK_ARG(rows >= 0 && V >= 1, "zk_sample_truncate: bad shape (rows=%d V=%d)", rows, V);
  ZK_CHECK_ARG(ld >= V, "zk_sample_truncate: ld=%d is smaller than V=%d", ld, V);
  ZK_CHECK_ARG(topk >= 0, "zk_sample_truncate: topk=%d is negative", topk);
  ZK_CHECK_ARG(topp >= 0.f && topp <= 1.f, "zk_sample_truncate: topp=%g outside [0, 1]", (double)topp);
  ZK_CHECK_ARG(min_keep >= 1, "zk_sample_truncate: min_keep=%d", min_keep);
  ZK_CHECK_ARG(rows == 0 || logits != nullptr, "zk_sample_truncate: logits is required");
  if ((topk == 0 && topp == 0.f) || rows == 0) return 0;
  int lg = 0;
  while (lg < 31 && (1u << lg) < (unsigned)V) ++lg;
  const int S = 62 - lg < 40 ? 62 - lg : 40;
  const float scale = (float)(1ull << S);
  const bool staged = V <= ZS_LDS_MAX_V;
  const size_t lds = sizeof(ZsShared) + (staged ? (size_t)((V + 3) & ~3) * 4 : 0);
  // rows that start on 16-byte boundaries are read and staged four words at a time
  const bool wide = (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
  auto kern = staged ? (wide ? k_sample_truncate<true, 4> : k_sample_truncate<true, 1>)
                     : (wide ? k_sample_truncate<false, 4> : k_sample_truncate<false, 1>);
  static bool raised[2] = {false, false};
  if (staged && !raised[wide]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)(sizeof(ZsShared) + (size_t)ZS_LDS_MAX_V * 4));
    if (e != hipSuccess) return zk_set_error((int)e, "zk_sample_truncate: hipFuncSetAttribute: %s", hipGetErrorString(e));
    raised[wide] = true;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)rows), dim3(ZS_THREADS), lds, stream, logits, ld, V, topk, topp, min_keep, value,
                     scale);
  ZK_LAUNCH_CHECK();
  return 0;
}
}  // extern "C"
