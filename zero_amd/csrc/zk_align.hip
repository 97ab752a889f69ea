// zk_align.hip -- word alignment from a decoder layer's cross-attention (hp.alignment_file; zero_amd/models/_align.py):
// the head-averaged attention weights of a block of decoder rows over the source positions and their arg-max, straight
// from the layer's q and k projections.  No attention launch of the library keeps its probabilities (they live in
// registers or LDS and only the context leaves), so this launch forms them once more -- without the value product.
//
//   P[b, t, j] = (1 / nh) sum_h softmax_j(scale q[b, t, h] . k[b, j, h] + (1 - kmask[b, j]) * -mask_inf)     heads ascending
//   best[b, t] = argmax_j P[b, t, j] over the positions with amask[b, j] != 0; lowest j on equal values; -1 when there is none
//
// (func.py:218-256: the weights of dot_attention with the additive mask of func.py:372-400; a masked key's weight is
// exp(-mask_inf - ..) = 0 exactly whenever the row has a valid key.)
//
// One workgroup (four waves) per (sentence, ALN_BR = 16 decoder rows); it loops over the heads in order:
//   scores   bf16 form: key tiles of 16 strided over the four waves; one v_mfma_f32_16x16x32_bf16 per 32 channels with the Q
//            rows as A and the K rows as B (zk_attn_dev.h frag / mfma16: lane l holds row l & 15, channels 8 (l >> 4) .. + 7 of
//            the 32 -- for BOTH operands, so each fragment is ONE 16-byte load of a contiguous piece of a row and nothing is
//            transposed); D: lane l holds key l & 15 of the tile, rows 4 (l >> 4) + reg.
//            fp32 form: key tiles of 64 strided over the four waves, lane = key; the head's 16 query rows sit in LDS
//            (broadcast reads), a key row is read 16 bytes at a time; fused multiply-adds, channels ascending.
//            s = dot * scale + (1 - kmask) * -mask_inf goes to the LDS row buffer sS [16][LD].
//   softmax  wave w owns rows 4 w .. 4 w + 3: row maximum, e = expf(s - max) (kept in sS), row sum, then
//            sA[r][j] (+)= e / sum -- the head average's accumulator, LDS [16][LD] as well; all fp32.
// and after the last head P = sA / nh is stored (probs) and reduced to the arg-max (best).  No atomics, one fixed
// order: two runs are bit-identical.
//
// LDS: two [16][LD] fp32 images, LD = Lk rounded up to 16, + 4: the D fragment's stores put rows r and r + 4 of one
// 32-lane group 4 LD floats apart, and 4 LD mod 32 = 16 keeps them on different banks; the softmax sweeps are along a
// row (consecutive lanes, consecutive addresses).  2 * 16 * 1028 * 4 = 128.5 KB at ALN_MAX_LK = 1024, + 8 KB of queries in the
// fp32 form, of the CU's 160 KB.
#include "zk_common.h"

typedef __bf16 aln_bf16x8_t __attribute__((ext_vector_type(8)));
typedef float aln_f32x4_t __attribute__((ext_vector_type(4)));

#define ALN_BR 16
#define ALN_MAX_LK 1024
#define ALN_LDS_MAX (160 * 1024)

static inline int aln_ld(int Lk) { return ((Lk + 15) & ~15) + 4; }

// one head's scores in sS -> its softmax rows, added onto sA (h == 0: stored)
__device__ __forceinline__ void aln_softmax_add(float* sS, float* sA, int LD, int Lk, int rows, bool first, int wave, int lane) {
  for (int rr = 0; rr < 4; ++rr) {
    const int r = wave * 4 + rr;
    if (r >= rows) break;                              // (wave-uniform)
    float* s = sS + r * LD;
    float* a = sA + r * LD;
    float m = -3.0e38f;
    for (int j = lane; j < Lk; j += 64) m = fmaxf(m, s[j]);
    m = wave_max(m);
    float l = 0.f;
    for (int j = lane; j < Lk; j += 64) {
      const float e = expf(s[j] - m);
      s[j] = e;
      l += e;
    }
    l = wave_sum(l);
    for (int j = lane; j < Lk; j += 64) {
      const float p = s[j] / l;
      a[j] = first ? p : a[j] + p;
    }
  }
}

// P = sA / nh for the block's rows: stored, and its arg-max over the eligible positions
__device__ __forceinline__ void aln_finish(const float* sA, int LD, int Lk, int rows, int nh, const float* __restrict__ elig,
                                           float* __restrict__ probs, int ldp, int* __restrict__ best, int wave, int lane) {
  const float fnh = (float)nh;
  for (int rr = 0; rr < 4; ++rr) {
    const int r = wave * 4 + rr;
    if (r >= rows) break;
    const float* a = sA + r * LD;
    float bv = -1.f;                                   // (every probability is >= 0)
    int bi = 0x7fffffff, t = 0;
    for (int j = lane; j < Lk; j += 64) {
      const float p = a[j] / fnh;
      if (probs != nullptr) probs[(size_t)r * ldp + j] = p;
      if ((elig == nullptr || elig[j] != 0.f) && p > bv) { bv = p; bi = j; }     // (j ascending: the first of equals stays)
    }
    if (best != nullptr) {
      wave_argbest(bv, bi, t, [](float s2, int i2, float s, int i) { return s2 > s || (s2 == s && i2 < i); });
      if (lane == 0) best[r] = bv >= 0.f ? bi : -1;
    }
  }
}

template <int DK>      // d = 32 DK
__global__ void __launch_bounds__(256) k_align_probs(const bf16_t* __restrict__ q, int ldq, long bsq, const bf16_t* __restrict__ k,
                                                     int ldk, long bsk, const float* __restrict__ kmask, int ldmask,
                                                     const float* __restrict__ amask, float* __restrict__ probs, int ldp,
                                                     long bsp, int* __restrict__ best, int nh, int Lq, int Lk, float scale,
                                                     float mask_inf, int nblk) {
  extern __shared__ __align__(16) float sm[];
  const int LD = ((Lk + 15) & ~15) + 4;
  float* sS = sm;                  // [16][LD] the head's scores, then its exponentials
  float* sA = sS + ALN_BR * LD;    // [16][LD] sum over the heads of the softmax rows
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int blk = blockIdx.x % nblk, b = blockIdx.x / nblk;
  const int i0 = blk * ALN_BR, rows = min(ALN_BR, Lq - i0);
  const int row = lane & 15, kq = (lane >> 4) * 8;
  const int nkt = (Lk + 15) >> 4;
  const float* km = kmask != nullptr ? kmask + (size_t)b * ldmask : nullptr;
  for (int h = 0; h < nh; ++h) {
    uint4 qa[DK];
    const bf16_t* qp = q + (size_t)b * bsq + (size_t)(i0 + row) * ldq + h * (DK * 32) + kq;
#pragma unroll
    for (int kk = 0; kk < DK; ++kk)
      qa[kk] = row < rows ? *reinterpret_cast<const uint4*>(qp + kk * 32) : make_uint4(0u, 0u, 0u, 0u);
    for (int kt = wave; kt < nkt; kt += 4) {
      const int key = kt * 16 + row;
      const bf16_t* kp = k + (size_t)b * bsk + (size_t)key * ldk + h * (DK * 32) + kq;
      aln_f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < DK; ++kk) {
        const uint4 kb = key < Lk ? *reinterpret_cast<const uint4*>(kp + kk * 32) : make_uint4(0u, 0u, 0u, 0u);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(aln_bf16x8_t, qa[kk]),
                                                      __builtin_bit_cast(aln_bf16x8_t, kb), acc, 0, 0, 0);
      }
      if (key < Lk) {
        const float mterm = km != nullptr ? (1.0f - km[key]) * (-mask_inf) : 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) sS[((lane >> 4) * 4 + g) * LD + key] = acc[g] * scale + mterm;
      }
    }
    __syncthreads();
    aln_softmax_add(sS, sA, LD, Lk, rows, h == 0, wave, lane);
    __syncthreads();
  }
  const float* el = amask != nullptr ? amask + (size_t)b * ldmask : km;
  aln_finish(sA, LD, Lk, rows, nh, el, probs != nullptr ? probs + (size_t)b * bsp + (size_t)i0 * ldp : nullptr, ldp,
             best != nullptr ? best + (size_t)b * Lq + i0 : nullptr, wave, lane);
}

__global__ void __launch_bounds__(256) k_f32_align_probs(const float* __restrict__ q, int ldq, long bsq, const float* __restrict__ k,
                                                         int ldk, long bsk, const float* __restrict__ kmask, int ldmask,
                                                         const float* __restrict__ amask, float* __restrict__ probs, int ldp,
                                                         long bsp, int* __restrict__ best, int nh, int Lq, int Lk, int d,
                                                         float scale, float mask_inf, int nblk) {
  extern __shared__ __align__(16) float sm[];
  const int LD = ((Lk + 15) & ~15) + 4;
  float* sS = sm;
  float* sA = sS + ALN_BR * LD;
  float* sQ = sA + ALN_BR * LD;    // [16][d] the head's query rows (rows past Lq: zeros)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int blk = blockIdx.x % nblk, b = blockIdx.x / nblk;
  const int i0 = blk * ALN_BR, rows = min(ALN_BR, Lq - i0);
  const float* km = kmask != nullptr ? kmask + (size_t)b * ldmask : nullptr;
  for (int h = 0; h < nh; ++h) {
    for (int e = tid; e < ALN_BR * d; e += 256) {
      const int r = e / d, c = e % d;
      sQ[e] = r < rows ? q[(size_t)b * bsq + (size_t)(i0 + r) * ldq + h * d + c] : 0.f;
    }
    __syncthreads();
    for (int j = tid; j < Lk; j += 256) {              // key tiles of 64: tile 4 n + wave is this wave's
      const float* kr = k + (size_t)b * bsk + (size_t)j * ldk + h * d;
      float s[ALN_BR];
#pragma unroll
      for (int r = 0; r < ALN_BR; ++r) s[r] = 0.f;
      for (int c = 0; c < d; c += 4) {
        const float4 kv = *reinterpret_cast<const float4*>(kr + c);
#pragma unroll
        for (int r = 0; r < ALN_BR; ++r) {
          const float4 qv = *reinterpret_cast<const float4*>(sQ + r * d + c);
          s[r] = fmaf(qv.x, kv.x, s[r]); s[r] = fmaf(qv.y, kv.y, s[r]);
          s[r] = fmaf(qv.z, kv.z, s[r]); s[r] = fmaf(qv.w, kv.w, s[r]);
        }
      }
      const float mterm = km != nullptr ? (1.0f - km[j]) * (-mask_inf) : 0.f;
#pragma unroll
      for (int r = 0; r < ALN_BR; ++r) sS[r * LD + j] = s[r] * scale + mterm;
    }
    __syncthreads();
    aln_softmax_add(sS, sA, LD, Lk, rows, h == 0, wave, lane);
    __syncthreads();
  }
  const float* el = amask != nullptr ? amask + (size_t)b * ldmask : km;
  aln_finish(sA, LD, Lk, rows, nh, el, probs != nullptr ? probs + (size_t)b * bsp + (size_t)i0 * ldp : nullptr, ldp,
             best != nullptr ? best + (size_t)b * Lq + i0 : nullptr, wave, lane);
}

// the checks both forms share; vec = elements per 16 bytes of the storage type
static int aln_check(const char* name, const void* q, int ldq, long bsq, const void* k, int ldk, long bsk, const float* kmask,
                     int ldmask, const float* amask, const float* probs, int ldp, long bsp, const int* best, int B, int nh,
                     int Lq, int Lk, int d) {
  ZK_CHECK_ARG(q != nullptr && k != nullptr && B >= 0 && nh >= 1 && Lq >= 1 && Lk >= 1 && d >= 1,
               "%s: bad arguments (B=%d nh=%d Lq=%d Lk=%d d=%d)", name, B, nh, Lq, Lk, d);
  ZK_CHECK_ARG(probs != nullptr || best != nullptr, "%s: neither probs nor best is given (at least one output)", name);
  ZK_CHECK_ARG(Lk <= ALN_MAX_LK, "%s: Lk=%d keys (at most %d: two [16][Lk] fp32 images of the block in LDS)", name, Lk,
               ALN_MAX_LK);
  ZK_CHECK_ARG(ldq >= nh * d && ldk >= nh * d, "%s: row strides ldq=%d ldk=%d are shorter than nh * d = %d", name, ldq, ldk,
               nh * d);
  ZK_CHECK_ARG(bsq >= 0 && bsk >= 0 && bsp >= 0, "%s: negative sentence strides", name);
  ZK_CHECK_ARG((kmask == nullptr && amask == nullptr) || ldmask >= Lk, "%s: mask rows of ldmask=%d elements are shorter than "
               "Lk=%d", name, ldmask, Lk);
  ZK_CHECK_ARG(probs == nullptr || (ldp >= Lk && (B <= 1 || bsp >= (long)(Lq - 1) * ldp + Lk)),
               "%s: probs rows of ldp=%d (sentence stride %ld) do not hold [Lq=%d, Lk=%d]", name, ldp, bsp, Lq, Lk);
  ZK_CHECK_ARG((long)B * ((Lq + ALN_BR - 1) / ALN_BR) < (1L << 31), "%s: too many row blocks", name);
  return 0;
}

template <typename KERN>
static int aln_raise(KERN kern, size_t lds, bool& raised, const char* name) {
  if (lds > 48 * 1024 && !raised) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       ALN_LDS_MAX);
    if (e != hipSuccess) return zk_set_error((int)e, "%s: hipFuncSetAttribute: %s", name, hipGetErrorString(e));
    raised = true;
  }
  return 0;
}

template <int DK>
static int launch_align_probs(const bf16_t* q, int ldq, long bsq, const bf16_t* k, int ldk, long bsk, const float* kmask,
                              int ldmask, const float* amask, float* probs, int ldp, long bsp, int* best, int B, int nh, int Lq,
                              int Lk, float scale, float mask_inf, hipStream_t stream) {
  auto kern = k_align_probs<DK>;
  static bool raised = false;
  const size_t lds = (size_t)2 * ALN_BR * aln_ld(Lk) * sizeof(float);
  if (int rc = aln_raise(kern, lds, raised, "zk_align_probs")) return rc;
  const int nblk = (Lq + ALN_BR - 1) / ALN_BR;
  hipLaunchKernelGGL(kern, dim3((unsigned)((long)B * nblk)), dim3(256), lds, stream, q, ldq, bsq, k, ldk, bsk, kmask, ldmask,
                     amask, probs, ldp, bsp, best, nh, Lq, Lk, scale, mask_inf, nblk);
  ZK_LAUNCH_CHECK();
  return 0;
}

extern "C" int zk_align_max_lk(void) { return ALN_MAX_LK; }

extern "C" int zk_align_probs(const void* q, int ldq, long bsq, const void* k, int ldk, long bsk, const float* kmask, int ldmask,
                              const float* amask, float* probs, int ldp, long bsp, int* best, int B, int nh, int Lq, int Lk,
                              int d, float scale, float mask_inf, hipStream_t stream) {
  if (int rc = aln_check("zk_align_probs", q, ldq, bsq, k, ldk, bsk, kmask, ldmask, amask, probs, ldp, bsp, best, B, nh, Lq, Lk, d))
    return rc;
  ZK_CHECK_ARG(d % 32 == 0 && d <= 128, "zk_align_probs: head size d=%d (a multiple of 32 up to 128: one 16x16x32 bf16 MFMA per "
               "32 channels; zk_f32_align_probs takes any multiple of 4)", d);
  ZK_CHECK_ARG(ldq % 8 == 0 && bsq % 8 == 0 && (((uintptr_t)q) & 15) == 0 && ldk % 8 == 0 && bsk % 8 == 0 &&
               (((uintptr_t)k) & 15) == 0, "zk_align_probs: q and k must be 16-byte aligned rows (ldq=%d bsq=%ld ldk=%d bsk=%ld)",
               ldq, bsq, ldk, bsk);
  if (B == 0) return 0;
  const bf16_t* qb = static_cast<const bf16_t*>(q);
  const bf16_t* kb = static_cast<const bf16_t*>(k);
#define ZK_ALIGN(DK_) \
  launch_align_probs<DK_>(qb, ldq, bsq, kb, ldk, bsk, kmask, ldmask, amask, probs, ldp, bsp, best, B, nh, Lq, Lk, scale, mask_inf, stream)
  switch (d / 32) {
    case 1: return ZK_ALIGN(1);
    case 2: return ZK_ALIGN(2);
    case 3: return ZK_ALIGN(3);
    default: return ZK_ALIGN(4);
  }
#undef ZK_ALIGN
}

extern "C" int zk_f32_align_probs(const float* q, int ldq, long bsq, const float* k, int ldk, long bsk, const float* kmask,
                                  int ldmask, const float* amask, float* probs, int ldp, long bsp, int* best, int B, int nh,
                                  int Lq, int Lk, int d, float scale, float mask_inf, hipStream_t stream) {
  if (int rc = aln_check("zk_f32_align_probs", q, ldq, bsq, k, ldk, bsk, kmask, ldmask, amask, probs, ldp, bsp, best, B, nh, Lq,
                         Lk, d))
    return rc;
  ZK_CHECK_ARG(d % 4 == 0 && d <= 128, "zk_f32_align_probs: head size d=%d (a multiple of 4 up to 128)", d);
  ZK_CHECK_ARG(ldk % 4 == 0 && bsk % 4 == 0 && (((uintptr_t)k) & 15) == 0, "zk_f32_align_probs: keys must be 16-byte aligned rows "
               "(ldk=%d bsk=%ld)", ldk, bsk);
  if (B == 0) return 0;
  static bool raised = false;
  const size_t lds = ((size_t)2 * ALN_BR * aln_ld(Lk) + (size_t)ALN_BR * d) * sizeof(float);
  if (int rc = aln_raise(k_f32_align_probs, lds, raised, "zk_f32_align_probs")) return rc;
  const int nblk = (Lq + ALN_BR - 1) / ALN_BR;
  hipLaunchKernelGGL(k_f32_align_probs, dim3((unsigned)((long)B * nblk)), dim3(256), lds, stream, q, ldq, bsq, k, ldk, bsk, kmask,
                     ldmask, amask, probs, ldp, bsp, best, nh, Lq, Lk, d, scale, mask_inf, nblk);
  ZK_LAUNCH_CHECK();
  return 0;
}
