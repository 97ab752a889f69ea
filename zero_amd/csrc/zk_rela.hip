// zk_rela.hip -- rectified linear attention with a gated RMSNorm at inference (modules/rela.py:13-109;
// models/transformer_rela.py is models/transformer.py with every func.dot_attention replaced by it).
//
// For one query row i of sentence b, head h of nh, d = H / nh, keys j < nkeys:
//     s_ijh = (q_ih * d^-0.5) . k_jh                                             rela.py:60-63
//     w_ijh = relu(s_ijh) * m_j      m_j = 1 where the reference's additive bias is 0    rela.py:66-72: MULTIPLIED, never added
//     c_i   = concat_h sum_j w_ijh v_jh      (no normalisation of the weights)   rela.py:77-78
//     ms_i  = mean over ALL H channels of c_i^2                                  rela.py:106 (after combine_heads)
//     o_i   = scale * c_i * rsqrt(ms_i + eps) * sigmoid(gate * c_i)              rela.py:109
// The RMS runs across the heads, so the workgroup that owns a query row owns all of its heads.
//
// One workgroup (4 waves) per block of up to RELA_RB query rows that read the SAME keys: the Lq query positions of the
// kv_group sentences that share one memory (a decode step: Lq = 1 and the K beam rows of a sentence; the encoder:
// kv_group = 1 and a block of positions of one sentence).  Wave w owns the heads w, w + 4, ..:
//   per tile of 64 keys   lane j forms the scores of key j against every row of the block (the key's d channels are read
//                         ONCE for the block, 16 bytes per load), w = relu(s) m goes to the wave's LDS tile;
//                         lane c then adds sum_j w_j v_j[c] to its accumulators (coalesced rows of v);
//   per head              the context replaces the head's (consumed) query in LDS;
//   per row               sum of squares over the workgroup, then the gated normalisation and 16-byte stores.
// Every launch argument is static; the number of valid keys of a cached step is *nkeys_dev + 1.  No key slot at or after
// that count is read.  LDS: RELA_RB * H floats + 4 KiB.  The wave-local LDS tile is fenced by workgroup barriers, so
// every wave runs every loop with the same trip count.
#include <math.h>
#include "zk_common.h"

#define RELA_RB 4          // query rows per workgroup (1 when a memory has a single query row: a beam of one, the cached self-attention)
#define RELA_CC 4          // 64-channel chunks of a head a lane accumulates: d <= 256

// NV consecutive elements of a key row as floats: bf16 x 8 (16 bytes), fp32 x 4 (16 bytes) or fp32 x 1
template <bool F32, int NV>
__device__ __forceinline__ void rela_load(const void* base, size_t elem, float (&f)[NV]) {
  if constexpr (!F32) {
    unpack8(*reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(base) + elem), f);
  } else if constexpr (NV == 4) {
    const float4 v = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + elem);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  } else {
    f[0] = reinterpret_cast<const float*>(base)[elem];
  }
}
template <bool F32>
__device__ __forceinline__ float rela_load1(const void* base, size_t elem) {
  return F32 ? reinterpret_cast<const float*>(base)[elem] : bf2f(reinterpret_cast<const bf16_t*>(base)[elem]);
}

template <bool F32, int NV, int RB>
__global__ void __launch_bounds__(256) k_rela_attn(const void* __restrict__ q, const void* __restrict__ k,
                                                   const void* __restrict__ v, void* __restrict__ out, int B, int nh, int Lq,
                                                   int Lk, int d, int ldq, int ldk, int ldv, int ldo, long bsq, long bsk,
                                                   long bsv, long bso, const float* __restrict__ kmask, int ldmask,
                                                   int kv_group, float qscale, const int* __restrict__ nkeys_dev,
                                                   const float* __restrict__ post_scale, const float* __restrict__ post_gate,
                                                   float eps, int blocks_per_mem) {
  extern __shared__ float sm[];
  const int H = nh * d;
  float* sq = sm;                                   // [RB][H]: the scaled queries, then the contexts
  float* sw = sm + (size_t)RB * H;                  // [4 waves][RB][64]: the weights of one key tile
  float* red = sw + 4 * RB * 64;                    // [4]: block_sum
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int bk = blockIdx.x / blocks_per_mem;                         // whose keys
  const int r0 = (blockIdx.x % blocks_per_mem) * RB;                  // first of this block's rows among kv_group * Lq
  const int nrows = min(RB, kv_group * Lq - r0);
  const int nk = nkeys_dev != nullptr ? min(*nkeys_dev + 1, Lk) : Lk;

  for (int r = 0; r < RB; ++r) {
    const int rg = r0 + r, b = bk * kv_group + rg / Lq, i = rg % Lq;
    const size_t row = (size_t)b * bsq + (size_t)i * ldq;
    for (int c = threadIdx.x; c < H; c += 256) sq[r * H + c] = r < nrows ? rela_load1<F32>(q, row + c) * qscale : 0.f;
  }
  __syncthreads();

  float* swv = sw + wave * RB * 64;
  for (int h0 = 0; h0 < nh; h0 += 4) {              // (uniform trip counts: every wave meets every barrier)
    const int h = h0 + wave;
    const bool act = h < nh;
    float acc[RB][RELA_CC];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
      for (int cc = 0; cc < RELA_CC; ++cc) acc[r][cc] = 0.f;
    for (int j0 = 0; j0 < nk; j0 += 64) {
      const int j = j0 + lane;
      float s[RB];
#pragma unroll
      for (int r = 0; r < RB; ++r) s[r] = 0.f;
      if (act && j < nk) {
        const size_t krow = (size_t)bk * bsk + (size_t)j * ldk + (size_t)h * d;
        const float* qh = sq + h * d;
        for (int c = 0; c < d; c += NV) {
          float kf[NV];
          rela_load<F32, NV>(k, krow + c, kf);
#pragma unroll
          for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int e = 0; e < NV; ++e) s[r] = fmaf(qh[r * H + c + e], kf[e], s[r]);
        }
        const float m = (kmask == nullptr || kmask[(size_t)bk * ldmask + j] != 0.f) ? 1.f : 0.f;
#pragma unroll
        for (int r = 0; r < RB; ++r) s[r] = fmaxf(s[r], 0.f) * m;
      }
#pragma unroll
      for (int r = 0; r < RB; ++r) swv[r * 64 + lane] = s[r];     // (0 behind the last key)
      __syncthreads();
      if (act) {
        const int jn = min(64, nk - j0);
#pragma unroll
        for (int cc = 0; cc < RELA_CC; ++cc) {
          const int c = cc * 64 + lane;
          if (c < d) {
            const size_t vcol = (size_t)bk * bsv + (size_t)h * d + c;
            for (int jj = 0; jj < jn; ++jj) {
              const float vf = rela_load1<F32>(v, vcol + (size_t)(j0 + jj) * ldv);
#pragma unroll
              for (int r = 0; r < RB; ++r) acc[r][cc] = fmaf(swv[r * 64 + jj], vf, acc[r][cc]);
            }
          }
        }
      }
      __syncthreads();
    }
    if (act) {                                      // the head's queries are consumed: its contexts take their place
#pragma unroll
      for (int cc = 0; cc < RELA_CC; ++cc) {
        const int c = cc * 64 + lane;
        if (c < d)
#pragma unroll
          for (int r = 0; r < RB; ++r) sq[r * H + h * d + c] = acc[r][cc];
      }
    }
  }
  __syncthreads();

  const float invh = 1.f / (float)H;
  for (int r = 0; r < RB; ++r) {                    // (block_sum holds barriers: every row slot, stores for the valid ones)
    float ss = 0.f;
    for (int c = threadIdx.x; c < H; c += 256) ss = fmaf(sq[r * H + c], sq[r * H + c], ss);
    const float rs = rsqrtf(block_sum<4>(ss, red) * invh + eps);
    if (r >= nrows) continue;
    const int rg = r0 + r, b = bk * kv_group + rg / Lq, i = rg % Lq;
    const size_t row = (size_t)b * bso + (size_t)i * ldo;
    if (F32) {
      float* op = reinterpret_cast<float*>(out) + row;
      for (int c = threadIdx.x; c < H; c += 256) {
        const float x = sq[r * H + c];
        op[c] = post_scale[c] * x * rs * (1.f / (1.f + expf(-post_gate[c] * x)));
      }
    } else {
      bf16_t* op = reinterpret_cast<bf16_t*>(out) + row;
      for (int c = threadIdx.x * 8; c < H; c += 2048) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float x = sq[r * H + c + e];
          o[e] = post_scale[c + e] * x * rs * (1.f / (1.f + expf(-post_gate[c + e] * x)));
        }
        *reinterpret_cast<uint4*>(op + c) = pack8(o);
      }
    }
  }
}

template <bool F32, int NV>
static int rela_launch(const void* q, const void* k, const void* v, void* out, int B, int nh, int Lq, int Lk, int d, int ldq,
                       int ldk, int ldv, int ldo, long bsq, long bsk, long bsv, long bso, const float* kmask, int ldmask,
                       int kv_group, float qscale, const int* nkeys_dev, const float* post_scale, const float* post_gate,
                       float eps, hipStream_t stream) {
  const int H = nh * d;
  const int rb = (long)kv_group * Lq > 1 ? RELA_RB : 1;
  const size_t lds = ((size_t)rb * H + 4 * rb * 64 + 4) * sizeof(float);
  const long per_mem = ((long)kv_group * Lq + rb - 1) / rb;
  const long blocks = (long)(B / kv_group) * per_mem;
  if (blocks > 0x7fffffffL) return zk_set_error(-1, "zk_rela_attn: %ld workgroups exceed the grid", blocks);
  if (rb == 1)
    hipLaunchKernelGGL((k_rela_attn<F32, NV, 1>), dim3((unsigned)blocks), dim3(256), lds, stream, q, k, v, out, B, nh, Lq, Lk, d,
                       ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, kmask, ldmask, kv_group, qscale, nkeys_dev, post_scale, post_gate,
                       eps, (int)per_mem);
  else
    hipLaunchKernelGGL((k_rela_attn<F32, NV, RELA_RB>), dim3((unsigned)blocks), dim3(256), lds, stream, q, k, v, out, B, nh, Lq,
                       Lk, d, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, kmask, ldmask, kv_group, qscale, nkeys_dev, post_scale,
                       post_gate, eps, (int)per_mem);
  ZK_LAUNCH_CHECK();
  return 0;
}

#define RELA_CHECK_COMMON(NAME)                                                                                              \
  ZK_CHECK_ARG(q != nullptr && k != nullptr && v != nullptr && out != nullptr && post_scale != nullptr && post_gate != nullptr, \
               NAME ": q, k, v, out, post_scale and post_gate are required");                                                \
  ZK_CHECK_ARG(B >= 0 && nh >= 1 && Lq >= 1 && Lk >= 1 && d >= 1 && kv_group >= 1 && B % kv_group == 0,                      \
               NAME ": bad shape (B=%d nh=%d Lq=%d Lk=%d d=%d kv_group=%d; B must be a multiple of kv_group)", B, nh, Lq, Lk, \
               d, kv_group);                                                                                                 \
  ZK_CHECK_ARG(kmask == nullptr || ldmask >= Lk, NAME ": mask rows of ldmask=%d elements are shorter than Lk=%d", ldmask, Lk); \
  ZK_CHECK_ARG(ldq >= nh * d && ldo >= nh * d && ldk >= nh * d && ldv >= nh * d,                                             \
               NAME ": a leading dimension is smaller than H=%d (ldq=%d ldk=%d ldv=%d ldo=%d)", nh * d, ldq, ldk, ldv, ldo)

extern "C" {

int zk_rela_attn(const void* q, const void* k, const void* v, void* out, int B, int nh, int Lq, int Lk, int d, int ldq, int ldk,
                 int ldv, int ldo, long bsq, long bsk, long bsv, long bso, const float* kmask, int ldmask, int kv_group,
                 float qscale, const int* nkeys_dev, const float* post_scale, const float* post_gate, float eps,
                 hipStream_t stream) {
  RELA_CHECK_COMMON("zk_rela_attn");
  ZK_CHECK_ARG(d % 8 == 0 && d <= 128 && (long)nh * d <= 2048,
               "zk_rela_attn: the bf16 form needs a head size that is a multiple of 8 and at most 128 and a hidden size of at "
               "most 2048 (got d=%d, H=%ld); zk_f32_rela_attn takes any head size", d, (long)nh * d);
  ZK_CHECK_ARG(ldk % 8 == 0 && bsk % 8 == 0 && (((uintptr_t)k) & 15) == 0 && ldo % 8 == 0 && bso % 8 == 0 &&
               (((uintptr_t)out) & 15) == 0, "zk_rela_attn: key rows and output rows must be 16-byte aligned");
  if (B == 0) return 0;
  return rela_launch<false, 8>(q, k, v, out, B, nh, Lq, Lk, d, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, kmask, ldmask, kv_group,
                               qscale, nkeys_dev, post_scale, post_gate, eps, stream);
}

int zk_f32_rela_attn(const float* q, const float* k, const float* v, float* out, int B, int nh, int Lq, int Lk, int d, int ldq,
                     int ldk, int ldv, int ldo, long bsq, long bsk, long bsv, long bso, const float* kmask, int ldmask,
                     int kv_group, float qscale, const int* nkeys_dev, const float* post_scale, const float* post_gate,
                     float eps, hipStream_t stream) {
  RELA_CHECK_COMMON("zk_f32_rela_attn");
  ZK_CHECK_ARG(d <= 64 * RELA_CC && (long)nh * d <= 2048,
               "zk_f32_rela_attn: a head size of at most %d and a hidden size of at most 2048 (got d=%d, H=%ld)", 64 * RELA_CC, d,
               (long)nh * d);
  if (B == 0) return 0;
  const bool vec = d % 4 == 0 && ldk % 4 == 0 && bsk % 4 == 0 && (((uintptr_t)k) & 15) == 0;
  if (vec)
    return rela_launch<true, 4>(q, k, v, out, B, nh, Lq, Lk, d, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, kmask, ldmask, kv_group,
                                qscale, nkeys_dev, post_scale, post_gate, eps, stream);
  return rela_launch<true, 1>(q, k, v, out, B, nh, Lq, Lk, d, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, kmask, ldmask, kv_group,
                              qscale, nkeys_dev, post_scale, post_gate, eps, stream);
}

}  // extern "C"
