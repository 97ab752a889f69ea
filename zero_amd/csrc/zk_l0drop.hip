// zk_l0drop.hip -- L0Drop at inference (models/transformer_l0drop.py:103-135, 244-273; modules/l0norm.py:75-96, 166-177):
// a learned hard-concrete gate drops most encoder outputs, the decoder's cross-attention runs over the survivors plus
// ONE counting slot that stands in for the dropped ones.
//
//   zk_l0_gate      per sentence: log_alpha[j] = enc[j, :] . W + b0 (fp32 accumulation from fp32 master weights: the keep
//                   decision is discrete), gate = clip(sigmoid(log_alpha) * 1.2 - 0.1, 0, 1), keep = gate != 0 and the
//                   position is no padding; the ascending list of kept positions (tf.nn.top_k on a 0/1 vector: ties go
//                   to the lower index), the counts, and the largest kept count of the batch.
//   zk_l0_compact   mem[b] = [0 | enc[b, pos[b, i], :] * gate | 0 ..], its mask and the log-count bias of slot 0.
//
// The count-weighted softmax itself lives in the attention kernels (zk_dec_cross_kb, zk_f32_attn_kb): exp(l + log c)
// is the reference's exp(l) * c.
#include <math.h>
#include "zk_common.h"

template <bool F32IN>
__device__ __forceinline__ void l0_load4(const void* base, size_t elem, float (&f)[4]) {
  if (F32IN) {
    const float4 v = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + elem);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  } else {
    const uint2 v = *reinterpret_cast<const uint2*>(reinterpret_cast<const bf16_t*>(base) + elem);
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
  }
}

// One workgroup (4 waves) per sentence.  Wave w computes the rows w, w + 4, ..: lane l owns the 4-column chunks l,
// l + 64, ..; then wave 0 compacts the keep flags 64 positions at a time (ballot + prefix popcount, a running base).
template <bool F32IN>
__global__ void __launch_bounds__(256) k_l0_gate(const void* __restrict__ enc, int ld, const float* __restrict__ smask,
                                                 const float* __restrict__ W, const float* __restrict__ b0, int Ls, int H,
                                                 float* __restrict__ gate, int* __restrict__ pos, int* __restrict__ nkeep,
                                                 int* __restrict__ ndrop, int* __restrict__ kmax) {
  extern __shared__ int sflag[];                  // [Ls]: bit 0 = kept, bit 1 = valid (no padding)
  const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float bias = *b0;
  for (int j = wave; j < Ls; j += 4) {
    const size_t row = ((size_t)b * Ls + j) * ld;
    float acc = 0.f;
    for (int c = lane * 4; c < H; c += 256) {
      float x[4];
      l0_load4<F32IN>(enc, row + c, x);
      const float4 w4 = *reinterpret_cast<const float4*>(W + c);
      acc = fmaf(x[0], w4.x, acc); acc = fmaf(x[1], w4.y, acc); acc = fmaf(x[2], w4.z, acc); acc = fmaf(x[3], w4.w, acc);
    }
    const float la = wave_sum(acc) + bias;
    const float g = fminf(fmaxf((1.f / (1.f + expf(-la))) * 1.2f - 0.1f, 0.f), 1.f);   // GAMMA = -0.1, ZETA = 1.1
    if (lane == 0) {
      const bool valid = smask[(size_t)b * Ls + j] != 0.f;
      gate[(size_t)b * Ls + j] = g;
      sflag[j] = ((g != 0.f && valid) ? 1 : 0) | (valid ? 2 : 0);
    }
  }
  __syncthreads();
  if (wave != 0) return;
  int base = 0, nvalid = 0;
  for (int j0 = 0; j0 < Ls; j0 += 64) {
    const int j = j0 + lane;
    const int f = j < Ls ? sflag[j] : 0;
    const unsigned long long kept = __ballot(f & 1), valid = __ballot(f & 2);
    if (f & 1) pos[(size_t)b * Ls + base + __popcll(kept & ((1ull << lane) - 1ull))] = j;
    base += __popcll(kept);
    nvalid += __popcll(valid);
  }
  for (int i = base + lane; i < Ls; i += 64) pos[(size_t)b * Ls + i] = -1;
  if (lane == 0) {
    nkeep[b] = base;
    ndrop[b] = nvalid - base;
    atomicMax(kmax, base);
  }
}

// One workgroup per slot (b, s) of the compacted memory.
template <bool F32IN>
__global__ void __launch_bounds__(128) k_l0_compact(const void* __restrict__ enc, int ld, const float* __restrict__ gate,
                                                    const int* __restrict__ pos, const int* __restrict__ nkeep,
                                                    const int* __restrict__ ndrop, int Ls, int H, int Lm,
                                                    void* __restrict__ mem, int ldm, float* __restrict__ gmask,
                                                    float* __restrict__ kbias) {
  const int b = blockIdx.x / Lm, s = blockIdx.x % Lm, i = s - 1;
  int j = -1;
  if (s >= 1 && i < nkeep[b]) j = pos[(size_t)b * Ls + i];      // (nkeep <= Ls and 0 <= pos < Ls: zk_l0_gate's lists)
  if (threadIdx.x == 0) {
    const int nd = ndrop[b];
    gmask[(size_t)b * Lm + s] = s == 0 ? (nd > 0 ? 1.f : 0.f) : (j >= 0 ? 1.f : 0.f);
    kbias[(size_t)b * Lm + s] = s == 0 ? logf((float)max(nd, 1)) : 0.f;
  }
  const float g = j >= 0 ? gate[(size_t)b * Ls + j] : 0.f;
  const size_t src = ((size_t)b * Ls + max(j, 0)) * ld, dst = ((size_t)b * Lm + s) * ldm;
  for (int c = threadIdx.x * 4; c < H; c += 512) {
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    if (j >= 0) {
      l0_load4<F32IN>(enc, src + c, x);
#pragma unroll
      for (int q = 0; q < 4; ++q) x[q] *= g;
    }
    if (F32IN) {
      *reinterpret_cast<float4*>(reinterpret_cast<float*>(mem) + dst + c) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
      *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(mem) + dst + c) = make_uint2(pack2bf(x[0], x[1]), pack2bf(x[2], x[3]));
    }
  }
}

extern "C" {

int zk_l0_gate(const void* enc, int ld, int f32, const float* smask, const float* W, const float* b0, int B, int Ls, int H,
               float* gate, int* pos, int* nkeep, int* ndrop, int* kmax, hipStream_t stream) {
  ZK_CHECK_ARG(B >= 0 && Ls >= 1 && Ls <= 8192 && H >= 4 && H % 4 == 0 && ld >= H && ld % 4 == 0,
               "zk_l0_gate: bad shape (B=%d Ls=%d H=%d ld=%d; H and ld multiples of 4, Ls <= 8192)", B, Ls, H, ld);
  ZK_CHECK_ARG(enc && smask && W && b0 && gate && pos && nkeep && ndrop && kmax, "zk_l0_gate: every pointer is required");
  ZK_CHECK_ARG((((uintptr_t)enc) & (f32 ? 15 : 7)) == 0 && (((uintptr_t)W) & 15) == 0,
               "zk_l0_gate: rows and W must be aligned to four elements");
  hipError_t e = hipMemsetAsync(kmax, 0, sizeof(int), stream);
  if (e != hipSuccess) return zk_set_error((int)e, "zk_l0_gate: hipMemsetAsync: %s", hipGetErrorString(e));
  if (B == 0) return 0;
  const size_t lds = (size_t)Ls * sizeof(int);
  if (f32) hipLaunchKernelGGL(k_l0_gate<true>, dim3(B), dim3(256), lds, stream, enc, ld, smask, W, b0, Ls, H, gate, pos, nkeep,
                              ndrop, kmax);
  else hipLaunchKernelGGL(k_l0_gate<false>, dim3(B), dim3(256), lds, stream, enc, ld, smask, W, b0, Ls, H, gate, pos, nkeep,
                          ndrop, kmax);
  ZK_LAUNCH_CHECK();
  return 0;
}

int zk_l0_compact(const void* enc, int ld, int f32, const float* gate, const int* pos, const int* nkeep, const int* ndrop,
                  int B, int Ls, int H, int Lm, void* mem, int ldm, float* gmask, float* kbias, hipStream_t stream) {
  ZK_CHECK_ARG(B >= 0 && Ls >= 1 && Lm >= 1 && H >= 4 && H % 4 == 0 && ld >= H && ld % 4 == 0 && ldm >= H && ldm % 4 == 0,
               "zk_l0_compact: bad shape (B=%d Ls=%d Lm=%d H=%d ld=%d ldm=%d)", B, Ls, Lm, H, ld, ldm);
  ZK_CHECK_ARG(enc && gate && pos && nkeep && ndrop && mem && gmask && kbias, "zk_l0_compact: every pointer is required");
  ZK_CHECK_ARG(((((uintptr_t)enc) | ((uintptr_t)mem)) & (f32 ? 15 : 7)) == 0,
               "zk_l0_compact: rows must be aligned to four elements");
  ZK_CHECK_ARG((long)B * Lm <= 0x7fffffffL, "zk_l0_compact: B * Lm = %ld slots exceed the grid", (long)B * Lm);
  if (B == 0) return 0;
  if (f32) hipLaunchKernelGGL(k_l0_compact<true>, dim3((unsigned)(B * Lm)), dim3(128), 0, stream, enc, ld, gate, pos, nkeep, ndrop,
                              Ls, H, Lm, mem, ldm, gmask, kbias);
  else hipLaunchKernelGGL(k_l0_compact<false>, dim3((unsigned)(B * Lm)), dim3(128), 0, stream, enc, ld, gate, pos, nkeep, ndrop,
                          Ls, H, Lm, mem, ldm, gmask, kbias);
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
