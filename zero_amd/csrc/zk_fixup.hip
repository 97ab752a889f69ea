// zk_fixup.hip -- the sub-layer boundary and the middle of the feed-forward layer of transformer_fixup at inference
// (modules/fixup.py:15-26, 29-55; models/transformer_fixup.py:47-73, 136-189).  Fixup is the Transformer without
// LayerNorm: every sub-layer input is shifted by a learned scalar (x - offset), every sub-layer output scaled by one
// (y * scale), and the residual stream is never re-normalised.
//
//   zk_fixup_residual     x_out  = x + a y                a = *scale (NULL: 1), x NULL: 0, y NULL: 0      fixup.py:21-26, residual_fn
//                         xs_out = b (x_out - o)          o = *offset (NULL: 0), b = *scale2 (NULL: 1)   fixup.py:15-18 (b: transformer_fixup.py:73)
//   zk_fixup_relu_shift   h      = relu(h - o) - o        the SAME offset twice                           fixup.py:45-50
//
// x / x_out are fp32 (the residual stream), y / xs_out / h of the storage type (bf16, or fp32 in the zk_f32_ forms).  xs_out
// is formed from the unrounded fp32 x_out and rounded once.  Every product and sum is rounded on its own (no contraction):
// the fp32 forms round where the reference's fp32 graph rounds.  The scalars are read on the device at run time -- one
// uniform load each -- so a captured graph follows a weight reload.
//
// Shape: one pass, one lane per 16 bytes of the storage type (8 bf16 / 4 fp32 columns), 16-byte loads and stores, no LDS.
// A decode step has <= 128 rows: the launch is latency bound, and the point of the fusion is ONE launch per boundary.
#include "zk_common.h"

template <int NV>
__device__ __forceinline__ void fx_load_f32(const float* p, float (&f)[NV]) {
#pragma unroll
  for (int i = 0; i < NV; i += 4) {
    const float4 v = *reinterpret_cast<const float4*>(p + i);
    f[i] = v.x; f[i + 1] = v.y; f[i + 2] = v.z; f[i + 3] = v.w;
  }
}
template <int NV>
__device__ __forceinline__ void fx_store_f32(float* p, const float (&f)[NV]) {
#pragma unroll
  for (int i = 0; i < NV; i += 4) *reinterpret_cast<float4*>(p + i) = make_float4(f[i], f[i + 1], f[i + 2], f[i + 3]);
}
// NV elements of the storage type: 8 bf16 or 4 fp32, 16 bytes either way
template <bool F32, int NV>
__device__ __forceinline__ void fx_load_st(const void* base, size_t elem, float (&f)[NV]) {
  if constexpr (F32) fx_load_f32<NV>(reinterpret_cast<const float*>(base) + elem, f);
  else unpack8(*reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(base) + elem), f);
}
template <bool F32, int NV>
__device__ __forceinline__ void fx_store_st(void* base, size_t elem, const float (&f)[NV]) {
  if constexpr (F32) fx_store_f32<NV>(reinterpret_cast<float*>(base) + elem, f);
  else *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(base) + elem) = pack8(f);
}

// (x / x_out and h / its output may be the same buffer: no __restrict__ on the matrices; a lane reads its 16 bytes before it
// writes them)
template <bool F32>
__global__ void __launch_bounds__(256) k_fixup_residual(const float* x, int ldx, const void* y, int ldy,
                                                        const float* __restrict__ scale, const float* __restrict__ offset,
                                                        const float* __restrict__ scale2, float* x_out, int ldxo,
                                                        void* xs_out, int ldxs, long chunks, int per_row) {
  constexpr int NV = F32 ? 4 : 8;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= chunks) return;
  const float a = scale ? *scale : 1.f, o = offset ? *offset : 0.f, b = scale2 ? *scale2 : 1.f;
  const size_t r = (size_t)(i / per_row);
  const int c = (int)(i - (long)r * per_row) * NV;
  float s[NV];
  if (x) fx_load_f32<NV>(x + r * ldx + c, s);
  else {
#pragma unroll
    for (int j = 0; j < NV; ++j) s[j] = 0.f;
  }
  if (y) {
    float yv[NV];
    fx_load_st<F32, NV>(y, r * ldy + c, yv);
#pragma unroll
    for (int j = 0; j < NV; ++j) s[j] = __fadd_rn(s[j], __fmul_rn(a, yv[j]));
  }
  if (x_out) fx_store_f32<NV>(x_out + r * ldxo + c, s);
  if (xs_out) {
    float t[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) t[j] = __fmul_rn(b, __fsub_rn(s[j], o));
    fx_store_st<F32, NV>(xs_out, r * ldxs + c, t);
  }
}

template <bool F32>
__global__ void __launch_bounds__(256) k_fixup_relu_shift(const void* h, int ldh, const float* __restrict__ offset, void* out,
                                                          int ldo, long chunks, int per_row) {
  constexpr int NV = F32 ? 4 : 8;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= chunks) return;
  const float o = offset ? *offset : 0.f;
  const size_t r = (size_t)(i / per_row);
  const int c = (int)(i - (long)r * per_row) * NV;
  float v[NV];
  fx_load_st<F32, NV>(h, r * ldh + c, v);
#pragma unroll
  for (int j = 0; j < NV; ++j) v[j] = __fsub_rn(fmaxf(__fsub_rn(v[j], o), 0.f), o);
  fx_store_st<F32, NV>(out, r * ldo + c, v);
}

static inline bool fx_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
// a matrix operand: absent, or 16-byte aligned rows of at least H elements with a stride that keeps them aligned
static inline bool fx_rows_ok(const void* p, int ld, int H) { return p == nullptr || (fx_al16(p) && ld % 8 == 0 && ld >= H); }

template <bool F32>
static int fixup_residual_launch(const char* name, const float* x, int ldx, const void* y, int ldy, const float* scale,
                                 const float* offset, const float* scale2, float* x_out, int ldxo, void* xs_out, int ldxs,
                                 int rows, int H, hipStream_t stream) {
  ZK_CHECK_ARG(rows >= 0 && H >= 8 && H % 8 == 0, "%s: H must be a positive multiple of 8 and rows >= 0 (got rows=%d H=%d)", name,
               rows, H);
  ZK_CHECK_ARG(x_out != nullptr || xs_out != nullptr, "%s: neither x_out nor xs_out is given", name);
  ZK_CHECK_ARG(fx_rows_ok(x, ldx, H) && fx_rows_ok(y, ldy, H) && fx_rows_ok(x_out, ldxo, H) && fx_rows_ok(xs_out, ldxs, H),
               "%s: every row stride must be a multiple of 8 elements and at least H=%d, every matrix 16-byte aligned "
               "(ldx=%d ldy=%d ldxo=%d ldxs=%d)", name, H, ldx, ldy, ldxo, ldxs);
  ZK_CHECK_ARG(x == nullptr || x_out != x || ldxo == ldx, "%s: x_out aliases x with another row stride (%d vs %d)", name, ldxo, ldx);
  if (rows == 0) return 0;
  const int per_row = H / (F32 ? 4 : 8);
  const long chunks = (long)rows * per_row;
  const long blocks = (chunks + 255) / 256;
  if (blocks > 0x7fffffffL) return zk_set_error(-1, "%s: %ld workgroups exceed the grid", name, blocks);
  hipLaunchKernelGGL((k_fixup_residual<F32>), dim3((unsigned)blocks), dim3(256), 0, stream, x, ldx, y, ldy, scale, offset, scale2,
                     x_out, ldxo, xs_out, ldxs, chunks, per_row);
  ZK_LAUNCH_CHECK();
  return 0;
}

template <bool F32>
static int fixup_relu_shift_launch(const char* name, const void* h, int ldh, const float* offset, void* out, int ldo, int rows,
                                   int F, hipStream_t stream) {
  ZK_CHECK_ARG(rows >= 0 && F >= 8 && F % 8 == 0, "%s: the width must be a positive multiple of 8 and rows >= 0 (got rows=%d F=%d)",
               name, rows, F);
  ZK_CHECK_ARG(h != nullptr && out != nullptr, "%s: h and out are required", name);
  ZK_CHECK_ARG(fx_rows_ok(h, ldh, F) && fx_rows_ok(out, ldo, F),
               "%s: every row stride must be a multiple of 8 elements and at least F=%d, every matrix 16-byte aligned "
               "(ldh=%d ldo=%d)", name, F, ldh, ldo);
  ZK_CHECK_ARG(out != h || ldo == ldh, "%s: out aliases h with another row stride (%d vs %d)", name, ldo, ldh);
  if (rows == 0) return 0;
  const int per_row = F / (F32 ? 4 : 8);
  const long chunks = (long)rows * per_row;
  const long blocks = (chunks + 255) / 256;
  if (blocks > 0x7fffffffL) return zk_set_error(-1, "%s: %ld workgroups exceed the grid", name, blocks);
  hipLaunchKernelGGL((k_fixup_relu_shift<F32>), dim3((unsigned)blocks), dim3(256), 0, stream, h, ldh, offset, out, ldo, chunks,
                     per_row);
  ZK_LAUNCH_CHECK();
  return 0;
}

extern "C" {

int zk_fixup_residual(const float* x, int ldx, const void* y, int ldy, const float* scale, const float* offset,
                      const float* scale2, float* x_out, int ldxo, void* xs_out, int ldxs, int rows, int H, hipStream_t stream) {
  return fixup_residual_launch<false>("zk_fixup_residual", x, ldx, y, ldy, scale, offset, scale2, x_out, ldxo, xs_out, ldxs, rows,
                                      H, stream);
}

int zk_f32_fixup_residual(const float* x, int ldx, const float* y, int ldy, const float* scale, const float* offset,
                          const float* scale2, float* x_out, int ldxo, float* xs_out, int ldxs, int rows, int H,
                          hipStream_t stream) {
  return fixup_residual_launch<true>("zk_f32_fixup_residual", x, ldx, y, ldy, scale, offset, scale2, x_out, ldxo, xs_out, ldxs,
                                     rows, H, stream);
}

int zk_fixup_relu_shift(const void* h, int ldh, const float* offset, void* out, int ldo, int rows, int F, hipStream_t stream) {
  return fixup_relu_shift_launch<false>("zk_fixup_relu_shift", h, ldh, offset, out, ldo, rows, F, stream);
}

int zk_f32_fixup_relu_shift(const float* h, int ldh, const float* offset, float* out, int ldo, int rows, int F,
                            hipStream_t stream) {
  return fixup_relu_shift_launch<true>("zk_f32_fixup_relu_shift", h, ldh, offset, out, ldo, rows, F, stream);
}

}  // extern "C"
