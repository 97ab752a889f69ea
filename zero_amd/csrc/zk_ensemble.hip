// zk_ensemble.hip -- per-step combination of the members' distributions in ensemble decoding (gfx950).
//
// main.py:65-115 (tower_ensemble_graph), the combination at main.py:101-103: every member's decoding_fn yields logits
// [B*K, V]; the search continues on
//     combined[r, v] = log( (1/M) * sum_m softmax(logits_m[r, :])[v] ).
// Evaluated here in the stable form, fp32 arithmetic and fp32 accumulation throughout:
//     lse_m[r]       = logsumexp_v logits_m[r, v]
//     combined[r, v] = logsumexp_m (logits_m[r, v] - lse_m[r]) - log M
// With M = 1 this is a plain fp32 log-softmax (logsumexp over one term adds log(1) = 0 exactly).
//
// The one intended deviation from the reference: its literal form takes tf.log of a mean of probabilities, which is
// -inf where every member's probability underflows fp32; the stable form gives the finite, very negative log-probability
// there.  Everywhere else the two agree to fp32 rounding.
//
// Shape: a streaming kernel, M * rows * V * 4 bytes read twice (the second time mostly from the caches: a decode step's
// 128 x 32000 logits are 16 MB per member) and rows * V * 4 written.  One workgroup per row would leave half of the 256
// CUs idle at the decode shape (rows = B*K = 128), so a row is split over several workgroups in both passes:
//   k_ens_stats    grid (S, rows, M): online (max, sum exp) of one column chunk of one member's row -> partials
//   k_ens_combine  grid (S2, rows):   merges the S partials of each member into lse_m, then combines its column chunk
// 16-byte loads and stores; DPP wave reductions (zk_common.h).  The member pointers and leading dimensions travel BY VALUE
// in the kernels' argument block: no allocation, no copy and no synchronisation per call, so the call can be captured in
// a hipGraph.
#include "zk_common.h"

#define ZK_ENS_MAX 8          // members per call
#define ZK_ENS_SPLIT_MAX 16   // column chunks per row
#define ZK_ENS_BLOCKS 2048    // workgroups a pass aims at (8 per CU)

extern "C" {
int zk_ensemble_max(void);
size_t zk_ensemble_logprob_workspace(int rows, int M, int V);
int zk_ensemble_logprob(const float* const* logits, const int* ld, int M, int rows, int V, float* out, int ld_out,
                        void* workspace, size_t ws_bytes, hipStream_t stream);
}

struct EnsArgs {
  const float* x[ZK_ENS_MAX];
  int ld[ZK_ENS_MAX];
};

// column chunks per row for `lists` rows' worth of workgroup columns; every chunk keeps >= one 16-byte load per thread
static int ens_split(int lists, int V) {
  const int v4 = (V + 3) / 4;
  int s = ZK_ENS_BLOCKS / (lists > 0 ? lists : 1);
  const int cap = (v4 + 255) / 256;
  if (s > cap) s = cap;
  if (s > ZK_ENS_SPLIT_MAX) s = ZK_ENS_SPLIT_MAX;
  if (s < 1) s = 1;
  return s;
}

// columns >= V of the 16-byte group that starts at column `col` (col < V) take no part
__device__ __forceinline__ float4 ens_mask_tail(float4 v, int col, int V) {
  if (col + 1 >= V) v.y = -INFINITY;
  if (col + 2 >= V) v.z = -INFINITY;
  if (col + 3 >= V) v.w = -INFINITY;
  return v;
}

__global__ void __launch_bounds__(256) k_ens_stats(EnsArgs a, float2* __restrict__ part, int rows, int V, int chunk4, int S) {
  __shared__ float sm[4];
  const int s = blockIdx.x, r = blockIdx.y, m = blockIdx.z;
  const float* __restrict__ x = a.x[m] + (size_t)r * a.ld[m];
  const int v4 = (V + 3) >> 2;
  const int c0 = s * chunk4, c1 = min(c0 + chunk4, v4);
  float mx = -INFINITY, sum = 0.f;
  for (int c = c0 + (int)threadIdx.x; c < c1; c += 256) {
    const float4 v = ens_mask_tail(*reinterpret_cast<const float4*>(x + 4 * (size_t)c), 4 * c, V);
    const float m4 = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
    if (m4 > mx) {
      sum *= expf(mx - m4);          // (first group: 0 * exp(-inf) = 0)
      mx = m4;
    }
    sum += (expf(v.x - mx) + expf(v.y - mx)) + (expf(v.z - mx) + expf(v.w - mx));
  }
  const float bmx = block_max<4>(mx, sm);
  const float tot = block_sum<4>(mx == -INFINITY ? 0.f : sum * expf(mx - bmx), sm);
  if (threadIdx.x == 0) part[((size_t)m * rows + r) * S + s] = make_float2(bmx, tot);
}

template <int M>
__global__ void __launch_bounds__(256) k_ens_combine(EnsArgs a, const float2* __restrict__ part, float* __restrict__ out,
                                                     int ld_out, int rows, int V, int chunk4, int S, float log_m) {
  __shared__ float lse_sm[ZK_ENS_MAX];
  const int r = blockIdx.y;
  if ((int)threadIdx.x < M) {
    // logsumexp of member threadIdx.x's row from the partials of its S column chunks (an empty chunk holds (-inf, 0))
    const float2* __restrict__ p = part + ((size_t)threadIdx.x * rows + r) * S;
    float mx = -INFINITY;
    for (int s = 0; s < S; ++s) mx = fmaxf(mx, p[s].x);
    float tot = 0.f;
    for (int s = 0; s < S; ++s)
      if (p[s].x != -INFINITY) tot += p[s].y * expf(p[s].x - mx);
    lse_sm[threadIdx.x] = mx + logf(tot);
  }
  __syncthreads();
  float lse[M];
  const float* __restrict__ x[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    lse[m] = lse_sm[m];
    x[m] = a.x[m] + (size_t)r * a.ld[m];
  }
  float* __restrict__ o = out + (size_t)r * ld_out;
  const int v4 = (V + 3) >> 2;
  const int c0 = blockIdx.x * chunk4, c1 = min(c0 + chunk4, v4);
  for (int c = c0 + (int)threadIdx.x; c < c1; c += 256) {
    float4 v[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      v[m] = *reinterpret_cast<const float4*>(x[m] + 4 * (size_t)c);
      v[m].x -= lse[m]; v[m].y -= lse[m]; v[m].z -= lse[m]; v[m].w -= lse[m];
    }
    float4 mx = v[0];
#pragma unroll
    for (int m = 1; m < M; ++m) {
      mx.x = fmaxf(mx.x, v[m].x); mx.y = fmaxf(mx.y, v[m].y); mx.z = fmaxf(mx.z, v[m].z); mx.w = fmaxf(mx.w, v[m].w);
    }
    float4 res = v[0];                 // M == 1: logsumexp over one term is the term itself
    if (M > 1) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int m = 0; m < M; ++m) {
        acc.x += expf(v[m].x - mx.x); acc.y += expf(v[m].y - mx.y);
        acc.z += expf(v[m].z - mx.z); acc.w += expf(v[m].w - mx.w);
      }
      res = make_float4(mx.x + logf(acc.x) - log_m, mx.y + logf(acc.y) - log_m, mx.z + logf(acc.z) - log_m,
                        mx.w + logf(acc.w) - log_m);
    }
    const int col = 4 * c;
    if (col + 3 < V) {
      *reinterpret_cast<float4*>(o + col) = res;
    } else {                           // the last group of a row whose V is not a multiple of 4: columns >= V stay untouched
      o[col] = res.x;
      if (col + 1 < V) o[col + 1] = res.y;
      if (col + 2 < V) o[col + 2] = res.z;
    }
  }
}

extern "C" {

int zk_ensemble_max(void) { return ZK_ENS_MAX; }

size_t zk_ensemble_logprob_workspace(int rows, int M, int V) {
  if (rows <= 0 || M <= 0 || V <= 0) return 0;
  return (size_t)M * rows * ens_split(rows * M, V) * sizeof(float2);
}

int zk_ensemble_logprob(const float* const* logits, const int* ld, int M, int rows, int V, float* out, int ld_out,
                        void* workspace, size_t ws_bytes, hipStream_t stream) {
  ZK_CHECK_ARG(M >= 1 && M <= ZK_ENS_MAX, "zk_ensemble_logprob: M=%d members out of range (1..%d)", M, ZK_ENS_MAX);
  ZK_CHECK_ARG(rows >= 0 && rows <= 65535 && V >= 0, "zk_ensemble_logprob: rows=%d must be in 0..65535, V=%d >= 0", rows, V);
  if (rows == 0 || V == 0) return 0;
  ZK_CHECK_ARG(logits != nullptr && ld != nullptr && out != nullptr, "zk_ensemble_logprob: logits, ld and out are required");
  ZK_CHECK_ARG(ld_out % 4 == 0 && ld_out >= V && ((uintptr_t)out & 15) == 0,
               "zk_ensemble_logprob: ld_out=%d must be a multiple of 4 and >= V=%d, out 16-byte aligned", ld_out, V);
  EnsArgs a;
  for (int m = 0; m < ZK_ENS_MAX; ++m) {
    a.x[m] = m < M ? logits[m] : nullptr;
    a.ld[m] = m < M ? ld[m] : 0;
    if (m < M)
      ZK_CHECK_ARG(a.x[m] != nullptr && ((uintptr_t)a.x[m] & 15) == 0 && a.ld[m] % 4 == 0 && a.ld[m] >= V,
                   "zk_ensemble_logprob: member %d needs a 16-byte aligned pointer and ld=%d a multiple of 4 and >= V=%d", m,
                   a.ld[m], V);
  }
  ZK_CHECK_ARG(workspace != nullptr && ((uintptr_t)workspace & 7) == 0 && ws_bytes >= zk_ensemble_logprob_workspace(rows, M, V),
               "zk_ensemble_logprob: workspace too small (need %zu bytes)", zk_ensemble_logprob_workspace(rows, M, V));
  const int v4 = (V + 3) / 4;
  const int S = ens_split(rows * M, V), S2 = ens_split(rows, V);
  const int chunk_a = (v4 + S - 1) / S, chunk_b = (v4 + S2 - 1) / S2;
  float2* part = (float2*)workspace;
  hipLaunchKernelGGL(k_ens_stats, dim3(S, rows, M), dim3(256), 0, stream, a, part, rows, V, chunk_a, S);
  ZK_LAUNCH_CHECK();
  const float log_m = logf((float)M);
#define ZK_ENS_CASE(N)                                                                                                  \
  case N:                                                                                                               \
    hipLaunchKernelGGL(k_ens_combine<N>, dim3(S2, rows), dim3(256), 0, stream, a, (const float2*)part, out, ld_out, rows, \
                       V, chunk_b, S, log_m);                                                                           \
    break;
  switch (M) {
    ZK_ENS_CASE(1) ZK_ENS_CASE(2) ZK_ENS_CASE(3) ZK_ENS_CASE(4) ZK_ENS_CASE(5) ZK_ENS_CASE(6) ZK_ENS_CASE(7) ZK_ENS_CASE(8)
  }
#undef ZK_ENS_CASE
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
