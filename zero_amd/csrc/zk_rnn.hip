// zk_rnn.hip -- the recurrent family at inference: `rnnsearch` (models/rnnsearch.py; rnns/rnn.py, rnns/atr.py,
// func.py:107-161 additive_attention) and `rnnsearch_deepatt` (models/rnnsearch_deepatt.py; the same launches plus the GRU
// cell of rnns/gru.py, whose two launches are described where they are defined) and `deepnmt` (models/deepnmt.py; the same
// launches plus a layer's ff product with its residual add, zk_rnn_ff_residual, described where it is defined); and the lrn /
// olrn cells of both (rnns/lrn.py, rnns/olrn.py: no recurrent product, so a WHOLE scan is one launch, zk_rnn_lrn_scan, described
// where it is defined).  bf16 forms (bf16 GEMM operands, fp32 arithmetic) and fp32 forms (zk_f32_*).
//
// ATR cell (rnns/atr.py:32-60, twin gates) for one time step of R rows, with the mask carry of rnns/rnn.py:41-49:
//     q = h_prev U + b      i = sigmoid(p + q)      f = sigmoid(p - q)      h = i p + f h_prev
//     out = m h + (1 - m) h_prev
// p is the input projection (x W, computed for the whole sequence by one GEMM), h_prev the fp32 state, optionally
// gathered by a row index (the beam reorder of a decode step) or absent (the zero state).  The state is fp32 in BOTH
// forms: nothing re-normalises a recurrent state, so a bf16 state would lose every update below half an ulp of h and
// the loss would compound over the sequence.  In the bf16 form only the MFMA operand is a rounded copy of h_prev;
// f h_prev and the carry use the fp32 value.  out_copy is the state in the storage type: the operand of the next GEMM.
//
// The dense cell launches -- the ATR step, the two GRU launches, ff + residual -- are four epilogues (AtrCell, GruGatesCell,
// GruOutCell, FfCell, each written once for both storage types) over ONE tile driver per form (rnn_bf16_tile, rnn_f32_tile);
// the kernels are k_rnn_atr_step<T>, k_rnn_gru_gates<T>, k_rnn_gru_out<T> and k_rnn_ff_residual<T>, T = bf16_t or float.
// bf16 driver: one workgroup (4 waves) per 16 output columns and 64 rows, wave w owns rows 16 w .. 16 w + 15.
// Why: R is 32 .. 128 rows and H about 1000, so one step is ~0.25 GFLOP against 2 MB of U -- the launch is a latency
// chain, not a throughput problem.  16-column tiles give H / 16 = 63 workgroups for H = 1000 (two for R = 128), each of
// which streams a 32-row-stride slab of U ONCE (H x 16 bf16 = 32 KB) into a transposed LDS image [16][K + 8] so that the
// B fragments are 16-byte LDS reads; wider tiles would halve the number of CUs that pull U, narrower ones waste the
// MFMA's 16 columns.  The A fragments (h_prev rows, fp32 -> bf16) come straight from global memory: every wave reads
// its own 16 rows once.  Edge tiles in rows, columns and K are zero-filled.  v_mfma_f32_16x16x32_bf16 fragment maps
// (zk_attn_dev.h frag / mfma16): A lane l = row l & 15, k = 8 (l >> 4) + j; B the same with the column; D column l & 15,
// row 4 (l >> 4) + reg.
// fp32 driver: one workgroup per 64 columns and 32 rows; lane = column (coalesced rows of U), wave w owns rows 8 w .. 8 w + 7
// whose chunk [32][64] of the A operand sits in LDS (broadcast reads); k ascending, fused multiply-adds.
//
// Additive attention of one decode step (func.py:107-161; one head, rnns/rnn.py:131-136):
//     logit_j = v . tanh(qa + pm_j) + (1 - mask_j) * -inf_const        a = softmax_j        c = sum_j a_j mem_j
// (feed_logits/b_0 shifts a whole row and drops out of the softmax).  One workgroup per block of up to ADD_RB beam rows
// that share one source sentence (kv_group rows per sentence): projected memory pm and memory mem are read once for the
// block.  Keys in tiles of 64 with an online softmax, so any Ls:
//   phase A   wave w forms the logits of the keys 16 w .. 16 w + 15 of the tile, lanes over the channels (16-byte loads);
//   phase B   wave r rescales row r: new running maximum, p_j = exp(logit_j - max), running sum;
//   phase C   thread c adds sum_j p_j mem_j[c] to its accumulators (coalesced rows of mem).
// A masked key's logit is about -inf_const, its weight exp(-inf_const - max) is exactly 0.  tanhf saturates to +-1.
#include <float.h>
#include <math.h>
#include <type_traits>
#include "zk_common.h"

typedef __bf16 rbf16x8_t __attribute__((ext_vector_type(8)));
typedef float rf32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float rnn_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// an element of the storage type (bf16_t or float) as fp32
__device__ __forceinline__ float rnn_load(const bf16_t* p, size_t i) { return bf2f(p[i]); }
__device__ __forceinline__ float rnn_load(const float* p, size_t i) { return p[i]; }
__device__ __forceinline__ void rnn_store(bf16_t* p, size_t i, float v) { p[i] = f2bf(v); }
__device__ __forceinline__ void rnn_store(float* p, size_t i, float v) { p[i] = v; }

// the state operand of a cell launch: fp32 rows, gathered by idx (NULL: row r is row r); h_prev NULL: the zero state
struct RnnState {
  const float* h_prev;
  int ldh, n_prev;
  const int* idx;
  __device__ __forceinline__ int src(int row) const { return min(max(idx != nullptr ? idx[row] : row, 0), n_prev - 1); }
  __device__ __forceinline__ float at(int row, int col) const {
    return h_prev != nullptr ? h_prev[(size_t)src(row) * ldh + col] : 0.f;
  }
  // the row a lane feeds the product; a lane past R (not valid) points at row 0 and loads nothing
  __device__ __forceinline__ const float* a_row(int row, bool valid) const {
    const int s = min(max(valid ? (idx != nullptr ? idx[row] : row) : 0, 0), n_prev - 1);
    return h_prev + (size_t)s * ldh;
  }
};

// true when some row [a + r lda, + w) (r < ra) shares an element with some row [b + s ldb, + w) (s < rb)
static bool rnn_rows_overlap(const float* a, long lda, long ra, const float* b, long ldb, long rb, long w) {
  if (a == nullptr || b == nullptr || ra <= 0 || rb <= 0 || w <= 0) return false;
  const uintptr_t a0 = (uintptr_t)a, a1 = (uintptr_t)(a + (ra - 1) * lda + w);
  const uintptr_t b0 = (uintptr_t)b, b1 = (uintptr_t)(b + (rb - 1) * ldb + w);
  if (a1 <= b0 || b1 <= a0) return false;
  if (lda != ldb || lda < w) return true;                      // different pitches: the enclosing ranges decide
  const long bytes = (long)((intptr_t)a0 - (intptr_t)b0);
  if (bytes % 4 != 0) return true;
  // equal pitch: row r of a sits delta + (r - s) ld elements from row s of b; the two candidates nearest to zero
  const long delta = bytes / 4, ld = lda;
  long m = delta % ld;
  if (m < 0) m += ld;
  const long d_lo = -(delta - m) / ld;                         // delta + d_lo ld = m          (0 <= m < ld)
  const long cand[2][2] = {{d_lo, m}, {d_lo - 1, m - ld}};
  for (int i = 0; i < 2; ++i) {
    const long d = cand[i][0], diff = cand[i][1];
    if (d >= -(rb - 1) && d <= ra - 1 && diff < w && -diff < w) return true;
  }
  return false;
}

// ---------------------------------------------------------------- the two tile drivers of the dense cells
// A dense cell launch is out = epilogue(A W) for R rows: the ATR step, the two GRU launches and ff + residual differ in the
// A operand (the gathered fp32 state, or rows of the storage type), in the number NT of 16- or 64-column blocks of W a
// workgroup takes (2 for the GRU gates: z and r; else 1) and in the epilogue.  Each storage form has ONE driver; a cell is a
// struct that names its A rows and W and states its arithmetic once, for both forms (`Cell<T>`, T the storage type):
//     bool product()                 false: the zero state, no product (the accumulators stay 0)
//     a_row(row, valid)              the A row of `row`; STATE_A: it is the fp32 state
//     W, ldw, b                      block t of the product is A W[:, t N .. t N + N - 1] + b[t N .. t N + N - 1]
//     operator()(t, row, col, q)     the epilogue of one element q of block t
// bf16 form (rnn_bf16_tile): 16 columns x 64 rows per workgroup, the slabs in the LDS image [NT][16][K + 8] (rnn_stage_slab),
// v_mfma_f32_16x16x32_bf16 (rnn_product); the largest image is 132 KB (ATR H = 4096, ff K = 4096; GRU gates H = GRU_MAX_H).
// fp32 form (rnn_f32_tile): 64 columns x 32 rows, lane = column, eight rows per wave (rnn_f32_product); the grid has NT x
// ceil(N / 64) column tiles, block t after block t - 1.
#define ATR_BN 16          // bf16 form: output columns per workgroup
#define ATR_BM 64          //            rows per workgroup (16 per wave)
#define ATRF_BN 64         // fp32 form: output columns per workgroup
#define ATRF_BM 32         //            rows per workgroup (8 per wave)
#define GRU_MAX_H 2048

// sT [16][KS] = U[0 .. K - 1][n0 .. n0 + 15] transposed; the columns n0 + c >= N and the rows k >= K are zero
__device__ __forceinline__ void rnn_stage_slab(bf16_t* sT, int KS, const bf16_t* __restrict__ U, int ldu, int n0, int K, int N,
                                               int Kr) {
  for (int k = threadIdx.x; k < Kr; k += 256) {
    uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = lo;
    if (k < K) {                                               // (N % 8 == 0: a group of 8 columns is inside or outside)
      const bf16_t* up = U + (size_t)k * ldu + n0;
      if (n0 < N) lo = *reinterpret_cast<const uint4*>(up);
      if (n0 + 8 < N) hi = *reinterpret_cast<const uint4*>(up + 8);
    }
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      sT[(2 * c) * KS + k] = (bf16_t)(w[c] & 0xffffu);
      sT[(2 * c + 1) * KS + k] = (bf16_t)(w[c] >> 16);
    }
  }
}

// acc[t] += A[row][0 .. K - 1] . sU tile t for the 16 rows of a wave; A_F32: the row is fp32 (rounded here), else bf16 already
template <int NT, bool A_F32>
__device__ __forceinline__ void rnn_product(rf32x4_t (&acc)[NT], const bf16_t* sU, int KS, int Kr, int K, const void* arow,
                                            bool valid, int vec_a, int lane) {
  const bf16_t* bt = sU + (lane & 15) * KS + (lane >> 4) * 8;
  for (int kk = 0; kk < Kr; kk += 32) {
    const int k = kk + (lane >> 4) * 8;
    uint4 af = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (A_F32) {
      const float* hp = reinterpret_cast<const float*>(arow);
      float a[8];
      if (vec_a) {
        float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), x1 = x0;
        if (valid && k < K) {
          x0 = *reinterpret_cast<const float4*>(hp + k);
          x1 = *reinterpret_cast<const float4*>(hp + k + 4);
        }
        a[0] = x0.x; a[1] = x0.y; a[2] = x0.z; a[3] = x0.w; a[4] = x1.x; a[5] = x1.y; a[6] = x1.z; a[7] = x1.w;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = (valid && k + e < K) ? hp[k + e] : 0.f;
      }
      af = pack8(a);
    } else {
      const bf16_t* ap = reinterpret_cast<const bf16_t*>(arow);
      if (vec_a) {
        if (valid && k < K) af = *reinterpret_cast<const uint4*>(ap + k);
      } else {
        float a[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = (valid && k + e < K) ? bf2f(ap[k + e]) : 0.f;
        af = pack8(a);                                         // (exact: the values are bf16 already)
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const uint4 bf = *reinterpret_cast<const uint4*>(bt + (size_t)t * 16 * KS + kk);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(rbf16x8_t, af), __builtin_bit_cast(rbf16x8_t, bf),
                                                       acc[t], 0, 0, 0);
    }
  }
}

template <int NT, typename Cell>
__device__ __forceinline__ void rnn_bf16_tile(const Cell& cell, int R, int K, int N, int vec_a) {
  extern __shared__ __align__(16) unsigned char rnn_lds[];
  bf16_t* sW = reinterpret_cast<bf16_t*>(rnn_lds);            // [NT][ATR_BN][KS]: W[:, t N + n0 .. + 15] transposed
  const int Kr = (K + 31) / 32 * 32, KS = Kr + 8;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n0 = blockIdx.x * ATR_BN, r0 = blockIdx.y * ATR_BM + wave * 16;
  rf32x4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = rf32x4_t{0.f, 0.f, 0.f, 0.f};
  if (cell.product()) {
#pragma unroll
    for (int t = 0; t < NT; ++t) rnn_stage_slab(sW + (size_t)t * ATR_BN * KS, KS, cell.W + t * N, cell.ldw, n0, K, N, Kr);
    __syncthreads();
    if (r0 < R) {                                              // wave-uniform: the MFMA runs with all 64 lanes
      const int row = r0 + (lane & 15);
      const bool valid = row < R;
      rnn_product<NT, Cell::STATE_A>(acc, sW, KS, Kr, K, cell.a_row(row, valid), valid, vec_a, lane);
    }
  }
  const int col = n0 + (lane & 15);
  if (col >= N) return;
  float bias[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) bias[t] = cell.b[t * N + col];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = r0 + (lane >> 4) * 4 + r;
    if (row >= R) continue;
#pragma unroll
    for (int t = NT - 1; t >= 0; --t) cell(t, row, col, acc[t][r] + bias[t]);       // (the GRU gates: the piece that gathers first)
  }
}

// fp32 forms: acc[j] += sum_k A[row j of the wave][k] U[k][col], k < K, col < N; the block's 32 rows of A pass through LDS in
// chunks of 64 k.  arow: the row this thread stages (NULL: a row past R, zeros)
__device__ __forceinline__ void rnn_f32_product(float (&acc)[8], float (*sh)[64], const float* arow, const float* __restrict__ U,
                                                int ldu, int K, int N, int col, int wave) {
  const int lr = threadIdx.x >> 3, lk = (threadIdx.x & 7) * 8;
  for (int k0 = 0; k0 < K; k0 += 64) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) sh[lr][lk + e] = (arow != nullptr && k0 + lk + e < K) ? arow[k0 + lk + e] : 0.f;
    __syncthreads();
    const int kn = min(64, K - k0);
    if (col < N) {
      int kk = 0;
      for (; kk + 8 <= kn; kk += 8) {                          // eight rows of U in flight per lane, then their products
        float u[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) u[e] = U[(size_t)(k0 + kk + e) * ldu + col];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float4 a0 = *reinterpret_cast<const float4*>(&sh[wave * 8 + j][kk]);
          const float4 a1 = *reinterpret_cast<const float4*>(&sh[wave * 8 + j][kk + 4]);
          const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[j] = fmaf(a[e], u[e], acc[j]);       // (k ascending per output)
        }
      }
      for (; kk < kn; ++kk) {
        const float u = U[(size_t)(k0 + kk) * ldu + col];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(sh[wave * 8 + j][kk], u, acc[j]);
      }
    }
  }
}

template <int NT, typename Cell>
__device__ __forceinline__ void rnn_f32_tile(const Cell& cell, int R, int K, int N) {
  static_assert(NT == 1 || NT == 2, "one block of W, or the two of the GRU gates");
  __shared__ __align__(16) float sh[ATRF_BM][64];              // A[rows of the block][k chunk]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nct = gridDim.x / NT;
  const int t = NT == 2 && (int)blockIdx.x >= nct ? 1 : 0;     // block-uniform: the block of W this tile belongs to
  const int col = ((int)blockIdx.x - t * nct) * ATRF_BN + lane, r0 = blockIdx.y * ATRF_BM;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (cell.product()) {
    const int grow = r0 + (threadIdx.x >> 3);                  // the row this thread stages
    rnn_f32_product(acc, sh, grow < R ? cell.a_row(grow, true) : nullptr, cell.W + t * N, cell.ldw, K, N, col, wave);
  }
  if (col >= N) return;
  const float bias = cell.b[t * N + col];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = r0 + wave * 8 + j;
    if (row >= R) continue;
    cell(t, row, col, acc[j] + bias);
  }
}

template <int NT, typename Cell>
__device__ __forceinline__ void rnn_tile(const Cell& cell, int R, int K, int N, int vec_a) {
  if constexpr (std::is_same<typename Cell::st_t, float>::value) rnn_f32_tile<NT>(cell, R, K, N);
  else rnn_bf16_tile<NT>(cell, R, K, N, vec_a);
}

// ---------------------------------------------------------------- the four cells
// The kernels keep plain `__restrict__` parameters (the compiler's alias information hangs on them, not on struct members)
// and only fill their cell in.  out / out_copy with the mask carry of rnns/rnn.py:41-49, shared by the cells that end a step:
template <typename T>
struct RnnOut {
  const float* mask;
  int ldm;
  float* out;
  int ldo;
  T* out_copy;
  int ldc;
  __device__ __forceinline__ void put(int row, int col, float h, float hv) const {
    if (mask != nullptr) {
      const float m = mask[(size_t)row * ldm];
      h = m * h + (1.f - m) * hv;
    }
    out[(size_t)row * ldo + col] = h;
    if (out_copy != nullptr) rnn_store(out_copy, (size_t)row * ldc + col, h);
  }
};

// ATR (head of the file): q = h U + b, h' = sigmoid(p + q) p + sigmoid(p - q) h
template <typename T>
struct AtrCell {
  typedef T st_t;
  static constexpr bool STATE_A = true;
  RnnState s;
  const T* W;
  int ldw;
  const float* b;
  const T* p;
  int ldp;
  RnnOut<T> o;
  __device__ __forceinline__ bool product() const { return s.h_prev != nullptr; }
  __device__ __forceinline__ const float* a_row(int row, bool valid) const { return s.a_row(row, valid); }
  __device__ __forceinline__ void operator()(int, int row, int col, float q) const {
    const float hv = s.at(row, col);
    const float pv = rnn_load(p, (size_t)row * ldp + col);
    o.put(row, col, rnn_sigmoid(pv + q) * pv + rnn_sigmoid(pv - q) * hv, hv);
  }
};

template <typename T>
__global__ void __launch_bounds__(256) k_rnn_atr_step(const float* __restrict__ h_prev, int ldh, int n_prev,
                                                      const int* __restrict__ idx, const T* __restrict__ U, int ldu,
                                                      const float* __restrict__ b, const T* __restrict__ p, int ldp,
                                                      const float* __restrict__ mask, int ldm, float* __restrict__ out, int ldo,
                                                      T* __restrict__ out_copy, int ldc, int R, int H, int vec_a) {
  rnn_tile<1>(AtrCell<T>{{h_prev, ldh, n_prev, idx}, U, ldu, b, p, ldp, {mask, ldm, out, ldo, out_copy, ldc}}, R, H, H, vec_a);
}

// GRU step (rnns/gru.py:32-57), two launches
//     [z | r] = sigmoid(xg + h Ug + bg)        rh = r (.) h                               (zk_rnn_gru_gates)
//     c = tanh(xh + rh Uh + bh)                o = z h + (1 - z) c      out = m o + (1 - m) h   (zk_rnn_gru_out)
// The candidate product contracts r (.) h over ALL of K and r needs the gate product of every column, so the two products
// cannot share a launch without an exchange between workgroups: the launch boundary is that exchange.  The gates take the
// two blocks of Ug (NT = 2): block 0 forms z, block 1 r and rh.  In the bf16 form a workgroup owns 16 columns j AND the 16
// columns H + j (two accumulators per wave; LDS image [32][K + 8] bf16: 66 KB for H = 1000, and GRU_MAX_H = 2048, 129 KB of
// the 160 KB of a CU, is the largest H of the bf16 forms); in the fp32 form the grid is 2 x H / 64 column tiles -- the first
// half forms z, the second rh -- so twice as many CUs pull Ug as a paired tile would give.  rh is the MFMA operand of the
// second launch: formed from the fp32 state and rounded ONCE to the storage type.  z stays fp32; z h and the carry read the
// fp32 state in the second launch, so a carried row is the gathered state bit for bit.  The fp32 forms take any H.
template <typename T>
struct GruGatesCell {
  typedef T st_t;
  static constexpr bool STATE_A = true;
  RnnState s;
  const T* W;
  int ldw;
  const float* b;
  const T* xg;
  int ldx;
  float* z;
  int ldz;
  T* rh;
  int ldr, H;
  __device__ __forceinline__ bool product() const { return s.h_prev != nullptr; }
  __device__ __forceinline__ const float* a_row(int row, bool valid) const { return s.a_row(row, valid); }
  __device__ __forceinline__ void operator()(int t, int row, int col, float q) const {
    const float hv = t == 0 ? 0.f : s.at(row, col);             // (first: the gather is two dependent loads)
    const float g = rnn_sigmoid(rnn_load(xg, (size_t)row * ldx + t * H + col) + q);
    if (t == 0) z[(size_t)row * ldz + col] = g;
    else rnn_store(rh, (size_t)row * ldr + col, g * hv);
  }
};

template <typename T>
__global__ void __launch_bounds__(256) k_rnn_gru_gates(const float* __restrict__ h_prev, int ldh, int n_prev,
                                                       const int* __restrict__ idx, const T* __restrict__ Ug, int ldu,
                                                       const float* __restrict__ bg, const T* __restrict__ xg, int ldx,
                                                       float* __restrict__ z, int ldz, T* __restrict__ rh, int ldr, int R, int H,
                                                       int vec_a) {
  rnn_tile<2>(GruGatesCell<T>{{h_prev, ldh, n_prev, idx}, Ug, ldu, bg, xg, ldx, z, ldz, rh, ldr, H}, R, H, H, vec_a);
}

template <typename T>
struct GruOutCell {
  typedef T st_t;
  static constexpr bool STATE_A = false;
  RnnState s;
  const T* rh;
  int ldr;
  const T* W;
  int ldw;
  const float* b;
  const T* xh;
  int ldx;
  const float* z;
  int ldz;
  RnnOut<T> o;
  __device__ __forceinline__ bool product() const { return s.h_prev != nullptr; }         // (the zero state: rh = 0)
  __device__ __forceinline__ const T* a_row(int row, bool valid) const { return rh + (size_t)(valid ? row : 0) * ldr; }
  __device__ __forceinline__ void operator()(int, int row, int col, float q) const {
    const float hv = s.at(row, col);
    const float c = tanhf(rnn_load(xh, (size_t)row * ldx + col) + q);
    const float zv = z[(size_t)row * ldz + col];
    o.put(row, col, zv * hv + (1.f - zv) * c, hv);
  }
};

template <typename T>
__global__ void __launch_bounds__(256) k_rnn_gru_out(const T* __restrict__ rh, int ldr, const T* __restrict__ Uh, int ldu,
                                                     const float* __restrict__ bh, const T* __restrict__ xh, int ldx,
                                                     const float* __restrict__ z, int ldz, const float* __restrict__ h_prev,
                                                     int ldh, int n_prev, const int* __restrict__ idx,
                                                     const float* __restrict__ mask, int ldm, float* __restrict__ out, int ldo,
                                                     T* __restrict__ out_copy, int ldc, int R, int H, int vec_a) {
  rnn_tile<1>(GruOutCell<T>{{h_prev, ldh, n_prev, idx}, rh, ldr, Uh, ldu, bh, xh, ldx, z, ldz,
                            {mask, ldm, out, ldo, out_copy, ldc}}, R, H, H, vec_a);
}

// ff + residual of a deepnmt layer
// models/deepnmt.py:73-79 (encoder) and 166-172 (decoder): y = linear(outputs, embed_size, scope="ff"); x = x + y, with
// layer_norm off -- so NOTHING re-normalises x from the embedding to the last layer.  One launch:
//     out[r, :] = x[r, :] + (a[r, :] W + b)          out_copy = the same in the storage type (the next product's operand)
// The stream x / out is fp32 in BOTH forms for the reason the recurrent state is: a bf16 stream would drop every layer's
// update below half an ulp of x, and the loss would add up over the layers (6j has the same argument for
// transformer_fixup).  In the bf16 form only the MFMA operands a and W are bf16.  out may BE x (same address, same stride):
// an element is read and written by the one lane that owns it, and no lane reads another's.  No workgroup waits for another.
template <typename T>
struct FfCell {
  typedef T st_t;
  static constexpr bool STATE_A = false;
  const T* a;
  int lda;
  const T* W;
  int ldw;
  const float* b;
  const float* x;
  int ldx;
  RnnOut<T> o;
  __device__ __forceinline__ bool product() const { return true; }
  __device__ __forceinline__ const T* a_row(int row, bool valid) const { return a + (size_t)(valid ? row : 0) * lda; }
  __device__ __forceinline__ void operator()(int, int row, int col, float q) const {
    o.put(row, col, x[(size_t)row * ldx + col] + q, 0.f);
  }
};

template <typename T>
__global__ void __launch_bounds__(256) k_rnn_ff_residual(const T* __restrict__ a, int lda, const T* __restrict__ W, int ldw,
                                                         const float* __restrict__ b, const float* x, int ldx, float* out,
                                                         int ldo, T* __restrict__ out_copy, int ldc, int R, int K, int N,
                                                         int vec_a) {
  rnn_tile<1>(FfCell<T>{a, lda, W, ldw, b, x, ldx, {nullptr, 0, out, ldo, out_copy, ldc}}, R, K, N, vec_a);
}

template <typename Kern>
static int rnn_lds_attr(const char* name, Kern kern, size_t lds) {
  if (lds < 64 * 1024) return 0;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return zk_set_error((int)e, "%s: hipFuncSetAttribute: %s", name, hipGetErrorString(e));
  return 0;
}

// true when the byte ranges that ENCLOSE the rows of p ([rp, wp] elements of ep bytes, stride ldp) and of q meet.  Conservative:
// two column slices of one wider buffer share no element and are refused all the same (their operands differ in width and
// element size, which rnn_rows_overlap does not take); no caller lays a, out and out_copy out that way
static bool rnn_spans_meet(const void* p, long ldp, long rp, long wp, long ep, const void* q, long ldq, long rq, long wq, long eq) {
  if (p == nullptr || q == nullptr || rp <= 0 || rq <= 0) return false;
  const uintptr_t p0 = (uintptr_t)p, p1 = p0 + (uintptr_t)(((rp - 1) * ldp + wp) * ep);
  const uintptr_t q0 = (uintptr_t)q, q1 = q0 + (uintptr_t)(((rq - 1) * ldq + wq) * eq);
  return p0 < q1 && q0 < p1;
}

// ---------------------------------------------------------------- host side of the dense cells
// One launch function per cell, `F32` the form; the storage-type operands arrive as void pointers.
template <bool F32>
using rnn_st_t = typename std::conditional<F32, float, bf16_t>::type;

static int rnn_check_n_prev(const char* name, const RnnState& s, int R) {
  ZK_CHECK_ARG(s.h_prev == nullptr || (s.idx != nullptr ? s.n_prev >= 1 : s.n_prev >= R),
               "%s: h_prev has n_prev=%d rows (R=%d without an index, at least 1 with one)", name, s.n_prev, R);
  return 0;
}

// grid, LDS and launch of a cell kernel: NT blocks of N columns of W, K rows (the geometry at the two tile drivers)
template <bool F32, int NT, typename Kern, typename... Args>
static int rnn_cell_launch(const char* name, Kern kern, int R, int K, int N, hipStream_t stream, Args... args) {
  const size_t lds = F32 ? 0 : (size_t)NT * ATR_BN * ((K + 31) / 32 * 32 + 8) * sizeof(bf16_t);
  if (rnn_lds_attr(name, kern, lds) != 0) return -1;
  const dim3 grid = F32 ? dim3((unsigned)(NT * ((N + ATRF_BN - 1) / ATRF_BN)), (unsigned)((R + ATRF_BM - 1) / ATRF_BM))
                        : dim3((unsigned)((N + ATR_BN - 1) / ATR_BN), (unsigned)((R + ATR_BM - 1) / ATR_BM));
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, stream, args...);
  ZK_LAUNCH_CHECK();
  return 0;
}

// the 16-byte loads of the A operand: fp32 state rows (4 floats) or bf16 rows (8 elements); the fp32 form has none
static int rnn_vec_a(const void* a, int lda, int per16) { return a != nullptr && lda % per16 == 0 && (((uintptr_t)a) & 15) == 0; }

template <bool F32>
static int rnn_atr_launch(const char* name, RnnState s, const void* U, int ldu, const float* b, const void* p, int ldp,
                          const float* mask, int ldm, float* out, int ldo, void* out_copy, int ldc, int R, int H,
                          hipStream_t stream) {
  typedef rnn_st_t<F32> T;
  ZK_CHECK_ARG(U != nullptr && b != nullptr && p != nullptr && out != nullptr, "%s: U, b, p and out are required", name);
  ZK_CHECK_ARG(R >= 0 && H >= 1, "%s: bad shape (R=%d H=%d)", name, R, H);
  ZK_CHECK_ARG(ldu >= H && ldp >= H && ldo >= H && (out_copy == nullptr || ldc >= H) && (s.h_prev == nullptr || s.ldh >= H),
               "%s: a leading dimension is smaller than H=%d (ldh=%d ldu=%d ldp=%d ldo=%d ldc=%d)", name, H, s.ldh, ldu, ldp,
               ldo, ldc);
  if (rnn_check_n_prev(name, s, R) != 0) return -1;
  ZK_CHECK_ARG(mask == nullptr || ldm >= 1, "%s: the mask stride must be at least 1 (ldm=%d)", name, ldm);
  ZK_CHECK_ARG(!rnn_rows_overlap(out, ldo, R, s.h_prev, s.ldh, s.n_prev, H),
               "%s: out overlaps h_prev (every column tile reads whole rows of h_prev while others write out)", name);
  if (F32)
    ZK_CHECK_ARG(!rnn_rows_overlap(reinterpret_cast<const float*>(out_copy), ldc, R, s.h_prev, s.ldh, s.n_prev, H),
                 "%s: out_copy overlaps h_prev", name);
  else
    ZK_CHECK_ARG(H % 8 == 0 && H <= 4096 && ldu % 8 == 0 && (((uintptr_t)U) & 15) == 0,
                 "%s: the bf16 form needs H a multiple of 8 and at most 4096 and 16-byte aligned rows of U (H=%d ldu=%d); "
                 "zk_f32_rnn_atr_step takes any H", name, H, ldu);
  if (R == 0) return 0;
  return rnn_cell_launch<F32, 1>(name, k_rnn_atr_step<T>, R, H, H, stream, s.h_prev, s.ldh, s.n_prev, s.idx,
                                 reinterpret_cast<const T*>(U), ldu, b, reinterpret_cast<const T*>(p), ldp, mask, ldm, out, ldo,
                                 reinterpret_cast<T*>(out_copy), ldc, R, H, F32 ? 0 : rnn_vec_a(s.h_prev, s.ldh, 4));
}

// what the two GRU launches refuse alike; the bf16 forms name their fp32 twin (zk_f32_ + the name past its zk_)
static int gru_check_state(const char* name, const RnnState& s, int R, int H) {
  ZK_CHECK_ARG(R >= 0 && H >= 1, "%s: bad shape (R=%d H=%d)", name, R, H);
  ZK_CHECK_ARG(s.h_prev == nullptr || s.ldh >= H, "%s: ldh=%d is smaller than H=%d", name, s.ldh, H);
  return rnn_check_n_prev(name, s, R);
}

static int gru_check_bf16(const char* name, const void* U, int ldu, int H) {
  ZK_CHECK_ARG(H % 8 == 0 && H <= GRU_MAX_H && ldu % 8 == 0 && (((uintptr_t)U) & 15) == 0,
               "%s: the bf16 form needs H a multiple of 8 and at most %d (its LDS image of the recurrent matrix) and "
               "16-byte aligned rows of the matrix (H=%d ldu=%d); zk_f32_%s takes any H", name, GRU_MAX_H, H, ldu, name + 3);
  return 0;
}

template <bool F32>
static int rnn_gru_gates_launch(const char* name, RnnState s, const void* Ug, int ldu, const float* bg, const void* xg, int ldx,
                                float* z, int ldz, void* rh, int ldr, int R, int H, hipStream_t stream) {
  typedef rnn_st_t<F32> T;
  ZK_CHECK_ARG(Ug != nullptr && bg != nullptr && xg != nullptr && z != nullptr && rh != nullptr,
               "%s: Ug, bg, xg, z and rh are required", name);
  if (gru_check_state(name, s, R, H) != 0) return -1;
  ZK_CHECK_ARG(ldu >= 2 * H && ldx >= 2 * H && ldz >= H && ldr >= H,
               "%s: a leading dimension is too small for H=%d (ldu=%d and ldx=%d hold 2 H columns, ldz=%d ldr=%d)", name, H,
               ldu, ldx, ldz, ldr);
  ZK_CHECK_ARG(!rnn_rows_overlap(z, ldz, R, s.h_prev, s.ldh, s.n_prev, H),
               "%s: z overlaps h_prev (every column tile reads whole rows of h_prev while others write z)", name);
  if (F32)
    ZK_CHECK_ARG(!rnn_rows_overlap(reinterpret_cast<const float*>(rh), ldr, R, s.h_prev, s.ldh, s.n_prev, H),
                 "%s: rh overlaps h_prev", name);
  else if (gru_check_bf16(name, Ug, ldu, H) != 0)
    return -1;
  if (R == 0) return 0;
  return rnn_cell_launch<F32, 2>(name, k_rnn_gru_gates<T>, R, H, H, stream, s.h_prev, s.ldh, s.n_prev, s.idx,
                                 reinterpret_cast<const T*>(Ug), ldu, bg, reinterpret_cast<const T*>(xg), ldx, z, ldz,
                                 reinterpret_cast<T*>(rh), ldr, R, H, F32 ? 0 : rnn_vec_a(s.h_prev, s.ldh, 4));
}

template <bool F32>
static int rnn_gru_out_launch(const char* name, const void* rh, int ldr, const void* Uh, int ldu, const float* bh, const void* xh,
                              int ldx, const float* z, int ldz, RnnState s, const float* mask, int ldm, float* out, int ldo,
                              void* out_copy, int ldc, int R, int H, hipStream_t stream) {
  typedef rnn_st_t<F32> T;
  ZK_CHECK_ARG(rh != nullptr && Uh != nullptr && bh != nullptr && xh != nullptr && z != nullptr && out != nullptr,
               "%s: rh, Uh, bh, xh, z and out are required", name);
  if (gru_check_state(name, s, R, H) != 0) return -1;
  ZK_CHECK_ARG(ldr >= H && ldu >= H && ldx >= H && ldz >= H && ldo >= H && (out_copy == nullptr || ldc >= H),
               "%s: a leading dimension is smaller than H=%d (ldr=%d ldu=%d ldx=%d ldz=%d ldo=%d ldc=%d)", name, H, ldr, ldu,
               ldx, ldz, ldo, ldc);
  ZK_CHECK_ARG(mask == nullptr || ldm >= 1, "%s: the mask stride must be at least 1 (ldm=%d)", name, ldm);
  ZK_CHECK_ARG(!rnn_rows_overlap(out, ldo, R, s.h_prev, s.ldh, s.n_prev, H),
               "%s: out overlaps h_prev (a row of h_prev may be gathered by several rows while others write out)", name);
  ZK_CHECK_ARG(!rnn_rows_overlap(out, ldo, R, z, ldz, R, H), "%s: out overlaps z", name);
  if (F32) {
    const float* cp = reinterpret_cast<const float*>(out_copy);
    const float* rf = reinterpret_cast<const float*>(rh);
    ZK_CHECK_ARG(!rnn_rows_overlap(cp, ldc, R, s.h_prev, s.ldh, s.n_prev, H), "%s: out_copy overlaps h_prev", name);
    ZK_CHECK_ARG(!rnn_rows_overlap(out, ldo, R, rf, ldr, R, H) && !rnn_rows_overlap(cp, ldc, R, rf, ldr, R, H),
                 "%s: out or out_copy overlaps rh (every column tile reads whole rows of rh)", name);
  } else if (gru_check_bf16(name, Uh, ldu, H) != 0) {
    return -1;
  }
  if (R == 0) return 0;
  return rnn_cell_launch<F32, 1>(name, k_rnn_gru_out<T>, R, H, H, stream, reinterpret_cast<const T*>(rh), ldr,
                                 reinterpret_cast<const T*>(Uh), ldu, bh, reinterpret_cast<const T*>(xh), ldx, z, ldz, s.h_prev,
                                 s.ldh, s.n_prev, s.idx, mask, ldm, out, ldo, reinterpret_cast<T*>(out_copy), ldc, R, H,
                                 F32 ? 0 : rnn_vec_a(rh, ldr, 8));
}

template <bool F32>
static int rnn_ff_residual_launch(const char* name, const void* a, int lda, const void* W, int ldw, const float* b, const float* x,
                                  int ldx, float* out, int ldo, void* out_copy, int ldc, int R, int K, int N,
                                  hipStream_t stream) {
  typedef rnn_st_t<F32> T;
  const long esz = sizeof(T);                                  // bytes of an element of the storage type (a, W, out_copy)
  ZK_CHECK_ARG(a != nullptr && W != nullptr && b != nullptr && x != nullptr && out != nullptr,
               "%s: a, W, b, x and out are required", name);
  ZK_CHECK_ARG(R >= 0 && K >= 1 && N >= 1, "%s: bad shape (R=%d K=%d N=%d)", name, R, K, N);
  ZK_CHECK_ARG(lda >= K && ldw >= N && ldx >= N && ldo >= N && (out_copy == nullptr || ldc >= N),
               "%s: a leading dimension is too small for K=%d N=%d (lda=%d ldw=%d ldx=%d ldo=%d ldc=%d)", name, K, N, lda,
               ldw, ldx, ldo, ldc);
  ZK_CHECK_ARG((out == x && ldo == ldx) || !rnn_rows_overlap(out, ldo, R, x, ldx, R, N),
               "%s: out overlaps x without being x (in place needs the same address and the same stride: then every "
               "element is read and written by the one lane that owns it)", name);
  ZK_CHECK_ARG(!rnn_spans_meet(a, lda, R, K, esz, out, ldo, R, N, 4) &&
               !rnn_spans_meet(a, lda, R, K, esz, out_copy, ldc, R, N, esz),
               "%s: the span of out or out_copy meets the span of a (every column tile reads whole rows of a while "
               "others write; the check is by enclosing byte ranges: keep a in a buffer of its own)", name);
  ZK_CHECK_ARG(!rnn_spans_meet(out_copy, ldc, R, N, esz, out, ldo, R, N, 4) &&
               !rnn_spans_meet(out_copy, ldc, R, N, esz, x, ldx, R, N, 4),
               "%s: the span of out_copy meets the span of x or out (by enclosing byte ranges)", name);
  if (!F32) {
    ZK_CHECK_ARG(K % 8 == 0 && N % 8 == 0 && K <= 4096,
                 "%s: the bf16 form needs K and N multiples of 8 and K at most 4096 (its LDS image of 16 columns "
                 "of W: 131 KB there) -- got K=%d N=%d; zk_f32_rnn_ff_residual takes any K and N", name, K, N);
    ZK_CHECK_ARG(ldw % 8 == 0 && (((uintptr_t)W) & 15) == 0,
                 "%s: the bf16 form reads W 16 bytes at a time: its rows must be 16-byte aligned (ldw=%d, W %% 16 "
                 "= %d)", name, ldw, (int)(((uintptr_t)W) & 15));
  }
  if (R == 0) return 0;
  return rnn_cell_launch<F32, 1>(name, k_rnn_ff_residual<T>, R, K, N, stream, reinterpret_cast<const T*>(a), lda,
                                 reinterpret_cast<const T*>(W), ldw, b, x, ldx, out, ldo, reinterpret_cast<T*>(out_copy), ldc, R, K,
                                 N, F32 ? 0 : rnn_vec_a(a, lda, 8));
}

// ---------------------------------------------------------------- additive attention
#define ADD_RB 4          // beam rows per workgroup (1 when a sentence has a single row)
#define ADD_CC 8           // 256-channel chunks a thread accumulates: M <= 2048

template <bool F32, int NV>
__device__ __forceinline__ void add_load(const void* base, size_t elem, float (&f)[NV]) {
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
__device__ __forceinline__ float add_load1(const void* base, size_t elem) {
  return F32 ? reinterpret_cast<const float*>(base)[elem] : bf2f(reinterpret_cast<const bf16_t*>(base)[elem]);
}

template <bool F32, int NV, int RB>
__global__ void __launch_bounds__(256) k_add_attn(const void* __restrict__ qa, int ldq, const void* __restrict__ pm, int ldpm,
                                                  long bspm, const void* __restrict__ mem, int ldmem, long bsmem,
                                                  const float* __restrict__ v, const float* __restrict__ kmask, int ldmask,
                                                  float* __restrict__ ctx, int ldo, void* __restrict__ ctx_copy, int ldc,
                                                  int kv_group, int Ls, int M, float neg, int blocks_per_mem) {
  extern __shared__ float add_sm[];
  float* sq = add_sm;                               // [RB][M]: the projected queries
  float* sv = sq + (size_t)RB * M;                  // [M]: feed_logits/W_0_0
  float* sw = sv + M;                               // [RB][64]: logits, then weights of one key tile
  float* st = sw + RB * 64;                         // [3][RB]: running maximum, running sum, rescale factor of the tile
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int bk = blockIdx.x / blocks_per_mem;
  const int g0 = (blockIdx.x % blocks_per_mem) * RB;
  const int nrows = min(RB, kv_group - g0);
  for (int r = 0; r < RB; ++r) {
    const size_t row = (size_t)(bk * kv_group + g0 + r) * ldq;
    for (int c = threadIdx.x; c < M; c += 256) sq[r * M + c] = r < nrows ? add_load1<F32>(qa, row + c) : 0.f;
  }
  for (int c = threadIdx.x; c < M; c += 256) sv[c] = v[c];
  if (threadIdx.x < RB) {
    st[threadIdx.x] = -FLT_MAX;
    st[RB + threadIdx.x] = 0.f;
    st[2 * RB + threadIdx.x] = 0.f;
  }
  __syncthreads();

  float acc[RB][ADD_CC];
#pragma unroll
  for (int r = 0; r < RB; ++r)
#pragma unroll
    for (int cc = 0; cc < ADD_CC; ++cc) acc[r][cc] = 0.f;

  for (int j0 = 0; j0 < Ls; j0 += 64) {             // (uniform trip counts: every wave meets every barrier)
    for (int jj = 0; jj < 16; ++jj) {
      const int slot = wave * 16 + jj, j = j0 + slot;
      float s[RB];
#pragma unroll
      for (int r = 0; r < RB; ++r) s[r] = -FLT_MAX;
      if (j < Ls) {                                 // wave-uniform: the reductions run with all 64 lanes
#pragma unroll
        for (int r = 0; r < RB; ++r) s[r] = 0.f;
        const size_t krow = (size_t)bk * bspm + (size_t)j * ldpm;
        for (int c = lane * NV; c < M; c += 64 * NV) {
          float pf[NV];
          add_load<F32, NV>(pm, krow + c, pf);
#pragma unroll
          for (int e = 0; e < NV; ++e) {
            const float vv = sv[c + e];
#pragma unroll
            for (int r = 0; r < RB; ++r) s[r] = fmaf(vv, tanhf(sq[r * M + c + e] + pf[e]), s[r]);
          }
        }
        const float madd = kmask != nullptr ? (1.f - kmask[(size_t)bk * ldmask + j]) * -neg : 0.f;
#pragma unroll
        for (int r = 0; r < RB; ++r) s[r] = wave_sum(s[r]) + madd;
      }
      if (lane == 0) {
#pragma unroll
        for (int r = 0; r < RB; ++r) sw[r * 64 + slot] = s[r];
      }
    }
    __syncthreads();
    if (wave < RB) {                                // wave r owns row r of the block
      const float s = sw[wave * 64 + lane];
      const bool valid = j0 + lane < Ls;
      const float m_old = st[wave];
      const float m_new = fmaxf(m_old, wave_max(s));
      const float pj = valid ? expf(s - m_new) : 0.f;
      const float psum = wave_sum(pj);
      const float alpha = expf(m_old - m_new);      // (the first tile: exp(-FLT_MAX - m) = 0 scales the empty sums)
      const float l_old = st[RB + wave];
      sw[wave * 64 + lane] = pj;
      if (lane == 0) {
        st[wave] = m_new;
        st[RB + wave] = l_old * alpha + psum;
        st[2 * RB + wave] = alpha;
      }
    }
    __syncthreads();
    const int jn = min(64, Ls - j0);
#pragma unroll
    for (int cc = 0; cc < ADD_CC; ++cc) {
      const int c = cc * 256 + threadIdx.x;
      if (c < M) {
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r][cc] *= st[2 * RB + r];
        const size_t mcol = (size_t)bk * bsmem + c;
        for (int jj = 0; jj < jn; ++jj) {
          const float mf = add_load1<F32>(mem, mcol + (size_t)(j0 + jj) * ldmem);
#pragma unroll
          for (int r = 0; r < RB; ++r) acc[r][cc] = fmaf(sw[r * 64 + jj], mf, acc[r][cc]);
        }
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int r = 0; r < RB; ++r) {
    if (r >= nrows) continue;
    const float inv = 1.f / st[RB + r];
    const size_t row = (size_t)(bk * kv_group + g0 + r);
#pragma unroll
    for (int cc = 0; cc < ADD_CC; ++cc) {
      const int c = cc * 256 + threadIdx.x;
      if (c < M) {
        const float o = acc[r][cc] * inv;
        ctx[row * ldo + c] = o;
        if (ctx_copy != nullptr) {
          if (F32) reinterpret_cast<float*>(ctx_copy)[row * ldc + c] = o;
          else reinterpret_cast<bf16_t*>(ctx_copy)[row * ldc + c] = f2bf(o);
        }
      }
    }
  }
}

template <bool F32, int NV>
static int add_attn_launch(const void* qa, int ldq, const void* pm, int ldpm, long bspm, const void* mem, int ldmem, long bsmem,
                           const float* v, const float* kmask, int ldmask, float* ctx, int ldo, void* ctx_copy, int ldc, int R,
                           int kv_group, int Ls, int M, float neg, hipStream_t stream) {
  const int rb = kv_group > 1 ? ADD_RB : 1;
  const size_t lds = ((size_t)rb * M + M + rb * 64 + 3 * rb) * sizeof(float);
  const long per_mem = (kv_group + rb - 1) / rb;
  const long blocks = (long)(R / kv_group) * per_mem;
  if (blocks > 0x7fffffffL) return zk_set_error(-1, "zk_add_attn: %ld workgroups exceed the grid", blocks);
  if (rb == 1)
    hipLaunchKernelGGL((k_add_attn<F32, NV, 1>), dim3((unsigned)blocks), dim3(256), lds, stream, qa, ldq, pm, ldpm, bspm, mem,
                       ldmem, bsmem, v, kmask, ldmask, ctx, ldo, ctx_copy, ldc, kv_group, Ls, M, neg, (int)per_mem);
  else
    hipLaunchKernelGGL((k_add_attn<F32, NV, ADD_RB>), dim3((unsigned)blocks), dim3(256), lds, stream, qa, ldq, pm, ldpm, bspm,
                       mem, ldmem, bsmem, v, kmask, ldmask, ctx, ldo, ctx_copy, ldc, kv_group, Ls, M, neg, (int)per_mem);
  ZK_LAUNCH_CHECK();
  return 0;
}

#define ADD_CHECK_COMMON(NAME)                                                                                              \
  ZK_CHECK_ARG(qa != nullptr && pm != nullptr && mem != nullptr && v != nullptr && ctx != nullptr,                          \
               NAME ": qa, pm, mem, v and ctx are required");                                                               \
  ZK_CHECK_ARG(R >= 0 && kv_group >= 1 && R % kv_group == 0 && Ls >= 1 && M >= 1 && M <= 256 * ADD_CC,                      \
               NAME ": bad shape (R=%d kv_group=%d Ls=%d M=%d; R must be a multiple of kv_group, M at most %d)", R,         \
               kv_group, Ls, M, 256 * ADD_CC);                                                                              \
  ZK_CHECK_ARG(kmask == nullptr || ldmask >= Ls, NAME ": mask rows of ldmask=%d elements are shorter than Ls=%d", ldmask,   \
               Ls);                                                                                                         \
  ZK_CHECK_ARG(ldq >= M && ldpm >= M && ldmem >= M && ldo >= M && (ctx_copy == nullptr || ldc >= M),                        \
               NAME ": a leading dimension is smaller than M=%d (ldq=%d ldpm=%d ldmem=%d ldo=%d ldc=%d)", M, ldq, ldpm,     \
               ldmem, ldo, ldc)

// ---------------------------------------------------------------- row-local launches
// out[r] = table[ids[r]] + bias, or zeros where EVERY id of the launch equals pad (models/rnnsearch.py:101-103); pad < 0:
// no such rule (the encoder input, rnnsearch.py:28-29).  No sqrt(H) scale, no timing signal.  An id outside [0, V) is
// clamped: a negative id reads row 0, an id >= V reads row V - 1.
template <bool F32>
__global__ void __launch_bounds__(256) k_rnn_embed(const int* __restrict__ ids, int rows, const void* __restrict__ table,
                                                   int V, const float* __restrict__ bias, void* __restrict__ out, int ldo, int E,
                                                   int pad) {
  int other = 0;
  if (pad >= 0)
    for (int i = threadIdx.x; i < rows; i += 256) other |= ids[i] != pad;
  const bool zero = pad >= 0 && !__syncthreads_or(other);
  const int r = blockIdx.x;
  const int id = min(max(ids[r], 0), V - 1);
  for (int c = threadIdx.x; c < E; c += 256) {
    const float x = zero ? 0.f : add_load1<F32>(table, (size_t)id * E + c) + bias[c];
    if (F32) reinterpret_cast<float*>(out)[(size_t)r * ldo + c] = x;
    else reinterpret_cast<bf16_t*>(out)[(size_t)r * ldo + c] = f2bf(x);
  }
}

// y = tanh(x + bias) for fp32 rows x (a GEMM's fp32 output); input row r goes to the output rows r rep .. r rep + rep - 1
// (the beam tiling of decoder_initializer); out_f32 and / or out_copy (storage type)
template <bool F32>
__global__ void __launch_bounds__(256) k_rnn_bias_tanh(const float* __restrict__ x, int ldx, const float* __restrict__ bias,
                                                       float* __restrict__ out_f32, int ldo, void* __restrict__ out_copy, int ldc,
                                                       int cols, int rep) {
  const int r = blockIdx.x;
  for (int c = threadIdx.x; c < cols; c += 256) {
    const float y = tanhf(x[(size_t)r * ldx + c] + (bias != nullptr ? bias[c] : 0.f));
    for (int k = 0; k < rep; ++k) {
      const size_t ro = (size_t)r * rep + k;
      if (out_f32 != nullptr) out_f32[ro * ldo + c] = y;
      if (out_copy != nullptr) {
        if (F32) reinterpret_cast<float*>(out_copy)[ro * ldc + c] = y;
        else reinterpret_cast<bf16_t*>(out_copy)[ro * ldc + c] = f2bf(y);
      }
    }
  }
}

template <bool F32>
static int rnn_embed_launch(const char* name, const int* ids, int rows, const void* table, int V, const float* bias, void* out,
                            int ldo, int E, int pad, hipStream_t stream) {
  if (!(ids != nullptr && table != nullptr && bias != nullptr && out != nullptr))
    return zk_set_error(-1, "%s: ids, table, bias and out are required", name);
  if (!(rows >= 0 && V >= 1 && E >= 1 && ldo >= E)) return zk_set_error(-1, "%s: bad shape (rows=%d V=%d E=%d ldo=%d)", name, rows, V, E, ldo);
  if (rows == 0) return 0;
  hipLaunchKernelGGL(k_rnn_embed<F32>, dim3((unsigned)rows), dim3(256), 0, stream, ids, rows, table, V, bias, out, ldo, E, pad);
  ZK_LAUNCH_CHECK();
  return 0;
}

template <bool F32>
static int rnn_bias_tanh_launch(const char* name, const float* x, int ldx, const float* bias, float* out_f32, int ldo,
                                void* out_copy, int ldc, int rows, int cols, int rep, hipStream_t stream) {
  if (!(x != nullptr && (out_f32 != nullptr || out_copy != nullptr))) return zk_set_error(-1, "%s: x and an output are required", name);
  if (!(rows >= 0 && cols >= 1 && rep >= 1 && ldx >= cols && (out_f32 == nullptr || ldo >= cols) &&
        (out_copy == nullptr || ldc >= cols)))
    return zk_set_error(-1, "%s: bad shape (rows=%d cols=%d rep=%d ldx=%d ldo=%d ldc=%d)", name, rows, cols, rep, ldx, ldo, ldc);
  if (rows == 0) return 0;
  hipLaunchKernelGGL(k_rnn_bias_tanh<F32>, dim3((unsigned)rows), dim3(256), 0, stream, x, ldx, bias, out_f32, ldo, out_copy, ldc,
                     cols, rep);
  ZK_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- LRN / OLRN scans (rnns/lrn.py:32-53, rnns/olrn.py:32-58)
// These cells have NO recurrent product: the input projection [p | q | r (| s)] = x W of the whole sequence is one GEMM and
// the recurrence is element-wise per channel,
//     u = sigmoid(p + h_) r + sigmoid(q - h_) h_            cell = u  (lrn)      cell = u sigmoid(s - u)  (olrn, `gated`)
// so T time steps of one cell -- or of a lower / higher pair, cond_rnn(one2one=True), rnns/rnn.py:119-146 -- are ONE launch:
//     single:  h = carry(m_t, cell(h, lo_t), h)
//     paired:  s = carry(m_t, cell(h, lo_t), h);   h = carry(m_t, cell(s, hi_t), s)          carry(m, a, b) = m a + (1 - m) b
// for t = 0 .. T-1, or T-1 .. 0 with `reverse` (positions stay where they are in memory).  A thread owns ONE row and one
// 16-byte group of channels (8 in the bf16 form, 4 in the fp32 form) and walks the time axis with the state in registers; a
// workgroup is one wave, so the R H / 8 threads of a scan spread over as many CUs as there are waves (32 rows x 512 channels:
// 32 waves) -- the scan is a latency chain per thread, not a throughput problem, and nothing is shared between threads.
// The operands of the positions after t do not depend on the state: they sit in a register ring of LRN_PD stages of raw
// 16-byte vectors (3 or 4 per cell, and the mask word), each refilled as soon as its arithmetic is done, so the loads of the
// next LRN_PD - 1 positions are in flight under the arithmetic of this one (counted vmcnt waits: loads return in order).  The
// state is fp32 in BOTH forms; only the reads of lo / hi and the writes of seq are of the storage type.  Every product and
// sum is rounded on its own (`#pragma clang fp contract(off)` in the cell: the loop body exists in LRN_PD unrolled copies,
// and the compiler, where it may, fuses a product into an add in some copies and not in others), so a T-step launch equals T
// chained one-step launches bit for bit and the tests' bound can be derived term by term.  A position with m = 0 leaves the
// state untouched bit for bit.
#define LRN_PD 4          // stages of the operand ring: LRN_PD - 1 positions in flight under the arithmetic of one

template <bool F32, int NV>
__device__ __forceinline__ void lrn_unpack(const uint4& v, float (&f)[NV]) {
  if constexpr (F32) {
    f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y); f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
  } else {
    unpack8(v, f);
  }
}

// one cell on the NV channels of a thread: h <- carry(m, cell(h, [p | q | r (| s)]), h)
template <bool F32, bool GATED, int NV>
__device__ __forceinline__ void lrn_cell(float (&h)[NV], const uint4 (&in)[4], float m, bool has_mask) {
#pragma clang fp contract(off)      // every product and sum below is rounded on its own, in every unrolled copy of the loop body
  float p[NV], q[NV], r[NV], s[NV];
  lrn_unpack<F32, NV>(in[0], p);
  lrn_unpack<F32, NV>(in[1], q);
  lrn_unpack<F32, NV>(in[2], r);
  if constexpr (GATED) lrn_unpack<F32, NV>(in[3], s);
  const bool carried = has_mask && m == 0.f;                    // the state bit for bit (a select: no branch in the scan loop)
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    const float hv = h[e];
    const float i = rnn_sigmoid(p[e] + hv);
    const float f = rnn_sigmoid(q[e] - hv);
    float u = i * r[e] + f * hv;
    if constexpr (GATED) u = u * rnn_sigmoid(s[e] - u);
    if (has_mask) u = m * u + (1.f - m) * hv;
    h[e] = carried ? hv : u;
  }
}

struct LrnStage {
  uint4 lo[4], hi[4];
  float m;
};

template <bool F32, bool PAIRED, bool GATED>
__global__ void __launch_bounds__(64) k_rnn_lrn_scan(const float* __restrict__ h_prev, int ldh, int n_prev,
                                                     const int* __restrict__ idx, const void* __restrict__ lo, long lo_ps,
                                                     long lo_rs, const void* __restrict__ hi, long hi_ps, long hi_rs,
                                                     const float* __restrict__ mask, long m_ps, long m_rs,
                                                     float* __restrict__ out, int ldo, void* __restrict__ seq, long sq_ps,
                                                     long sq_rs, int R, int H, int T, int reverse, int vec_h, int vec_o) {
  constexpr int NV = F32 ? 4 : 8, NG = GATED ? 4 : 3;
  typedef typename std::conditional<F32, float, bf16_t>::type st_t;
  const int groups = H / NV;
  const long gid = (long)blockIdx.x * 64 + threadIdx.x;
  if (gid >= (long)R * groups) return;
  const int row = (int)(gid / groups), c0 = (int)(gid % groups) * NV;
  const st_t* plo = reinterpret_cast<const st_t*>(lo) + (size_t)row * lo_rs + c0;
  const st_t* phi = PAIRED ? reinterpret_cast<const st_t*>(hi) + (size_t)row * hi_rs + c0 : nullptr;
  // (the loop below has no branch around a load, so that the waits are counted: without a mask the thread reads a word of its
  // own lo operand in its place and drops it)
  const bool has_mask = mask != nullptr;
  const float* pm = has_mask ? mask + (size_t)row * m_rs : reinterpret_cast<const float*>(plo);
  const long mps = has_mask ? m_ps : 0;

  auto fetch = [&](LrnStage& s, int n) {                        // the operands of the n-th scanned position (n clamped)
    n = min(n, T - 1);
    const long t = reverse ? T - 1 - n : n;
#pragma unroll
    for (int g = 0; g < NG; ++g) s.lo[g] = *reinterpret_cast<const uint4*>(plo + t * lo_ps + (size_t)g * H);
    if constexpr (PAIRED) {
#pragma unroll
      for (int g = 0; g < NG; ++g) s.hi[g] = *reinterpret_cast<const uint4*>(phi + t * hi_ps + (size_t)g * H);
    }
    s.m = pm[t * mps];
  };

  LrnStage ring[LRN_PD];

  float h[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) h[e] = 0.f;
  if (h_prev != nullptr) {
    const int src = min(max(idx != nullptr ? idx[row] : row, 0), n_prev - 1);
    const float* hp = h_prev + (size_t)src * ldh + c0;
    if (vec_h) {
#pragma unroll
      for (int e = 0; e < NV; e += 4) {
        const float4 v = *reinterpret_cast<const float4*>(hp + e);
        h[e] = v.x; h[e + 1] = v.y; h[e + 2] = v.z; h[e + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < NV; ++e) h[e] = hp[e];
    }
  }

  st_t* pseq = seq != nullptr ? reinterpret_cast<st_t*>(seq) + (size_t)row * sq_rs + c0 : nullptr;
  // (the state has arrived before the loop: a load still pending at its head would be waited for in every trip)
#pragma unroll
  for (int e = 0; e < NV; ++e) asm volatile("" : "+v"(h[e]));
  // unrolled by the ring: a stage is a fixed set of registers.  The first trip (n0 = -LRN_PD) only fills the ring, so every
  // load of the ring is issued from ONE place in the loop and the compiler's wait counts are exact at the loop's head
  for (int n0 = -LRN_PD; n0 < T; n0 += LRN_PD) {
#pragma unroll
    for (int k = 0; k < LRN_PD; ++k) {
      const int n = n0 + k;
      if (n0 >= 0 && n < T) {                                   // (uniform; no load inside)
        lrn_cell<F32, GATED, NV>(h, ring[k].lo, ring[k].m, has_mask);
        if constexpr (PAIRED) lrn_cell<F32, GATED, NV>(h, ring[k].hi, ring[k].m, has_mask);
        if (pseq != nullptr) {
          const long t = reverse ? T - 1 - n : n;
          if constexpr (F32) *reinterpret_cast<float4*>(pseq + t * sq_ps) = make_float4(h[0], h[1], h[2], h[3]);
          else *reinterpret_cast<uint4*>(pseq + t * sq_ps) = pack8(h);
        }
      }
      // refill the stage its arithmetic has just freed, into the SAME registers (no copies at the loop's back edge, which
      // would wait for every load): consumed LRN_PD positions on, under the arithmetic of LRN_PD - 1.  Past the end: the
      // last position again, dropped
      fetch(ring[k], n + LRN_PD);
    }
  }

  float* po = out + (size_t)row * ldo + c0;
  if (vec_o) {
#pragma unroll
    for (int e = 0; e < NV; e += 4) *reinterpret_cast<float4*>(po + e) = make_float4(h[e], h[e + 1], h[e + 2], h[e + 3]);
  } else {
#pragma unroll
    for (int e = 0; e < NV; ++e) po[e] = h[e];
  }
}

template <bool F32>
static int lrn_scan_launch(const char* name, const char* other, const float* h_prev, int ldh, int n_prev, const int* idx,
                           const void* lo, long lo_ps, long lo_rs, const void* hi, long hi_ps, long hi_rs, const float* mask,
                           long m_ps, long m_rs, float* out, int ldo, void* seq, long sq_ps, long sq_rs, int R, int H, int T,
                           int reverse, int gated, hipStream_t stream) {
  const int NV = F32 ? 4 : 8, esz = F32 ? 4 : 2;
  const long W = (long)(gated ? 4 : 3) * H;
  if (!(lo != nullptr && out != nullptr)) return zk_set_error(-1, "%s: lo and out are required", name);
  if (T < 1) return zk_set_error(-1, "%s: a scan has at least one position (T=%d)", name, T);
  if (!(R >= 0 && H >= 1)) return zk_set_error(-1, "%s: bad shape (R=%d H=%d)", name, R, H);
  if (H % NV != 0) {
    if (F32) return zk_set_error(-1, "%s: the fp32 form needs H a multiple of 4 (H=%d): a thread owns 16 bytes of channels", name, H);
    return zk_set_error(-1, "%s: the bf16 form needs H a multiple of 8 (H=%d): a thread owns 16 bytes of channels; %s takes "
                        "multiples of 4", name, H, other);
  }
  const bool al = (((uintptr_t)lo) & 15) == 0 && lo_ps % NV == 0 && lo_rs % NV == 0 &&
                  (hi == nullptr || ((((uintptr_t)hi) & 15) == 0 && hi_ps % NV == 0 && hi_rs % NV == 0)) &&
                  (seq == nullptr || ((((uintptr_t)seq) & 15) == 0 && sq_ps % NV == 0 && sq_rs % NV == 0));
  if (!al) {
    if (F32) return zk_set_error(-1, "%s: lo, hi and seq are read and written 16 bytes at a time: their bases must be 16-byte "
                                 "aligned and their strides multiples of 4 elements", name);
    return zk_set_error(-1, "%s: the bf16 form reads lo / hi and writes seq 16 bytes at a time: unaligned rows (bases must be "
                        "16-byte aligned, strides multiples of 8 elements); %s takes strides that are multiples of 4", name, other);
  }
  if (!(lo_ps >= 0 && lo_rs >= 0 && hi_ps >= 0 && hi_rs >= 0 && sq_ps >= 0 && sq_rs >= 0 && m_ps >= 0 && m_rs >= 0))
    return zk_set_error(-1, "%s: strides must not be negative (reverse walks the positions backwards)", name);
  if (!(ldo >= H && (h_prev == nullptr || ldh >= H))) return zk_set_error(-1, "%s: ldo=%d or ldh=%d is smaller than H=%d", name, ldo, ldh, H);
  if (!(h_prev == nullptr || (idx != nullptr ? n_prev >= 1 : n_prev >= R)))
    return zk_set_error(-1, "%s: h_prev has n_prev=%d rows (R=%d without an index, at least 1 with one)", name, n_prev, R);
  if (rnn_rows_overlap(out, ldo, R, h_prev, ldh, n_prev, H))
    return zk_set_error(-1, "%s: out overlaps h_prev (a row of h_prev may be gathered by several rows while others write out)", name);
  if (seq != nullptr) {
    const long sw = (T - 1) * sq_ps + H;                        // a "row" of the span: the T positions of one sentence row
    if (rnn_spans_meet(seq, sq_rs, R, sw, esz, lo, lo_rs, R, (T - 1) * lo_ps + W, esz) ||
        rnn_spans_meet(seq, sq_rs, R, sw, esz, hi, hi_rs, R, (T - 1) * hi_ps + W, esz))
      return zk_set_error(-1, "%s: seq overlaps lo / hi (by enclosing byte ranges: later positions are read while earlier "
                          "ones are written)", name);
    if (rnn_spans_meet(seq, sq_rs, R, sw, esz, h_prev, ldh, n_prev, H, 4) || rnn_spans_meet(seq, sq_rs, R, sw, esz, out, ldo, R, H, 4))
      return zk_set_error(-1, "%s: seq overlaps h_prev or out (by enclosing byte ranges)", name);
  }
  if (R == 0) return 0;
  const long threads = (long)R * (H / NV), blocks = (threads + 63) / 64;
  if (blocks > 0x7fffffffL) return zk_set_error(-1, "%s: %ld workgroups exceed the grid", name, blocks);
  const int vec_h = h_prev != nullptr && ldh % 4 == 0 && (((uintptr_t)h_prev) & 15) == 0;
  const int vec_o = ldo % 4 == 0 && (((uintptr_t)out) & 15) == 0;
#define LRN_LAUNCH(P, G)                                                                                                    \
  hipLaunchKernelGGL((k_rnn_lrn_scan<F32, P, G>), dim3((unsigned)blocks), dim3(64), 0, stream, h_prev, ldh, n_prev, idx, lo,  \
                     lo_ps, lo_rs, hi, hi_ps, hi_rs, mask, m_ps, m_rs, out, ldo, seq, sq_ps, sq_rs, R, H, T, reverse ? 1 : 0, \
                     vec_h, vec_o)
  if (hi != nullptr) {
    if (gated) LRN_LAUNCH(true, true); else LRN_LAUNCH(true, false);
  } else {
    if (gated) LRN_LAUNCH(false, true); else LRN_LAUNCH(false, false);
  }
#undef LRN_LAUNCH
  ZK_LAUNCH_CHECK();
  return 0;
}

extern "C" {

int zk_rnn_atr_step(const float* h_prev, int ldh, int n_prev, const int* idx, const void* U, int ldu, const float* b,
                    const void* p, int ldp, const float* mask, int ldm, float* out, int ldo, void* out_copy, int ldc, int R,
                    int H, hipStream_t stream) {
  return rnn_atr_launch<false>("zk_rnn_atr_step", {h_prev, ldh, n_prev, idx}, U, ldu, b, p, ldp, mask, ldm, out, ldo, out_copy,
                               ldc, R, H, stream);
}

int zk_f32_rnn_atr_step(const float* h_prev, int ldh, int n_prev, const int* idx, const float* U, int ldu, const float* b,
                        const float* p, int ldp, const float* mask, int ldm, float* out, int ldo, float* out_copy, int ldc,
                        int R, int H, hipStream_t stream) {
  return rnn_atr_launch<true>("zk_f32_rnn_atr_step", {h_prev, ldh, n_prev, idx}, U, ldu, b, p, ldp, mask, ldm, out, ldo,
                              out_copy, ldc, R, H, stream);
}

int zk_rnn_gru_gates(const float* h_prev, int ldh, int n_prev, const int* idx, const void* Ug, int ldu, const float* bg,
                     const void* xg, int ldx, float* z, int ldz, void* rh, int ldr, int R, int H, hipStream_t stream) {
  return rnn_gru_gates_launch<false>("zk_rnn_gru_gates", {h_prev, ldh, n_prev, idx}, Ug, ldu, bg, xg, ldx, z, ldz, rh, ldr, R, H,
                                     stream);
}

int zk_f32_rnn_gru_gates(const float* h_prev, int ldh, int n_prev, const int* idx, const float* Ug, int ldu, const float* bg,
                         const float* xg, int ldx, float* z, int ldz, float* rh, int ldr, int R, int H, hipStream_t stream) {
  return rnn_gru_gates_launch<true>("zk_f32_rnn_gru_gates", {h_prev, ldh, n_prev, idx}, Ug, ldu, bg, xg, ldx, z, ldz, rh, ldr, R,
                                    H, stream);
}

int zk_rnn_gru_out(const void* rh, int ldr, const void* Uh, int ldu, const float* bh, const void* xh, int ldx, const float* z,
                   int ldz, const float* h_prev, int ldh, int n_prev, const int* idx, const float* mask, int ldm, float* out,
                   int ldo, void* out_copy, int ldc, int R, int H, hipStream_t stream) {
  return rnn_gru_out_launch<false>("zk_rnn_gru_out", rh, ldr, Uh, ldu, bh, xh, ldx, z, ldz, {h_prev, ldh, n_prev, idx}, mask, ldm,
                                   out, ldo, out_copy, ldc, R, H, stream);
}

int zk_f32_rnn_gru_out(const float* rh, int ldr, const float* Uh, int ldu, const float* bh, const float* xh, int ldx,
                       const float* z, int ldz, const float* h_prev, int ldh, int n_prev, const int* idx, const float* mask,
                       int ldm, float* out, int ldo, float* out_copy, int ldc, int R, int H, hipStream_t stream) {
  return rnn_gru_out_launch<true>("zk_f32_rnn_gru_out", rh, ldr, Uh, ldu, bh, xh, ldx, z, ldz, {h_prev, ldh, n_prev, idx}, mask,
                                  ldm, out, ldo, out_copy, ldc, R, H, stream);
}

int zk_rnn_ff_residual(const void* a, int lda, const void* W, int ldw, const float* b, const float* x, int ldx, float* out,
                       int ldo, void* out_copy, int ldc, int R, int K, int N, hipStream_t stream) {
  return rnn_ff_residual_launch<false>("zk_rnn_ff_residual", a, lda, W, ldw, b, x, ldx, out, ldo, out_copy, ldc, R, K, N, stream);
}

int zk_f32_rnn_ff_residual(const float* a, int lda, const float* W, int ldw, const float* b, const float* x, int ldx, float* out,
                           int ldo, float* out_copy, int ldc, int R, int K, int N, hipStream_t stream) {
  return rnn_ff_residual_launch<true>("zk_f32_rnn_ff_residual", a, lda, W, ldw, b, x, ldx, out, ldo, out_copy, ldc, R, K, N,
                                      stream);
}

int zk_add_attn(const void* qa, int ldq, const void* pm, int ldpm, long bspm, const void* mem, int ldmem, long bsmem,
                const float* v, const float* kmask, int ldmask, float* ctx, int ldo, void* ctx_copy, int ldc, int R,
                int kv_group, int Ls, int M, float neg, hipStream_t stream) {
  ADD_CHECK_COMMON("zk_add_attn");
  ZK_CHECK_ARG(M % 8 == 0 && ldpm % 8 == 0 && bspm % 8 == 0 && (((uintptr_t)pm) & 15) == 0,
               "zk_add_attn: the bf16 form reads the projected memory 16 bytes at a time: M, ldpm and bspm multiples of 8 and "
               "an aligned pm (M=%d ldpm=%d bspm=%ld); zk_f32_add_attn takes any M", M, ldpm, bspm);
  if (R == 0) return 0;
  return add_attn_launch<false, 8>(qa, ldq, pm, ldpm, bspm, mem, ldmem, bsmem, v, kmask, ldmask, ctx, ldo, ctx_copy, ldc, R,
                                   kv_group, Ls, M, neg, stream);
}

int zk_f32_add_attn(const float* qa, int ldq, const float* pm, int ldpm, long bspm, const float* mem, int ldmem, long bsmem,
                    const float* v, const float* kmask, int ldmask, float* ctx, int ldo, float* ctx_copy, int ldc, int R,
                    int kv_group, int Ls, int M, float neg, hipStream_t stream) {
  ADD_CHECK_COMMON("zk_f32_add_attn");
  if (R == 0) return 0;
  const bool vec = M % 4 == 0 && ldpm % 4 == 0 && bspm % 4 == 0 && (((uintptr_t)pm) & 15) == 0;
  if (vec)
    return add_attn_launch<true, 4>(qa, ldq, pm, ldpm, bspm, mem, ldmem, bsmem, v, kmask, ldmask, ctx, ldo, ctx_copy, ldc, R,
                                    kv_group, Ls, M, neg, stream);
  return add_attn_launch<true, 1>(qa, ldq, pm, ldpm, bspm, mem, ldmem, bsmem, v, kmask, ldmask, ctx, ldo, ctx_copy, ldc, R,
                                  kv_group, Ls, M, neg, stream);
}

int zk_rnn_embed(const int* ids, int rows, const void* table, int V, const float* bias, void* out, int ldo, int E, int pad,
                 hipStream_t stream) {
  return rnn_embed_launch<false>("zk_rnn_embed", ids, rows, table, V, bias, out, ldo, E, pad, stream);
}

int zk_f32_rnn_embed(const int* ids, int rows, const float* table, int V, const float* bias, float* out, int ldo, int E,
                     int pad, hipStream_t stream) {
  return rnn_embed_launch<true>("zk_f32_rnn_embed", ids, rows, table, V, bias, out, ldo, E, pad, stream);
}

int zk_rnn_bias_tanh(const float* x, int ldx, const float* bias, float* out_f32, int ldo, void* out_copy, int ldc, int rows,
                     int cols, int rep, hipStream_t stream) {
  return rnn_bias_tanh_launch<false>("zk_rnn_bias_tanh", x, ldx, bias, out_f32, ldo, out_copy, ldc, rows, cols, rep, stream);
}

int zk_f32_rnn_bias_tanh(const float* x, int ldx, const float* bias, float* out_f32, int ldo, float* out_copy, int ldc,
                         int rows, int cols, int rep, hipStream_t stream) {
  return rnn_bias_tanh_launch<true>("zk_f32_rnn_bias_tanh", x, ldx, bias, out_f32, ldo, out_copy, ldc, rows, cols, rep, stream);
}

int zk_rnn_lrn_scan(const float* h_prev, int ldh, int n_prev, const int* idx, const void* lo, long lo_ps, long lo_rs,
                    const void* hi, long hi_ps, long hi_rs, const float* mask, long m_ps, long m_rs, float* out, int ldo,
                    void* seq, long seq_ps, long seq_rs, int R, int H, int T, int reverse, int gated, hipStream_t stream) {
  return lrn_scan_launch<false>("zk_rnn_lrn_scan", "zk_f32_rnn_lrn_scan", h_prev, ldh, n_prev, idx, lo, lo_ps, lo_rs, hi, hi_ps,
                                hi_rs, mask, m_ps, m_rs, out, ldo, seq, seq_ps, seq_rs, R, H, T, reverse, gated, stream);
}

int zk_f32_rnn_lrn_scan(const float* h_prev, int ldh, int n_prev, const int* idx, const float* lo, long lo_ps, long lo_rs,
                        const float* hi, long hi_ps, long hi_rs, const float* mask, long m_ps, long m_rs, float* out, int ldo,
                        float* seq, long seq_ps, long seq_rs, int R, int H, int T, int reverse, int gated, hipStream_t stream) {
  return lrn_scan_launch<true>("zk_f32_rnn_lrn_scan", "zk_rnn_lrn_scan", h_prev, ldh, n_prev, idx, lo, lo_ps, lo_rs, hi, hi_ps,
                               hi_rs, mask, m_ps, m_rs, out, ldo, seq, seq_ps, seq_rs, R, H, T, reverse, gated, stream);
}

}  // extern "C"
