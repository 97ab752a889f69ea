// zk_gemm2.hip -- second-generation bf16 MFMA GEMM: LDS-DMA ring + hardware-transpose reads.
//
// Same contract as k_gemm_mfma (zk_gemm.hip).  What changed, and why (rocprof of round 1: the
// step's GEMMs are small -- 4096x512x512 is 0.9 us of MFMA work per CU -- so the K loop was
// bound by exposed L2/fabric latency, one tile ahead was not enough):
//   * operands go HBM/L2 -> LDS by `global_load_lds_dwordx4` (16 B per lane, no VGPR staging)
//     into an NS-stage ring; NS-1 K tiles are in flight per workgroup, tracked with a counted
//     `s_waitcnt vmcnt(N)` and ONE raw s_barrier per K step;
//   * LDS-DMA writes lane-linear 1 KiB pieces, so the bank-conflict swizzle is applied to the
//     per-lane SOURCE address and undone in the fragment read (same XOR both sides);
//   * operands whose contraction dim is not contiguous in HBM (W[K,N] forward, both wgrad
//     operands) are stored UN-transposed ([k][rows]) and read with ds_read_b64_tr_b16, the
//     hardware 4x16 transpose read (semantics probed on the device: zk_probe_tr16) -- no
//     register transposes, no row permutation;
//   * the epilogue goes through LDS: every thread finishes 8 contiguous outputs with 16-byte
//     loads/stores (bias, residual, ReLU, ReLU-backward mask, dropout fused as before).
#include "zk_gemm2_dev.h"

template <int BM, int BN, int NS, bool TA, bool TB, int NW = 4, int PW = 0, int LN = 0>
__global__ void __launch_bounds__((NW + PW) * 64) k_gemm_dlds(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B, int M,
                                                   int N, int K, int lda, int ldb, int kchunk,
                                                   float* __restrict__ slabs, TileSched ts, GemmEpi e, EpiVec ev) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[DldsCfg<BM, BN, NS>::LDS_BYTES];   // the ring (LN: + 2 x BM float2 of row statistics)
  int tm_, tn_, z_;
  tile_of_block(ts, tm_, tn_, z_);
  const int kbeg = z_ * kchunk;
  const int kend = min(K, kbeg + kchunk);
  gemm_tile<BM, BN, NS, TA, TB, NW, PW, false, false, LN>(smem, A, B, M, N, lda, ldb, kbeg, kend, tm_ * BM, tn_ * BN,
                                    slabs ? slabs + (size_t)z_ * M * N : nullptr, e, ev.vec_ok);
  __builtin_amdgcn_sched_barrier(0);
  ZK_E(4);
}

template <int BM, int BN, int NS, bool TB, int PW>
__global__ void __launch_bounds__((4 + PW) * 64) k_gemm_kseg(KSegDesc ks, int M, int N, int lda, int ldb, TileSched ts,
                                                             GemmEpi e, EpiVec ev) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[DldsCfg<BM, BN, NS>::LDS_BYTES];
  int tm_, tn_, z_;
  tile_of_block(ts, tm_, tn_, z_);
  gemm_tile<BM, BN, NS, false, TB, 4, PW, true>(smem, nullptr, nullptr, M, N, lda, ldb, 0, ks.nseg * ks.tps * 64,
                                                tm_ * BM, tn_ * BN, nullptr, e, ev.vec_ok, &ks);
}

// Grouped launch: many independent GEMMs (same transposition flags) in ONE grid -- the deferred
// weight-gradient GEMMs of several layers, or the cross-attention K/V projections of all decoder
// layers.  Each problem is far too small to fill 256 CUs; together they do, with 128x128 tiles, the
// full K per tile and no split-K slabs.  Descriptors live in device memory.
struct GroupDesc {
  const bf16_t* A; const bf16_t* B; void* C; const float* bias;
  const bf16_t* res;          // optional bf16 residual added in the epilogue (may alias C), row stride ldr
  int M, N, K, lda, ldb, ldc, out_f32, tile_start, tiles_n, ldr;
  float* colsum;              // optional fp32 [N]: column sums of B (tb = 0) over K, written by the producer waves of the
                              // tm = 0 tiles (bias gradient beside a weight gradient): by the producer waves of the
  long pad_;                  // wide tiles, by two extra MFMAs per eight on the 256x256 tiles (gemm256_acc<.., CS>)
};                            // 96 bytes; mirrored by zero_amd/func.py:_GroupDesc

template <int BM, int BN, int NS, bool TA, bool TB, int PW = 0>
__global__ void __launch_bounds__((4 + PW) * 64) k_gemm_grouped(const GroupDesc* __restrict__ descs, int nprob) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[DldsCfg<BM, BN, NS>::LDS_BYTES];
  const int nb = gridDim.x, bid = blockIdx.x;
  const int q = nb >> 3, r = nb & 7, xcd = bid & 7, loc = bid >> 3;
  const int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  int p = 0;
  {   // the last problem whose first tile is <= t: binary search (a linear scan is one dependent global load per
      // problem -- 6 us before the first K tile with the 49 problems of a weight-gradient group)
    int hi = nprob - 1;
    while (p < hi) {
      const int mid = (p + hi + 1) >> 1;
      if (descs[mid].tile_start <= t) p = mid; else hi = mid - 1;
    }
  }
  const GroupDesc d = descs[p];
  const int local = t - d.tile_start;
  const int tm = local / d.tiles_n, tn = local - tm * d.tiles_n;
  GemmEpi e;
  e.C = d.C; e.ldc = d.ldc; e.out_f32 = d.out_f32; e.alpha = 1.f; e.bias = d.bias;
  e.res = d.res; e.ldr = d.ldr; e.act = 0; e.aux = nullptr; e.ldaux = 0; e.aux_scale = 1.f;
  e.thr = 0; e.inv_keep = 1.f; e.seed = nullptr; e.sid = 0;
  const uintptr_t al = (uintptr_t)d.C | (uintptr_t)d.bias | (uintptr_t)d.res;
  const int vec_ok = ((al & 15) == 0) && (d.ldc % 8 == 0) && (d.res == nullptr || d.ldr % 8 == 0);
  gemm_tile<BM, BN, NS, TA, TB, 4, PW>(smem, d.A, d.B, d.M, d.N, d.lda, d.ldb, 0, d.K, tm * BM, tn * BN, nullptr, e,
                                       vec_ok, nullptr, (PW > 0 && tm == 0) ? d.colsum : nullptr);
}

// =====================================================================================
// 256x256 tiles for the large fp32-output GEMMs (grouped weight gradients incl. the logits problem: 40 % of the
// step's FLOPs).  scripts/gemm_big_bench.py + the K-step arithmetic: these GEMMs are bound by the L2 -> LDS path at
// ~10-13 TB/s chip-wide (the same rate the best published gfx950 kernels sustain), so the lever is bytes per FLOP:
// 256x256x64 moves 64 KB for 8.4 MFLOP (7.8 KB/MFLOP; 128x256: 11.7, 128x128: 15.6).
// Eight waves as 2 x 4, each a 128x64 register tile (TM = 4, TN = 2: 128 accumulator registers), all of them issue
// LDS-DMA (two pieces after every 16-deep K slice's MFMAs, so the issue stalls sit behind matrix work), two ring
// stages of 64 KiB.  The tile leaves straight from the accumulators (a 32x32 MFMA tile stores two full 128-byte
// lines per instruction for fp32) -- the fp32 tile would not fit in LDS.  fp32 output only, no epilogue options.
// =====================================================================================
// accumulators of one 256x256 tile: acc[i][j][e] = element (row m0 + wm*128 + i*32 + (e&3) + 8*(e>>2) + 4*(lane>>5),
// column n0 + wn*64 + j*32 + (lane&31)) with wave = wm * 4 + wn.  smem: the 128 KiB ring (free again on return, after a
// barrier by the caller).
// CS (tb = 0 only): acc_cs[j] additionally accumulates ones[32 x 16] x B-fragment, i.e. every row of it holds the column
// sums over k of this wave's 32 columns of B -- the bias gradient sum_k dY[k][n] (func.py:16, 58-60) of a weight-gradient
// problem, from the fragments the wave has in registers anyway (2 extra MFMAs per 8; waves with cs_on only).
template <bool TA, bool TB, bool SPREAD, bool CS = false>
__device__ __forceinline__ void gemm256_acc(unsigned char* smem, const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
                                            int lda, int ldb, int M, int N, int K, int m0, int n0, f32x16_t (&acc)[4][2],
                                            bool cs_on = false, f32x16_t* acc_cs = nullptr, int sched = 0) {
  constexpr int BM = 256, BN = 256, NS = 2, NW = 8, NWN = 4, WTM = 128, WTN = 64, TM = 4, TN = 2;
  constexpr int STAGE = (BM + BN) * 64;
  bf16_t* ring = reinterpret_cast<bf16_t*>(smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / NWN, wn = wave % NWN;
  const int nk = (K + 63) >> 6;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  bf16x8_t ones;
  if (CS) {
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc_cs[j][e] = 0.f;
    typedef short v8s_ __attribute__((ext_vector_type(8)));
    const v8s_ o = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};     // bf16 1.0
    ones = __builtin_bit_cast(bf16x8_t, o);
  }
  constexpr int NI = DmaPlan<BM, NW>::NINSTR;     // pieces per wave and operand (4)
  DmaPlan<BM, NW> planA;
  DmaPlan<BN, NW> planB;
  dma_plan<BM, TA, NW>(planA, lda, m0, M, wave, lane);
  dma_plan<BN, !TB, NW>(planB, ldb, n0, N, wave, lane);
  const size_t stepA = TA ? (size_t)64 * lda : (size_t)64;
  const size_t stepB = !TB ? (size_t)64 * ldb : (size_t)64;
  const uint32_t ring_addr = lds_addr(ring);
  // LDS-DMA of K tile t, pieces [j0, j1) of this wave's NI + NI.  The pieces are 32-bit offsets against the tile's
  // wave-uniform base (glds16s): no vector instruction per piece.
  auto issue_part = [&](int tt, int j0, int j1) {
    if (tt * 64 >= K) return;                       // (past the end: nothing to bring in; the waits are vmcnt(0))
    const uint32_t st = ring_addr + (uint32_t)((tt % NS) * STAGE * 2);
    const bf16_t* bA = A + (size_t)tt * stepA;
    const bf16_t* bB = B + (size_t)tt * stepB;
    const bool tail = tt * 64 + 64 > K;              // the one tile that crosses K: pointer form with the per-lane select
#pragma unroll
    for (int j = 0; j < 2 * NI; ++j) {
      if (j < j0 || j >= j1) continue;
      const bool isA = j < NI;
      const int jj = isA ? j : j - NI;
      const uint32_t dst = isA ? st + (uint32_t)(wave * DmaPlan<BM, NW>::PER_WAVE + jj * 64) * 16u
                               : st + BM * 128 + (uint32_t)(wave * DmaPlan<BN, NW>::PER_WAVE + jj * 64) * 16u;
      const uint32_t off = isA ? planA.off[jj] : planB.off[jj];
      const bf16_t* base = isA ? bA : bB;
      if (!tail) {
        glds16s(off, base, dst);
      } else {
        const int kofs = isA ? planA.kofs[jj] : planB.kofs[jj];
        const bf16_t* g = reinterpret_cast<const bf16_t*>(reinterpret_cast<const char*>(base) + off);
        g = (tt * 64 + kofs < K) ? g : reinterpret_cast<const bf16_t*>(zk_zero_page);
        glds16(g, dst);
      }
    }
  };
  // `sched` (round 5, tuning key 14; !SPREAD only): WHEN the second-dispatched half of the workgroup (waves 4-7, the
  // partner of waves 0-3 on each SIMD) issues its eight LDS-DMA pieces of the next K tile.  With every wave issuing right
  // behind the barrier, both waves of a SIMD sit in their DMA-issue stalls (~100-185 cycles a piece while the CU's
  // texture-address path is busy) at the same time and the matrix pipe idles; shifted, one wave's issue stalls run under
  // its partner's MFMAs (MI355X_MICROARCH.md "Two waves per SIMD": pair matrix with memory, not matrix with matrix).
  //   bits 0-1: 0 = with the first half (rounds 2-4); 1 = four pieces after the first and four after the second 16-deep
  //             slice's MFMAs; 2 = all eight after the second slice; 3 = two after every slice
  //   bit 2:    the second half runs at s_setprio 1 (the arbitration loser otherwise)
  const bool g1 = wave >= 4;
  //   bit 7: the placements of bits 0-1 apply to the FIRST half instead (the second half issues behind the barrier and
  //          the first, older, half multiplies first)
  const bool late = (sched & 128) ? !g1 : g1;
  int place = late ? (sched & 3) : 0;
  //   bits 3-4: the eight pieces of a wave go out in ONE slot of the step (slot 0 = behind the barrier, slot s = behind
  //             the MFMAs of slice s - 1), the slots dealt by SIMD so that few waves queue on the CU's one texture-address
  //             path at a time (64 pieces a step at ~16 cycles each: a wave that issues ALONE is through in ~130 cycles,
  //             eight at once block each other for ~1000): 1 = slot w % 4 for both waves of a SIMD, 2 = w % 4 for the
  //             first half and (w + 2) % 4 for the second (a SIMD always has one wave multiplying), 3 = w % 4 / (w + 1) % 4
  const int stag = (sched >> 3) & 3;
  int slot = -1;
  if (stag == 1) slot = wave & 3;
  else if (stag == 2) slot = g1 ? ((wave + 2) & 3) : (wave & 3);
  else if (stag == 3) slot = g1 ? ((wave + 1) & 3) : (wave & 3);
  if (slot >= 0) place = slot == 0 ? 0 : 4;      // 4: none of the fixed placements below
  if (g1 && (sched & 4)) __builtin_amdgcn_s_setprio(1);
  issue_part(0, 0, 8);
  __builtin_amdgcn_sched_barrier(0);
  // make TRACE=1 (scripts/trace_gemm256.py): waves 0 and 4 of workgroup 100 stamp the 100 MHz clock at the phase
  // boundaries of their first 64 K steps: [0] loop top, [1] LDS-DMA of this tile landed, [2] barrier passed, [3] next
  // tile's LDS-DMA issued (schedule 0), [4..7] the 16-deep slices' MFMAs issued
#ifdef ZK_GEMM_TRACE
  const bool tr256 = blockIdx.x == 100 && (tid == 0 || tid == 256);
#define ZK_T256(slot) do { if (tr256 && kt < 64) zk_trace_buf[kt * 16 + (tid ? 8 : 0) + (slot)] = __builtin_readcyclecounter(); } while (0)
#else
#define ZK_T256(slot) do { } while (0)
#endif
  for (int kt = 0; kt < nk; ++kt) {
    ZK_T256(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // tile kt has landed (it was issued one compute phase ago)
    ZK_T256(1);
    __builtin_amdgcn_s_barrier();                          // ... for every wave, and everybody is done with tile kt-1
    __builtin_amdgcn_sched_barrier(0);
    ZK_T256(2);
    if (!SPREAD) { if (place == 0) issue_part(kt + 1, 0, 8); __builtin_amdgcn_sched_barrier(0); }
    ZK_T256(3);
    const bf16_t* sA = ring + (kt % NS) * STAGE;
    const bf16_t* sB = sA + BM * 64;
    bf16x8_t af[2][TM], bfr[2][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) af[0][i] = load_frag<BM, TA>(sA, wm * WTM + i * 32, 0, lane);
#pragma unroll
    for (int j = 0; j < TN; ++j) bfr[0][j] = load_frag<BN, !TB>(sB, wn * WTN + j * 32, 0, lane);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      if (kk < 3) {
#pragma unroll
        for (int i = 0; i < TM; ++i) af[(kk + 1) & 1][i] = load_frag<BM, TA>(sA, wm * WTM + i * 32, kk + 1, lane);
#pragma unroll
        for (int j = 0; j < TN; ++j) bfr[(kk + 1) & 1][j] = load_frag<BN, !TB>(sB, wn * WTN + j * 32, kk + 1, lane);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[kk & 1][i], bfr[kk & 1][j], acc[i][j], 0, 0, 0);
      if (CS && cs_on) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc_cs[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, bfr[kk & 1][j], acc_cs[j], 0, 0, 0);
      }
#ifdef ZK_GEMM_TRACE
      __builtin_amdgcn_sched_barrier(0);
      ZK_T256(4 + kk);
#endif
      if (SPREAD) issue_part(kt + 1, kk * 2, kk * 2 + 2);   // the other stage is free since this step's barrier
      else if (place != 0) {
        __builtin_amdgcn_sched_barrier(0);
        if (place == 1 && kk < 2) issue_part(kt + 1, kk * 4, kk * 4 + 4);
        if (place == 2 && kk == 1) issue_part(kt + 1, 0, 8);
        if (place == 3) issue_part(kt + 1, kk * 2, kk * 2 + 2);
        if (place == 4 && kk == slot - 1) issue_part(kt + 1, 0, 8);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the trailing (all-zero) pieces
  if (g1 && (sched & 4)) __builtin_amdgcn_s_setprio(0);
}

// sched: gemm256_acc's LDS-DMA issue schedule (tuning key 14)
template <bool TA, bool TB, bool SPREAD, bool CS = false>
__global__ void __launch_bounds__(512) k_gemm_grouped256(const GroupDesc* __restrict__ descs, int nprob, int sched) {
  constexpr int BM = 256, BN = 256, NS = 2, NWN = 4, WTM = 128, WTN = 64, TM = 4, TN = 2;
  constexpr int STAGE = (BM + BN) * 64;
  __shared__ __attribute__((aligned(16))) unsigned char smem[NS * STAGE * 2];   // the ONLY LDS object (128 KiB)
  const int nb = gridDim.x, bid = blockIdx.x;
  const int q = nb >> 3, r = nb & 7, xcd = bid & 7, loc = bid >> 3;
  const int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  int p = 0;
  {   // the last problem whose first tile is <= t: binary search (a linear scan is one dependent global load per
      // problem -- 6 us before the first K tile with the 49 problems of a weight-gradient group)
    int hi = nprob - 1;
    while (p < hi) {
      const int mid = (p + hi + 1) >> 1;
      if (descs[mid].tile_start <= t) p = mid; else hi = mid - 1;
    }
  }
  const GroupDesc d = descs[p];
  const int local = t - d.tile_start;
  // tile order inside a problem: blocks of 4 x 8 tiles, the blocks of one 8-tile column group one after the other.  An XCD
  // runs 32 consecutive tiles at a time (its chunk of the launch is contiguous): a block keeps 4 A row blocks + 8 B column
  // blocks = 3 MB at K = 512 in its 4-MB L2, and the next block reuses the 8 column blocks.  Row-major order made the
  // logits forward (16 x 125 tiles) fetch the whole 33-MB softmax table once per row of tiles: FETCH_SIZE 543 MB against
  // 37 MB of operands (profiles/r03_pmc_traffic.json), as much HBM traffic again as the 525 MB of logits it writes.
  // Problems with fewer than 4 x 8 tiles (every weight gradient) keep the row-major order.
  int tm, tn;
  {
    constexpr int GM = 4, GN = 8;
    const int tiles_m = (d.M + BM - 1) / BM;
    const int nbm = tiles_m / GM, nbn = d.tiles_n / GN;
    const int full = nbm * nbn * GM * GN;
    if (nbm == 0 || nbn == 0) {
      tm = local / d.tiles_n; tn = local - tm * d.tiles_n;
    } else if (local < full) {
      const int blk = local / (GM * GN), within = local - blk * (GM * GN);
      const int bn = blk / nbm, bm = blk - bn * nbm;
      tm = bm * GM + within / GN; tn = bn * GN + within % GN;
    } else {
      // what the blocks leave: the right stripe (all rows, the last tiles_n % 8 columns), then the bottom stripe
      int r = local - full;
      const int wr = d.tiles_n - nbn * GN, right = wr * tiles_m;
      if (r < right) { tm = r / wr; tn = nbn * GN + r - tm * wr; }
      else { r -= right; const int wb = nbn * GN; tm = nbm * GM + r / wb; tn = r % wb; }
    }
  }
  const int m0 = tm * BM, n0 = tn * BN, M = d.M, N = d.N;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / NWN, wn = wave % NWN;
  f32x16_t acc[TM][TN];
  if (CS) {
    // fp32 tile + bias gradient: the waves of the first row of waves (wm = 0) of the tm = 0 tiles carry the column sums
    f32x16_t acc_cs[TN];
    const bool cs_on = d.colsum != nullptr && tm == 0 && wm == 0;
    gemm256_acc<TA, TB, SPREAD, true>(smem, d.A, d.B, d.lda, d.ldb, M, N, d.K, m0, n0, acc, cs_on, acc_cs, sched);
    if (cs_on && lane < 32) {
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = n0 + wn * WTN + j * 32 + lane;
        if (col < N) d.colsum[col] = acc_cs[j][0];
      }
    }
  } else {
    gemm256_acc<TA, TB, SPREAD, false>(smem, d.A, d.B, d.lda, d.ldb, M, N, d.K, m0, n0, acc, false, nullptr, sched);
  }
  float* C = reinterpret_cast<float*>(d.C);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = n0 + wn * WTN + j * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * WTM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        // streaming store: the tile is written once and read by a later kernel -- with an ordinary store the L2
        // fetches every line it is about to overwrite (FETCH_SIZE == output size, profiles/r02_pmc_traffic.json)
        if (row < M && col < N) __builtin_nontemporal_store(acc[i][j][e], &C[(size_t)row * d.ldc + col]);
      }
    }
}

template <int BM, int BN, int NS, int NW = 4, int PW = 0>
static int launch_dlds(const bf16_t* A, const bf16_t* B, int M, int N, int K, int lda, int ldb, int ta, int tb,
                       int splits, int kchunk, float* slabs, const GemmEpi& e, int sched_flags, hipStream_t stream) {
  TileSched ts;
  ts.tiles_m = (M + BM - 1) / BM;
  ts.tiles_n = (N + BN - 1) / BN;
  ts.n_major = ((long)N > (long)M) ? 1 : 0;
  if (sched_flags & 2) ts.n_major ^= 1;
  ts.xcd_remap = (sched_flags & 1) ? 0 : 1;
  EpiVec ev;
  const uintptr_t al = (uintptr_t)e.C | (uintptr_t)e.bias | (uintptr_t)e.res | (uintptr_t)e.aux;
  ev.vec_ok = ((al & 15) == 0) && (e.ldc % 8 == 0) && (e.res == nullptr || e.ldr % 8 == 0) &&
              (e.aux == nullptr || e.ldaux % 8 == 0);
  dim3 grid((unsigned)((long)ts.tiles_m * ts.tiles_n * splits));
  if (!ta && !tb)
    hipLaunchKernelGGL((k_gemm_dlds<BM, BN, NS, false, false, NW, PW>), grid, dim3((NW + PW) * 64), 0, stream, A, B, M, N, K, lda, ldb, kchunk, slabs, ts, e, ev);
  else if (!ta && tb)
    hipLaunchKernelGGL((k_gemm_dlds<BM, BN, NS, false, true, NW, PW>), grid, dim3((NW + PW) * 64), 0, stream, A, B, M, N, K, lda, ldb, kchunk, slabs, ts, e, ev);
  else if (ta && !tb)
    hipLaunchKernelGGL((k_gemm_dlds<BM, BN, NS, true, false, NW, PW>), grid, dim3((NW + PW) * 64), 0, stream, A, B, M, N, K, lda, ldb, kchunk, slabs, ts, e, ev);
  else
    hipLaunchKernelGGL((k_gemm_dlds<BM, BN, NS, true, true, NW, PW>), grid, dim3((NW + PW) * 64), 0, stream, A, B, M, N, K, lda, ldb, kchunk, slabs, ts, e, ev);
  ZK_LAUNCH_CHECK();
  return 0;
}

extern "C" {
// descs: device array of `nprob` GroupDesc (96 bytes each, see zk_gemm2.hip) whose tile_start
// fields are the running sum of ceil(M/bm)*ceil(N/bn); total_tiles = that sum.
int zk_gemm_grouped(const void* descs, int nprob, int total_tiles, int ta, int tb, int tile, hipStream_t stream) {
  ZK_CHECK_ARG(nprob >= 1 && total_tiles >= 1, "zk_gemm_grouped: empty group");
  // bit 8 of `tile` (256x256 tiles, ta = 1, tb = 0): some problem carries a column-sum output (GroupDesc.colsum)
  const bool cs = (tile & 256) != 0;
  tile &= 255;
  ZK_CHECK_ARG(tile == 1 || tile == 4 || tile == 5 || tile == 6 || tile == 7 || tile == 8,
               "zk_gemm_grouped: tile must be 1 (128x128), 4 (64x64), 5 (256x128), 6 (128x256) or 7 / 8 (256x256)");
  ZK_CHECK_ARG(!cs || ((tile == 7 || tile == 8) && ta && !tb), "zk_gemm_grouped: column sums on 256x256 tiles need ta = 1, tb = 0");
  const GroupDesc* d = (const GroupDesc*)descs;
  dim3 grid((unsigned)total_tiles);
  if (tile == 7 || tile == 8) {     // fp32 outputs without epilogue options only (checked on the host copy by the caller)
    const dim3 blk(512);
    const int sched = g_tune[14];   // LDS-DMA issue schedule of the second half of the workgroup (gemm256_acc)
#define ZK_G256(SP_)                                                                                         \
    do {                                                                                                     \
      if (!ta && !tb) hipLaunchKernelGGL((k_gemm_grouped256<false, false, SP_>), grid, blk, 0, stream, d, nprob, sched);   \
      else if (!ta && tb) hipLaunchKernelGGL((k_gemm_grouped256<false, true, SP_>), grid, blk, 0, stream, d, nprob, sched); \
      else if (ta && !tb && cs) hipLaunchKernelGGL((k_gemm_grouped256<true, false, SP_, true>), grid, blk, 0, stream, d, nprob, sched); \
      else if (ta && !tb) hipLaunchKernelGGL((k_gemm_grouped256<true, false, SP_>), grid, blk, 0, stream, d, nprob, sched); \
      else hipLaunchKernelGGL((k_gemm_grouped256<true, true, SP_>), grid, blk, 0, stream, d, nprob, sched);               \
    } while (0)
    if (tile == 7) ZK_G256(true); else ZK_G256(false);
#undef ZK_G256
    ZK_LAUNCH_CHECK();
    return 0;
  }
#define ZK_GROUP_LAUNCH(BM_, BN_, NS_, PW_)                                                                     \
  do {                                                                                                         \
    const dim3 blk((4 + PW_) * 64);                                                                            \
    if (!ta && !tb) hipLaunchKernelGGL((k_gemm_grouped<BM_, BN_, NS_, false, false, PW_>), grid, blk, 0, stream, d, nprob); \
    else if (!ta && tb) hipLaunchKernelGGL((k_gemm_grouped<BM_, BN_, NS_, false, true, PW_>), grid, blk, 0, stream, d, nprob); \
    else if (ta && !tb) hipLaunchKernelGGL((k_gemm_grouped<BM_, BN_, NS_, true, false, PW_>), grid, blk, 0, stream, d, nprob); \
    else hipLaunchKernelGGL((k_gemm_grouped<BM_, BN_, NS_, true, true, PW_>), grid, blk, 0, stream, d, nprob);     \
  } while (0)
  const bool pw = (g_tune[6] >> 16) & 1;          // producer-wave workgroups (see gemm_tile_to_lds)
  if (tile == 1) { if (pw) ZK_GROUP_LAUNCH(128, 128, 2, 4); else ZK_GROUP_LAUNCH(128, 128, 2, 0); }
  // 256x128 / 128x256: four compute waves with a 128x64 register tile each (half the LDS fragment bytes and 3/4
  // of the L1->LDS bytes per MFMA of the 128x128 tile) + four producer waves, three-stage ring (144 KiB: one
  // workgroup per CU)
  else if (tile == 5) { if (g_tune[6] & (1 << 17)) ZK_GROUP_LAUNCH(256, 128, 2, 4); else ZK_GROUP_LAUNCH(256, 128, 3, 4); }
  else if (tile == 6) { if (g_tune[6] & (1 << 17)) ZK_GROUP_LAUNCH(128, 256, 2, 4); else ZK_GROUP_LAUNCH(128, 256, 3, 4); }
  else { if (pw) ZK_GROUP_LAUNCH(64, 64, 4, 4); else ZK_GROUP_LAUNCH(64, 64, 4, 0); }
#undef ZK_GROUP_LAUNCH
  ZK_LAUNCH_CHECK();
  return 0;
}
// C bf16 [M, ldc] = sum_s A_s [M, kseg] (lda) x B_s (+ residual bf16 [M, ldr], may alias C).
//   tb = 1: B_s is [N, ldb] with K contiguous (dgrad through W stored [in, out]);  tb = 0: B_s is [kseg, ldb].
// a_segs / b_segs: HOST arrays of nseg (<= 16) device pointers; kseg a multiple of 64; 16-byte aligned operands,
// leading dimensions multiples of 8.
int zk_gemm_kseg(const void* const* a_segs, const void* const* b_segs, int nseg, int kseg, void* C, int M, int N,
                 int lda, int ldb, int ldc, int tb, const void* residual, int ldr, hipStream_t stream) {
  ZK_CHECK_ARG(nseg >= 1 && nseg <= ZK_KSEG_MAX, "zk_gemm_kseg: nseg=%d out of range (<= %d)", nseg, ZK_KSEG_MAX);
  ZK_CHECK_ARG(kseg >= 64 && kseg % 64 == 0, "zk_gemm_kseg: kseg=%d must be a positive multiple of 64", kseg);
  ZK_CHECK_ARG(M >= 0 && N >= 1 && C != nullptr, "zk_gemm_kseg: bad output");
  ZK_CHECK_ARG(lda % 8 == 0 && ldb % 8 == 0 && ldc % 8 == 0 && (residual == nullptr || ldr % 8 == 0) && (tb || N % 8 == 0),
               "zk_gemm_kseg: leading dimensions must be multiples of 8");
  if (M == 0) return 0;
  KSegDesc ks;
  uintptr_t al = (uintptr_t)C | (uintptr_t)residual;
  for (int i = 0; i < nseg; ++i) {
    ks.A[i] = (const bf16_t*)a_segs[i]; ks.B[i] = (const bf16_t*)b_segs[i];
    ZK_CHECK_ARG(a_segs[i] != nullptr && b_segs[i] != nullptr, "zk_gemm_kseg: null segment %d", i);
    al |= (uintptr_t)a_segs[i] | (uintptr_t)b_segs[i];
  }
  ZK_CHECK_ARG((al & 15) == 0, "zk_gemm_kseg: operands must be 16-byte aligned");
  for (int i = nseg; i < ZK_KSEG_MAX; ++i) { ks.A[i] = ks.A[0]; ks.B[i] = ks.B[0]; }
  ks.nseg = nseg; ks.tps = kseg / 64;
  GemmEpi e;
  e.C = C; e.ldc = ldc; e.out_f32 = 0; e.alpha = 1.f; e.bias = nullptr; e.res = (const bf16_t*)residual; e.ldr = ldr;
  e.act = 0; e.aux = nullptr; e.ldaux = 0; e.aux_scale = 1.f; e.thr = 0; e.inv_keep = 1.f; e.seed = nullptr; e.sid = 0;
  TileSched ts;
  ts.tiles_m = (M + 63) / 64; ts.tiles_n = (N + 63) / 64; ts.n_major = ((long)N > (long)M) ? 1 : 0; ts.xcd_remap = 1;
  EpiVec ev;
  ev.vec_ok = 1;
  dim3 grid((unsigned)((long)ts.tiles_m * ts.tiles_n));
  if (tb) hipLaunchKernelGGL((k_gemm_kseg<64, 64, 4, true, 4>), grid, dim3(512), 0, stream, ks, M, N, lda, ldb, ts, e, ev);
  else hipLaunchKernelGGL((k_gemm_kseg<64, 64, 4, false, 4>), grid, dim3(512), 0, stream, ks, M, N, lda, ldb, ts, e, ev);
  ZK_LAUNCH_CHECK();
  return 0;
}

#ifdef ZK_GEMM_TRACE
int zk_debug_trace_read(unsigned long long* out, int n) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(zk_trace_buf), sizeof(unsigned long long) * n);
}
#endif
}  // extern "C"

// Producer waves of the gen-2 kernel for a bm x bn tile: tuning key 6 holds one nibble per tile class
// (64x64 | 128x128 << 4 | 128x64 and 64x128 << 12; bit 8: ring depth 3 for 128x128; bit 16: grouped launches).
// Default 0x44 -- in-step A/B on the bench configuration: 5.41 -> 5.32 ms (profiles/r01_gemm_producer_waves.txt).
int zk_gemm_dlds_pw(int bm, int bn) {
  const int t = g_tune[6];
  int pw = 0;
  if (bm == 64 && bn == 64) pw = t & 15;
  else if (bm == 128 && bn == 128) pw = (t >> 4) & 15;
  else if ((bm == 128 && bn == 64) || (bm == 64 && bn == 128)) pw = (t >> 12) & 15;
  const bool deep128 = bm == 128 && bn == 128 && ((t >> 8) & 1);
  if (pw == 2) return (bm == bn && !deep128) ? 2 : 0;      // instantiated: 64x64 and 128x128 with ring depth 2
  return (pw == 4 || pw == 8) ? pw : 0;
}

// residual + LayerNorm inside the producing launch (zk_gemm_add_ln; A [M,K] x B [K,N], no split-K): the 64x64 tile with
// four producer waves that the default dispatch gives the sub-layer output products, with the LN = 3 epilogue.  Tile
// order: row-block major, so that the N/64 workgroups that wait for each other are consecutive in the dispatch order (and, with the XCD remap, on one XCD whenever the grid is a multiple
// of 64): a workgroup only ever waits for workgroups that are already resident or next in line.
template <int BM, int NS, int PW>
static int launch_dlds_sync_ln(const bf16_t* A, const bf16_t* B, int M, int N, int K, int lda, int ldb, const GemmEpi& e,
                               hipStream_t stream) {
  TileSched ts;
  ts.tiles_m = (M + BM - 1) / BM;
  ts.tiles_n = N / 64;
  ts.n_major = 0;
  ts.xcd_remap = 1;
  EpiVec ev;
  ev.vec_ok = 1;
  const long nwg = (long)ts.tiles_m * ts.tiles_n;
  dim3 grid((unsigned)nwg);
  GemmEpi el = e;
  // every XCD owns a contiguous range of nwg / 8 tiles: with that a multiple of the group size no group straddles two
  // XCDs and the exchange stays in their L2 (tuning key 15 = 1: never assume it -- exchange through memory)
  el.sy_local = (nwg % (8 * ts.tiles_n) == 0 && !(g_tune[15] & 1)) ? 1 : 0;
  el.sy_fault = (g_tune[15] & 2) ? 1 : 0;       // fault injection for tests/test_gpu_sync_ln.py: a peer that never publishes
  hipLaunchKernelGGL((k_gemm_dlds<BM, 64, NS, false, false, 4, PW, 3>), grid, dim3((4 + PW) * 64), 0, stream, A, B, M, N, K,
                     lda, ldb, K, (float*)nullptr, ts, el, ev);
  ZK_LAUNCH_CHECK();
  return 0;
}
int zk_gemm_dlds_sync_ln_dispatch(const bf16_t* A, const bf16_t* B, int M, int N, int K, int lda, int ldb, int bm,
                                  const GemmEpi& e, hipStream_t stream) {
  (void)bm;
  return launch_dlds_sync_ln<64, 4, 4>(A, B, M, N, K, lda, ldb, e, stream);
}

// the backward form (zk_gemm_ln_bwd): dgrad A [M,K] x B[N,K]^T on 64x64 tiles with the LN = 4 epilogue
int zk_gemm_dlds_sync_ln_bwd_dispatch(const bf16_t* A, const bf16_t* B, int M, int N, int K, int lda, int ldb,
                                      const GemmEpi& e, hipStream_t stream) {
  TileSched ts;
  ts.tiles_m = (M + 63) / 64;
  ts.tiles_n = N / 64;
  ts.n_major = 0;
  ts.xcd_remap = 1;
  EpiVec ev;
  ev.vec_ok = 1;
  const long nwg = (long)ts.tiles_m * ts.tiles_n;
  GemmEpi el = e;
  el.sy_local = (nwg % (8 * ts.tiles_n) == 0 && !(g_tune[15] & 1)) ? 1 : 0;
  el.sy_fault = (g_tune[15] & 2) ? 1 : 0;       // fault injection for tests/test_gpu_sync_ln.py: a peer that never publishes
  hipLaunchKernelGGL((k_gemm_dlds<64, 64, 4, false, true, 4, 4, 4>), dim3((unsigned)nwg), dim3(512), 0, stream, A, B, M, N, K,
                     lda, ldb, K, (float*)nullptr, ts, el, ev);
  ZK_LAUNCH_CHECK();
  return 0;
}

// entry used by zk_gemm (zk_gemm.hip)
int zk_gemm_dlds_dispatch(const bf16_t* A, const bf16_t* B, int M, int N, int K, int lda, int ldb, int ta, int tb,
                          int bm, int bn, int splits, int kchunk, float* slabs, const GemmEpi& e, int sched_flags,
                          hipStream_t stream) {
  if (sched_flags & 0x100) {          // wide register tiles (tile overrides 6 / 7): 4 compute waves of 128x64 + 4 producers
    const int ns_w = (sched_flags >> 4) & 15;
    if (bm == 256 && bn == 128) {
      if (ns_w == 2) return launch_dlds<256, 128, 2, 4, 4>(A, B, M, N, K, lda, ldb, ta, tb, splits, kchunk, slabs, e, sched_flags, stream);
      return launch_dlds<256, 128, 3, 4, 4>(A, B, M, N, K, lda, ldb, ta, tb, splits, kchunk, slabs, e, sched_flags, stream);
    }
    if (bm == 128 && bn == 256) {
      if (ns_w == 2) return launch_dlds<128, 256, 2, 4, 4>(A, B, M, N, K, lda, ldb, ta, tb, splits, kchunk, slabs, e, sched_flags, stream);
      return launch_dlds<128, 256, 3, 4, 4>(A, B, M, N, K, lda, ldb, ta, tb, splits, kchunk, slabs, e, sched_flags, stream);
    }
  }
  if (g_tune[2] == 3 && bm == 128 && bn == 64) {
    // A/B: ONE 128x64 workgroup per CU with a deep ring (tuning key 3 = 4 / 5 / 6 stages of 24 KiB) + producer waves:
    // 25 % fewer L2 -> LDS bytes than two 64x64 workgroups and more of them in flight
    if (g_tune[3] == 6) return launch_dlds<128, 64, 6, 4, 4>(A, B, M, N, K, lda, ldb, ta, tb, splits, kchunk, slabs, e, sched_flags, stream);
    if (g_tune[3] == 5) return launch_dlds<128, 64, 5, 4, 4>(A, B, M, N, K, lda, ldb, ta, tb, splits, kchunk, slabs, e, sched_flags, stream);
    return launch_dlds<128, 64, 4, 4, 4>(A, B, M, N, K, lda, ldb, ta, tb, splits, kchunk, slabs, e, sched_flags, stream);
  }
  int ns = (sched_flags >> 4) & 15;   // ring-depth override (tuning)
  if (!ns && bm == 64 && bn == 64 && g_tune[3] && g_tune[3] != 5) ns = g_tune[3];     // A/B: ring depth of the 64x64 tile in-step
  if (bm == 64 && bn == 64 && g_tune[4] == 2)                       // A/B: two-wave workgroups, ring depth 2
    return launch_dlds<64, 64, 2, 2>(A, B, M, N, K, lda, ldb, ta, tb, splits, kchunk, slabs, e, sched_flags, stream);
  if (bm == 64 && bn == 64 && g_tune[4] == 4)                       // two-wave workgroups, ring depth 4
    return launch_dlds<64, 64, 4, 2>(A, B, M, N, K, lda, ldb, ta, tb, splits, kchunk, slabs, e, sched_flags, stream);
  if (!ns) {                                                        // producer-wave workgroups (default for 64x64, 128x128)
    const int t = g_tune[6], pw = zk_gemm_dlds_pw(bm, bn), ns3 = (t >> 8) & 1;
#define ZK_PW(BM_, BN_, NS_, PW_) return launch_dlds<BM_, BN_, NS_, 4, PW_>(A, B, M, N, K, lda, ldb, ta, tb, splits, kchunk, slabs, e, sched_flags, stream)
    // tuning key 3 = 5: five ring stages (80 KiB: two workgroups fill the CU's 160 KiB of LDS, 128 KiB in flight)
    if (bm == 64 && bn == 64 && g_tune[3] == 5 && pw == 4) ZK_PW(64, 64, 5, 4);
    if (bm == 64 && bn == 64) { if (pw == 2) ZK_PW(64, 64, 4, 2); if (pw == 4) ZK_PW(64, 64, 4, 4); if (pw == 8) ZK_PW(64, 64, 4, 8); }
    if (bm == 128 && bn == 128 && !ns3) { if (pw == 2) ZK_PW(128, 128, 2, 2); if (pw == 4) ZK_PW(128, 128, 2, 4); if (pw == 8) ZK_PW(128, 128, 2, 8); }
    if (bm == 128 && bn == 128 && ns3) { if (pw == 4) ZK_PW(128, 128, 3, 4); if (pw == 8) ZK_PW(128, 128, 3, 8); }
    if (bm == 128 && bn == 64) { if (pw == 4) ZK_PW(128, 64, 2, 4); if (pw == 8) ZK_PW(128, 64, 2, 8); }
    if (bm == 64 && bn == 128) { if (pw == 4) ZK_PW(64, 128, 2, 4); if (pw == 8) ZK_PW(64, 128, 2, 8); }
#undef ZK_PW
  }
  if (ns) {
#define ZK_NS(BM_, BN_, NS_) return launch_dlds<BM_, BN_, NS_>(A, B, M, N, K, lda, ldb, ta, tb, splits, kchunk, slabs, e, sched_flags, stream)
    if (bm == 64 && bn == 64) { if (ns == 2) ZK_NS(64, 64, 2); if (ns == 6) ZK_NS(64, 64, 6); if (ns == 8) ZK_NS(64, 64, 8); }
    if (bm == 128 && bn == 64) { if (ns == 3) ZK_NS(128, 64, 3); if (ns == 6) ZK_NS(128, 64, 6); }
    if (bm == 128 && bn == 128) { if (ns == 3) ZK_NS(128, 128, 3); if (ns == 4) ZK_NS(128, 128, 4); }
#undef ZK_NS
  }
  // ring depth 2 for the larger tiles: the measured optimum is MORE workgroups per CU (64 KiB /
  // 48 KiB of LDS each), not deeper prefetch
  if (bm == 256 && bn == 128) return launch_dlds<256, 128, 2, 8>(A, B, M, N, K, lda, ldb, ta, tb, splits, kchunk, slabs, e, sched_flags, stream);
  if (bm == 128 && bn == 128) return launch_dlds<128, 128, 2>(A, B, M, N, K, lda, ldb, ta, tb, splits, kchunk, slabs, e, sched_flags, stream);
  if (bm == 128 && bn == 64) return launch_dlds<128, 64, 2>(A, B, M, N, K, lda, ldb, ta, tb, splits, kchunk, slabs, e, sched_flags, stream);
  if (bm == 64 && bn == 128) return launch_dlds<64, 128, 2>(A, B, M, N, K, lda, ldb, ta, tb, splits, kchunk, slabs, e, sched_flags, stream);
  return launch_dlds<64, 64, 4>(A, B, M, N, K, lda, ldb, ta, tb, splits, kchunk, slabs, e, sched_flags, stream);
}
