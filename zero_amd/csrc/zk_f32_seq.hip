// zk_f32_seq.hip -- the full-sequence fp32 kernels of the fp32 scorer (hp.score_dtype = "float32";
// zero_amd/models/_score_f32.py): the training-path forward of models/transformer.py:15-216 needs attention over Lq > 1
// query rows per sentence (encoder, causal decoder self-attention, cross-attention), the train-time average of
// transformer_aan.py:92-108 and the shifted target embedding of transformer.py:108-112 -- none of which the decode-step
// kernels of zk_f32.hip have (zk_f32_attn gives a wave to ONE query row and streams all keys and values of the sentence
// from memory for it: right for Lq = 1, Lq times the traffic for a scored sentence; it has no causal form).
//
//   zk_f32_attn_seq     func.py:218-256 (+ func.py:372-400 masks, modules/rpr.py:10-75) for a block of query rows
//   zk_f32_cumavg       transformer_aan.py:92-108 / func.py:258-275: out = (add +) running mean of x over positions
//   zk_f32_embed_shift  transformer.py:88-112: row i embeds token i - 1, row 0 is zero, + timing signal of position i
#include "zk_common.h"

// ------------------------------------------------------------------------------------------------ attention
// One workgroup (four waves) owns SEQ_BR = 32 consecutive query rows of one (sentence, head) and walks the keys in tiles
// of SEQ_TK = 64; a tile's keys AND values are staged in LDS once per workgroup (a key row is fetched from memory once
// per 32 query rows, not once per row).  Wave w owns the rows 8 w .. 8 w + 7 of the block:
//
//   scores   lane j of the wave holds key j of the tile: s_r = fmaf chain over the head's d channels, in channel order,
//            of (q_r * scale) . k_j for its eight rows at once -- one 16-byte LDS read of the key row per four channels,
//            shared by the eight rows, whose query values are broadcast reads.  (The chain is the one of k_f32_attn.)
//            + the relative-position chain q . r_k[clip(i - j)] where given (table rows read from LDS like key rows), + (1 - kmask_j) * (-mask_inf).
//   softmax  online: per row a running maximum m and sum l; a tile rescales by exp(m_old - m_new).  A key past Lk, or
//            above the diagonal with `causal`, takes no part: its probability is 0 exactly (the reference's additive
//            -1e8 gives exp(-1e8 - ..) = 0 in fp32 as well, key 0 being visible to every row).  With `causal`, tiles
//            that begin above the block's last row are not visited at all.
//   values   lane c holds channel c: acc_r = acc_r * corr + sum_j p_rj v_jc over the tile's keys in order; p is handed
//            from the key lanes to the channel lanes through LDS (64 floats per row).  out = acc / l.
//
// LDS layout (floats; nothing grows with Lk): sQ [32][d] scaled queries, sK [64][dk], sV [64][d], sP [4][8][64] and, with
// relative positions, both tables [2 max_rel + 1][dk] / [..][d], staged once per block (the value pass reads a table
// row per (key, query row): from global memory that was eight dependent loads per key).
// The key tile is the only image read "down a column": lane j reads 16 bytes of ROW j, so with a row stride of d = 64
// floats (256 bytes = one bank row) all 16 lanes of a ds_read_b128 lane group would hit the same four banks (16-way).
// dk = d + 4 when d is a multiple of 8, else d: dk / 4 is then ODD, lane j's 16-byte slot is (j dk / 4) mod 16, and any 16
// lanes with distinct j mod 16 -- which each of the four lane groups of ds_read_b128 has -- fall on 16 distinct slots:
// conflict-free by padding one access width.  sV is read along a row (lane = channel, 4-byte reads of consecutive
// addresses) and sQ / sP by broadcast (every lane the same address): no padding needed.  Arithmetic is plain fp32 VALU
// (fmaf, libm expf, IEEE division); no inline assembly.
#define SEQ_BR 32
#define SEQ_TK 64
#define SEQ_RW 8          // rows per wave
#define SEQ_LDS_MAX (160 * 1024)

template <int DC, bool RPR>      // DC: channels per lane of the value pass (d <= 64 DC)
__global__ void __launch_bounds__(256) k_f32_attn_seq(const float* __restrict__ q, const float* __restrict__ k,
                                                      const float* __restrict__ v, float* __restrict__ out, int nh, int Lq,
                                                      int Lk, int d, int ldq, int ldk, int ldv, int ldo, long bsq, long bsk,
                                                      long bsv, long bso, const float* __restrict__ kmask, int ldmask,
                                                      float scale, float mask_inf, const float* __restrict__ rpr_k,
                                                      const float* __restrict__ rpr_v, int max_rel, int q_pos0, int causal,
                                                      int nblk) {
  extern __shared__ __align__(16) float sm[];
  const int dk = d + ((d & 7) == 0 ? 4 : 0);
  float* sQ = sm;                                 // [SEQ_BR][d]
  float* sK = sQ + SEQ_BR * d;                    // [SEQ_TK][dk]
  float* sV = sK + SEQ_TK * dk;                   // [SEQ_TK][d]
  float* sP = sV + SEQ_TK * d;                    // [4][SEQ_RW][SEQ_TK]
  float* sRK = sP + 4 * SEQ_RW * SEQ_TK;          // RPR: [2 max_rel + 1][dk]  (read like sK: 16 bytes of a row per lane)
  float* sRV = sRK + (2 * max_rel + 1) * dk;      // RPR: [2 max_rel + 1][d]   (read like sV: lane = channel)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int blk = blockIdx.x % nblk, h = (blockIdx.x / nblk) % nh, b = blockIdx.x / (nblk * nh);
  const int i0 = blk * SEQ_BR;                    // first query row of the block
  const int iw = i0 + wave * SEQ_RW;              // first query row of the wave
  const int d4 = d >> 2;
  // scaled queries of the block (rows past Lq: zeros, computed and never stored)
  for (int e = tid; e < SEQ_BR * d4; e += 256) {
    const int r = e / d4, c = (e % d4) * 4;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i0 + r < Lq) {
      const float* qp = q + (size_t)b * bsq + (size_t)(i0 + r) * ldq + h * d + c;
      x = make_float4(qp[0] * scale, qp[1] * scale, qp[2] * scale, qp[3] * scale);
    }
    *reinterpret_cast<float4*>(sQ + r * d + c) = x;
  }
  if constexpr (RPR) {     // both tables, once per block
    for (int e = tid; e < (2 * max_rel + 1) * d4; e += 256) {
      const int r = e / d4, c = (e % d4) * 4;
      *reinterpret_cast<float4*>(sRK + r * dk + c) = *reinterpret_cast<const float4*>(rpr_k + (size_t)r * d + c);
      const float* vp = rpr_v + (size_t)r * d + c;
      *reinterpret_cast<float4*>(sRV + r * d + c) = make_float4(vp[0], vp[1], vp[2], vp[3]);
    }
  }
  float m[SEQ_RW], l[SEQ_RW], acc[SEQ_RW][DC], acc2[RPR ? SEQ_RW : 1][DC];
#pragma unroll
  for (int r = 0; r < SEQ_RW; ++r) {
    m[r] = -3.0e38f;
    l[r] = 0.f;
#pragma unroll
    for (int u = 0; u < DC; ++u) {
      acc[r][u] = 0.f;
      if constexpr (RPR) acc2[r][u] = 0.f;
    }
  }
  // keys a row of the block can see: all Lk, or (causal) 0 .. its own index
  const int kend = causal ? min(Lk, min(i0 + SEQ_BR, Lq)) : Lk;
  const float* kb = k + (size_t)b * bsk + h * d;
  const float* vb = v + (size_t)b * bsv + h * d;
  float* pw = sP + wave * SEQ_RW * SEQ_TK;
  for (int j0 = 0; j0 < kend; j0 += SEQ_TK) {
    __syncthreads();                              // (the previous tile's readers are done; sQ is written)
    for (int e = tid; e < SEQ_TK * d4; e += 256) {
      const int r = e / d4, c = (e % d4) * 4;
      float4 kx = make_float4(0.f, 0.f, 0.f, 0.f), vx = kx;
      if (j0 + r < Lk) {
        kx = *reinterpret_cast<const float4*>(kb + (size_t)(j0 + r) * ldk + c);
        const float* vp = vb + (size_t)(j0 + r) * ldv + c;
        vx = make_float4(vp[0], vp[1], vp[2], vp[3]);
      }
      *reinterpret_cast<float4*>(sK + r * dk + c) = kx;
      *reinterpret_cast<float4*>(sV + r * d + c) = vx;
    }
    __syncthreads();
    // ---- scores of key j = j0 + lane for the wave's eight rows
    const int j = j0 + lane;
    float s[SEQ_RW];
#pragma unroll
    for (int r = 0; r < SEQ_RW; ++r) s[r] = 0.f;
    {
      const float* kr = sK + lane * dk;
      const float* qr = sQ + wave * SEQ_RW * d;
      for (int c = 0; c < d; c += 4) {
        const float4 kv = *reinterpret_cast<const float4*>(kr + c);
#pragma unroll
        for (int r = 0; r < SEQ_RW; ++r) {
          const float4 qv = *reinterpret_cast<const float4*>(qr + r * d + c);
          s[r] = fmaf(qv.x, kv.x, s[r]); s[r] = fmaf(qv.y, kv.y, s[r]);
          s[r] = fmaf(qv.z, kv.z, s[r]); s[r] = fmaf(qv.w, kv.w, s[r]);
        }
      }
    }
    if constexpr (RPR) if (j < Lk) {       // modules/rpr.py:10-41: logits = q k^T + q r^T, r = table[clip(i - j, -m, m) + m]
      const float* qr = sQ + wave * SEQ_RW * d;
#pragma unroll
      for (int r = 0; r < SEQ_RW; ++r) {
        const int rel = min(max(q_pos0 + iw + r - j, -max_rel), max_rel) + max_rel;
        const float* rp = sRK + rel * dk;
        float s2 = 0.f;
        for (int c = 0; c < d; c += 4) {
          const float4 rv4 = *reinterpret_cast<const float4*>(rp + c);
          const float4 qv = *reinterpret_cast<const float4*>(qr + r * d + c);
          s2 = fmaf(qv.x, rv4.x, s2); s2 = fmaf(qv.y, rv4.y, s2); s2 = fmaf(qv.z, rv4.z, s2); s2 = fmaf(qv.w, rv4.w, s2);
        }
        s[r] = s[r] + s2;
      }
    }
    const float mterm = (kmask != nullptr && j < Lk) ? (1.0f - kmask[(size_t)b * ldmask + j]) * (-mask_inf) : 0.f;
    // ---- online softmax: every lane of the wave holds the row's m and l
#pragma unroll
    for (int r = 0; r < SEQ_RW; ++r) {
      const bool live = j < Lk && (!causal || j <= iw + r);
      const float sv = live ? s[r] + mterm : -3.0e38f;
      const float mn = fmaxf(m[r], wave_max(sv));
      const float corr = expf(m[r] - mn);         // (first tile: exp(-3e38 - mn) = 0 on l = 0, acc = 0)
      const float p = live ? expf(sv - mn) : 0.f;
      l[r] = l[r] * corr + wave_sum(p);
      m[r] = mn;
#pragma unroll
      for (int u = 0; u < DC; ++u) {
        acc[r][u] *= corr;
        if constexpr (RPR) acc2[r][u] *= corr;
      }
      pw[r * SEQ_TK + lane] = p;
    }
    __syncthreads();
    // ---- values: lane = channel; the keys of the tile in order, four at a time (p = 0 beyond the row's last key)
    int jn = min(SEQ_TK, Lk - j0);
    if (causal) jn = min(jn, iw + SEQ_RW - j0);    // (keys above the wave's last row have p = 0 for all of its rows)
    jn = max(jn, 0);
    const int jn4 = (jn + 3) & ~3;                 // (<= SEQ_TK; rows past Lk are staged as zeros, their p is 0)
#pragma unroll
    for (int u = 0; u < DC; ++u) {
      const int c = u * 64 + lane;
      if (c < d) {
        for (int jj = 0; jj < jn4; jj += 4) {
          const float v0 = sV[(jj + 0) * d + c], v1 = sV[(jj + 1) * d + c], v2 = sV[(jj + 2) * d + c],
                      v3 = sV[(jj + 3) * d + c];
#pragma unroll
          for (int r = 0; r < SEQ_RW; ++r) {
            const float4 p4 = *reinterpret_cast<const float4*>(pw + r * SEQ_TK + jj);
            acc[r][u] = fmaf(p4.x, v0, acc[r][u]); acc[r][u] = fmaf(p4.y, v1, acc[r][u]);
            acc[r][u] = fmaf(p4.z, v2, acc[r][u]); acc[r][u] = fmaf(p4.w, v3, acc[r][u]);
          }
        }
        if constexpr (RPR) {   // o = P V + sum_j P_j r_v[clip(i - j) + m]
          for (int jj = 0; jj < jn; ++jj) {
#pragma unroll
            for (int r = 0; r < SEQ_RW; ++r) {
              const int rel = min(max(q_pos0 + iw + r - (j0 + jj), -max_rel), max_rel) + max_rel;
              acc2[r][u] = fmaf(pw[r * SEQ_TK + jj], sRV[rel * d + c], acc2[r][u]);
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < SEQ_RW; ++r) {
    const int i = iw + r;
    if (i < Lq) {
      float* op = out + (size_t)b * bso + (size_t)i * ldo + h * d;
#pragma unroll
      for (int u = 0; u < DC; ++u) {
        const int c = u * 64 + lane;
        if (c < d) {
          float o = acc[r][u];
          if constexpr (RPR) o = o + acc2[r][u];
          op[c] = o / l[r];
        }
      }
    }
  }
}

template <int DC, bool RPR>
static int launch_f32_attn_seq(const float* q, const float* k, const float* v, float* out, int B, int nh, int Lq, int Lk, int d,
                               int ldq, int ldk, int ldv, int ldo, long bsq, long bsk, long bsv, long bso, const float* kmask,
                               int ldmask, float scale, float mask_inf, const float* rpr_k, const float* rpr_v, int max_rel,
                               int q_pos0, int causal, size_t lds, hipStream_t stream) {
  auto kern = k_f32_attn_seq<DC, RPR>;
  // the product head size (d = 64) needs 49 KiB: the limit is raised once per instantiation, to the most the entry point
  // admits, not on every launch
  static bool raised = false;
  if (lds > 48 * 1024 && !raised) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       SEQ_LDS_MAX);
    if (e != hipSuccess) return zk_set_error((int)e, "zk_f32_attn_seq: hipFuncSetAttribute: %s", hipGetErrorString(e));
    raised = true;
  }
  const int nblk = (Lq + SEQ_BR - 1) / SEQ_BR;
  hipLaunchKernelGGL(kern, dim3((unsigned)((long)B * nh * nblk)), dim3(256), lds, stream, q, k, v, out, nh, Lq, Lk, d, ldq, ldk,
                     ldv, ldo, bsq, bsk, bsv, bso, kmask, ldmask, scale, mask_inf, rpr_k, rpr_v, max_rel, q_pos0, causal, nblk);
  ZK_LAUNCH_CHECK();
  return 0;
}

extern "C" int zk_f32_attn_seq(const float* q, const float* k, const float* v, float* out, int B, int nh, int Lq, int Lk, int d,
                               int ldq, int ldk, int ldv, int ldo, long bsq, long bsk, long bsv, long bso, const float* kmask,
                               int ldmask, float scale, float mask_inf, const float* rpr_k, const float* rpr_v, int max_rel,
                               int q_pos0, int causal, hipStream_t stream) {
  ZK_CHECK_ARG(q != nullptr && k != nullptr && v != nullptr && out != nullptr && B >= 0 && nh >= 1 && Lq >= 1 && Lk >= 1 &&
               d >= 4 && d % 4 == 0, "zk_f32_attn_seq: bad shape (B=%d nh=%d Lq=%d Lk=%d d=%d; d must be a multiple of 4)", B, nh,
               Lq, Lk, d);
  ZK_CHECK_ARG(d <= 128, "zk_f32_attn_seq: head size d=%d (at most 128: two channels per lane)", d);
  ZK_CHECK_ARG(ldk % 4 == 0 && bsk % 4 == 0 && (((uintptr_t)k) & 15) == 0, "zk_f32_attn_seq: keys must be 16-byte aligned rows");
  ZK_CHECK_ARG(ldq >= nh * d && ldk >= nh * d && ldv >= nh * d && ldo >= nh * d,
               "zk_f32_attn_seq: row strides ldq=%d ldk=%d ldv=%d ldo=%d are shorter than nh * d = %d", ldq, ldk, ldv, ldo, nh * d);
  ZK_CHECK_ARG(causal == 0 || causal == 1, "zk_f32_attn_seq: causal must be 0 or 1");
  ZK_CHECK_ARG(!(causal && kmask != nullptr), "zk_f32_attn_seq: causal together with kmask is not built (the reference "
               "puts no padding mask on the target side, transformer.py:136)");
  ZK_CHECK_ARG(kmask == nullptr || ldmask >= Lk, "zk_f32_attn_seq: kmask rows of ldmask=%d elements are shorter than Lk=%d",
               ldmask, Lk);
  ZK_CHECK_ARG((rpr_k == nullptr) == (rpr_v == nullptr) && (rpr_k == nullptr || (max_rel >= 0 && ((((uintptr_t)rpr_k) & 15) == 0))),
               "zk_f32_attn_seq: relative positions need both tables (16-byte aligned) and max_rel >= 0");
  ZK_CHECK_ARG((long)B * nh * ((Lq + SEQ_BR - 1) / SEQ_BR) < (1L << 31), "zk_f32_attn_seq: too many row blocks");
  if (B == 0) return 0;
  const int dk = d + ((d & 7) == 0 ? 4 : 0);
  const size_t lds = ((size_t)SEQ_BR * d + (size_t)SEQ_TK * dk + (size_t)SEQ_TK * d + 4 * SEQ_RW * SEQ_TK +
                      (rpr_k != nullptr ? (size_t)(2 * max_rel + 1) * (dk + d) : 0)) * sizeof(float);
  ZK_CHECK_ARG(lds <= SEQ_LDS_MAX, "zk_f32_attn_seq: max_rel=%d with d=%d needs %zu bytes of LDS for the two tables and the "
               "tiles (at most %d)", max_rel, d, lds, SEQ_LDS_MAX);
#define ZK_F32_SEQ(DC_, RPR_)                                                                                              \
  launch_f32_attn_seq<DC_, RPR_>(q, k, v, out, B, nh, Lq, Lk, d, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, kmask, ldmask, scale, \
                                 mask_inf, rpr_k, rpr_v, max_rel, q_pos0, causal, lds, stream)
  if (d <= 64) return rpr_k != nullptr ? ZK_F32_SEQ(1, true) : ZK_F32_SEQ(1, false);
  return rpr_k != nullptr ? ZK_F32_SEQ(2, true) : ZK_F32_SEQ(2, false);
#undef ZK_F32_SEQ
}

// ------------------------------------------------------------------------------------------------ cumulative average
// transformer_aan.py:92-108 on the training path, per (sentence b, channel c), over the positions t = 0 .. L - 1 IN ORDER:
//   use_mask = 1 (aan_mask, func.py:388-400: the softmax of the masked lower triangle, times the mask):
//       run += m_t x_t;  cnt += m_t;  avg_t = m_t run / max(cnt, 1)          (a padded row averages to exact zeros)
//   use_mask = 0 (transformer_aan.py:102-107): run += x_t;  cnt += m_t;  avg_t = run / (cnt <= 0 ? 1 : cnt)
//   out[b L + t][c] = (add != NULL ? add[b L + t][c] : 0) + avg_t            (func.py:258-275: o + aan_o)
// x, add and out are row windows (ldx / lda / ldo): out may be the right half of the [x | avg] input of z_project.
__global__ void __launch_bounds__(256) k_f32_cumavg(const float* __restrict__ x, int ldx, const float* __restrict__ mask,
                                                    const float* add, int lda, float* out, int ldo, int B, int L, int H,
                                                    int use_mask) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)B * H) return;
  const int b = (int)(idx / H), c = (int)(idx % H);
  float run = 0.f, cnt = 0.f;
  for (int t = 0; t < L; ++t) {
    const size_t r = (size_t)b * L + t;
    const float mt = mask[r];
    const float xv = x[r * ldx + c];
    cnt += mt;
    float avg;
    if (use_mask) {
      run += mt * xv;
      avg = mt * run / fmaxf(cnt, 1.f);
    } else {
      run += xv;
      avg = run / (cnt <= 0.f ? 1.f : cnt);
    }
    out[r * ldo + c] = add != nullptr ? add[r * lda + c] + avg : avg;
  }
}

extern "C" int zk_f32_cumavg(const float* x, int ldx, const float* mask, const float* add, int lda, float* out, int ldo, int B,
                             int L, int H, int use_mask, hipStream_t stream) {
  ZK_CHECK_ARG(x != nullptr && mask != nullptr && out != nullptr && B >= 0 && L >= 1 && H >= 1,
               "zk_f32_cumavg: bad arguments (B=%d L=%d H=%d)", B, L, H);
  ZK_CHECK_ARG(ldx >= H && ldo >= H && (add == nullptr || lda >= H), "zk_f32_cumavg: row strides ldx=%d lda=%d ldo=%d are shorter "
               "than H=%d", ldx, lda, ldo, H);
  ZK_CHECK_ARG(use_mask == 0 || use_mask == 1, "zk_f32_cumavg: use_mask must be 0 or 1");
  if (B == 0) return 0;
  const long n = (long)B * H;
  hipLaunchKernelGGL(k_f32_cumavg, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, ldx, mask, add, lda, out, ldo, B, L,
                     H, use_mask);
  ZK_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------ shifted embedding
// transformer.py:88-112 (training path): inputs = pad(emb * sqrt(H) + bias, one row in front)[:-1] + timing signal.
// Row i of a sentence: i == 0 -> exact zeros, else table[ids[r - 1]] * scale + bias; + timing[i] for every row.
// One wave per row.
__global__ void __launch_bounds__(256) k_f32_embed_shift(const int* __restrict__ ids, int rows, int L,
                                                         const float* __restrict__ table, const float* __restrict__ bias,
                                                         const float* __restrict__ timing, int timing_rows,
                                                         float* __restrict__ out, int H, float scale) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const int i = r % L;
  const float* t = timing + (size_t)min(i, timing_rows - 1) * H;
  const float* e = i > 0 ? table + (size_t)ids[r - 1] * H : nullptr;
  for (int c = lane; c < H; c += 64) {
    float v = 0.f;
    if (e != nullptr) { v = e[c] * scale; v = v + bias[c]; }
    out[(size_t)r * H + c] = v + t[c];
  }
}

extern "C" int zk_f32_embed_shift(const int* ids, int rows, int L, const float* table, const float* bias, const float* timing,
                                  int timing_rows, float* out, int H, float scale, hipStream_t stream) {
  ZK_CHECK_ARG(ids != nullptr && table != nullptr && bias != nullptr && timing != nullptr && out != nullptr && L >= 1 &&
               H >= 1 && timing_rows >= L, "zk_f32_embed_shift: bad arguments (L=%d H=%d timing_rows=%d)", L, H, timing_rows);
  if (rows <= 0) return 0;
  hipLaunchKernelGGL(k_f32_embed_shift, dim3((rows + 3) / 4), dim3(256), 0, stream, ids, rows, L, table, bias, timing,
                     timing_rows, out, H, scale);
  ZK_LAUNCH_CHECK();
  return 0;
}
