// zk_diverse.hip -- diverse_beam_groups / diverse_beam_strength: the group selection of a decode step under diverse beam
// search (Vijayakumar et al. 2016, the Hamming penalty; zero_amd/models/_decode.py search_tail; the rule is stated in
// tests/diverse_ref.py).
//
// The K beam rows of a sentence are G groups of Kg = K / G consecutive rows; row b K + g Kg + j is beam j of group g.  The
// step's per-row candidate lists (zk_beam_topk with B K "sentences" of beam 1: the k2 best (score, token) of every row, the
// score being (prev + logp) / length_penalty) come in; per group the 2 Kg best of its Kg k2 candidates go out, after
//   score -= lambda * cnt(v) / length_penalty,   cnt(v) = how often groups 0 .. g-1 of the sentence counted token v,
// ties to the lower beam_in_group * V + v.  A group counts the tokens of its Kg best picks that are not EOS.
//
// One wave per sentence (one 64-thread workgroup) walks the groups in order.  A lane holds up to two of the group's Kg k2
// <= 128 candidates; the counted tokens are a table of at most (G - 1) Kg <= 64 entries in LDS (a token counted twice is
// there twice); a pick is one wave arg-max round, its owner then retires the candidate.  Lane 0 stores the picks with plain
// vector stores; no atomics, nothing shared between workgroups.
#include "zk_common.h"

#define ZK_DIVERSE_K2_MAX 16      // the depth of zk_beam_topk's lists (TOPK_MAX of zk_decode.hip)
#define ZK_DIVERSE_TAB 64
#define ZK_DIVERSE_NONE 0x7fffffff

__device__ __forceinline__ bool dv_better(float s2, int i2, float s1, int i1) { return s2 > s1 || (s2 == s1 && i2 < i1); }

__global__ void __launch_bounds__(64) k_diverse_select(const float* __restrict__ cand_s, const int* __restrict__ cand_i,
                                                       float* __restrict__ out_s, int* __restrict__ out_i, int K, int G,
                                                       int k2, int V, float lambda, float penalty,
                                                       const float* __restrict__ penalty_dev, int eos_id) {
  __shared__ int tab[ZK_DIVERSE_TAB];
  const int lane = threadIdx.x, b = blockIdx.x;
  const int Kg = K / G, n = Kg * k2, keep = 2 * Kg;
  if (penalty_dev != nullptr) penalty = *penalty_dev;
  int ntab = 0;                               // wave-uniform: the table grows by the broadcast winners
  for (int g = 0; g < G; ++g) {
    float s[2];
    int f[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = lane + 64 * h;
      s[h] = -INFINITY;
      f[h] = ZK_DIVERSE_NONE;
      if (c < n) {
        const int j = c / k2, slot = c - j * k2;
        const size_t off = ((size_t)b * K + (size_t)g * Kg + j) * k2 + slot;
        const float raw = cand_s[off];
        const int v = cand_i[off];
        int cnt = 0;
        for (int i = 0; i < ntab; ++i) cnt += (tab[i] == v);
        s[h] = cnt > 0 ? raw - (lambda * (float)cnt) / penalty : raw;
        f[h] = j * V + v;
      }
    }
    float* os = out_s + ((size_t)b * G + g) * keep;
    int* oi = out_i + ((size_t)b * G + g) * keep;
    for (int r = 0; r < keep; ++r) {
      const bool second = dv_better(s[1], f[1], s[0], f[0]);
      float bs = second ? s[1] : s[0];
      int bi = second ? f[1] : f[0];
      int bt = second ? lane + 64 : lane;
      wave_argbest(bs, bi, bt, [](float s2, int i2, float s1, int i1) { return dv_better(s2, i2, s1, i1); });
      if (bt == lane) { s[0] = -INFINITY; f[0] = ZK_DIVERSE_NONE; }
      if (bt == lane + 64) { s[1] = -INFINITY; f[1] = ZK_DIVERSE_NONE; }
      if (lane == 0) { os[r] = bs; oi[r] = bi; }
      if (r < Kg && g + 1 < G) {              // the group's Kg best count, EOS excepted; the last group's are read by nobody
        const int v = bi % V;
        if (v != eos_id && ntab < ZK_DIVERSE_TAB) {
          if (lane == 0) tab[ntab] = v;
          ++ntab;
        }
      }
    }
    __syncthreads();                          // the next group's lanes read what lane 0 appended
  }
}

extern "C" {
int zk_diverse_select(const float* cand_scores, const int* cand_index, float* topk_scores, int* topk_index, int B, int K,
                      int G, int k2, int V, float lambda, float length_penalty, const float* penalty_dev, int eos_id,
                      hipStream_t stream) {
  ZK_CHECK_ARG(B >= 0 && K >= 1 && G >= 1 && V >= 1, "zk_diverse_select: bad shape (B=%d K=%d G=%d V=%d)", B, K, G, V);
  ZK_CHECK_ARG(K % G == 0, "zk_diverse_select: K=%d is no multiple of G=%d", K, G);
  const int Kg = K / G;
  ZK_CHECK_ARG(k2 >= 2 && k2 <= ZK_DIVERSE_K2_MAX, "zk_diverse_select: k2=%d outside 2 .. %d", k2, ZK_DIVERSE_K2_MAX);
  ZK_CHECK_ARG(Kg * k2 <= 128, "zk_diverse_select: a group has K/G * k2 = %d * %d candidates, more than 128", Kg, k2);
  ZK_CHECK_ARG((G - 1) * Kg <= ZK_DIVERSE_TAB, "zk_diverse_select: (G - 1) * K/G = %d counted tokens, more than %d",
               (G - 1) * Kg, ZK_DIVERSE_TAB);
  // (strictly below: 0x7fffffff is the flat index of a retired candidate)
  ZK_CHECK_ARG((long)Kg * V < 0x7fffffffL, "zk_diverse_select: K/G * V = %d * %d overflows the flat index", Kg, V);
  ZK_CHECK_ARG(lambda >= 0.f && lambda <= 3.0e38f, "zk_diverse_select: lambda=%g is negative or not finite", (double)lambda);
  ZK_CHECK_ARG(penalty_dev != nullptr || (length_penalty > 0.f && length_penalty <= 3.0e38f),
               "zk_diverse_select: length_penalty=%g is not a positive finite number", (double)length_penalty);
  if (B == 0) return 0;
  ZK_CHECK_ARG(cand_scores != nullptr && cand_index != nullptr && topk_scores != nullptr && topk_index != nullptr,
               "zk_diverse_select: the candidate lists and the outputs are required");
  hipLaunchKernelGGL(k_diverse_select, dim3((unsigned)B), dim3(64), 0, stream, cand_scores, cand_index, topk_scores,
                     topk_index, K, G, k2, V, lambda, length_penalty, penalty_dev, eos_id);
  ZK_LAUNCH_CHECK();
  return 0;
}
}  // extern "C"
