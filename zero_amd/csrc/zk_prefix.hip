// zk_prefix.hip -- tgt_prefix_file: the forced target prefix of a decode step (zero_amd/models/_decode.py search_tail; the
// rule is stated in tests/prefix_ref.py).
//
// Sentence b = r / rows_per_sentence of beam row r has a prefix p_b[0 .. n_b - 1] of target ids in [1, V), right-padded with
// 0 in prefix[b, 0 .. ldp - 1].  At step t < n_b (the step that chooses y_{t+1}) the row's logits become
//   value        for every column v != p_b[t], v != eos        (value: the finite forbid value of the search tail, -1e8)
//   2 * value    for v == eos
//   untouched    for v == p_b[t]
// BEFORE the log-softmax of the tail, which then gives the forced token a log-probability of exactly 0.  EOS goes lower so
// that none of the equal fillers that complete the step's top-2K is the one that ends a hypothesis.
//
// A row is spread over ceil(V / 4096) workgroups of 256 threads; thread x of workgroup c stores the 16-byte vectors
// c * 1024 + x, + 256, + 512, + 768 of the row, so a wave's store covers 1 KiB of consecutive bytes.  Vectors are counted from
// the first 16-byte aligned column of the row (a row base need not be aligned: a shortlist view, a guarded test window); the
// up to three columns ahead of it and behind the last whole vector are single stores of the row's first workgroup, and so
// are the three neighbours of the forced token in its vector.  The row's logits are never read.  Whether a row is forced is
// the same for every thread of a workgroup (one time word, one prefix word), so the exit is uniform.  Plain vector stores
// only: no atomics.
#include "zk_common.h"

#define ZK_PREFIX_THREADS 256
#define ZK_PREFIX_VECS 4          // 16-byte stores per thread: a workgroup covers 256 x 4 x 4 = 4096 columns

__global__ void __launch_bounds__(ZK_PREFIX_THREADS) k_prefix_force(float* __restrict__ logits, int ld, int V,
                                                                    const int* __restrict__ prefix, int ldp, int rps, int time,
                                                                    const int* __restrict__ time_dev, int eos_id, float value,
                                                                    int chunks) {
  const int r = blockIdx.x / chunks;
  const int chunk = blockIdx.x - r * chunks;
  const int t = time_dev != nullptr ? *time_dev : time;
  if (t < 0 || t >= ldp) return;                       // past the table: the prefix has ended for every sentence
  const int tok = prefix[(size_t)(r / rps) * ldp + t];
  if (tok <= 0 || tok >= V) return;                    // padding (or an id the row does not have): the row is free
  float* row = logits + (size_t)r * ld;
  const float low = 2.0f * value;
  int head = (int)((4u - (unsigned)(((uintptr_t)row >> 2) & 3u)) & 3u);      // columns ahead of the first aligned one
  if (head > V) head = V;
  const int nvec = (V - head) >> 2;
  int i = chunk * (ZK_PREFIX_THREADS * ZK_PREFIX_VECS) + (int)threadIdx.x;
#pragma unroll
  for (int u = 0; u < ZK_PREFIX_VECS; ++u, i += ZK_PREFIX_THREADS) {
    if (i >= nvec) break;
    const int c0 = head + 4 * i;
    if (tok >= c0 && tok < c0 + 4) {
      for (int j = 0; j < 4; ++j)
        if (c0 + j != tok) row[c0 + j] = (c0 + j == eos_id) ? low : value;
    } else {
      float4 v;
      v.x = (c0 == eos_id) ? low : value;
      v.y = (c0 + 1 == eos_id) ? low : value;
      v.z = (c0 + 2 == eos_id) ? low : value;
      v.w = (c0 + 3 == eos_id) ? low : value;
      *reinterpret_cast<float4*>(row + c0) = v;
    }
  }
  if (chunk == 0) {
    // [0, head) and [head + 4 nvec, V): at most three columns each
    const int tail0 = head + 4 * nvec;
    const int x = (int)threadIdx.x;
    const int c = x < head ? x : tail0 + (x - head);
    if (c < V && c != tok) row[c] = (c == eos_id) ? low : value;
  }
}

extern "C" {
int zk_prefix_force(float* logits, int ld, int rows, int V, const int* prefix, int ldp, int rows_per_sentence, int time,
                    const int* time_dev, int eos_id, float value, hipStream_t stream) {
  ZK_CHECK_ARG(rows >= 0 && V >= 1, "zk_prefix_force: bad shape (rows=%d V=%d)", rows, V);
  ZK_CHECK_ARG(ld >= V, "zk_prefix_force: ld=%d is smaller than V=%d", ld, V);
  ZK_CHECK_ARG(rows_per_sentence >= 1 && rows % rows_per_sentence == 0,
               "zk_prefix_force: rows=%d is no multiple of rows_per_sentence=%d", rows, rows_per_sentence);
  ZK_CHECK_ARG(ldp >= 1, "zk_prefix_force: ldp=%d", ldp);
  if (time_dev == nullptr) {
    ZK_CHECK_ARG(time >= 0, "zk_prefix_force: time=%d", time);
    if (time >= ldp) return 0;          // no sentence's prefix reaches this step
  }
  if (rows == 0) return 0;
  ZK_CHECK_ARG(logits != nullptr && prefix != nullptr, "zk_prefix_force: logits and prefix are required");
  const int per = ZK_PREFIX_THREADS * ZK_PREFIX_VECS;
  int chunks = (V / 4 + per - 1) / per;
  if (chunks < 1) chunks = 1;
  ZK_CHECK_ARG((long long)rows * chunks <= 0x7fffffffLL, "zk_prefix_force: rows=%d x %d workgroups per row", rows, chunks);
  hipLaunchKernelGGL(k_prefix_force, dim3((unsigned)(rows * chunks)), dim3(ZK_PREFIX_THREADS), 0, stream, logits, ld, V,
                     prefix, ldp, rows_per_sentence, time, time_dev, eos_id, value, chunks);
  ZK_LAUNCH_CHECK();
  return 0;
}
}  // extern "C"
