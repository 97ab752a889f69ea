// zk_ngram.hip -- no_repeat_ngram_size: the n-gram ban of a decode step (zero_amd/models/_decode.py search_tail; the rule
// is stated in tests/ngram_ref.py).
//
// A beam row has generated y_1 .. y_t (hist[r, 1 .. t]; hist[r, 0] is the start symbol of search.py:50 and belongs to no
// n-gram).  Token v is banned at step t when some start i >= 1 with i + n - 1 <= t has
//   y_i .. y_{i+n-2} == y_{t-n+2} .. y_t   and   v == y_{i+n-1},
// i.e. when emitting v would complete an n-gram the row already holds.  The banned entries of the row's logits are
// overwritten with `value` (the finite forbid value of the search tail) BEFORE the log-softmax of the tail.
//
// One wave per beam row, four rows per workgroup.  Lanes walk the start positions i = 1 + lane, + 64, ..; the history of a
// row is at most a few KiB that every lane reads through the vector L1 (the n - 1 suffix tokens are the same addresses in
// every lane: one broadcast line), so nothing is staged.  A match stores `value` with a plain vector store; several lanes
// may store the same value to the same entry, which needs no order.  No atomics, nothing but the banned entries written.
#include "zk_common.h"

#define ZK_NGRAM_MAX 16

__global__ void __launch_bounds__(256) k_ngram_ban(float* __restrict__ logits, int ld, int rows, int V,
                                                   const int* __restrict__ hist, int ldh, int time,
                                                   const int* __restrict__ time_dev, int n, float value) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int t = time_dev != nullptr ? *time_dev : time;
  if (t < n - 1 || t >= ldh) return;          // nothing to ban yet; a time word past the history is never followed
  const int* h = hist + (size_t)r * ldh;
  float* row = logits + (size_t)r * ld;
  const int* suf = h + (t - n + 2);           // y_{t-n+2} .. y_t, n - 1 tokens (none for n = 1)
  for (int i = 1 + lane; i + n - 1 <= t; i += 64) {
    bool same = true;
    for (int j = 0; j < n - 1; ++j) same = same && (h[i + j] == suf[j]);
    if (!same) continue;
    const int v = h[i + n - 1];
    if ((unsigned)v < (unsigned)V) row[v] = value;
  }
}

extern "C" {
int zk_ngram_ban(float* logits, int ld, int rows, int V, const int* hist, int ldh, int time, const int* time_dev, int n,
                 float value, hipStream_t stream) {
  ZK_CHECK_ARG(n >= 1 && n <= ZK_NGRAM_MAX, "zk_ngram_ban: n=%d outside 1 .. %d", n, ZK_NGRAM_MAX);
  ZK_CHECK_ARG(rows >= 0 && V >= 1, "zk_ngram_ban: bad shape (rows=%d V=%d)", rows, V);
  ZK_CHECK_ARG(ld >= V, "zk_ngram_ban: ld=%d is smaller than V=%d", ld, V);
  ZK_CHECK_ARG(ldh >= 1, "zk_ngram_ban: ldh=%d", ldh);
  if (time_dev == nullptr) {
    ZK_CHECK_ARG(time >= 0 && ldh > time, "zk_ngram_ban: ldh=%d does not hold y_1 .. y_t of t=%d", ldh, time);
    if (time < n - 1) return 0;
  }
  if (rows == 0) return 0;
  ZK_CHECK_ARG(logits != nullptr && hist != nullptr, "zk_ngram_ban: logits and hist are required");
  hipLaunchKernelGGL(k_ngram_ban, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, logits, ld, rows, V, hist, ldh,
                     time, time_dev, n, value);
  ZK_LAUNCH_CHECK();
  return 0;
}
}  // extern "C"
