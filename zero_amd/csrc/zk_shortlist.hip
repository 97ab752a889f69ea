// zk_shortlist.hip -- the per-batch output vocabulary of lexical shortlist decoding (zero_amd/shortlist.py; the
// candidates of search.py:143-176 are then the shortlist's ids, not the whole target vocabulary).
//
// S = {0 .. first)  U  {the first min(best, len) entries of the lexical row of every source token of the batch}, filled
// with the lowest ids not yet in S up to Vs = min(V, roundup(|S|, round)), written in ascending order.
//
// The set is a bit mask over V in the caller's workspace.  Three stream-ordered phases behind the one entry point, so no
// workgroup ever waits for another:
//   1. hipMemsetAsync clears the mask;
//   2. k_sl_mark (many workgroups): one wave per source token, its lanes stride the token's table row and set bits with
//      vector atomics (atomicOr on a mask word; the result does not depend on their order);
//   3. k_sl_finish (ONE workgroup of 1024 threads): popcount of the mask words (the `first` lowest ids are ORed in on the
//      fly) -> n and Vs; then per chunk of 1024 words an exclusive scan of the zero counts picks the words that take
//      part of the fill, an exclusive scan of the one counts gives every word the output offset of its first id, and each
//      thread writes its word's ids (a stable compaction: word order is id order).
#include "zk_common.h"

#define ZK_SL_MAX_V (1 << 22)      // 4 194 304 ids = a 512 KiB mask: what the single finishing workgroup is sized for
#define ZK_SL_THREADS 1024

// bits of word `w` that belong to ids below `limit`
__device__ __forceinline__ uint32_t sl_below(int w, int limit) {
  const int lo = w * 32;
  if (limit >= lo + 32) return 0xffffffffu;
  if (limit <= lo) return 0u;
  return (1u << (limit - lo)) - 1u;
}

__global__ void __launch_bounds__(256) k_sl_mark(const int* __restrict__ src, int rows, int ld_src, int Ls,
                                                 const int* __restrict__ lex_off, const int* __restrict__ lex_ids, int Vsrc,
                                                 int best, int V, uint32_t* __restrict__ mask) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
  const long tokens = (long)rows * Ls;
  const int nnz = lex_off[Vsrc];
  for (long t = wave; t < tokens; t += nwaves) {
    const int s = src[(t / Ls) * ld_src + (t % Ls)];
    if (s <= 0 || s >= Vsrc) continue;                    // pad, or no row in the table
    const int beg = lex_off[s], end = lex_off[s + 1];
    if (beg < 0 || end > nnz || end <= beg) continue;     // (a table that is not a CSR is not followed out of bounds)
    const int len = min(end - beg, best);
    for (int i = lane; i < len; i += 64) {
      const int id = lex_ids[beg + i];
      if (id >= 0 && id < V) atomicOr(&mask[id >> 5], 1u << (id & 31));
    }
  }
}

// exclusive prefix sum of v over the 1024 threads; total: the sum over all of them.  sm: 16 ints.
__device__ __forceinline__ int sl_scan(int v, int* sm, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  __syncthreads();                       // (the previous scan's sums have been read)
  if (lane == 63) sm[wave] = x;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < ZK_SL_THREADS / 64; ++i) {
    const int c = sm[i];
    if (i < wave) base += c;
    tot += c;
  }
  total = tot;
  return base + x - v;
}

__global__ void __launch_bounds__(ZK_SL_THREADS) k_sl_finish(const uint32_t* __restrict__ mask, int words, int V, int first,
                                                             int round, int* __restrict__ ids, int cap,
                                                             int* __restrict__ count) {
  __shared__ int sm[ZK_SL_THREADS / 64];
  const int tid = threadIdx.x;
  int mine = 0;
  for (int w = tid; w < words; w += ZK_SL_THREADS) mine += __popc((mask[w] | sl_below(w, first)) & sl_below(w, V));
  int n;
  sl_scan(mine, sm, n);
  const long up = ((long)n + round - 1) / round * round;
  const int Vs = (int)(up < (long)V ? up : (long)V);
  const int need = Vs - n;               // ids the fill adds: the lowest ones that are not in the set
  int zbase = 0, obase = 0;
  for (int w0 = 0; w0 < words; w0 += ZK_SL_THREADS) {
    const int w = w0 + tid;
    uint32_t m = 0u, zeros = 0u;
    if (w < words) {
      const uint32_t valid = sl_below(w, V);
      m = (mask[w] | sl_below(w, first)) & valid;
      zeros = valid & ~m;
    }
    const int z = __popc(zeros);
    int ztot, otot;
    const int zb = zbase + sl_scan(z, sm, ztot);
    const int take = min(max(need - zb, 0), z);
    if (take == z) {
      m |= zeros;
    } else {
      for (int i = 0; i < take; ++i) {   // the `take` lowest zero bits of the word
        const uint32_t b = zeros & (0u - zeros);
        m |= b;
        zeros ^= b;
      }
    }
    int o = obase + sl_scan(__popc(m), sm, otot);
    while (m) {
      const int b = __ffs(m) - 1;
      if (o < cap) ids[o] = w * 32 + b;  // (o < Vs <= cap by the arithmetic above)
      ++o;
      m &= m - 1u;
    }
    zbase += ztot;
    obase += otot;
  }
  for (int i = Vs + tid; i < cap; i += ZK_SL_THREADS) ids[i] = -1;
  if (tid == 0) {
    count[0] = n;
    count[1] = Vs;
  }
}

extern "C" {

int zk_shortlist_max_vocab(void) { return ZK_SL_MAX_V; }

size_t zk_shortlist_workspace(int V) { return V > 0 ? ((size_t)V + 31) / 32 * sizeof(uint32_t) : 0; }

int zk_shortlist_build(const int* src, int rows, int ld_src, int Ls, const int* lex_off, const int* lex_ids, int Vsrc,
                       int best, int first, int V, int round, int* ids, int cap, int* count, void* workspace,
                       size_t ws_bytes, hipStream_t stream) {
  ZK_CHECK_ARG(first >= 3, "zk_shortlist_build: first = %d, at least 3 is required (pad / unk / eos keep ids 0, 1, 2)", first);
  ZK_CHECK_ARG(round >= 8 && round % 8 == 0, "zk_shortlist_build: round = %d is not a positive multiple of 8", round);
  ZK_CHECK_ARG(V >= 3 && V <= ZK_SL_MAX_V, "zk_shortlist_build: V = %d is outside 3 .. %d, the vocabulary the bit mask holds",
               V, ZK_SL_MAX_V);
  // min(V, roundup(V, round)) is V: the largest shortlist is the whole vocabulary
  ZK_CHECK_ARG(cap >= V, "zk_shortlist_build: cap = %d is smaller than min(V, roundup(V, round)) = %d", cap, V);
  ZK_CHECK_ARG(ws_bytes >= zk_shortlist_workspace(V), "zk_shortlist_build: workspace of %zu bytes is too small, %zu are needed",
               ws_bytes, zk_shortlist_workspace(V));
  ZK_CHECK_ARG(rows >= 0 && Ls >= 0 && ld_src >= Ls && Vsrc >= 0 && best >= 0,
               "zk_shortlist_build: bad shape (rows=%d Ls=%d ld_src=%d Vsrc=%d best=%d)", rows, Ls, ld_src, Vsrc, best);
  ZK_CHECK_ARG(ids && count && workspace && lex_off && (src || (long)rows * Ls == 0) && (lex_ids || best == 0),
               "zk_shortlist_build: src, lex_off, lex_ids, ids, count and workspace are required");
  ZK_CHECK_ARG((((uintptr_t)workspace) & 3) == 0, "zk_shortlist_build: workspace must be aligned to 4 bytes");
  const int words = (V + 31) / 32;
  uint32_t* mask = reinterpret_cast<uint32_t*>(workspace);
  hipError_t e = hipMemsetAsync(mask, 0, (size_t)words * sizeof(uint32_t), stream);
  if (e != hipSuccess) return zk_set_error((int)e, "zk_shortlist_build: hipMemsetAsync: %s", hipGetErrorString(e));
  const long tokens = (long)rows * Ls;
  if (tokens > 0 && best > 0 && Vsrc > 0) {
    const long blocks = (tokens + 3) / 4;
    hipLaunchKernelGGL(k_sl_mark, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, stream, src, rows, ld_src, Ls,
                       lex_off, lex_ids, Vsrc, best, V, mask);
    ZK_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_sl_finish, dim3(1), dim3(ZK_SL_THREADS), 0, stream, mask, words, V, first < V ? first : V, round, ids,
                     cap, count);
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
