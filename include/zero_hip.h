/* zero_hip.h -- C-ABI of libzero_hip.so, the MI355X (gfx950) kernels behind the
 * Transformer training / decode hot path of bzhangGo/zero.
 *
 * The reference has NO native layer: every entry point below replaces a group of stock
 * TF1 ops issued by the cited reference lines (paths relative to the reference root).
 * A maintainer binds these with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain pointers and sizes only; device pointers unless noted; the caller owns every
 *     buffer including workspaces (query the size with the *_workspace function);
 *   - "bf16" = raw uint16 bfloat16 storage; activations and weight matrices are bf16,
 *     vectors / statistics / gradients of parameters / optimiser state are fp32;
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t); no call
 *     synchronises, allocates or keeps global state, so the calls are re-entrant and can
 *     be captured into a hipGraph;
 *   - return 0 = ok, <0 = argument error, >0 = hipError_t; message in
 *     zk_last_error_string() (thread local);
 *   - dropout: `drop_p` in [0,1), `seed` = DEVICE pointer to a uint64 step seed (read at
 *     kernel run time so a captured graph sees fresh seeds), `sid` = site id; the mask is
 *     a pure function of (seed, sid, element index) and is regenerated in the backward;
 *   - `impl`: 0 = auto (MFMA kernel when the shape allows, else the reference HIP kernel),
 *     1 = reference HIP kernel, 2 = MFMA kernel (error if unsupported).
 */
#ifndef ZERO_HIP_H_
#define ZERO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* zk_stream_t; /* hipStream_t */

int zk_version(void);
const char* zk_last_error_string(void);

/* ---- func.py:14-65 linear / func.py:327-338 ffn_layer / transformer.py:182-196 logits,
 *      and the autodiff mirrors TF builds for them (main.py:28).
 * C[M,N] = alpha * op(A)[M,K] x op(B)[K,N] (+bias[N]) (+residual[M,N]) (act) (dropout)
 *   ta=0: A is [M,lda] (K contiguous), ta=1: A is [K,lda] (M contiguous)
 *   tb=0: B is [K,ldb] (N contiguous), tb=1: B is [N,ldb] (K contiguous)
 *   out_f32: C is fp32 (else bf16).  act: 0 none, 1 ReLU (func.py:332), 2 multiply by
 *   (aux>0)*aux_scale (ReLU+dropout backward through the saved activation).          */
size_t zk_gemm_workspace(int M, int N, int K);
size_t zk_gemm_workspace_split(int M, int N, int splits);
/* Split-K product left as its partial sums (no epilogue, no reduction launch): part z = A[:, K_z] B[K_z, :] as fp32
 * [M, N] at parts + z*M*N for the z-th of *nparts_out <= splits K ranges (multiples of 64).  The consumer adds them in the
 * order z = 0, 1, .. : zk_ln_decode(parts, nparts, part_stride = M*N, bias) for the decode step's FFN output projection
 * (func.py:327-338 ffn_layer "output" at 128 rows: 64 workgroups instead of 16). */
int zk_gemm_parts(const void* A, const void* B, float* parts, int M, int N, int K, int lda, int ldb, int ta, int tb,
                  int splits, int* nparts_out, zk_stream_t stream);
/* The tail of a post-LN sub-layer in ONE launch: s = residual + dropout(bf16(A B + bias)); y = LayerNorm(s)
 * (func.py:321-324 residual_fn + func.py:289-303 layer_norm in the order of transformer.py:57-58; replaces zk_gemm followed by
 * zk_add_ln_fwd).  A [M, lda] x B [K, ldb] (no transposition), N % 64 == 0, N <= 1024.  The N/64 workgroups holding a block
 * of rows exchange the {sum, M2} of their 64 columns through `slots` (zk_gemm_add_ln_workspace bytes, zero-filled once,
 * shared by all calls on a stream) and normalise their own columns.  s_out (bf16 [M, N]), mean, rstd (fp32 [M]): what
 * zk_add_ln_bwd reads, may be null.  `epoch`: device word advanced by zk_ln_epoch_bump once per forward pass (start it at
 * 0 and bump before the first use); `site` in 1..255 differs between the calls of one pass.  *err (device int, may be
 * null) is set to 1 if a workgroup gave up waiting for a peer. */
size_t zk_gemm_add_ln_workspace(int rows, int N);
int zk_ln_epoch_bump(uint32_t* epoch, zk_stream_t stream);
int zk_gemm_add_ln(const void* A, const void* B, int M, int N, int K, int lda, int ldb, const float* bias,
                   const void* residual, int ldr, float drop_p, const uint64_t* seed, uint32_t sid, const float* gamma,
                   const float* beta, float eps, void* s_out, void* y, float* mean, float* rstd, void* slots,
                   size_t slots_bytes, const uint32_t* epoch, uint32_t site, int* err, zk_stream_t stream);
/* The backward of that tail inside the dgrad launch that completes its input gradient: dout = bf16(dY W^T + residual) is
 * never stored; dsum = d(loss)/d(s) (bf16 [M, N]), dy_out = dsum x the dropout mask of (seed, sid) (null without dropout),
 * partials (zk_gemm_ln_bwd_partials bytes: [ceil(M/64)][3][N]) = the per-row-block column sums {dout xhat, dout, dy} that
 * zk_add_ln_bwd_reduce / zk_reduce_grouped finish with nblk = ceil(M/64).  dY [M, lda], W [N, ldb] (both K contiguous).
 * Replaces zk_gemm(tb = 1, residual) + zk_add_ln_bwd(defer_reduce = 1); slots / epoch / site / err as for zk_gemm_add_ln. */
/* Attention forward + output projection + residual + LayerNorm of a sub-layer in ONE launch: workgroup (sentence, head)
 * computes its attention output (func.py:218-256, as zk_attn_fwd's MFMA kernel: att and lse are still written), waits for
 * the other heads of its sentence and runs its 64-column tile of zk_gemm_add_ln over the sentence's rows.  d = 64,
 * Lq <= 64, Lk <= 256, no relative positions; W_o [nh*64, nh*64]; flags: zk_attn_out_ln_flags bytes, zero-filled once;
 * slots / epoch / site / err as for zk_gemm_add_ln.  Returns 2 (nothing launched) when the shape is not covered. */
size_t zk_attn_out_ln_flags(int B, int nh);
int zk_attn_out_ln(const void* q, const void* k, const void* v, void* att, float* lse, int B, int nh, int Lq, int Lk, int d,
                   int ldq, int ldk, int ldv, int ldatt, const float* kmask, int causal, float scale, float mask_inf,
                   float attn_drop_p, const uint64_t* seed, uint32_t attn_sid, int kv_group, const void* Wo, int ldw,
                   const float* bias, const void* residual, int ldr, float drop_p, uint32_t sid, const float* gamma,
                   const float* beta, float eps, void* s_out, void* y, float* mean, float* rstd, void* slots,
                   size_t slots_bytes, void* flags, size_t flags_bytes, const uint32_t* epoch, uint32_t site, int* err,
                   zk_stream_t stream);
/* The same launch with the projection in FRONT of the attention inside it as well (func.py:206-216): workgroup (sentence,
 * head) first computes its own head's 64 columns of q (k, v) = x Wp + bp over its sentence's rows -- it is their only
 * consumer in the forward pass, so no exchange between workgroups is needed -- writes them (the backward reads them) and
 * goes on as zk_attn_out_ln.  pro = 3: Wp [Kp, 3 nh 64] = the merged qkv_map of a self-attention (k = q + nh*64 and
 * v = q + 2 nh*64 columns of one [B*Lq, ldq] matrix, Lk = Lq, kv_group = 1); pro = 1: Wp [Kp, nh 64] = the q_map of a
 * cross-attention (k, v given as before).  x [B*Lq, ldx] bf16, Kp a multiple of 64.  Replaces zk_gemm + zk_attn_out_ln with
 * bit-identical results (same tile function and K order).  Returns 2 (nothing launched) when the shape is not covered. */
int zk_proj_attn_out_ln(const void* x, int ldx, const void* Wp, int ldwp, const float* bp, int Kp, int pro,
                   const void* q, const void* k, const void* v, void* att, float* lse, int B, int nh, int Lq, int Lk, int d,
                   int ldq, int ldk, int ldv, int ldatt, const float* kmask, int causal, float scale, float mask_inf,
                   float attn_drop_p, const uint64_t* seed, uint32_t attn_sid, int kv_group, const void* Wo, int ldw,
                   const float* bias, const void* residual, int ldr, float drop_p, uint32_t sid, const float* gamma,
                   const float* beta, float eps, void* s_out, void* y, float* mean, float* rstd, void* slots,
                   size_t slots_bytes, void* flags, size_t flags_bytes, const uint32_t* epoch, uint32_t site, int* err,
                   zk_stream_t stream);
size_t zk_gemm_ln_bwd_partials(int rows, int N);
int zk_gemm_ln_bwd(const void* dY, const void* W, int M, int N, int K, int lda, int ldb, const void* residual, int ldr,
                   const void* s, const float* mean, const float* rstd, const float* gamma, float drop_p,
                   const uint64_t* seed, uint32_t sid, void* dsum, void* dy_out, float* partials, void* slots,
                   size_t slots_bytes, const uint32_t* epoch, uint32_t site, int* err, zk_stream_t stream);
int zk_gemm_plan(int M, int N, int K, int out_f32, int plain);  /* gen | (bm/8)<<8 | (bn/8)<<16 | splits<<24 | producer waves<<28 chosen by impl=0 */
int zk_gemm_set_generation(int gen);   /* 1 = register-staged kernel, 2 = LDS-DMA ring kernel (default) */
/* K-segmented GEMM: C bf16 [M, ldc] = sum_s A_s [M, kseg] x B_s (+ bf16 residual, may alias C) in ONE launch --
   gradient contributions that the reference accumulates with add_n over the users of a tensor (the encoder
   output feeds the cross-attention K / V projections of every decoder layer, transformer.py:120-160).
   a_segs / b_segs: host arrays of nseg (<= 16) device pointers, all segments share lda / ldb;
   tb = 1: B_s is [N, ldb] with K contiguous, tb = 0: [kseg, ldb].  kseg % 64 == 0. */
int zk_gemm_kseg(const void* const* a_segs, const void* const* b_segs, int nseg, int kseg, void* C, int M, int N,
                 int lda, int ldb, int ldc, int tb, const void* residual, int ldr, zk_stream_t stream);
int zk_gemm(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
            int ta, int tb, int out_f32, float alpha, const float* bias, const void* residual, int ldr,
            int act, const void* aux, int ldaux, float aux_scale, float drop_p, const uint64_t* seed,
            uint32_t sid, int impl, void* workspace, size_t ws_bytes, zk_stream_t stream);

/* Grouped launch of independent GEMMs with the same ta/tb in one grid (the deferred weight
 * gradients of several layers; the cross-attention k_map / v_map projections of every decoder
 * layer, func.py:206-216).  descs: DEVICE array of nprob records
 *   { const void* A, B; void* C; const float* bias; const void* res /* bf16 residual or NULL,
 *     may alias C */; int M, N, K, lda, ldb, ldc, out_f32, tile_start, tiles_n, ldr;
 *     float* colsum /* NULL, or fp32 [N]: receives sum_k B[k][n] (tb = 0, tiles 5 / 6: the bias gradient beside a
 *     weight gradient, func.py:16,58-60) */; long pad; }   (96 bytes)
 * tile_start = running sum of ceil(M/T)*ceil(N/T) with T = 128 (tile=1) or 64 (tile=4). */
int zk_gemm_grouped(const void* descs, int nprob, int total_tiles, int ta, int tb, int tile,
                    zk_stream_t stream);

/* ---- func.py:218-256 dot_attention core (+ modules/rpr.py:10-75 relative positions).
 * q/k/v/out: [B*L, ld] bf16, head h at columns [h*d,(h+1)*d) (split/combine_heads,
 * func.py:68-104, folded into addressing).  kmask: fp32 [B,Lk] (1 valid / 0 pad) or NULL;
 * causal: mask keys j > q_pos0+i; masked logits get -mask_inf added (func.py:372-387,
 * finite 1e8).  lse: fp32 [B,nh,Lq] log-sum-exp saved for the backward (may be NULL).
 * rpr_k/rpr_v: bf16 [2*max_rel+1, d] tables or NULL.  bsq/bsk/bsv: batch strides in
 * elements (0 = L*ld); kv_group: k/v/kmask batch index = b / kv_group (decode: beam-tiled
 * queries attend to un-tiled per-sentence encoder keys, search.py:36-39 never materialised).
 * pos_dev (device int, may be NULL) carries the decode time step for hipGraph replay: pos_flags bit 0
 * -> q_pos0 = *pos_dev, bit 1 -> only keys 0..*pos_dev are valid (self-attention over the k/v cache,
 * func.py:199-205, with Lk = the allocated cache length).
 * Relative positions on the MFMA kernels (d = 64) are DECOMPOSED (modules/rpr.py:10-75): the caller
 * computes rpr_gq = Q_h . rpr_k^T (FP32 [B*Lq, rpr_ldg], entry (t, h, r) at t*rpr_ldg + h*rpr_nrp + r)
 * with a GEMM, the kernel gathers it into the scores and writes rpr_pb = sums of P over the keys of each
 * relative index (same layout, bf16); the caller finishes O += rpr_pb . rpr_v.  The backward takes
 * rpr_gq, rpr_gd = dO_h . rpr_v^T (fp32) and writes rpr_pb, rpr_dsb (bf16 bucket sums of P and dS): dQ += dsb . rpr_k,
 * d rpr_k = dsb^T Q, d rpr_v = pb^T dO are the caller's GEMMs.  Without rpr_gq the reference kernels
 * apply the tables directly (any head size).
 * zk_attn_fwd with impl | 256 and rpr_k / rpr_v but no rpr_gq: the relative-position terms are FOLDED into the MFMA tile
 * (d = 64, 2*max_rel+1 <= 64): both tables are staged in LDS, G = Q_h . rpr_k^T is one MFMA pass, the scores gather from it,
 * the bucket sums of P stay in LDS and O += PB . rpr_v follows the P.V product -- no table products through HBM, no extra
 * launches, single-query decode steps included; shapes it does not cover fall back to the reference kernel (impl 0). */
int zk_attn_fwd(const void* q, const void* k, const void* v, void* out, float* lse, int B, int nh, int Lq,
                int Lk, int d, int ldq, int ldk, int ldv, int ldo, const float* kmask, int causal,
                int q_pos0, float scale, float mask_inf, const void* rpr_k, const void* rpr_v, int max_rel,
                float drop_p, const uint64_t* seed, uint32_t sid, long bsq, long bsk, long bsv, int kv_group,
                int impl, const int* pos_dev, int pos_flags, const void* rpr_gq, void* rpr_pb, int rpr_ldg,
                int rpr_nrp, zk_stream_t stream);
size_t zk_attn_bwd_workspace(int B, int nh, int Lq);
/* zk_attn_bwd with impl | 256, rpr_k / rpr_v / drpr_k / drpr_v but no decomposed products, Lq, Lk <= 64, d = 64 and a
 * workspace of zk_attn_bwd_rpr_workspace bytes: relative positions FOLDED into the single-tile backward kernel (tables,
 * G = Q.Rk^T, Gd = dO.Rv^T, bucket sums of dS / P and dQ += dsb.Rk in LDS; per-(sentence, head) table-gradient partials
 * in the workspace, summed into drpr_k / drpr_v by one reduction launch).
 * Table-gradient contract: WITH impl | 256 the call OVERWRITES drpr_k / drpr_v on every path (when the folded kernel
 * declines a shape -- alignment, ld % 8, Lq / Lk > 64, workspace -- the reference kernels run on tables the entry
 * point has cleared itself); WITHOUT the bit the reference kernels ADD to drpr_k / drpr_v with atomics and the
 * caller clears them beforehand.
 * impl | 512 (together with | 256): when the folded kernel runs, its per-(sentence, head) partials are LEFT in the
 * workspace -- fp32 [B*nh][2][64][64] behind the B*nh*Lq floats of D, (2*max_rel+1)*64 leading elements of each slab
 * valid -- and the call returns 1 instead of 0: the caller sums them (all attention layers of a step in one
 * zk_reduce_grouped launch).  When it does not run the bit is ignored and 0 is returned.
 * impl | 1024 (together with | 256): the folded kernel in its first form -- every tile of both phases resident, 151 KB of
 * LDS, one workgroup per CU -- instead of the 72-KB form (two workgroups per CU, identical results); for A/B runs and tests.
 * (oproj_dy, oproj_w) non-null: the gradient of the attention output is not read from `dout` (which may be null) but
 * computed inside the single-tile kernel as dY . W_o[h*64 .. h*64+63, :]^T -- dY bf16 [B*Lq, oproj_lddy], W_o = the
 * o_map weight [nh*64, oproj_ldw] row-major, oproj_n columns (a multiple of 128) -- i.e. the dgrad GEMM of the output
 * projection (func.py:226-240 `o = linear(o, ..., scope="o_map")` differentiated) folded into the attention backward:
 * one launch and one [B*Lq, nh*64] matrix in HBM less.  Only the single-tile kernel does it (Lq, Lk <= 64, d = 64, no
 * decomposed rpr products): when the call would run any other kernel NOTHING is launched and 2 is returned, and the caller
 * forms `dout` itself and calls again without the pair. */
size_t zk_attn_bwd_rpr_workspace(int B, int nh, int Lq);
int zk_attn_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout,
                const float* lse, void* dq, void* dk, void* dv, float* drpr_k, float* drpr_v, int B, int nh,
                int Lq, int Lk, int d, int ldq, int ldk, int ldv, int ldo, int lddo, int lddq, int lddk,
                int lddv, const float* kmask, int causal, int q_pos0, float scale, float mask_inf,
                const void* rpr_k, const void* rpr_v, int max_rel, float drop_p, const uint64_t* seed,
                uint32_t sid, int impl, void* workspace, size_t ws_bytes, const void* rpr_gq,
                const void* rpr_gd, void* rpr_pb, void* rpr_dsb, int rpr_ldg, int rpr_nrp, const void* oproj_dy,
                int oproj_lddy, const void* oproj_w, int oproj_ldw, int oproj_n, zk_stream_t stream);
/* out[i] (+)= sum over s of in[s*stride + i], i < n  (fp32; head-wise partial table gradients of the
   decomposed rpr path) */
int zk_sum_slices(float* out, const float* in, int nslices, size_t n, size_t stride, int accumulate,
                  zk_stream_t stream);

/* ---- transformer.py:16-33 / 88-119 embedding * sqrt(H) + shared bias + timing signal
 * (func.py:341-369; `timing` = host-precomputed fp32 [Lmax,H] table).  shift=1: decoder
 * training input (zero first step, transformer.py:108-110).  zero_flag: device int, !=0
 * zeroes the embedding term (transformer.py:113-115).  pos0_dev (device int, may be NULL)
 * overrides pos0 at run time, so a captured decode-step graph sees the current time step.  */
int zk_embed_fwd(const int* ids, const void* table, const float* bias, const float* timing, void* out, int B,
                 int L, int H, float scale, int shift, int pos0, const int* zero_flag, float drop_p,
                 const uint64_t* seed, uint32_t sid, const int* pos0_dev, zk_stream_t stream);
/* round 6: the encoder's and the decoder's input embeddings of a training step in ONE launch (side a: ids [B, La] as they
 * are; side b: ids [B, Lb] shifted right by one position, transformer.py:104-108); per side the arithmetic of zk_embed_fwd.
 * ln_epoch (may be NULL): the epoch word of the in-launch LayerNorm exchanges, advanced as zk_ln_epoch_bump advances it */
int zk_embed_fwd_pair(const int* ids_a, const void* table_a, void* out_a, int La, uint32_t sid_a, const int* ids_b,
                      const void* table_b, void* out_b, int Lb, uint32_t sid_b, const float* bias, const float* timing, int B,
                      int H, float scale, float drop_p, const uint64_t* seed, uint32_t* ln_epoch, zk_stream_t stream);
/* round 6: more small launches of the training step merged pairwise.  zk_embed_bwd_sorted_pair: the gradient scatters of
 * two DIFFERENT embedding tables (arguments per side as zk_embed_bwd_sorted) in one launch.  zk_colsum_pair: out = colsum(a)
 * + colsum(b) (the shared input bias of transformer.py:16-33 / 88-119; rows r % skip == 0 of a side left out when skip > 0)
 * in two launches instead of four; workspace >= zk_colsum_workspace(rows_a, N) + zk_colsum_workspace(rows_b, N). */
int zk_embed_bwd_sorted_pair(const int* rows_a, const int* seg_a, const int* uid_a, const int* n_a, int max_a, const void* dout_a,
                             float* dtable_a, int acc_a, uint32_t sid_a, const int* rows_b, const int* seg_b, const int* uid_b,
                             const int* n_b, int max_b, const void* dout_b, float* dtable_b, int acc_b, uint32_t sid_b, int H,
                             float scale, float drop_p, const uint64_t* seed, zk_stream_t stream);
int zk_colsum_pair(const void* a, int rows_a, int lda, int skip_a, uint32_t sid_a, const void* b, int rows_b, int ldb,
                   int skip_b, uint32_t sid_b, int N, float* out, float drop_p, const uint64_t* seed, void* workspace,
                   size_t ws_bytes, zk_stream_t stream);
/* The tail of the backward pass in ONE launch (+ the final k_partials_reduce of the bias sum): the grouped reductions of
 * zk_reduce_grouped (red_descs / nred / red_blocks as there; bias gradients of func.py:58-60, LayerNorm gradients of
 * func.py:289-303), both scatters of zk_embed_bwd_sorted_pair and both sides of zk_colsum_pair (the embedding and shared
 * input-bias gradients of transformer.py:16-33 / 88-119), as block ranges of one grid: they do not depend on one another,
 * each keeps the arithmetic and the summation order of the launch it replaces (same bits).  dout_x: bf16 [T_x, H], ld = H,
 * also the column sum's input (rows r % skip_x == 0 left out when skip_x > 0); T_x is max_uniq of the sort arrays too.
 * zero_rows_b > 0 (needs acc_b = 0): every row r < zero_rows_b of dtable_b whose id is NOT in uid_b is written as zeros
 * (the rows in uid_b are the ones the scatter writes), so dtable_b needs no zero fill before the backward.
 * workspace >= zk_colsum_workspace(T_a, H) + zk_colsum_workspace(T_b, H). */
int zk_step_tail(const void* red_descs, int nred, int red_blocks, const int* rows_a, const int* seg_a, const int* uid_a,
                 const int* n_a, int T_a, const void* dout_a, float* dtable_a, int acc_a, int skip_a, uint32_t sid_a,
                 const int* rows_b, const int* seg_b, const int* uid_b, const int* n_b, int T_b, const void* dout_b,
                 float* dtable_b, int acc_b, int skip_b, uint32_t sid_b, int H, float scale, int zero_rows_b, float* dbias,
                 float drop_p, const uint64_t* seed, void* workspace, size_t ws_bytes, zk_stream_t stream);
/* dtable (fp32 [V,H]) and dbias (fp32 [H]) are ACCUMULATED into with atomics. */
int zk_embed_bwd(const int* ids, const void* dout, float* dtable, float* dbias, int B, int L, int H,
                 float scale, int shift, float drop_p, const uint64_t* seed, uint32_t sid, zk_stream_t stream);

/* Same gradient without atomics: the host (which owns the ids) sorts token rows by id; one wave
 * per distinct id sums its rows.  rows_sorted [n_used], seg [n_uniq+1], uid [n_uniq] int32 device
 * arrays, n_uniq_dev device int (<= max_uniq).  accumulate=0 overwrites the touched rows.      */
int zk_embed_bwd_sorted(const int* rows_sorted, const int* seg, const int* uid, const int* n_uniq_dev,
                        int max_uniq, const void* dout, float* dtable, int H, float scale, int accumulate,
                        float drop_p, const uint64_t* seed, uint32_t sid, zk_stream_t stream);

/* ---- func.py:321-324 residual_fn + func.py:289-303 layer_norm (post-LN, eps inside
 * rsqrt): out = LN(x + dropout(y)).  sum_out/mean/rstd are saved for the backward.    */
int zk_add_ln_fwd(const void* x, const void* y, const float* gamma, const float* beta, void* out,
                  void* sum_out, float* mean, float* rstd, int rows, int H, float eps, float drop_p,
                  const uint64_t* seed, uint32_t sid, zk_stream_t stream);
size_t zk_add_ln_bwd_workspace(int rows, int H);
/* dsum = d(x + drop(y)); dy = dsum*dropmask (only written when drop_p>0); dgamma/dbeta and
 * dbias_prev (= column sum of dy: bias grad of the linear that produced y) are OVERWRITTEN. */
int zk_add_ln_bwd(const void* dout, const void* sum, const float* mean, const float* rstd, const float* gamma,
                  void* dsum, void* dy, float* dgamma, float* dbeta, float* dbias_prev, int rows, int H,
                  float drop_p, const uint64_t* seed, uint32_t sid, void* workspace, size_t ws_bytes,
                  int defer_reduce, zk_stream_t stream);
/* defer_reduce=1: only the per-block partial sums are written to `workspace` (which must then be
 * private to this call); finish them later, possibly on another stream, with: */
int zk_add_ln_bwd_reduce(const void* workspace, int rows, int H, float* dgamma, float* dbeta, float* dbias_prev,
                         zk_stream_t stream);

/* column sum of a bf16 [rows,N] matrix -> fp32 [N] (bias gradients, func.py:58-60) */
size_t zk_colsum_workspace(int rows, int N);
int zk_colsum(const void* a, int rows, int N, int lda, float* out, void* workspace, size_t ws_bytes,
              zk_stream_t stream);
/* skip_L>0: skip rows r with r%skip_L==0 (shifted decoder input); accumulate: out += ;
 * dropout mask index = r*N + c (the shared embedding bias gradient, transformer.py:27,102) */
int zk_colsum_ex(const void* a, int rows, int N, int lda, float* out, int skip_L, int accumulate, float drop_p,
                 const uint64_t* seed, uint32_t sid, void* workspace, size_t ws_bytes, zk_stream_t stream);

/* Grouped column reductions (all bias / LayerNorm-parameter gradients of a layer group in two
 * launches).  DEVICE descriptor arrays:
 *   colsum : { const void* a; float* partials; int rows, N, lda, gy, block_start, pad; }   (40 B)
 *            gy = zk_colsum_rowchunks(rows); blocks of problem = ceil(N/64)*gy
 *   reduce : { const float* partials; float* out[3]; int nblk, nq, H, block_start; }       (48 B)
 *            blocks of problem = nq*ceil(H/16); nblk = gy (colsum) or zk_ln_bwd_blocks(rows) */
int zk_colsum_grouped(const void* descs, int nprob, int total_blocks, zk_stream_t stream);
int zk_reduce_grouped(const void* descs, int nprob, int total_blocks, zk_stream_t stream);
int zk_ln_bwd_blocks(int rows);
int zk_colsum_rowchunks(int rows);

/* ---- util.py:88-103 label_smooth + transformer.py:198-207 cross entropy on fp32 logits.
 * ce_out[r] = -sum soft*log_softmax - normaliser; dlogits (bf16 [rows,ld], NULL to skip)
 * = w[r]*(softmax - soft).                                                            */
int zk_ce_fused(const float* logits, const int* ids, const float* w, float* ce_out, void* dlogits, int rows,
                int V, int ld, float label_smooth, zk_stream_t stream);
/* zk_ce_fused with the per-sentence loss and its mean (zk_loss_reduce; util.py:88-103, transformer.py:198-211) formed by the
 * block that arrives LAST instead of a launch of its own -- the same code and order of sums.  arrive: a device word the
 * caller zeroed ONCE; every call leaves it zero again.  ids [B, L], rows = B * L; loss may be NULL. */
int zk_ce_fused_tail(const float* logits, const int* ids, const float* w, float* ce_out, void* dlogits, int rows, int V,
                     int ld, float label_smooth, float* per_sample, float* loss, int B, int L, uint32_t* arrive,
                     zk_stream_t stream);
/* transformer.py:208-216: mask=(id!=0); w = loss_scale*mask/(len_b*B); per-sentence loss and mean */
int zk_target_stats(const int* ids, float* mask, float* w, int B, int L, float loss_scale, zk_stream_t stream);
int zk_loss_reduce(const float* ce, const int* ids, float* per_sample, float* loss, int B, int L,
                   zk_stream_t stream);
int zk_make_mask(const int* ids, float* mask, int n, zk_stream_t stream);
/* Everything the training step derives from the ids alone, in ONE launch at the head of the (captured) step
 * (zk_prep.hip): what TensorFlow does on the device for the reference -- the grouping of the token rows by id inside the
 * gradient of tf.nn.embedding_lookup (tf.IndexedSlices / unsorted_segment_sum, main.py:28), the padding masks
 * (func.py:372-387) and the loss weights (transformer.py:198-211).
 *   src_ids int32 [B, Ls], tgt_ids int32 [B, Lt] (NULL: source side only);
 *   *_rows [B*L], *_seg [B*L + 1], *_uid [B*L], *_n [1]: the inputs of zk_embed_bwd_sorted -- token rows sorted by
 *   (id, row), i.e. the stable grouping; target side: row (b, t) carries id[b, t-1], rows with t = 0 none
 *   (transformer.py:99-113).  A NULL *_rows pointer skips that side's sort;
 *   smask [B, Ls], tmask / tw [B, Lt] fp32 (each optional): as zk_make_mask / zk_target_stats;
 *   max_id: every id is below it (the larger vocabulary; 0 = unknown): lets the sort run on 32-bit keys (id << bits(rows)
 *   | row) when they fit, ~3x faster than the 64-bit network;
 *   scratch: zk_batch_prep_workspace(B*Ls) + zk_batch_prep_workspace(B*Lt) bytes (0 up to 16384 rows per side). */
size_t zk_batch_prep_workspace(int rows);
int zk_batch_prep(const int* src_ids, const int* tgt_ids, int B, int Ls, int Lt, int* src_rows, int* src_seg,
                  int* src_uid, int* src_n, int* tgt_rows, int* tgt_seg, int* tgt_uid, int* tgt_n, float* smask,
                  float* tmask, float* tw, float loss_scale, int max_id, void* scratch, size_t scratch_bytes,
                  zk_stream_t stream);
/* Up to 16 small device-to-device copies in one launch (host arrays of device pointers / byte counts, 4-byte granularity):
 * the id-dependent arrays of the next batch move from the staging buffers a side stream filled (upload + zk_batch_prep,
 * overlapping the previous step) into the static buffers of the captured step. */
int zk_copy_many(void* const* dsts, const void* const* srcs, const size_t* nbytes, int n, zk_stream_t stream);
int zk_all_equal(const int* ids, int n, int value, int* flag, zk_stream_t stream);

/* ---- transformer_aan.py:92-117,165-192 average attention network (train-time scan + gate) */
int zk_aan_fwd(const void* x, const float* mask, void* cat, int B, int L, int H, int use_mask,
               zk_stream_t stream);
/* use_mask bit 0: aan_mask (run.py:117); bit 1 (backward only): dcat[:, H:] is already folded into dyg
   (the use_ffn variant, transformer_aan.py:176-183) */
int zk_add_bf16(void* out, int ldo, const void* a, int lda, const void* b, int ldb, int rows, int cols,
                zk_stream_t stream);
int zk_aan_bwd(const void* dcat, const void* dxg, const void* dyg, const void* ds, const float* mask, void* dx,
               int B, int L, int H, int use_mask, zk_stream_t stream);
int zk_aan_gate_fwd(const void* z, const void* cat, void* out, int rows, int H, zk_stream_t stream);
int zk_aan_gate_bwd(const void* dg, const void* z, const void* cat, void* dz, void* dxg, void* dyg, int rows,
                    int H, zk_stream_t stream);

/* ---- utils/cycle.py:86-101 + tf.train.AdamOptimizer (main.py:178-181) on flat buffers.
 * hyper (device fp32[12]): lr_t, beta1, beta2, eps, grad_scale, clip_norm(0=off), gnorm(in), skipped(out),
 * EMA decay (zk_ema), gnorm upper bound of safe_nan (main.py:325-329; 0 = off), [10] STICKY count of updates that
 * were skipped or saw a non-finite gradient norm (never cleared by the kernels: the loop reads it before every
 * display / checkpoint, main.py:316-319), 1 reserved.
 * zk_l2norm: out[0] = scale*||x||_2; zk_adam's pnorm_out = ||p|| before the update.  The update (and the EMA)
 * is skipped, and hyper[7] set, when gnorm is not finite or exceeds the bound.
 * zk_adam_step: the whole update of a step.  norm_free = 1 (cycle.py:98-101: clip_grad_norm 0.0, and no safe_nan --
 * the update does not depend on the global norm, which is only reported): gradient norm -> hyper[6] (+ flags),
 * TF1 Adam, bf16 shadow refresh and parameter norm in ONE pass over the flat buffers (the reference fetches
 * train_op and gradient_norm together, main.py:309-312); norm_free = 0: hyper[6] must hold the norm (zk_l2norm).
 * seed (device uint64, may be NULL): the dropout step seed, advanced by one in the same launch.
 * skip_word (device int, may be NULL; round 5): non-zero = a launch of this step reported a fault of its own (the error word
 * of the in-launch LayerNorm exchange, zk_gemm_add_ln's `err`): the update is NOT applied, hyper[6] = NaN, hyper[7] = 1 and
 * the sticky hyper[10] is incremented -- the failure-detection rule of main.py:316-332 applied on the device, on the step
 * that failed.  The word itself is left as it is (the host reads and reports it).
 * zk_norm_flag: fold a norm that zk_l2norm wrote to hyper[6] AFTER per-bucket updates into hyper[7] / hyper[10]. */
size_t zk_norm_workspace(void);
int zk_l2norm(const float* x, size_t n, float scale, float* out, void* workspace, size_t ws_bytes,
              zk_stream_t stream);
int zk_adam(float* p, const float* g, float* m, float* v, void* shadow_bf16, size_t n, float* hyper,
            float* pnorm_out, void* workspace, size_t ws_bytes, zk_stream_t stream);
size_t zk_adam_step_workspace(void);
int zk_adam_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, size_t n, float* hyper,
                 float* pnorm_out, uint64_t* seed, int norm_free, const int* skip_word, void* workspace, size_t ws_bytes,
                 zk_stream_t stream);
/* zk_adam_step with the finish of its norm_free form (cycle.py:94-101: gradient norm -> hyper[6] / [7] / [10], parameter
 * norm -> pnorm_out) done by the block of the Adam pass that arrives LAST instead of a one-block launch of its own: the
 * same per-block partials added in the same order (same bits), one launch for the whole update.  arrive: a device word
 * the caller zeroed ONCE; every call leaves it zero again (a graph replay starts clean).  No block waits for another.
 * norm_free = 0: exactly zk_adam_step. */
int zk_adam_step_fold(float* p, const float* g, float* m, float* v, void* shadow_bf16, size_t n, float* hyper,
                      float* pnorm_out, uint64_t* seed, int norm_free, const int* skip_word, void* workspace,
                      size_t ws_bytes, uint32_t* arrive, zk_stream_t stream);
int zk_norm_flag(float* hyper, zk_stream_t stream);
int zk_cast_f32_bf16(const float* x, void* y, size_t n, zk_stream_t stream);
int zk_cast_bf16_f32(const void* x, float* y, size_t n, zk_stream_t stream);
int zk_zero(void* p, size_t bytes, zk_stream_t stream);
/* Row-sparse exchange of an embedding-table gradient between data-parallel ranks (the reference moves it as
 * tf.IndexedSlices: values / indices concatenated across towers and de-duplicated, utils/parallel.py:142-181).
 * Payload of one rank = [ids int32 x R][rows x R x H] (fp32 or bf16 rows; unused slots carry id -1):
 *   zk_rows_pack        slot u < *n_uniq_dev: ids[u] = uid[u], rows[u] = dtable[uid[u]] (cast); clear_rows != 0 also
 *                       zeroes that table row, so that the table is rebuilt from the payloads of ALL ranks
 *   zk_rows_scatter_add dtable[ids[u]] += rows[u] for every valid slot of ONE payload (ids unique inside a payload: no
 *                       atomics; the payloads of the N ranks are added by N launches in rank order, so every rank ends
 *                       with a bit-identical table)
 * R, H multiples of 4. */
size_t zk_rows_payload_bytes(int R, int H, int bf16);
/* dst bf16 [cols, ld_dst] = transpose of src bf16 [rows, ld_src]: the operand layout of the fused decode kernels (a
 * projection weight with its input dimension contiguous), made once per weight version */
int zk_transpose_bf16(const void* src, int ld_src, void* dst, int ld_dst, int rows, int cols, zk_stream_t stream);
int zk_rows_pack(float* dtable, const int* uid, const int* n_uniq_dev, void* out, int R, int H, int out_bf16,
                 int clear_rows, zk_stream_t stream);
int zk_rows_scatter_add(float* dtable, const void* payload, int R, int H, int in_bf16, int vocab_rows,
                        zk_stream_t stream);
/* host-only CRC32C of a byte range (seed crc = 0 for a fresh checksum): TensorFlow-bundle checkpoint
   tensors, utils/saver.py:75,131-170 */
uint32_t zk_crc32c(const void* data, size_t n, uint32_t crc);
int zk_spin(uint32_t usec, zk_stream_t stream);   /* measurement aid: occupy the stream for usec (<= 200 ms) */
int zk_tune(int key, int value);   /* A/B switches for measurements; key 0 = wide LayerNorm-backward kernel */
/* utils/cycle.py:113-119 (tf.train.ExponentialMovingAverage): ema -= (1 - hyper[8]) * (ema - p); skipped like
   the Adam update when hyper[6] (gradient norm) is not finite */
int zk_ema(float* ema, const float* p, const float* hyper, size_t n, zk_stream_t stream);
int zk_axpby_f32(float* y, const float* x, float a, float b, size_t n, zk_stream_t stream);

/* ---- utils/parallel.py:134-208 average_gradients -> RCCL sum collectives over xGMI on the caller's stream (the 1/N
 * of the tower mean is zk_adam_step's grad_scale).  The communicator is an opaque handle OWNED BY THE CALLER:
 * rank 0 draws a 128-byte id (zk_comm_unique_id) and ships it to the other ranks by its own means (here: the
 * torch.distributed store), every rank calls zk_comm_init (collective; the current HIP device is the rank's GPU) and
 * later zk_comm_destroy.  librccl is dlopen()ed on first use: zk_comm_available() = 0 on a box without it.
 * dtype: 0 fp32, 1 bf16 (all-gather also 2 = int32).  Errors: 1000 + ncclResult_t. */
int zk_comm_available(void);
int zk_comm_unique_id(void* id128);
int zk_comm_init(const void* id128, int nranks, int rank, void** comm_out);
int zk_comm_destroy(void* comm);
int zk_comm_size(const void* comm);
int zk_comm_allreduce(void* comm, void* buf, size_t count, int dtype, zk_stream_t stream);
/* n in-place all-reduces in ONE RCCL group; bufs / counts are HOST arrays */
int zk_comm_allreduce_multi(void* comm, void* const* bufs, const size_t* counts, int n, int dtype,
                            zk_stream_t stream);
/* recv[r*count .. (r+1)*count) <- send of rank r (row-sparse source-embedding gradient, parallel.py:142-181) */
int zk_comm_allgather(void* comm, const void* send, void* recv, size_t count, int dtype, zk_stream_t stream);
/* round 6: ordering a second stream behind the compute stream WITHOUT an event on the compute stream (an event recorded
 * there slows every dispatch of that stream: 40-65 us per training step, DESIGN.md 6e).  flag: an 8-byte aligned device
 * word that only ever grows.  zk_flag_add (on the producer's stream): flag += 1 with agent-scope release; zk_flag_wait (on
 * the consumer's stream): a one-thread kernel that ends once flag >= target (gives up after ~2 s and sets *err, may be
 * NULL).  zero_amd/utils/parallel.py RcclComm uses the pair per gradient bucket under ZERO_HIP_COMM_HANDOFF=flag. */
int zk_flag_add(void* flag, zk_stream_t stream);
int zk_flag_wait(const void* flag, unsigned long long target, int* err, zk_stream_t stream);

/* dropout plumbing */
int zk_dropout_mask(float* out, size_t n, float drop_p, const uint64_t* seed, uint32_t sid, zk_stream_t stream);
int zk_seed_advance(uint64_t* seed, uint64_t inc, zk_stream_t stream);

/* ---- search.py:143-176 decode step tail (see zk_decode.hip) */
/* Precondition of zk_beam_topk / zk_beam_topk_advance and their EOS-ban scalars (forbid_id / forbid_value, stepbuf[2]): the
   logits are finite everywhere; what the kernels return for inf or NaN logits is undefined. */
size_t zk_beam_topk_workspace(int B, int K, int k2);
int zk_beam_topk(const float* logits, const float* prev_log_probs, float* topk_scores, int* topk_index, int B,
                 int K, int V, int ld, int k2, float temperature, float length_penalty, int forbid_id,
                 float forbid_value, const int* scal_dev, void* workspace, size_t ws_bytes, zk_stream_t stream);
/* search.py:198-210 beam reordering: dst row r <- src row index[r] (NULL: r); bytes, multiples of 16 */
int zk_gather_rows(const void* src, size_t src_stride, const int* index, void* dst, size_t dst_stride, int rows,
                   size_t row_bytes, zk_stream_t stream);
/* period > 0: rows = n_tables * period stacked tables share one index of length period (the caches of every
   decoder layer reordered by one launch) */
int zk_gather_rows_ex(const void* src, size_t src_stride, const int* index, void* dst, size_t dst_stride, int rows,
                      size_t row_bytes, int period, zk_stream_t stream);
/* transformer_fuse (func.py:258-275) merged attention: the averaged v_map(query) term summed into the
   cross-attention heads.  train: out = att + cumavg_mask(vq) and its transpose; decode: cache += vq,
   att += cache/(t+1) (func.py:262-272) */
int zk_cumavg_add_fwd(const void* vq, const float* mask, const void* att, void* out, int B, int L, int H,
                      zk_stream_t stream);
int zk_cumavg_bwd(const void* dy, const float* mask, void* dvq, int B, int L, int H, zk_stream_t stream);
int zk_fuse_decode(const void* vq, float* cache, void* att, int rows, int H, float inv_count, const int* time_dev,
                   zk_stream_t stream);
/* Host side of a beam-search step in C (pure host code, no device work): the stop test of search.py:85-113
   and the alive / finished bookkeeping of search.py:168-228 on int32 [B, K, Tcap] sequence buffers. */
int zk_beam_host_should_stop(int B, int K, const float* log_probs, const float* fin_scores,
                             const unsigned char* fin_flags, const float* max_target_length, const int* mtl_i,
                             int time, float alpha);
int zk_beam_host_step(int B, int K, int V, int Tcap, int time, const float* topk_scores, const int* topk_idx,
                      int* seq, int* fin_seq, float* log_probs, float* scores, float* fin_scores,
                      unsigned char* fin_flags, const int* mtl_i, int eos_id, int pad_id, float penalty,
                      int* flat_idx, int* next_tok);
/* The same two statements with the search state RESIDENT ON THE DEVICE, as the first and the last node of
   the decode-step graph (no host round trip per step; replaces the per-step session.run boundary of
   search.py:60-275 / main.py:399-460).  ctrl int32[4]: [0] steps taken (= next time step), [1] stopped,
   [2] error (the step ran into the cache cap Tmax).  stepbuf int32[>=3]: [0] time, [1] length penalty of the
   step (fp32 bits), [2] banned symbol or -1 -- the per-step scalars the other kernels of the graph read.
   pen_table[t] = ((5 + t + 1) / 6)^alpha for t < Tcap and max_lp[b] = ((5 + max_target_length[b]) / 6)^alpha
   are computed by the caller in fp32.  prepare: stop test of the coming step; when it fires the state is
   frozen (advance becomes a no-op), otherwise it publishes the step scalars.  advance: alive / finished
   update from the step's [B, 2K] survivors; writes the next step's tokens, log-probs (prev) and flat beam
   indices.  seq / fin_seq: int32 [B, K, Tcap]; fin_flags: int32 [B, K].  K <= 16, 2*K*Tcap*4 <= 64 KiB. */
int zk_beam_dev_prepare(int* ctrl, int* stepbuf, const float* pen_table, const float* max_lp, const int* mtl_i,
                        const float* topk_scores, const int* topk_idx, int* seq, int* fin_seq, float* log_probs,
                        float* scores, float* fin_scores, int* fin_flags, int* flat_idx, int* next_tok,
                        float* prev, int B, int K, int V, int Tcap, int Tmax, int eos_id, int pad_id,
                        zk_stream_t stream);
int zk_beam_dev_advance(int* ctrl, int* stepbuf, const float* pen_table, const float* max_lp, const int* mtl_i,
                        const float* topk_scores, const int* topk_idx, int* seq, int* fin_seq, float* log_probs,
                        float* scores, float* fin_scores, int* fin_flags, int* flat_idx, int* next_tok,
                        float* prev, int B, int K, int V, int Tcap, int Tmax, int eos_id, int pad_id,
                        zk_stream_t stream);
/* zk_beam_topk on the step's logits (k2 = 2K, log-softmax, length penalty and EOS ban read from stepbuf[1..2]) followed by
 * zk_beam_dev_advance, with the merge of the chunked top-k and the bookkeeping in ONE launch (both are one block per
 * sentence; search.py:115-236).  Same results as the two calls.  Returns -2 with nothing launched when the shape needs
 * the unchunked top-k: call the two entry points then.  workspace: zk_beam_topk_workspace(B, K, 2K). */
int zk_beam_topk_advance(const float* logits, int ld, float temperature, float forbid_value, void* workspace,
                         size_t ws_bytes, int* ctrl, int* stepbuf, const float* pen_table, const float* max_lp,
                         const int* mtl_i, const float* topk_scores, const int* topk_idx, int* seq, int* fin_seq,
                         float* log_probs, float* scores, float* fin_scores, int* fin_flags, int* flat_idx, int* next_tok,
                         float* prev, int B, int K, int V, int Tcap, int Tmax, int eos_id, int pad_id, zk_stream_t stream);
/* search.py:143-145 (enable_noise_beam_search): logits += Gumbel noise -log(-log(u + eps) + eps), util.py:189-195 */
int zk_add_gumbel(float* logits, int rows, int V, int ld, float eps, const uint64_t* seed, uint32_t sid,
                  zk_stream_t stream);
/* ---- main.py:65-115 ensemble decoding, the combination of main.py:101-103 (see zk_ensemble.hip):
 * out[r, v] = log( (1/M) * sum_m softmax(logits_m[r, :])[v] ) for v < V (columns >= V of `out` are left untouched), in the
 * stable form logsumexp_m(logits_m[r, v] - logsumexp(logits_m[r, :])) - log M with fp32 arithmetic and accumulation: where
 * every member's probability underflows, the result is the finite log-probability instead of the reference's tf.log(0) =
 * -inf (the one intended deviation); M = 1 is a plain fp32 log-softmax.
 * logits / ld: HOST arrays of M device pointers (fp32 [rows, ld[m]], 16-byte aligned) and leading dimensions (multiples
 * of 4, >= V); they travel by value in the launch arguments, so the call allocates, copies and synchronises nothing and
 * can be captured.  M <= zk_ensemble_max() (8), otherwise an argument error.
 * workspace: zk_ensemble_logprob_workspace(rows, M, V) bytes (the per-chunk row statistics of the first pass). */
int zk_ensemble_max(void);
size_t zk_ensemble_logprob_workspace(int rows, int M, int V);
int zk_ensemble_logprob(const float* const* logits, const int* ld, int M, int rows, int V, float* out, int ld_out,
                        void* workspace, size_t ws_bytes, zk_stream_t stream);
/* k/v cache rows with the time step in device memory (hipGraph replay of func.py:199-205 and of the
   beam reorder search.py:206-209).  mode 0 (append): dst[r][*time_dev] <- src[r] (unit_bytes);
   mode 1 (reorder): dst[r][0 .. *time_dev) <- src[index[r]][0 .. *time_dev) in units of unit_bytes;
   max_units bounds the launch; period as in zk_gather_rows_ex. */
int zk_cache_rows(const void* src, size_t src_stride, const int* index, void* dst, size_t dst_stride, int rows,
                  size_t unit_bytes, int max_units, const int* time_dev, int mode, int period, zk_stream_t stream);
/* transformer_aan.py:110-112: cache += x; cat = [x | cache/(t+1)] */
/* Decode-step form of the residual + LayerNorm of the decoder with its row-local neighbours in the same launch
 * (transformer_aan.py:165-192, func.py:289-303): the sub-layer output y is ybuf (bf16 [rows, H]), or
 *   z/cat_in != NULL: the AAN gate bf16(sigma(z_i) x + sigma(z_f) y) of cat_in = [x | y], kept in registers (z NULL with
 *                     parts: z = bf16(sum_p parts + bias) over rows of 2H), or
 *   parts != NULL   : bf16(sum_p parts[p*part_stride + r*H + :] + bias) -- the output projection left as nparts fp32
 *                     partial products by zk_dec_cross / zk_dec_self (summed in the fixed order p = 0 .. nparts-1);
 * out = LayerNorm(x + y); cache/cat_out != NULL: the next layer's running sum and [x | average] follow (zk_aan_decode).
 * The row stays in registers from the loads to the output and is rounded to bf16 where the separate kernels stored bf16:
 * the first two forms equal zk_aan_gate_fwd + zk_add_ln_fwd + zk_aan_decode bit for bit.  ybuf is never written: it is
 * read in the first form and ignored in the others. */
int zk_ln_decode(const void* x, void* ybuf, const float* gamma, const float* beta, void* out, int rows, int H, float eps,
                 const void* z, const void* cat_in, const float* parts, int nparts, long part_stride, const float* bias,
                 float* cache, void* cat_out, float inv_count, const int* time_dev, zk_stream_t stream);
/* One attention sub-layer of a cached decode step in ONE launch (transformer.py:120-175 at Lq = 1; func.py:124-287):
 * grid B * nh, workgroup (sentence b, head h) owns the sentence's R <= 8 beam rows: [prologue: the previous sub-layer's
 * residual + LayerNorm, arguments x .. time_dev as zk_ln_decode; gamma == NULL: none, x is the block input; otherwise
 * xout receives the normalised rows] -> q_h = x Wq[:, h] + bq -> softmax(scale q_h K_h^T + mask) V_h -> the head's share
 * ctx_h Wo[h rows, :] of the output projection as fp32 out_parts[h][B*R][H].  The caller finishes with
 * zk_ln_decode(parts = out_parts, nparts = nh, part_stride = B*R*H, bias = o_map bias) or the next prologue.
 * The projection weights are passed TRANSPOSED (wqt = q_map^T [H, H], wot = o_map^T [H, H]: row = output channel, input
 * dimension contiguous, row strides ldwq / ldwo) so that a matrix-core fragment is one 16-byte load.
 * d = 64 per head, H = nh * 64 a power of two in 128 .. 2048.  Cross: keys / values of sentence b at k + b*bsk + j*ldk
 * (func.py:206-216 mk / mv), kmask [B, ldmask] (1 = valid) or NULL.  Values are rounded to bf16 where the launch-per-op
 * path stores bf16.
 * Relative positions (modules/rpr.py:10-75 with last = 1; round 4): rpr_k / rpr_v bf16 [2 max_rel + 1, 64] or NULL
 * (max_rel <= 31).  The query sits at position pos (*pos_dev when given; self-attention: its time step): key j adds
 * q . rpr_k[clip(pos - j) + max_rel] to its score and P_j rpr_v[clip(pos - j) + max_rel] to the context. */
int zk_dec_cross(const void* x, void* ybuf, const float* gamma, const float* beta, void* xout, int H, float eps,
                 const void* z, const void* cat_in, const float* parts, int nparts, long part_stride, const float* bias,
                 float* cache, void* cat_out, float inv_count, const int* time_dev, const void* wqt, int ldwq,
                 const float* bq, const void* k, const void* v, int ldk, int ldv, long bsk, long bsv, const float* kmask,
                 int ldmask, const void* wot, int ldwo, float* out_parts, int B, int R, int nh, int Lk, float scale,
                 float mask_inf, const void* rpr_k, const void* rpr_v, int max_rel, int pos, const int* pos_dev,
                 zk_stream_t stream);
/* Beam rows per workgroup of zk_dec_cross / zk_dec_self (1 .. 16; 0 = built-in default); returns the previous setting.
 * A measurement knob (scripts/dec_attn_trace.py): results do not depend on it. */
int zk_dec_group(int n);
/* Self-attention over per-beam caches (func.py:199-205): wqkvt = qkv_map^T [3H, H] (q | k | v rows), bias [3H];
 * kcache / vcache bf16 [B*R, Tmax, H]: this step's key / value are written at slot time (*time_dev when given), keys
 * 0 .. time attended. */
int zk_dec_self(const void* x, void* ybuf, const float* gamma, const float* beta, void* xout, int H, float eps,
                const void* z, const void* cat_in, const float* parts, int nparts, long part_stride, const float* bias,
                float* cache, void* cat_out, float inv_count, const int* ln_time_dev, const void* wqkvt, int ldw,
                const float* bqkv, void* kcache, void* vcache, int Tmax, int time, const int* time_dev, const void* wot,
                int ldwo, float* out_parts, int B, int R, int nh, float scale, const void* rpr_k, const void* rpr_v,
                int max_rel, zk_stream_t stream);
int zk_aan_decode(const void* x, float* cache, void* cat, int rows, int H, float inv_count, const int* time_dev,
                  zk_stream_t stream);
/* dynamic LDS bytes a zk_dec_cross / zk_dec_self workgroup needs for hidden size H and Lk keys (a CU has 160 KiB):
 * lets the caller choose the launch-per-op path for shapes that do not fit, before the batch starts decoding.
 * max_rel < 0: without relative-position tables. */
size_t zk_dec_attn_lds(int H, int Lk, int max_rel);
/* Decoder input of one decode position in one launch (transformer.py:88-119; was zk_all_equal + zk_embed_fwd +
 * zk_aan_decode): every fed id == pad_id (first step) -> zero embedding, else table[id] * scale + bias; + timing[pos];
 * cache / cat != NULL: the first layer's average-attention update (transformer_aan.py:110-112).  *pos_dev overrides
 * pos0 and inv_count (= 1 / (pos + 1)).
 * gather_src != NULL: the beam reorder of the running sums of all nl layers rides along (search.py:206-209):
 * cache [nl, rows, H] <- gather_src[l][gather_idx[r]] (+ the new row for layer 0). */
int zk_dec_embed(const int* ids, int pad_id, const void* table, const float* bias, const float* timing, void* out, int rows,
                 int H, float scale, int pos0, const int* pos_dev, float* cache, void* cat, float inv_count,
                 const float* gather_src, const int* gather_idx, int nl, zk_stream_t stream);

/* The replay loop of the device-resident search in one call (no interpreter between two decode steps): the two parity
 * graphs of the step alternately (starting with `parity`), poll replays per group, the search's 16-byte control block
 * {time, stop, overflow, -} copied into one of two pinned 4-int slots behind every group and read one group later; ends
 * when the stop flag is up or more than max_launch replays went out, with the stream drained.  search.py:85-113 (the stop
 * test) decides on the device; this only carries the flag to the host. */
int zk_beam_dev_run(void* graph_even, void* graph_odd, int parity, const int* ctrl_dev, int* ctrl_pinned8, int max_launch,
                    int poll, zk_stream_t stream, int* launched_out, int* newest_slot_out);

/* ---- round 5: the fp32 decode path (hp.decode_dtype = "float32"; zero_amd/csrc/zk_f32.hip, zero_amd/models/_decode_f32.py).
 * The reference computes in float32 by default (utils/dtype.py:12-15, run.py `default_dtype`); this mode rounds where it
 * rounds -- fp32 MASTER weights, fp32 activations, fp32 accumulation -- so that greedy / beam hypotheses can be compared
 * token for token with the fp32 oracle (the bf16 path cannot be: two correct implementations that round at different points
 * part on ~3 % of the sentences).  Every matrix is plain fp32 row-major; all pointers are device pointers.
 *   zk_f32_gemm       func.py:14-65 linear / transformer.py:182-196 logits: C[M,N] = A[M,K] x (tb ? B[N,K]^T : B[K,N])
 *                     (+ bias[N]) (act 1: ReLU, func.py:332).  K % 4 == 0, lda % 4 == 0 (tb: ldb % 4 == 0), A (tb: B) 16-byte
 *                     aligned.  v_mfma_f32_32x32x2_f32 = an fp32 fmaf chain per output in a fixed k order.
 *   zk_f32_embed      transformer.py:16-33 / 88-119: out[r] = table[ids[r]] * scale + bias + timing[pos0 (or *pos_dev) + r % L];
 *                     all_pad (device flag from zk_all_equal, may be NULL): non-zero -> the embedding part is exact zeros
 *                     (transformer.py:113-115, the first decode step).
 *   zk_f32_add_ln     func.py:321-324 + 289-303: out = gamma (s - mean) / sqrt(var + eps) + beta, s = x + y (y may be NULL).
 *   zk_f32_attn       func.py:218-256 on q [B][Lq][..] / k, v [B / kv_group][Lk][..] (row strides ld*, sentence strides bs*
 *                     in elements; head h at columns h d ..): q * scale, + (1 - kmask) * (-mask_inf) (func.py:372-387;
 *                     kmask fp32 [B / kv_group, ldmask] may be NULL), softmax, x V.  nkeys_dev (may be NULL): only the
 *                     first *nkeys_dev + 1 keys exist (the self-attention cache of decode position *nkeys_dev).
 *                     rpr_k / rpr_v (may be NULL; modules/rpr.py:10-75): relative-position tables [2 max_rel + 1, d] --
 *                     logits += q . r_k[clip(i - j) + max_rel], o += sum_j p_j r_v[...], i = q_pos0 (or *q_pos_dev) + row.
 *   zk_f32_add_rows   out[r] = a[r] + b[r]: the merged attention's o + aan_o (func.py:258-275, transformer_fuse).  Row strides
 *                     lda, ldb, ldo in elements, each >= cols (refused otherwise); out == a with ldo == lda is in place.
 *   zk_f32_aan_step   transformer_aan.py:110-112: cat[r] = [x[r] | (x[r] + cache[r]) / (t + 1)], cache[r] += x[r].
 *   zk_f32_gate       transformer_aan.py:186-189: g = sigmoid(z[:, :H]) cat[:, :H] + sigmoid(z[:, H:]) cat[:, H:].
 * (cache appends and beam reorders are byte moves: zk_cache_rows / zk_gather_rows_ex with 4-byte elements.) */
int zk_f32_gemm(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, int tb,
                const float* bias, int act, zk_stream_t stream);
int zk_f32_embed(const int* ids, int rows, int L, const float* table, const float* bias, const float* timing, int timing_rows,
                 float* out, int H, float scale, int pos0, const int* pos_dev, const int* all_pad, zk_stream_t stream);
int zk_f32_add_ln(const float* x, const float* y, const float* gamma, const float* beta, float* out, int rows, int H, float eps,
                  zk_stream_t stream);
int zk_f32_attn(const float* q, const float* k, const float* v, float* out, int B, int nh, int Lq, int Lk, int d, int ldq,
                int ldk, int ldv, int ldo, long bsq, long bsk, long bsv, long bso, const float* kmask, int ldmask, int kv_group,
                float scale, float mask_inf, const int* nkeys_dev, const float* rpr_k, const float* rpr_v, int max_rel,
                int q_pos0, const int* q_pos_dev, zk_stream_t stream);
int zk_f32_aan_step(const float* x, float* cache, float* cat, int rows, int H, int time, const int* time_dev,
                    zk_stream_t stream);
int zk_f32_gate(const float* z, const float* cat, float* g, int rows, int H, zk_stream_t stream);
int zk_f32_add_rows(const float* a, int lda, const float* b, int ldb, float* out, int ldo, int rows, int cols,
                    zk_stream_t stream);
/* round 6: row-local neighbours of the fp32 decode step's launches folded together (a step is a chain of ~5 us launches).
 *   zk_f32_ln_fused    zk_f32_add_ln with, optionally, the average-attention gate as the producer of y (z / cat_in given,
 *                      x = ybuf = NULL: y = sigmoid(z_i) x_c + sigmoid(z_f) y_c and the residual is x_c = cat_in[:, :H];
 *                      transformer_aan.py:186-192) and / or the NEXT layer's average attention from the normalised row
 *                      (cache / cat_out given: cache += out, cat_out = [out | cache / (t + 1)]; transformer_aan.py:110-112).
 *                      H % 4 == 0, H <= 2048, every pointer 16-byte aligned.
 *   zk_f32_embed_step  zk_f32_embed for one decode position with the all-pad test of transformer.py:113-115 inside the
 *                      launch (pad_id >= 0) and, optionally, the first layer's average attention (cache / cat_out).
 *   zk_f32_gemm_legacy A/B switch: 1 = the round-5 GEMM kernels for every shape; returns the old value (< 0: query). */
int zk_f32_ln_fused(const float* x, const float* ybuf, const float* z, const float* cat_in, const float* gamma,
                    const float* beta, float* out, int rows, int H, float eps, float* cache, float* cat_out, int time,
                    const int* time_dev, zk_stream_t stream);
int zk_f32_embed_step(const int* ids, int rows, const float* table, const float* bias, const float* timing, int timing_rows,
                      float* out, int H, float scale, int pos0, const int* pos_dev, int pad_id, float* cache, float* cat_out,
                      zk_stream_t stream);
int zk_f32_gemm_legacy(int on);

/* ---- the fp32 scorer (hp.score_dtype = "float32"; zero_amd/csrc/zk_f32_seq.hip, zero_amd/models/_score_f32.py): the
 * training-path forward of transformer.py:15-216 on fp32 masters, activations and accumulation.  It runs on the zk_f32_*
 * entry points above plus three full-sequence kernels:
 *   zk_f32_attn_seq     func.py:218-256 for Lq >= 1 query rows per sentence, operands as zk_f32_attn (ld* row strides, bs*
 *                       sentence strides in elements, head h at columns h d ..; kmask fp32 [B, ldmask] may be NULL:
 *                       + (1 - kmask) * (-mask_inf), func.py:372-387, finite -- a fully masked row comes out uniform;
 *                       rpr_k / rpr_v may be NULL, modules/rpr.py:10-75: logits += q . r_k[clip(i - j, -max_rel, max_rel)
 *                       + max_rel], o += sum_j p_j r_v[...], i = q_pos0 + row).  causal != 0 (func.py:388-391, the
 *                       decoder's self-attention, transformer.py:128-137): keys j > i take no part -- probability exactly 0,
 *                       which is what the reference's additive -1e8 gives in fp32 -- and key tiles above a row block are not
 *                       visited; causal together with kmask is refused (transformer.py:136 puts no padding mask on the
 *                       target side).  One workgroup per block of 32 query rows of a (sentence, head); keys and values
 *                       staged in LDS in tiles of 64, once per block; online softmax, fp32 throughout; LDS use does not
 *                       depend on Lk.  d % 4 == 0, d <= 128, key rows 16-byte aligned.  B = 0 returns 0.
 *   zk_f32_cumavg       transformer_aan.py:92-108 on the training path: out[b, t] = (add[b, t] +) the running mean of x[b, 0..t]
 *                       per channel, summed in position order.  use_mask 1 (aan_mask, func.py:392-400): padded positions
 *                       neither count nor contribute and average to zero; use_mask 0 (transformer_aan.py:102-107): every x
 *                       contributes, the divisor is the number of valid positions so far (1 where that is 0).  x / add / out
 *                       are row windows (ldx / lda / ldo elements): out may be the right half of z_project's [x | avg]
 *                       input; add (may be NULL) is the cross-attention output of transformer_fuse (func.py:258-275).
 *   zk_f32_embed_shift  transformer.py:88-112: row i of a sentence of L rows = table[ids[i - 1]] * scale + bias, row 0 = zeros;
 *                       + timing[i] on every row (func.py:341-369). */
int zk_f32_attn_seq(const float* q, const float* k, const float* v, float* out, int B, int nh, int Lq, int Lk, int d, int ldq,
                    int ldk, int ldv, int ldo, long bsq, long bsk, long bsv, long bso, const float* kmask, int ldmask,
                    float scale, float mask_inf, const float* rpr_k, const float* rpr_v, int max_rel, int q_pos0, int causal,
                    zk_stream_t stream);
int zk_f32_cumavg(const float* x, int ldx, const float* mask, const float* add, int lda, float* out, int ldo, int B, int L,
                  int H, int use_mask, zk_stream_t stream);
int zk_f32_embed_shift(const int* ids, int rows, int L, const float* table, const float* bias, const float* timing,
                       int timing_rows, float* out, int H, float scale, zk_stream_t stream);

/* ---- lexical shortlist decoding (zero_amd/shortlist.py; see zk_shortlist.hip): the per-batch output vocabulary.  The
 * candidates of search.py:143-176 are then the ids of the shortlist instead of the whole target vocabulary.
 *   src      int32 [rows, ld_src], the first Ls columns of a row are its source ids; ids outside (0, Vsrc) are skipped
 *            (0 = pad)
 *   lex_off  int32 [Vsrc + 1], lex_ids int32 [lex_off[Vsrc]]: the lexical table as CSR, row s = the target ids of source
 *            id s by falling probability; entries outside [0, V) are skipped
 *   S = {0 .. min(first, V)}  U  {the first min(best, len) entries of the row of every source id of the batch};  n = |S|;
 *   Vs = min(V, roundup(n, round)); the lowest ids not in S are added until |S| = Vs.
 *   ids[0 .. Vs) = S ascending, ids[Vs .. cap) = -1, count = {n, Vs}.     Exact and deterministic.
 * Argument errors (nothing launched, every buffer untouched): first < 3; round not a positive multiple of 8;
 * V outside 3 .. zk_shortlist_max_vocab() (4 194 304: the bit mask one finishing workgroup scans); cap < min(V,
 * roundup(V, round)) = V; ws_bytes < zk_shortlist_workspace(V) (the mask: 4 bytes per 32 ids). */
int zk_shortlist_max_vocab(void);
size_t zk_shortlist_workspace(int V);
int zk_shortlist_build(const int* src, int rows, int ld_src, int Ls, const int* lex_off, const int* lex_ids, int Vsrc,
                       int best, int first, int V, int round, int* ids, int cap, int* count, void* workspace,
                       size_t ws_bytes, zk_stream_t stream);

/* ---- no_repeat_ngram_size (see zk_ngram.hip; the rule is stated in tests/ngram_ref.py): the n-gram ban of a decode step,
 * between the optional Gumbel noise and the fused search tail (search.py:143-176).
 *   logits   fp32 [rows, ld], V candidates per row; hist int32 [rows, ldh]: row r has generated y_1 .. y_t, y_i at
 *            hist[r * ldh + i] (index 0 is the search's start symbol and belongs to no n-gram)
 *   t        = *time_dev when time_dev != NULL (device memory, read by the kernel: one captured node serves every step),
 *            else `time`
 *   Token v is banned when t >= n - 1 and some i with 1 <= i, i + n - 1 <= t has y_i .. y_{i+n-2} == y_{t-n+2} .. y_t and
 *   v == y_{i+n-1}; n = 1 bans every token generated so far.  logits[r * ld + v] = value for every banned v of row r;
 *   nothing else is written.  A history token outside [0, V) bans nothing.  Under time_dev a word outside [n - 1, ldh)
 *   makes the launch a no-op.
 * Argument errors (nothing launched, every buffer untouched): n outside 1 .. 16; ld < V; rows < 0; with time by value,
 * time < 0 or ldh <= time.  rows == 0, or time by value below n - 1: returns 0 without a launch. */
int zk_ngram_ban(float* logits, int ld, int rows, int V, const int* hist, int ldh, int time, const int* time_dev, int n,
                 float value, zk_stream_t stream);

/* ---- tgt_prefix_file (see zk_prefix.hip; the rule is stated in tests/prefix_ref.py): the forced target prefix of a decode
 * step, the last launch ahead of the search tail (search.py:143-176), after the n-gram ban, the truncation and the noise.
 *   logits   fp32 [rows, ld], V candidates per row; prefix int32 [rows / rows_per_sentence, ldp], right-padded with 0: the
 *            token sentence b must emit at step t is prefix[b * ldp + t]
 *   t        = *time_dev when time_dev != NULL (device memory, read by the kernel: one captured node serves every step),
 *            else `time`
 *   Row r (sentence r / rows_per_sentence) is forced when 0 <= t < ldp and its token p is in [1, V):
 *   logits[r * ld + v] = value for every v < V but p and eos_id, 2 * value for v == eos_id (eos_id < 0: no such entry);
 *   logits[r * ld + p] and the columns V .. ld - 1 are not written, and the row is never read.  A row that is not forced is
 *   not written at all.  ld need not be a multiple of 4 and a row base need not be 16-byte aligned.
 * Argument errors (nothing launched, every buffer untouched): ld < V; rows < 0; rows % rows_per_sentence != 0; ldp < 1;
 * with time by value, time < 0.  rows == 0, or time by value >= ldp: returns 0 without a launch. */
int zk_prefix_force(float* logits, int ld, int rows, int V, const int* prefix, int ldp, int rows_per_sentence, int time,
                    const int* time_dev, int eos_id, float value, zk_stream_t stream);

/* ---- sampling_topk / sampling_topp (see zk_sample.hip; the rule is stated in tests/sampling_ref.py): the truncation of a
 * decode step's logits, after the n-gram ban and before the Gumbel noise and the fused search tail.
 *   logits   fp32 [rows, ld], V finite candidates per row.  With s = softmax(row), c(v) = #{u : x_u > x_v} and
 *            M(v) = sum of s_u over x_u > x_v, token v is KEPT iff
 *              c(v) < min_keep  or  ((topk == 0 or c(v) < topk) and (topp == 0 or M(v) < topp));
 *            every other entry of the row is overwritten with `value`.  Tokens tied in value share their fate: the kept set
 *            is {v : x_v >= tau} for one threshold per row, and the result is deterministic (integer sums only).
 *   Only dropped entries are written; the columns V .. ld-1 never.  One launch, no workspace.  topk == 0 && topp == 0, or
 *   rows == 0: returns 0 without a launch.  topp == 1 keeps every token.  Rows of at most 32768 candidates are staged in LDS
 *   and fetched from memory once; longer rows are re-read per pass.
 * Argument errors (nothing launched, every buffer untouched): ld < V; V < 1; rows < 0; topk < 0; topp outside [0, 1];
 * min_keep < 1; logits NULL with rows > 0. */
int zk_sample_truncate(float* logits, int ld, int rows, int V, int topk, float topp, int min_keep, float value,
                       zk_stream_t stream);

/* ---- diverse_beam_groups / diverse_beam_strength (see zk_diverse.hip; the rule is stated in tests/diverse_ref.py): the
 * group selection of a decode step under diverse beam search.  The K rows of a sentence are G groups of K/G consecutive rows.
 *   cand_scores / cand_index   fp32 / int32 [B*K, k2]: every row's k2 best (score, token), best first -- zk_beam_topk with
 *            B*K "sentences" of beam 1, so the score is (prev + logp) / length_penalty and the index the token.
 *   topk_scores / topk_index   fp32 / int32 [B*G, 2K/G]: per group, in the order g = 0 .. G-1, the 2K/G best of its K/G * k2
 *            candidates under score - lambda * cnt(v) / length_penalty, where cnt(v) is how often the groups before it counted
 *            token v in this step; ties go to the lower index = beam_in_group * V + v.  A group counts the tokens, EOS
 *            (eos_id) excepted, of its K/G best picks.
 *   length_penalty by value, or read from penalty_dev (a device float, stepbuf + 1) at run time when that is not NULL.
 * One launch, one wave per sentence, no workspace, no atomics.  B == 0: returns 0 without a launch.
 * Argument errors (-1, nothing launched, every buffer untouched): B < 0; K, G or V < 1; K % G != 0; k2 outside 2 .. 16;
 * K/G * k2 > 128; (G-1) * K/G > 64; K/G * V >= INT_MAX; lambda negative or not finite; length_penalty not positive and finite
 * with penalty_dev NULL; a NULL buffer with B > 0. */
int zk_diverse_select(const float* cand_scores, const int* cand_index, float* topk_scores, int* topk_index, int B, int K,
                      int G, int k2, int V, float lambda, float length_penalty, const float* penalty_dev, int eos_id,
                      zk_stream_t stream);

/* ---- transformer_l0drop at inference (models/transformer_l0drop.py:16-135, 244-273; modules/l0norm.py:75-96, 166-177)
 * A learned hard-concrete gate drops encoder outputs; cross-attention runs over the kept ones plus ONE slot (index 0, a
 * zero key / value) that carries the number of dropped positions as its softmax weight.
 *   zk_l0_gate     enc: encoder rows [B*Ls, H] (row stride ld elements), bf16 or fp32 (f32 != 0); smask fp32 [B, Ls]
 *                  (non-zero = a source token); W fp32 [H], b0 fp32 [1]: the fp32 MASTERS of source_pruning in both modes
 *                  (the keep decision is discrete: the dot product runs in fp32).  Per sentence b:
 *                    gate[b, j] = clip(sigmoid(enc[b, j, :] . W + b0) * 1.2 - 0.1, 0, 1)         fp32 [B, Ls]
 *                    pos[b, 0 .. nkeep[b])  the kept positions (gate != 0 and smask != 0) in ascending order, -1 behind
 *                    nkeep[b], ndrop[b] = (number of source tokens) - nkeep[b];  *kmax = max_b nkeep[b]   (int32)
 *                  H and ld multiples of 4, rows aligned to four elements.
 *   zk_l0_compact  Lm >= 1 + *kmax slots per sentence, every element of the outputs is written:
 *                    mem[b, 0, :] = 0;  mem[b, 1 + i, :] = enc[b, pos[b, i], :] * gate (rounded to the storage type) for
 *                    i < nkeep[b], exact zeros behind                     [B*Lm, H] of enc's type, row stride ldm
 *                    gmask[b, 0] = ndrop[b] > 0;  gmask[b, 1 + i] = i < nkeep[b]               fp32 [B, Lm]
 *                    kbias[b, 0] = log(max(ndrop[b], 1));  0 elsewhere                         fp32 [B, Lm]
 *   zk_dec_cross_kb / zk_f32_attn_kb   zk_dec_cross / zk_f32_attn with kbias fp32 [.., ldmask] (may be NULL: then they ARE
 *                  those calls) added to the scaled score of key j next to the mask term: exp(l + log c) equals the
 *                  reference's exp(l) * c, so the softmax weighs slot 0 by its count. */
int zk_l0_gate(const void* enc, int ld, int f32, const float* smask, const float* W, const float* b0, int B, int Ls, int H,
               float* gate, int* pos, int* nkeep, int* ndrop, int* kmax, zk_stream_t stream);
int zk_l0_compact(const void* enc, int ld, int f32, const float* gate, const int* pos, const int* nkeep, const int* ndrop,
                  int B, int Ls, int H, int Lm, void* mem, int ldm, float* gmask, float* kbias, zk_stream_t stream);
int zk_dec_cross_kb(const void* x, void* ybuf, const float* gamma, const float* beta, void* xout, int H, float eps,
                    const void* z, const void* cat_in, const float* parts, int nparts, long part_stride, const float* bias,
                    float* cache, void* cat_out, float inv_count, const int* time_dev, const void* wqt, int ldwq,
                    const float* bq, const void* k, const void* v, int ldk, int ldv, long bsk, long bsv, const float* kmask,
                    int ldmask, const float* kbias, const void* wot, int ldwo, float* out_parts, int B, int R, int nh,
                    int Lk, float scale, float mask_inf, const void* rpr_k, const void* rpr_v, int max_rel, int pos,
                    const int* pos_dev, zk_stream_t stream);
int zk_f32_attn_kb(const float* q, const float* k, const float* v, float* out, int B, int nh, int Lq, int Lk, int d, int ldq,
                   int ldk, int ldv, int ldo, long bsq, long bsk, long bsv, long bso, const float* kmask, int ldmask,
                   const float* kbias, int kv_group, float scale, float mask_inf, const int* nkeys_dev, const float* rpr_k,
                   const float* rpr_v, int max_rel, int q_pos0, const int* q_pos_dev, zk_stream_t stream);

/* ---- transformer_rela at inference (modules/rela.py:13-109; models/transformer_rela.py:48, 134, 154 call it in place
 * of func.dot_attention): ReLU attention weights and a gated RMSNorm over ALL H channels of the combined heads.
 *   zk_rela_attn      bf16 q / k / v / out, fp32 arithmetic;  zk_f32_rela_attn   fp32 throughout.
 *                  Operands as zk_f32_attn: B query sentences of Lq rows, nh heads of d channels, Lk keys; ld* row strides
 *                  and bs* sentence strides in elements (q / k / v may be column slices of one matrix); sentence b reads
 *                  the keys / values / mask of sentence b / kv_group (B a multiple of kv_group); kmask fp32
 *                  [B / kv_group, ldmask], non-zero = the key takes part (may be NULL); nkeys_dev (may be NULL): the
 *                  number of valid keys is min(*nkeys_dev + 1, Lk), read on the device, and no later key slot is read.
 *                  post_scale / post_gate: the fp32 MASTERS of .../dot_attention/post/{scale, gate} [H] in both forms.
 *                    s_j = (q * qscale) . k_j  per head                                 (rela.py:60-63)
 *                    w_j = relu(s_j) * (kmask_j != 0)      multiplied, never added      (rela.py:66-72)
 *                    c   = concat over the heads of sum_j w_j v_j                       (rela.py:77-78)
 *                    out = post_scale * c * rsqrt(mean over H of c^2 + eps) * sigmoid(post_gate * c)   (rela.py:95-109)
 *                  A row without a positive score gives exact zeros.  bf16 form: d % 8 == 0, d <= 128, H <= 2048, key and
 *                  output rows 16-byte aligned; fp32 form: any d <= 256, H <= 2048.  Otherwise -1 and a message. */
int zk_rela_attn(const void* q, const void* k, const void* v, void* out, int B, int nh, int Lq, int Lk, int d, int ldq, int ldk,
                 int ldv, int ldo, long bsq, long bsk, long bsv, long bso, const float* kmask, int ldmask, int kv_group,
                 float qscale, const int* nkeys_dev, const float* post_scale, const float* post_gate, float eps,
                 zk_stream_t stream);
int zk_f32_rela_attn(const float* q, const float* k, const float* v, float* out, int B, int nh, int Lq, int Lk, int d, int ldq,
                     int ldk, int ldv, int ldo, long bsq, long bsk, long bsv, long bso, const float* kmask, int ldmask,
                     int kv_group, float qscale, const int* nkeys_dev, const float* post_scale, const float* post_gate,
                     float eps, zk_stream_t stream);

/* ---- transformer_fixup at inference and scoring (modules/fixup.py:15-26 shift_layer / scale_layer, 29-55 ffn_layer;
 * models/transformer_fixup.py:47-73, 136-189): the Transformer without LayerNorm.  Row-wise element-wise passes over
 * [rows, H] matrices, row strides ld* in elements.  Every scalar is an fp32 MASTER [1] read ON THE DEVICE at run time (a
 * captured step graph follows a weight reload); a NULL scalar pointer is the neutral value.
 *   zk_fixup_residual     the sub-layer boundary (fixup.py:15-26; transformer_fixup.py:59-60, 73, 154-155, 189):
 *                           x_out[r,c]  = x[r,c] + a * y[r,c]        a = *scale (NULL: 1);  x NULL: 0;  y NULL: 0
 *                           xs_out[r,c] = b * (x_out[r,c] - o)       o = *offset (NULL: 0);  b = *scale2 (NULL: 1)
 *                         x / x_out: fp32, the residual stream (may be the same buffer; x_out NULL: not written);
 *                         y / xs_out: the storage type (bf16; fp32 in zk_f32_fixup_residual); xs_out NULL: not written.
 *                         xs_out is formed from the unrounded fp32 x_out and rounded once (round to nearest even).
 *                         One launch is, by its arguments: residual + the next sub-layer's shift; the shift of an embedding
 *                         (x NULL, the embedding row as y); the encoder's final scale(shift(x)); the decoder's final shift.
 *   zk_fixup_relu_shift   the middle of the feed-forward layer (fixup.py:45-50): out = relu(h - o) - o, the SAME offset
 *                         twice (ffn_layer/shift/offset under AUTO_REUSE); out may be h; storage type, fp32 arithmetic.
 * H (F) and every row stride multiples of 8 elements, every matrix 16-byte aligned; otherwise -1 and a message, and
 * nothing is launched.  Every product and sum is rounded on its own (no fused multiply-add). */
int zk_fixup_residual(const float* x, int ldx, const void* y, int ldy, const float* scale, const float* offset,
                      const float* scale2, float* x_out, int ldxo, void* xs_out, int ldxs, int rows, int H, zk_stream_t stream);
int zk_f32_fixup_residual(const float* x, int ldx, const float* y, int ldy, const float* scale, const float* offset,
                          const float* scale2, float* x_out, int ldxo, float* xs_out, int ldxs, int rows, int H,
                          zk_stream_t stream);
int zk_fixup_relu_shift(const void* h, int ldh, const float* offset, void* out, int ldo, int rows, int F, zk_stream_t stream);
int zk_f32_fixup_relu_shift(const float* h, int ldh, const float* offset, float* out, int ldo, int rows, int F,
                            zk_stream_t stream);

/* ---- rnnsearch at inference (models/rnnsearch.py; rnns/rnn.py, rnns/atr.py:32-60; func.py:107-161): zk_rnn.hip.
 * bf16 forms: GEMM operands (U, p, the projected memory, the memory, the copies) are bf16, arithmetic fp32;
 * zk_f32_* forms: fp32 throughout.  Strides in elements.  -1 and a message on a bad argument, nothing launched.
 *   zk_rnn_atr_step   ONE time step of ONE ATR cell (twin gates) for R rows, with the mask carry of rnns/rnn.py:41-49:
 *                       q = h U + b;  i = sigmoid(p + q);  f = sigmoid(p - q);  o = i p + f h;  out = m o + (1 - m) h
 *                     h = h_prev[idx[r]] (idx NULL: row r; h_prev NULL: the zero state); h_prev fp32 [n_prev, H], row
 *                     stride ldh; index values are clamped to 0 .. n_prev - 1.  U [H, H] (bf16 shadow / fp32 master),
 *                     b fp32 [H], p [R, H] the precomputed input projection.  mask NULL or fp32, the value of row r at
 *                     mask[r ldm].  out: the fp32 state (stride ldo, so a scan can write into [B, Ls, H] at its
 *                     position); out_copy (may be NULL): the same in the storage type.  The state is fp32 in both forms;
 *                     in the bf16 form only the matrix-core operand is a rounded copy of h.  out must not overlap
 *                     h_prev (every column tile reads whole rows of it): refused.  bf16 form: H % 8 == 0, H <= 4096.
 *   zk_add_attn       additive attention of one decode step for R = (sentences x kv_group) beam rows:
 *                       logit_j = v . tanh(qa + pm_j) + (1 - kmask_j) * -neg;  a = softmax_j;  ctx = sum_j a_j mem_j
 *                     qa [R, M]; pm, mem [R / kv_group, Ls, M] (row stride ld*, sentence stride bs*): read once for the
 *                     kv_group rows of a sentence; v fp32 [M]; kmask NULL or fp32 [R / kv_group, ldmask] (1 = valid).
 *                     ctx fp32 [R, M]; ctx_copy (may be NULL) the same in the storage type.  Any Ls (online softmax over
 *                     tiles of 64 keys); M <= 2048; bf16 form: M, ldpm, bspm multiples of 8.
 *   zk_rnn_embed      out[r] = table[ids[r]] + bias (no scale, no timing signal); zeros where pad >= 0 and EVERY id of
 *                     the launch equals pad (rnnsearch.py:101-103).  table [V, E] of the storage type, bias fp32.  An id
 *                     outside [0, V) is CLAMPED: a negative id reads row 0, an id >= V reads row V - 1 (no fault, no error).
 *   zk_rnn_bias_tanh  y = tanh(x + bias) for fp32 rows x (bias may be NULL); input row r is written to the output rows
 *                     r rep .. r rep + rep - 1 of out_f32 (fp32) and / or out_copy (storage type). */
int zk_rnn_atr_step(const float* h_prev, int ldh, int n_prev, const int* idx, const void* U, int ldu, const float* b,
                    const void* p, int ldp, const float* mask, int ldm, float* out, int ldo, void* out_copy, int ldc, int R,
                    int H, zk_stream_t stream);
int zk_f32_rnn_atr_step(const float* h_prev, int ldh, int n_prev, const int* idx, const float* U, int ldu, const float* b,
                        const float* p, int ldp, const float* mask, int ldm, float* out, int ldo, float* out_copy, int ldc,
                        int R, int H, zk_stream_t stream);
/* ONE time step of ONE GRU cell (rnns/gru.py:32-57; models/rnnsearch_deepatt.py with cell=gru) as TWO launches -- the
 * candidate product contracts r (.) h over all of K and r needs the gate product of every column:
 *   zk_rnn_gru_gates  [z | r] = sigmoid(xg + h Ug + bg);  rh = r (.) h.   h = h_prev[idx[r]] as in zk_rnn_atr_step (idx NULL:
 *                     row r; h_prev NULL: the zero state -- no product, rh = 0).  Ug [H, 2 H] and xg [R, 2 H] (the input
 *                     projection x Wg) of the storage type, the z columns first; bg fp32 [2 H].  z: fp32 [R, H]; rh [R, H]
 *                     in the storage type: the operand of the second product, formed from the fp32 state, rounded once.
 *                     z (and, in the fp32 form, rh) must not overlap h_prev: refused.
 *   zk_rnn_gru_out    c = tanh(xh + rh Uh + bh);  o = z h + (1 - z) c;  out = m o + (1 - m) h.   Uh [H, H], xh [R, H] of the
 *                     storage type, bh fp32 [H]; z, h_prev, idx as given to zk_rnn_gru_gates (z h and the carry read the fp32
 *                     state: a carried row is the gathered state bit for bit); mask, out, out_copy as in zk_rnn_atr_step.
 *                     h_prev NULL: rh is not read.  out must not overlap h_prev or z: refused.
 * bf16 forms: H % 8 == 0 and H <= 2048 (the gates launch keeps a [32][H + 8] bf16 image of its columns of Ug in LDS: 66 KB
 * for H = 1000, 129 KB for H = 2048), 16-byte aligned rows of Ug / Uh; anything else is refused by name.  fp32 forms: any H. */
int zk_rnn_gru_gates(const float* h_prev, int ldh, int n_prev, const int* idx, const void* Ug, int ldu, const float* bg,
                     const void* xg, int ldx, float* z, int ldz, void* rh, int ldr, int R, int H, zk_stream_t stream);
int zk_f32_rnn_gru_gates(const float* h_prev, int ldh, int n_prev, const int* idx, const float* Ug, int ldu, const float* bg,
                         const float* xg, int ldx, float* z, int ldz, float* rh, int ldr, int R, int H, zk_stream_t stream);
int zk_rnn_gru_out(const void* rh, int ldr, const void* Uh, int ldu, const float* bh, const void* xh, int ldx, const float* z,
                   int ldz, const float* h_prev, int ldh, int n_prev, const int* idx, const float* mask, int ldm, float* out,
                   int ldo, void* out_copy, int ldc, int R, int H, zk_stream_t stream);
int zk_f32_rnn_gru_out(const float* rh, int ldr, const float* Uh, int ldu, const float* bh, const float* xh, int ldx,
                       const float* z, int ldz, const float* h_prev, int ldh, int n_prev, const int* idx, const float* mask,
                       int ldm, float* out, int ldo, float* out_copy, int ldc, int R, int H, zk_stream_t stream);
/* The ff product of ONE deepnmt layer with its bias and residual add (models/deepnmt.py:73-79 in the encoder, 166-172 in the
 * decoder: y = func.linear(outputs, embed_size, ln=False, scope="ff"), func.py:14-65; x = func.residual_fn(x, y), func.py:321-324
 * without dropout; layer_norm off, so the stream is never re-normalised) in ONE launch:
 *   zk_rnn_ff_residual   out[r, :] = x[r, :] + (a[r, :] W + b);   out_copy = the same in the storage type.
 *                        a [R, K] and W [K, N] (bf16 shadow / fp32 master) of the storage type; b fp32 [N]; x and out fp32
 *                        [R, N]: the residual stream is fp32 in BOTH forms, only the matrix-core operands are bf16; out_copy
 *                        (may be NULL) [R, N] of the storage type.  Every operand has its own row stride, so out_copy can be a
 *                        column slice of a wider operand buffer.  out == x with ldo == ldx is allowed (in place: an element is
 *                        read and written by the one lane that owns it); any other overlap of out with x is refused, element
 *                        by element.  a against out / out_copy and out_copy against x / out are checked CONSERVATIVELY, by the
 *                        byte ranges that enclose their rows: column slices of one buffer are refused although they share no
 *                        element -- keep a, and out_copy, in buffers apart from the stream.
 * bf16 form: K % 8 == 0, N % 8 == 0, K <= 4096 (a [16][K + 8] bf16 image of its columns of W in LDS: 131 KB there), 16-byte
 * aligned rows of W; anything else is refused by name, nothing launched.  fp32 form: any K and N, k ascending. */
int zk_rnn_ff_residual(const void* a, int lda, const void* W, int ldw, const float* b, const float* x, int ldx, float* out,
                       int ldo, void* out_copy, int ldc, int R, int K, int N, zk_stream_t stream);
int zk_f32_rnn_ff_residual(const float* a, int lda, const float* W, int ldw, const float* b, const float* x, int ldx, float* out,
                           int ldo, float* out_copy, int ldc, int R, int K, int N, zk_stream_t stream);
int zk_add_attn(const void* qa, int ldq, const void* pm, int ldpm, long bspm, const void* mem, int ldmem, long bsmem,
                const float* v, const float* kmask, int ldmask, float* ctx, int ldo, void* ctx_copy, int ldc, int R,
                int kv_group, int Ls, int M, float neg, zk_stream_t stream);
int zk_f32_add_attn(const float* qa, int ldq, const float* pm, int ldpm, long bspm, const float* mem, int ldmem, long bsmem,
                    const float* v, const float* kmask, int ldmask, float* ctx, int ldo, float* ctx_copy, int ldc, int R,
                    int kv_group, int Ls, int M, float neg, zk_stream_t stream);
int zk_rnn_embed(const int* ids, int rows, const void* table, int V, const float* bias, void* out, int ldo, int E, int pad,
                 zk_stream_t stream);
int zk_f32_rnn_embed(const int* ids, int rows, const float* table, int V, const float* bias, float* out, int ldo, int E,
                     int pad, zk_stream_t stream);
int zk_rnn_bias_tanh(const float* x, int ldx, const float* bias, float* out_f32, int ldo, void* out_copy, int ldc, int rows,
                     int cols, int rep, zk_stream_t stream);
int zk_f32_rnn_bias_tanh(const float* x, int ldx, const float* bias, float* out_f32, int ldo, float* out_copy, int ldc,
                         int rows, int cols, int rep, zk_stream_t stream);
/* LRN / OLRN cells (rnns/lrn.py:32-53, rnns/olrn.py:32-58) with the mask carry of rnns/rnn.py:41-49 and the lower / higher pair of
 * cond_rnn(one2one=True) (rnns/rnn.py:119-146): T >= 1 time steps of one cell, or of a pair, for R rows and H channels in ONE
 * launch.  The cells have no recurrent product; [p | q | r (| s)] is the input projection (x W, no bias, 3 H or 4 H wide):
 *   cell(h_, [p|q|r])   = sigmoid(p + h_) r + sigmoid(q - h_) h_                          (lrn, gated = 0)
 *   cell(h_, [p|q|r|s]) = u sigmoid(s - u),  u = sigmoid(p + h_) r + sigmoid(q - h_) h_   (olrn, gated = 1; the gated value is carried)
 *   single (hi == NULL):  h = carry(m_t, cell(h, lo_t), h)
 *   paired:               s = carry(m_t, cell(h, lo_t), h);   h = carry(m_t, cell(s, hi_t), s)      carry(m, a, b) = m a + (1 - m) b
 * for t = 0 .. T-1, or t = T-1 .. 0 with reverse != 0 (positions are never re-ordered in memory).
 *   h_prev, ldh, n_prev, idx   the initial state h = h_prev[idx[r]] as in zk_rnn_atr_step: fp32 [n_prev, H] or NULL (zero state),
 *                              idx int32 [R] or NULL, values clamped to 0 .. n_prev - 1.
 *   lo, hi                     storage type; element (t, r, c) at  base + t * ps + r * rs + c  (strides in elements, as ld / bs of
 *                              zk_add_attn): [B * Ls, W] sequence buffers and a [R, W] step operand (T = 1) pass without a copy.
 *   mask, m_ps, m_rs           fp32 or NULL (all ones); a position with m == 0 leaves the state bit for bit.
 *   out, ldo                   fp32 [R, H]: the state after the last scanned position; always written.
 *   seq, seq_ps, seq_rs        NULL, or the carried state of EVERY position in the storage type, written at that position (with
 *                              T = 1: the out_copy of the other cell launches; may be a column slice).
 * The state is fp32 in both forms; every product and sum is rounded on its own, so a T-step launch equals T chained one-step
 * launches bit for bit.  Refused (-1, nothing launched): T < 1; H % 8 != 0 or bases / strides of lo, hi, seq that are not
 * 16-byte aligned in the bf16 form (the message names zk_f32_rnn_lrn_scan); H % 4 != 0 or unaligned operands in the fp32 form;
 * out overlapping h_prev; seq overlapping lo / hi / h_prev / out (by enclosing byte ranges); negative strides. */
int zk_rnn_lrn_scan(const float* h_prev, int ldh, int n_prev, const int* idx, const void* lo, long lo_ps, long lo_rs,
                    const void* hi, long hi_ps, long hi_rs, const float* mask, long m_ps, long m_rs, float* out, int ldo,
                    void* seq, long seq_ps, long seq_rs, int R, int H, int T, int reverse, int gated, zk_stream_t stream);
int zk_f32_rnn_lrn_scan(const float* h_prev, int ldh, int n_prev, const int* idx, const float* lo, long lo_ps, long lo_rs,
                        const float* hi, long hi_ps, long hi_rs, const float* mask, long m_ps, long m_rs, float* out, int ldo,
                        float* seq, long seq_ps, long seq_rs, int R, int H, int T, int reverse, int gated, zk_stream_t stream);

/* Word alignment from one decoder layer's cross-attention (hp.alignment_file; zero_amd/models/_align.py, zk_align.hip): the
 * head-averaged attention weights of func.py:218-256 (additive mask of func.py:372-400) and their arg-max, from the layer's q
 * and k projections alone -- no value product, no context.  For sentence b, decoder row t, source position j:
 *   P[b, t, j] = (1 / nh) * sum_h softmax_j(scale * q[b, t, h] . k[b, j, h] + (1 - kmask[b, j]) * -mask_inf)   heads ascending
 *   best[b, t] = argmax_j P[b, t, j] over the ELIGIBLE positions (amask[b, j] != 0); the lowest j wins on equal values;
 *                -1 for a row without an eligible position.
 *   q, ldq, bsq   [B, Lq, >= nh * d] of the storage type; row stride ldq and sentence stride bsq in elements (a qkv-style
 *                 column slice passes: ldq = 3 H); head h in the columns h d .. h d + d - 1.
 *   k, ldk, bsk   [B, Lk, >= nh * d] likewise (the first H columns of a [., 2 H] kv buffer: ldk = 2 H).
 *   kmask, ldmask fp32 [B, ldmask >= Lk], 1 = valid key, or NULL (all valid).  A masked key's weight is exactly 0 in every row
 *                 that has a valid key.
 *   amask         fp32 [B, ldmask] (the same row stride), the positions the arg-max may return, or NULL (= kmask).
 *   probs, ldp, bsp   fp32 [B, Lq, ldp >= Lk], sentence stride bsp; only the Lk columns of a row are written.  May be NULL.
 *   best          int32 [B, Lq].  May be NULL; at least one of probs / best is given.
 *   scale, mask_inf   those of the layer (d^-0.5, dtype_inf).
 * All softmax arithmetic and the head average are fp32; no atomics, one fixed order: two runs are bit-identical.
 * zk_align_probs: bf16 q / k, scores by v_mfma_f32_16x16x32_bf16, d a multiple of 32 up to 128, q and k rows 16-byte aligned
 * (pointer, ld and bs multiples of 8).  zk_f32_align_probs: fp32 q / k, fused multiply-adds with the channels ascending, d a
 * multiple of 4 up to 128, k rows 16-byte aligned.  Lk <= zk_align_max_lk() = 1024 (two [16][Lk] fp32 images of a block of 16
 * decoder rows in LDS).  Anything else -- a longer source, a short stride, an unaligned row, another d, both outputs NULL --
 * is refused by name: nothing is launched and the buffers stay untouched. */
int zk_align_probs(const void* q, int ldq, long bsq, const void* k, int ldk, long bsk, const float* kmask, int ldmask,
                   const float* amask, float* probs, int ldp, long bsp, int* best, int B, int nh, int Lq, int Lk, int d,
                   float scale, float mask_inf, zk_stream_t stream);
int zk_f32_align_probs(const float* q, int ldq, long bsq, const float* k, int ldk, long bsk, const float* kmask, int ldmask,
                       const float* amask, float* probs, int ldp, long bsp, int* best, int B, int nh, int Lq, int Lk, int d,
                       float scale, float mask_inf, zk_stream_t stream);
int zk_align_max_lk(void);

/* hipGraph plumbing: capture a sequence of the calls above once, replay per step */
int zk_graph_begin(zk_stream_t stream);
int zk_graph_end(zk_stream_t stream, void** exec_out);
int zk_graph_launch(void* exec, zk_stream_t stream);
/* rewrite the arguments of the ONE zk_copy_many launch a captured graph holds (arguments as for zk_copy_many, n >= 1): the
 * training step's graph starts with the copy of the prepared batch out of one of several staging sets -- the feed_dict of
 * main.py:286-294 -- and the set changes from step to step (zero_amd/main.py Trainer.step) */
int zk_graph_set_copy_many(void* exec, void* const* dsts, const void* const* srcs, const size_t* nbytes, int n);
/* the most (dst, src) pairs one zk_copy_many launch takes (16): a commit with more pairs makes several launches and cannot
 * be the rewritable first node of a step graph */
int zk_copy_many_max(void);
int zk_graph_destroy(void* exec);
/* number of nodes (= kernel launches) of the graph the last zk_graph_end instantiated: lets bench.py report the
 * launches per captured step without a profiler */
int zk_graph_last_nodes(void);

/* hardware-layout probes used by the GPU tests */
int zk_probe_mfma32(const void* A, const void* Bt, float* D, zk_stream_t stream);
int zk_probe_mfma16(const void* A, const void* Bt, float* D, zk_stream_t stream);
int zk_probe_tr16(void* out, zk_stream_t stream);
/* measurement aid: reads each of `bytes` (16-byte aligned, multiple of 16 KB) once with access pattern 0..4 (zk_probe.hip)
 * -- a known byte count per access shape for calibrating the FETCH_SIZE counter (scripts/fetch_calibrate.sh) */
int zk_probe_read(const void* src, size_t bytes, int pattern, float* sink, zk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ZERO_HIP_H_ */
