# coding: utf-8
"""The op layer of the launch-per-op schedules: how a schedule names a buffer, fetches a weight and issues a product, an
attention or an embedding in the storage type of its mode.

An ops object belongs to one core, one storage type and one buffer prefix.  ``Bf16Ops`` issues the bf16 launches (``zk_gemm``,
``zk_attn_fwd``, ``zk_rela_attn``, ``zk_dec_embed``) on the bf16 shadow weights, ``F32Ops`` the ``zk_f32_*`` launches
(include/zero_hip.h) on the fp32 masters; ``ops_for`` picks between them.  The schedules of models/_decode.py (start-up),
_decode_f32.py, _score_f32.py, _fixup.py, _l0drop.py and of the recurrent models (_rnn.py with _rnnsearch.py, _deepatt.py and
_deepnmt.py) are written once against this interface.

The prefix keeps the buffers of two passes of one engine apart (DESIGN.md has the table): ``dc.`` / ``dq.`` for the bf16 / fp32
decode, ``fx.`` / ``dq.fx.`` for transformer_fixup, ``dc.rn.`` / ``dq.rn.`` for rnnsearch, rnnsearch_deepatt and deepnmt (each on its
own core's engine), ``sq.`` for the fp32 scorer.
"""

import collections
import os

import torch

from zero_amd.func import Mat
from zero_amd.utils import dtype as zdtype

F32 = torch.float32

# Where a decode mode keeps its per-beam caches: the prefix of its engine buffers (a bf16 and an fp32 decode of one engine
# never alias), the element type of the k / v caches and its size in bytes.  defer_aan: the step's input launch can take
# over the beam reorder of the average-attention sums (zk_dec_embed: gather_src / gather_idx); the fp32 step has no such
# launch and gathers at once.
Storage = collections.namedtuple("Storage", "prefix dtype esz defer_aan")
BF16_CACHES = Storage("dc.", torch.bfloat16, 2, True)
F32_CACHES = Storage("dq.", F32, 4, False)


class Ops(object):
    """What does not depend on the storage type.  A subclass sets ``storage`` and brings table / gemm / attn / rela_attn /
    embed_step."""

    storage = None

    def __init__(self, core, prefix=None, shortlist=None):
        self.core, self.e, self.lib = core, core.eng, core.eng.lib
        self.H, self.nh, self.d = core.H, getattr(core, "nh", None), getattr(core, "d", None)      # (rnnsearch has no heads)
        self.pre = self.storage.prefix if prefix is None else prefix
        # the decode state's shortlist (zero_amd/shortlist.py), or None: its compact tables stand in for the target-side
        # tables and its size for V
        self.sl = shortlist
        self.V = core.V if shortlist is None else shortlist.Vs

    def mat(self, name, rows, cols, dt=None):
        """Named persistent matrix of the storage type (or of dt)."""
        return Mat(self.e.buf(self.pre + name, (rows, cols), self.storage.dtype if dt is None else dt), rows, cols)

    def logits_mat(self, rows):
        """The fp32 logits of a decode step, under the storage's own prefix (models/_decode.py _graph_pointers)."""
        return self.logits_view(self.e.buf(self.storage.prefix + "logits", (rows, self.core.Vpad), F32), rows)

    def logits_view(self, buf, rows):
        """buf fp32 [rows, Vpad] as the step's logits Mat: as it is, or [rows, ld of the shortlist] of the same memory."""
        return Mat(buf, rows, self.core.Vpad) if self.sl is None else self.sl.logits(buf, rows)

    def _compact(self, name):
        return self.sl.table(name) if self.sl is not None else None

    def W(self, name):
        """The weight of the storage type (physical shape)."""
        t = self.table(name)
        return Mat(t, t.shape[0], t.shape[1])

    def b(self, name):
        """The fp32 master: biases, LayerNorm parameters and scalars are read in fp32 by both modes."""
        return self.core.store.w(name)

    def linear(self, x, scope, out, act=0):
        """func.py:14-65: out = x W + b (act 1: ReLU)."""
        W = self.W(scope + "/W_0_0")
        bias = None if self.core.fixup else self.b(scope + "/b_0")      # (fixup.py: every linear map is bias=False)
        self.gemm(x, W, out, x.rows, W.cols, W.rows, 0, bias, act)
        return out

    def project(self, x, name, out, bias=None):
        """out = x W (+ bias) with the variable's full name."""
        W = self.W(name)
        self.gemm(x, W, out, x.rows, W.cols, W.rows, 0, bias)
        return out


class Bf16Ops(Ops):
    storage = BF16_CACHES

    def table(self, name):
        t = self._compact(name)
        return self.core.store.s(name) if t is None else t

    def gemm(self, A, B, C, M, N, K, tb=0, bias=None, act=0):
        """C = A op(B) (+ bias).  C may be an fp32 Mat (the input of a tanh, the logits)."""
        self.e.gemm(A, B, C, M, N, K, 0, tb, bias=bias, act=act)

    def attn(self, q, k, v, out, B, Lq, Lk, bsq, bsk, bsv, kmask=None, ldmask=0, kv_group=1, nkeys_dev=None, rpr=None,
             q_pos0=0, q_pos_dev=None, kbias=None, max_rel=None, causal=False, cached=False):
        """func.dot_attention's core on zk_attn_fwd; the arguments of F32Ops.attn.  The kernel has ONE device position,
        q_pos_dev: the query's position and, with ``cached``, the last valid key of a per-row cache of Lk slots.  The mask
        has the row stride Lk."""
        if kbias is not None:
            raise NotImplementedError("the bf16 attention launch has no key bias (the fused decode launches take it)")
        rk = self.table(rpr + "rpr_keys/embeddings") if rpr is not None else None
        rv = self.table(rpr + "rpr_values/embeddings") if rpr is not None else None
        strided = cached or kv_group > 1 or bsq
        self.e.attn_fwd(q, k, v, out, None, B, self.nh, Lq, Lk, self.d, kmask=kmask, causal=causal, q_pos0=q_pos0,
                        rpr_k=rk, rpr_v=rv, max_rel=int(self.core.hp.max_relative_position if max_rel is None else max_rel),
                        bsq=bsq, bsk=bsk, bsv=bsv, kv_group=kv_group, pos_dev=q_pos_dev,
                        pos_flags=(3 if cached else 1) if strided else 0)
        return out

    def rela_attn(self, q, k, v, out, B, Lq, Lk, bsq, bsk, bsv, scope, kmask=None, ldmask=0, kv_group=1, nkeys_dev=None):
        self.core._rela_attn(q, k, v, out, B, Lq, Lk, scope, kmask, bsq=bsq, bsk=bsk, bsv=bsv, kv_group=kv_group,
                             nkeys_dev=nkeys_dev)
        return out

    def embed_step(self, ids, rows, out, max_pos, pos0, pos_dev, pad):
        """The embedding of one decode position (zk_dec_embed) without its average-attention half."""
        self.lib.call("zk_dec_embed", ids.data_ptr(), pad, self.table(self.core.tgt_emb).data_ptr(), self.b("bias").data_ptr(),
                      self.e.timing(max_pos + 1, self.H).data_ptr(), out.ptr, rows, self.H, float(self.H) ** 0.5, pos0, pos_dev,
                      None, None, 1.0, None, None, 0, self.e.stream)
        return out


class F32Ops(Ops):
    """Thin wrappers over the zk_f32_* entry points (include/zero_hip.h)."""

    storage = F32_CACHES

    def __init__(self, core, prefix=None, shortlist=None):
        Ops.__init__(self, core, prefix, shortlist)
        # round 6: row-local launches folded into their neighbours (ZERO_HIP_F32_FUSE=0: one launch per op, as in round 5 --
        # the two forms are compared in tests/test_gpu_decode_f32.py)
        self.fold = os.environ.get("ZERO_HIP_F32_FUSE", "1") != "0"

    def table(self, name):
        t = self._compact(name)
        return self.core.store.w(name) if t is None else t

    def embed(self, ids, rows, L, table, out, max_pos, pos0=0, pos_dev=None, zero_flag=None):
        """func.py:341-369: out = table[ids] * sqrt(H) + bias + timing signal of the row's position (row % L + pos0, or
        + *pos_dev); rows of a step whose ids are all pad (*zero_flag) are zero embeddings."""
        tim = self.e.timing(max_pos + 1, self.H)
        self.lib.call("zk_f32_embed", ids.data_ptr(), rows, L, self.table(table).data_ptr(), self.b("bias").data_ptr(),
                      tim.data_ptr(), int(tim.shape[0]), out.ptr, self.H, float(self.H) ** 0.5, pos0, pos_dev,
                      zero_flag.data_ptr() if zero_flag is not None else None, self.e.stream)
        return out

    def embed_step(self, ids, rows, out, max_pos, pos0, pos_dev, pad, aan=None, cat=None):
        """embed() of one decode position with the all-pad test inside the launch; aan / cat: the first layer's average
        attention from the embedded row (cache tensor, cat Mat) in the same launch."""
        tim = self.e.timing(max_pos + 1, self.H)
        self.lib.call("zk_f32_embed_step", ids.data_ptr(), rows, self.table(self.core.tgt_emb).data_ptr(),
                      self.b("bias").data_ptr(), tim.data_ptr(), int(tim.shape[0]), out.ptr, self.H, float(self.H) ** 0.5, pos0,
                      pos_dev, pad, aan.data_ptr() if aan is not None else None, cat.ptr if cat is not None else None,
                      self.e.stream)
        return out

    def embed_shift(self, ids, rows, L, out):
        """transformer.py:108-112: row i of a sentence embeds token i - 1 (the scorer's decoder input)."""
        tim = self.e.timing(L + 1, self.H)
        self.lib.call("zk_f32_embed_shift", ids.data_ptr(), rows, L, self.table(self.core.tgt_emb).data_ptr(),
                      self.b("bias").data_ptr(), tim.data_ptr(), int(tim.shape[0]), out.ptr, self.H, float(self.H) ** 0.5,
                      self.e.stream)
        return out

    def gemm(self, A, B, C, M, N, K, tb=0, bias=None, act=0):
        self.lib.call("zk_f32_gemm", A.ptr, B.ptr, C.ptr, M, N, K, A.ld, B.ld, C.ld, tb,
                      bias.data_ptr() if bias is not None else None, act, self.e.stream)

    def add_ln(self, x, y, scope, out):
        """func.py:321-324 + 289-303: LN(x + y) with the scope's scale / offset."""
        if self.fold and self.H % 4 == 0 and self.H <= 2048:
            # the 16-byte-load form (round 6: 4.8 us against 7.2 for a decode step's 128 rows)
            return self.ln_fused(x, y, scope, out)
        self.lib.call("zk_f32_add_ln", x.ptr, y.ptr if y is not None else None, self.b(scope + "/layer_norm/scale").data_ptr(),
                      self.b(scope + "/layer_norm/offset").data_ptr(), out.ptr, x.rows, self.H, zdtype.epsilon(), self.e.stream)
        return out

    def _rpr(self, rpr):
        if rpr is None:
            return None, None
        return self.b(rpr + "rpr_keys/embeddings").data_ptr(), self.b(rpr + "rpr_values/embeddings").data_ptr()

    def attn(self, q, k, v, out, B, Lq, Lk, bsq, bsk, bsv, kmask=None, ldmask=0, kv_group=1, nkeys_dev=None, rpr=None,
             q_pos0=0, q_pos_dev=None, kbias=None, max_rel=None, causal=False, cached=False):
        """rpr: attention scope prefix (".../dot_attention/") whose rpr_keys / rpr_values tables take part, or None.
        kbias: fp32 [.., ldmask] added to the scores (transformer_l0drop's log counts: zk_f32_attn_kb), or None.
        max_rel: the clipping distance handed to the kernel (default: the model's max_relative_position); 0: no relative
        positions at all, the query at position 0.  nkeys_dev: the keys 0 .. *nkeys_dev of every row are valid (``cached``
        is the bf16 launch's spelling of it)."""
        if causal:
            raise NotImplementedError("the fp32 mode has no causal attention over a block of rows (it decodes from caches; "
                                      "the scorer's attn_seq has one)")
        if max_rel == 0:
            q_pos0, q_pos_dev = 0, None
        rk, rv = self._rpr(rpr)
        head = (q.ptr, k.ptr, v.ptr, out.ptr, B, self.nh, Lq, Lk, self.d, q.ld, k.ld, v.ld, out.ld, int(bsq or Lq * q.ld),
                int(bsk or Lk * k.ld), int(bsv or Lk * v.ld), int(Lq * out.ld), kmask.data_ptr() if kmask is not None else None,
                int(ldmask))
        tail = (int(kv_group), float(self.d) ** -0.5, zdtype.inf(), nkeys_dev.data_ptr() if nkeys_dev is not None else None,
                rk, rv, int(self.core.hp.max_relative_position if max_rel is None else max_rel), int(q_pos0),
                q_pos_dev.data_ptr() if q_pos_dev is not None else None, self.e.stream)
        if kbias is not None:
            self.lib.call("zk_f32_attn_kb", *head, kbias.data_ptr(), *tail)
        else:
            self.lib.call("zk_f32_attn", *head, *tail)
        return out

    def attn_seq(self, q, k, v, out, B, Lq, Lk, bsq, bsk, bsv, kmask=None, ldmask=0, rpr=None, causal=False):
        """attn() of whole sentences (zk_f32_attn_seq: one workgroup per block of query rows, keys and values staged once
        per block), with a causal form."""
        rk, rv = self._rpr(rpr)
        self.lib.call("zk_f32_attn_seq", q.ptr, k.ptr, v.ptr, out.ptr, B, self.nh, Lq, Lk, self.d, q.ld, k.ld, v.ld, out.ld,
                      int(bsq), int(bsk), int(bsv), int(Lq * out.ld), kmask.data_ptr() if kmask is not None else None,
                      int(ldmask), float(self.d) ** -0.5, zdtype.inf(), rk, rv, int(self.core.hp.max_relative_position), 0,
                      1 if causal else 0, self.e.stream)
        return out

    def rela_attn(self, q, k, v, out, B, Lq, Lk, bsq, bsk, bsv, scope, kmask=None, ldmask=0, kv_group=1, nkeys_dev=None):
        """modules/rela.py:56-81 (zk_f32_rela_attn).  scope: the attention scope prefix (".../dot_attention/") whose
        post/{scale, gate} normalise the combined heads; the other arguments as attn()."""
        self.lib.call("zk_f32_rela_attn", q.ptr, k.ptr, v.ptr, out.ptr, B, self.nh, Lq, Lk, self.d, q.ld, k.ld, v.ld, out.ld,
                      int(bsq), int(bsk), int(bsv), int(Lq * out.ld), kmask.data_ptr() if kmask is not None else None,
                      int(ldmask), int(kv_group), float(self.d) ** -0.5,
                      nkeys_dev.data_ptr() if nkeys_dev is not None else None, self.b(scope + "post/scale").data_ptr(),
                      self.b(scope + "post/gate").data_ptr(), float(zdtype.epsilon()), self.e.stream)
        return out

    def cumavg(self, x, tmask, out, B, L, use_mask, add=None):
        """transformer_aan.py:92-108 at training time: the (masked) cumulative average over a sentence's rows (+ add)."""
        self.lib.call("zk_f32_cumavg", x.ptr, x.ld, tmask.data_ptr(), add.ptr if add is not None else None,
                      add.ld if add is not None else 0, out.ptr, out.ld, B, L, self.H, 1 if use_mask else 0, self.e.stream)
        return out

    def ln_fused(self, x, y, scope, out, gate=None, aan_next=None, time=0, time_dev=None):
        """zk_f32_ln_fused (round 6): LN(x + y) with row-local neighbours in the same launch.  gate = (z, cat): y is the
        average-attention gate of transformer_aan.py:186-189 and the residual is cat[:, :H] (x, y = None);
        aan_next = (cache tensor, cat Mat): the next layer's average attention from the normalised row."""
        z, cat = gate if gate is not None else (None, None)
        cache, cat_out = aan_next if aan_next is not None else (None, None)
        self.lib.call("zk_f32_ln_fused", x.ptr if x is not None else None, y.ptr if y is not None else None,
                      z.ptr if z is not None else None, cat.ptr if cat is not None else None,
                      self.b(scope + "/layer_norm/scale").data_ptr(), self.b(scope + "/layer_norm/offset").data_ptr(), out.ptr,
                      out.rows, self.H, zdtype.epsilon(), cache.data_ptr() if cache is not None else None,
                      cat_out.ptr if cat_out is not None else None, int(time), time_dev, self.e.stream)
        return out

    def ffn(self, x, scope, tag, aan_next=None, time=0, time_dev=None):
        """func.py:327-338 + residual + LayerNorm (transformer.py:62-69)."""
        h = self.mat(tag + ".h", x.rows, self.core.F)
        self.linear(x, scope + "/ffn_layer/enlarge", h, act=1)
        y = self.mat("y", x.rows, self.H)
        self.linear(h, scope + "/ffn_layer/output", y)
        if aan_next is not None:
            return self.ln_fused(x, y, scope, self.mat(tag + ".o", x.rows, self.H), aan_next=aan_next, time=time,
                                 time_dev=time_dev)
        return self.add_ln(x, y, scope, self.mat(tag + ".o", x.rows, self.H))


def ops_for(core, f32, prefix=None, shortlist=None):
    """The ops object of ``core`` in fp32 (``f32``) or bf16 storage, over buffers named prefix + name (default: the
    storage's own prefix, ``dq.`` / ``dc.``).  shortlist: the decode state's, for the ops of a decode STEP."""
    return (F32Ops if f32 else Bf16Ops)(core, prefix, shortlist)
