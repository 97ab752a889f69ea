# coding: utf-8
"""L0Drop at inference (reference: models/transformer_l0drop.py:103-135, 244-273): prune the encoder output on the device.

``prune`` runs between ``core.encode`` and the k_map / v_map projections of ``encoding_fn`` (models/_decode.py,
models/_decode_f32.py).  It returns the COMPACTED memory, its mask and its length, which take the place of the encoder
output, the source mask and the source length in the decode state -- so the projections, the LDS fit of the fused
attention launch, the step-graph cache key and the step itself follow unchanged -- plus ``kbias``, the log-count of the
slot that stands in for the dropped positions (zk_dec_cross_kb / zk_f32_attn_kb).

The shape is data dependent: one 4-byte copy and one stream synchronisation per batch read the largest kept count back
(``encoding_fn`` is eager already).  The memory length is rounded up to the multiple the source length is padded to
(ZERO_HIP_DECODE_PAD_LEN), so that batches fall into few step-graph shapes; every buffer has a fixed engine name, so a
step graph cached for (B, K, Lm, Tmax, ..) replays against the same addresses.
"""

import torch

F32 = torch.float32
I32 = torch.int32


def prune(core, enc, smask, B, Ls, pad, o):
    """enc: Mat [B*Ls, H] of the storage type of the decode mode's ops object ``o``, smask fp32 [B, Ls] -> (memory Mat
    [B*Lm, H] of enc's type, mask fp32 [B, Lm], Lm, kbias fp32 [B, Lm])."""
    e, H = core.eng, core.H
    pre = o.pre
    f32 = o.storage.dtype == F32             # the kernels' is_f32 flag
    gate = e.buf(pre + "l0.gate", (B, Ls), F32)
    pos = e.buf(pre + "l0.pos", (B, Ls), I32)
    cnt = e.buf(pre + "l0.cnt", (2, B), I32)
    kmax = e.buf(pre + "l0.kmax", (1,), I32)
    W, b0 = core.store.w("source_pruning/W_0_0"), core.store.w("source_pruning/b_0")
    e.lib.call("zk_l0_gate", enc.ptr, enc.ld, 1 if f32 else 0, smask.data_ptr(), W.data_ptr(), b0.data_ptr(), B, Ls, H,
               gate.data_ptr(), pos.data_ptr(), cnt[0].data_ptr(), cnt[1].data_ptr(), kmax.data_ptr(), e.stream)
    # the one read-back of the batch (the shape depends on the data): 4 bytes into pinned staging that outlives the batch
    pins = core.__dict__.setdefault("_decode_pins", {})
    host = pins.get("l0.kmax")
    if host is None:
        host = pins["l0.kmax"] = torch.zeros(1, dtype=I32).pin_memory()
    host.copy_(kmax, non_blocking=True)
    torch.cuda.current_stream(e.device).synchronize()
    k = int(host[0])
    if not 0 <= k <= Ls:
        raise RuntimeError("zk_l0_gate reported %d kept positions for a source of %d" % (k, Ls))
    Lm = -(-(1 + k) // pad) * pad
    mem = o.mat("enc", B * Lm, H)
    gmask = e.buf(pre + "smask", (B, Lm), F32)
    kbias = e.buf(pre + "kbias", (B, Lm), F32)
    e.lib.call("zk_l0_compact", enc.ptr, enc.ld, 1 if f32 else 0, gate.data_ptr(), pos.data_ptr(), cnt[0].data_ptr(),
               cnt[1].data_ptr(), B, Ls, H, Lm, mem.ptr, mem.ld, gmask.data_ptr(), kbias.data_ptr(), e.stream)
    return mem, gmask, Lm, kbias
