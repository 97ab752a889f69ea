# coding: utf-8
"""``transformer_fixup`` -- registered under the reference's name (models/transformer_fixup.py, last line).

The Transformer without LayerNorm (modules/fixup.py): a learned scalar shift in front of every sub-layer, a learned scalar
scale behind it, no bias in any linear map.  Decoding (``search_mode=cache``, both decode modes) and scoring run on the
existing GEMM and softmax-attention kernels with ``zk_fixup_residual`` / ``zk_fixup_relu_shift`` (zero_amd/csrc/zk_fixup.hip)
at the sub-layer boundaries (zero_amd/models/_fixup.py).  Training needs the backward of the scalars; it says so when called.
"""

from zero_amd.models import model
from zero_amd.models._factory import build

_, score_fn, infer_fn = build("transformer_fixup")


def train_fn(features, params, initializer=None, on_ready=None):
    raise NotImplementedError("transformer_fixup decodes and scores here, it does not train: the backward of the scalar "
                              "shifts and scales (modules/fixup.py:15-26) and the reductions of their gradients over "
                              "every row and column are not built")


# register the model, with a unique name
model.model_register("transformer_fixup", train_fn, score_fn, infer_fn)
