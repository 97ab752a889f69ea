# coding: utf-8
"""``transformer_rela`` -- registered under the reference's name (models/transformer_rela.py, last line).

Decode only.  The layers are those of ``transformer`` with every ``func.dot_attention`` replaced by
``modules/rela.py:dot_attention``: ReLU instead of softmax, the mask multiplied into the scores, and a gated RMSNorm over
the combined heads (``post/{scale, gate}``) in front of ``o_map`` (zero_amd/csrc/zk_rela.hip: zk_rela_attn,
zk_f32_rela_attn).  Training and scoring need the backward of both; they say so when called.
"""

from zero_amd.models import model
from zero_amd.models._factory import build

_, _, infer_fn = build("transformer_rela")


def train_fn(features, params, initializer=None, on_ready=None):
    raise NotImplementedError("transformer_rela is decode only here: training needs the backward of the ReLU attention "
                              "weights and of the gated RMSNorm (modules/rela.py:72, 95-109), which is not built")


def score_fn(features, params, initializer=None):
    raise NotImplementedError("transformer_rela is decode only here: scoring runs the training-path decoder, whose ReLU "
                              "attention and gated RMSNorm (modules/rela.py:72, 95-109) exist for the decode step only")


# register the model, with a unique name
model.model_register("transformer_rela", train_fn, score_fn, infer_fn)
