# coding: utf-8
"""``transformer_l0drop`` -- registered under the reference's name (models/transformer_l0drop.py, last line).

Decode only.  The layers are those of ``transformer``; ``encoding_fn`` prunes the encoder output with the learned
hard-concrete gate (zero_amd/models/_l0drop.py, zero_amd/csrc/zk_l0drop.hip) and the decoder's cross-attention runs over
the kept positions plus one counting slot (zk_dec_cross_kb / zk_f32_attn_kb).  Training needs the stochastic gate and its
backward; the reference's ``score_fn`` takes that same sampling branch.  Both say so when called.
"""

from zero_amd.models import model
from zero_amd.models._factory import build

_, _, infer_fn = build("transformer_l0drop")


def train_fn(features, params, initializer=None, on_ready=None):
    raise NotImplementedError("transformer_l0drop is decode only here: training needs the sampled hard-concrete gate "
                              "and its backward (models/transformer_l0drop.py:252-266)")


def score_fn(features, params, initializer=None):
    raise NotImplementedError("transformer_l0drop is decode only here: the reference's score_fn takes the training "
                              "branch and samples the gate's noise (models/transformer_l0drop.py:252-266, 401-415)")


# register the model, with a unique name
model.model_register("transformer_l0drop", train_fn, score_fn, infer_fn)
