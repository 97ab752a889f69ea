# coding: utf-8
"""``deepnmt`` -- registered under the reference's name (models/deepnmt.py, last line): stacked recurrent layers on a
residual stream.  Every encoder and decoder layer is a recurrent scan followed by ``x = x + linear(outputs, embed_size,
scope="ff")``; encoder layer 0 is bidirectional (or context-aware, ``caencoder``), decoder layer 0 -- every decoder layer
under ``use_deep_att`` -- attends over the encoder output, the other decoder layers read the context of the last attention.

Decode only, ``cell`` in {atr, gru, lrn, olrn}, ``layer_norm=False``, ``num_heads=1``, ``search_mode="cache"`` (zero_amd/models/_deepnmt.py
holds the schedule, zero_amd/csrc/zk_rnn.hip the kernels).  Everything else says what is missing when it is asked for, before a
core is built.
"""

import copy

from zero_amd.models import model
from zero_amd.models._factory import closing_dropout

CELLS = ("atr", "gru", "lrn", "olrn")


def train_fn(features, params, initializer=None, on_ready=None):
    raise NotImplementedError("deepnmt is decode only here: training needs the backward of the recurrent scans (one or two "
                              "launches per time step and cell, rnns/rnn.py:41-59, 119-158) and of the ff + residual of "
                              "every layer (models/deepnmt.py:73-79, 166-172), which is not built")


def score_fn(features, params, initializer=None):
    raise NotImplementedError("deepnmt is decode only here: scoring runs the teacher-forced decoder scan over the whole "
                              "target (models/deepnmt.py:103-218 with is_training), which is not built; only the cached "
                              "decode step is")


def check_params(params):
    """What this build of deepnmt does not do, from the parameters alone."""
    from zero_amd.models._decode import check_search_mode
    cell = str(params.cell).lower()
    if cell not in CELLS:
        raise NotImplementedError("deepnmt is built for cell=atr (rnns/atr.py), cell=gru (rnns/gru.py), cell=lrn (rnns/lrn.py) "
                                  "and cell=olrn (rnns/olrn.py) only: the %s cell has no step kernel here" % cell)
    if params.layer_norm:
        raise NotImplementedError("deepnmt with layer_norm=True is not built: it needs a LayerNorm behind every product of "
                                  "func.linear inside the cells, their input projections and the attention (func.py:36-53) "
                                  "and one on the residual stream after every layer (models/deepnmt.py:80-81, 173-174), "
                                  "which have no kernel here")
    if int(params.num_heads) != 1:
        raise NotImplementedError("deepnmt is built for num_heads=1: the additive attention kernel has one head, "
                                  "num_heads=%d splits the channels (func.py:130-152)" % int(params.num_heads))
    if int(params.num_encoder_layer) < 1 or int(params.num_decoder_layer) < 1:
        raise ValueError("deepnmt needs num_encoder_layer >= 1 (layer 0 produces the state the decoder starts from, "
                         "models/deepnmt.py:63-71) and num_decoder_layer >= 1 (layer 0 holds the attention) -- got %d and %d"
                         % (int(params.num_encoder_layer), int(params.num_decoder_layer)))
    check_search_mode("deepnmt", params)


def infer_fn(params):
    params = closing_dropout(copy.copy(params))
    from zero_amd import shortlist
    shortlist.check(params, "deepnmt")
    check_params(params)
    from zero_amd.models._rnn import make_infer_fns
    return make_infer_fns(params, "deepnmt")


# register the model, with a unique name
model.model_register("deepnmt", train_fn, score_fn, infer_fn)
