# coding: utf-8
"""``rnnsearch_deepatt`` -- registered under the reference's name (models/rnnsearch_deepatt.py, last line): Zhang et al.,
"Neural Machine Translation with Deep Attention" (TPAMI).  The encoder is a plain forward scan followed by
``num_encoder_layer`` conditional scans (cond_rnn(one2one=True), alternately reversed); the decoder step is a lower cell
followed by ``num_decoder_layer`` pairs (additive attention over ONE shared projected memory, higher cell).

Decode only, ``cell`` in {atr, gru, lrn, olrn}, ``layer_norm=False``, ``num_heads=1``, ``search_mode="cache"`` (zero_amd/models/_deepatt.py
holds the schedule, zero_amd/csrc/zk_rnn.hip the kernels).  Everything else says what is missing when it is asked for, before a
core is built.  The published recipe trains with ``layer_norm=True``: its checkpoints do not decode here yet.
"""

import copy

from zero_amd.models import model
from zero_amd.models._factory import closing_dropout

CELLS = ("atr", "gru", "lrn", "olrn")


def train_fn(features, params, initializer=None, on_ready=None):
    raise NotImplementedError("rnnsearch_deepatt is decode only here: training needs the backward of the recurrent scans "
                              "(one or two launches per time step and cell, rnns/rnn.py:41-59, 119-158) and of the deep "
                              "attention decoder (models/rnnsearch_deepatt.py:132-236), which is not built")


def score_fn(features, params, initializer=None):
    raise NotImplementedError("rnnsearch_deepatt is decode only here: scoring runs the teacher-forced decoder scan over the "
                              "whole target (models/rnnsearch_deepatt.py:240-327 with is_training), which is not built; only "
                              "the cached decode step is")


def check_params(params):
    """What this build of rnnsearch_deepatt does not do, from the parameters alone."""
    from zero_amd.models._decode import check_search_mode
    cell = str(params.cell).lower()
    if cell not in CELLS:
        raise NotImplementedError("rnnsearch_deepatt is built for cell=atr (rnns/atr.py), cell=gru (rnns/gru.py), cell=lrn "
                                  "(rnns/lrn.py) and cell=olrn (rnns/olrn.py) only: the %s cell has no step kernel here" % cell)
    if params.layer_norm:
        raise NotImplementedError("rnnsearch_deepatt with layer_norm=True is not built: it needs a LayerNorm behind every "
                                  "product of func.linear -- inside the cells, their input projections and the attention "
                                  "(func.py:36-53) --, which has no kernel here; the published recipe's checkpoints "
                                  "(layer_norm=True) do not decode yet")
    if int(params.num_heads) != 1:
        raise NotImplementedError("rnnsearch_deepatt is built for num_heads=1 (the recipe's value): the additive attention "
                                  "kernel has one head, num_heads=%d splits the channels (func.py:130-152)"
                                  % int(params.num_heads))
    if int(params.num_decoder_layer) < 1 or int(params.num_encoder_layer) < 0:
        raise ValueError("rnnsearch_deepatt needs num_decoder_layer >= 1 (the decoder's output is the last higher cell's, "
                         "models/rnnsearch_deepatt.py:235) and num_encoder_layer >= 0 -- got %d and %d"
                         % (int(params.num_decoder_layer), int(params.num_encoder_layer)))
    check_search_mode("rnnsearch_deepatt", params)


def infer_fn(params):
    params = closing_dropout(copy.copy(params))
    from zero_amd import shortlist
    shortlist.check(params, "rnnsearch_deepatt")
    check_params(params)
    from zero_amd.models._rnn import make_infer_fns
    return make_infer_fns(params, "rnnsearch_deepatt")


# register the model, with a unique name
model.model_register("rnnsearch_deepatt", train_fn, score_fn, infer_fn)
