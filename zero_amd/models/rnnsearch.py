# coding: utf-8
"""``rnnsearch`` -- registered under the reference's name (models/rnnsearch.py, last line): the ATR recurrent encoder
(forward scan + context-aware or plain backward scan, rnns/rnn.py) and the attentional decoder (cond_rnn: lower ATR cell,
additive attention over the encoder memory, higher ATR cell; func.py:107-161).

Decode only, ``cell="atr"``, ``layer_norm=False``, ``search_mode="cache"`` (zero_amd/models/_rnnsearch.py holds the
schedule, zero_amd/csrc/zk_rnn.hip the kernels).  Everything else says what is missing when it is asked for, before a
core is built.
"""

import copy

from zero_amd.models import model
from zero_amd.models._factory import closing_dropout


def train_fn(features, params, initializer=None, on_ready=None):
    raise NotImplementedError("rnnsearch is decode only here: training needs the backward of the ATR scans (one launch per "
                              "time step and cell, rnns/rnn.py:41-59, 119-158) and of the additive attention "
                              "(func.py:107-161), which is not built")


def score_fn(features, params, initializer=None):
    raise NotImplementedError("rnnsearch is decode only here: scoring runs the teacher-forced decoder scan over the whole "
                              "target (models/rnnsearch.py:78-160 with is_training), which is not built; only the cached "
                              "decode step is")


def check_params(params):
    """What this build of rnnsearch does not do, from the parameters alone."""
    from zero_amd.models._decode import check_search_mode
    cell = str(params.cell).lower()
    if cell != "atr":
        raise NotImplementedError("rnnsearch is built for cell=atr only (rnns/atr.py, twin gates): the %s cell has no "
                                  "step kernel here" % cell)
    if params.layer_norm:
        raise NotImplementedError("rnnsearch with layer_norm=True is not built: the per-product layer normalisation "
                                  "inside the ATR cell and the attention (func.py:36-53) has no kernel here")
    check_search_mode("rnnsearch", params)


def infer_fn(params):
    params = closing_dropout(copy.copy(params))
    from zero_amd import shortlist
    shortlist.check(params, "rnnsearch")
    check_params(params)
    from zero_amd.models._rnn import make_infer_fns
    return make_infer_fns(params, "rnnsearch")


# register the model, with a unique name
model.model_register("rnnsearch", train_fn, score_fn, infer_fn)
