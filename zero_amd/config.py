# coding: utf-8
"""HParams defaults of the hot path -- the run.py config contract.

Key names, value types and defaults follow the reference's ``global_params``
(run.py:24-239) so that an existing ``param.json`` / ``--config`` dict /
``--parameters`` string of the reference loads unchanged.  Keys that only
drive out-of-scope subsystems (RNN cells, l0drop, EMA ...) are kept as inert
values for that reason.
"""

from zero_amd.utils.hparams import HParams

# (name, default) in the reference's declaration order (run.py:24-239).
_DEFAULTS = [
    ("shared_source_target_embedding", False),
    ("shared_target_softmax_embedding", True),
    ("decode_length", 50), ("beam_size", 4), ("decode_alpha", 0.6),
    ("enable_noise_beam_search", False), ("beam_search_temperature", 1.0),
    ("top_beams", 1), ("search_mode", "cache"),
    ("max_relative_position", 16),
    ("nstable", 4), ("lrdecay_start", 600000), ("lrdecay_end", 1200000),
    ("warmup_steps", 400), ("lrate_strategy", "gnmt+"), ("lrate_decay", 0.5),
    ("lrate_patience", 1), ("cosine_period", 5000), ("cosine_factor", 1),
    ("estop_patience", 100),
    ("initializer", "uniform"), ("initializer_gain", 0.08),
    ("hidden_size", 1000), ("embed_size", 620),
    ("dropout", 0.1), ("relu_dropout", 0.1), ("residual_dropout", 0.1),
    ("label_smooth", 0.1),
    ("model_name", "rnnsearch"), ("scope_name", "rnnsearch"),
    ("cell", "atr"), ("caencoder", True), ("layer_norm", False),
    ("use_deep_att", False), ("swap_memory", True),
    ("filter_size", 2048), ("attention_dropout", 0.1),
    ("num_encoder_layer", 6), ("num_decoder_layer", 6), ("num_heads", 8),
    ("aan_mask", True), ("use_ffn", False),
    ("max_len", 100), ("eval_max_len", 1000000),
    ("batch_size", 80), ("token_size", 3000), ("batch_or_token", "token"),
    ("eval_batch_size", 32), ("shuffle_batch", True),
    ("strategies", ["aan"]),
    ("process_num", 1), ("buffer_size", 100),
    ("input_queue_size", 100), ("output_queue_size", 100),
    ("src_vocab_file", ""), ("tgt_vocab_file", ""),
    ("src_train_file", ""), ("tgt_train_file", ""),
    ("src_dev_file", ""), ("tgt_dev_file", ""),
    ("src_test_file", ""), ("tgt_test_file", ""),
    ("output_dir", ""), ("test_output", ""), ("pretrained_model", ""),
    ("beta1", 0.9), ("beta2", 0.999), ("epsilon", 1e-9),
    ("clip_grad_norm", 5.0), ("gnorm_upper_bound", 1e20),
    ("lrate", 1e-5), ("min_lrate", 0.0), ("max_lrate", 1.0),
    ("epoches", 10), ("update_cycle", 1), ("gpus", [0]),
    ("safe_nan", False), ("dl4mt_redict", True), ("ema_decay", -1.),
    ("data_leak_ratio", 0.5), ("deep_transformer_init", False),
    ("disp_freq", 100), ("eval_freq", 10000), ("save_freq", 5000),
    ("sample_freq", 1000), ("checkpoints", 5), ("best_checkpoints", 1),
    ("max_training_steps", 1000),
    ("nthreads", 6), ("random_seed", 1234), ("train_continue", True),
    ("default_dtype", "float32"), ("dtype_epsilon", 1e-8), ("dtype_inf", 1e8),
    ("loss_scale", 1.0),
    # build-specific (round 5): "bfloat16" = the product decode path; "float32" = fp32 masters / activations / accumulation
    # through zk_f32_* (zero_amd/models/_decode_f32.py): rounds where the reference's default dtype rounds
    ("decode_dtype", "bfloat16"),
    # build-specific: "bfloat16" = score_fn runs the bf16 training-path forward; "float32" (same spellings as decode_dtype) =
    # the fp32 scorer (zero_amd/models/_score_f32.py).  decode_dtype does not select it: it keeps meaning decoding only
    ("score_dtype", "bfloat16"),
    ("l0_norm_reg_scalar", 1.0), ("l0_norm_start_reg_ramp_up", 0),
    ("l0_norm_end_reg_ramp_up", 10000), ("l0_norm_warm_up", True),
    # build-specific: lexical shortlist decoding (zero_amd/shortlist.py).  shortlist_file: the lexical table, lines of
    # "tgt_token src_token probability"; "" = off.  Per batch the output vocabulary is the shortlist_first lowest target
    # ids (at least 3: pad / unk / eos) plus the shortlist_best most probable translations of every source token, filled
    # with the lowest missing ids up to a multiple of shortlist_round (a multiple of 8; the size is part of the step
    # graphs' shape)
    ("shortlist_file", ""), ("shortlist_first", 100), ("shortlist_best", 100), ("shortlist_round", 1024),
    # build-specific: n-gram blocking inside the decode step (zk_ngram_ban; models/_decode.py search_tail).  n > 0: a
    # hypothesis never completes an n-gram it already holds -- the step's logits of such tokens are overwritten with the
    # forbid value BEFORE the log-softmax, so the rest is renormalised; 0 = off, at most 16
    ("no_repeat_ngram_size", 0),
    # build-specific: truncated decoding (zk_sample_truncate; models/_decode.py search_tail; the rule is stated in
    # tests/sampling_ref.py).  sampling_topk = k > 0: only the k most probable tokens of a beam row survive the step;
    # sampling_topp = p in (0, 1]: only the smallest set of most probable tokens whose softmax mass reaches p (1.0 keeps
    # everything).  The other logits are overwritten with the forbid value after the n-gram ban and BEFORE the Gumbel noise
    # and the log-softmax, so the rest is renormalised; 0 / 0.0 = off
    ("sampling_topk", 0), ("sampling_topp", 0.0),
    # build-specific: diverse beam search (zk_diverse_select; models/_decode.py search_tail; the rule is stated in
    # tests/diverse_ref.py).  diverse_beam_groups = G > 1: the beam_size rows of a sentence are G groups of beam_size / G,
    # each a beam search of its own; within a step group g sees every candidate's score -- the normalised
    # (prev + logp) / length_penalty -- lowered by diverse_beam_strength (lambda >= 0) * cnt(v) / length_penalty, cnt(v) being
    # how often the groups before it chose token v in this step.  beam_size % G == 0 and beam_size + beam_size / G <= 16;
    # 1 = off (the strength is then ignored)
    ("diverse_beam_groups", 1), ("diverse_beam_strength", 0.5),
    # build-specific: forced target prefixes (zk_prefix_force; models/_decode.py search_tail; the rule is stated in
    # tests/prefix_ref.py).  A file parallel to src_test_file, one line of target tokens per source line (an empty line: no
    # prefix): every hypothesis of that sentence starts with them.  While a prefix lasts, every other logit of the step is
    # overwritten with the forbid value BEFORE the log-softmax, so a forced token scores exactly 0 and a hypothesis' score
    # is log P(continuation | prefix); "" = off.  Not together with shortlist_file
    ("tgt_prefix_file", ""),
    # build-specific: word alignments from the decoder's cross-attention (zero_amd/align.py, models/_align.py, zk_align_probs;
    # the rule is stated in tests/align_ref.py).  alignment_file: --mode test writes one line per source line there, the
    # space-separated 0-based pairs s-t of the best hypothesis (t ascending); --mode score aligns the given (source, target)
    # pairs.  The alignment is read off ONE teacher-forced pass behind the search (the head-averaged weights of one decoder
    # layer, arg-max over the source words), so every search option keeps working unchanged; "" = off
    ("alignment_file", ""),
    # the decoder layer whose cross-attention is read, a Python-style index (-1 = the last layer)
    ("alignment_layer", -1),
    # every <unk> of a hypothesis becomes the raw source word it is aligned to (needs alignment_file)
    ("replace_unk", False),
]


def default_params():
    """A fresh HParams holding the reference defaults (run.py:24-239)."""
    return HParams(**dict(_DEFAULTS))


def transformer_base_params(**overrides):
    """Canonical Transformer-base recipe (docs/l0drop/README.md:81-115)."""
    p = default_params()
    p.override_from_dict(dict(
        hidden_size=512, embed_size=512, filter_size=2048, num_heads=8,
        num_encoder_layer=6, num_decoder_layer=6,
        dropout=0.1, relu_dropout=0.1, residual_dropout=0.1,
        attention_dropout=0.1, label_smooth=0.1,
        model_name="transformer", scope_name="transformer",
        initializer="uniform_unit_scaling", initializer_gain=1.0,
        lrate_strategy="noam", lrate=1.0, warmup_steps=4000,
        beta1=0.9, beta2=0.98, epsilon=1e-8, clip_grad_norm=0.0,
        token_size=6250, update_cycle=4, max_len=256,
    ))
    p.override_from_dict(overrides)
    return p


class SyntheticVocab(object):
    """Vocabulary of a given size with the reference's reserved ids
    (vocab.py:16-22: pad=0, unk=1, eos=2)."""

    def __init__(self, size):
        self._size = int(size)

    def size(self):
        return self._size

    def find(self, token):
        """The token of id i is its decimal spelling; None for anything else (Vocab.find)."""
        return int(token) if token.isdigit() and int(token) < self._size else None

    def pad(self):
        return 0

    def unk(self):
        return 1

    def eos(self):
        return 2
