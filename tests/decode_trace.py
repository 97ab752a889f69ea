"""The launch trace of decoding: which library entry points the host code of a decode batch calls, in which order and
with which scalar arguments.  Shared by tests/golden/make_decode_launch_trace.py (records the pinned file) and
tests/test_gpu_decode_launch_trace.py (reproduces it); ``diff`` is checked on its own in
tests/test_decode_trace_checker.py.

A trace is ``{phase: [[entry point, [argument, ...]], ...], "graph_nodes": int}``.  An argument is recorded by the
prototype table parsed from include/zero_hip.h (``lib.protos``): a pointer as None (NULL) or "nonnull", everything else
by value.  Phases: ``encode`` (encoding_fn), ``step0`` / ``reorder`` / ``step1`` (two eager decoding_fn calls at
time = 0, 1 with an identity reorder of the caches between them); ``graph_nodes`` is ``core._decode_step_launches``
after one whole beam search of the same batch.  A scoring case has one phase, ``score`` (one score_fn call on a batch of
5 sentence pairs of at most 9 and 11 tokens), and no ``graph_nodes``: a case names its own phases.

Shapes: the smallest that take every arm -- H = 128, F = 256, 2 heads (head size 64: the fused attention launches
apply), 2 + 2 layers, B = 5 sources of at most 9 tokens, beam 4.
"""
import ctypes
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_launch_trace.json")
MODELS = ("transformer", "transformer_aan", "transformer_rpr", "transformer_fuse", "transformer_l0drop", "transformer_rela",
          "transformer_fixup")
SWITCHES = ("ZERO_HIP_DECODE_FUSE_ATT", "ZERO_HIP_DECODE_FUSE_LN", "ZERO_HIP_F32_FUSE")
PHASES = ("encode", "step0", "reorder", "step1")
K = 4
L0DROP_SEED = 43


def _cases():
    out = {}
    for m in MODELS:
        for dt in ("bfloat16", "float32"):
            out["%s-%s" % (m, dt)] = dict(models=(m,), dtype=dt)
    for m in ("transformer", "transformer_aan", "transformer_rpr"):
        out["%s-bfloat16-fuse_att0" % m] = dict(models=(m,), env={"ZERO_HIP_DECODE_FUSE_ATT": "0"})
    out["transformer_aan-bfloat16-fuse_ln0"] = dict(models=("transformer_aan",), env={"ZERO_HIP_DECODE_FUSE_LN": "0"})
    out["transformer_aan-bfloat16-use_ffn"] = dict(models=("transformer_aan",), hp={"use_ffn": True})
    for m in ("transformer", "transformer_aan"):
        out["%s-float32-f32_fuse0" % m] = dict(models=(m,), dtype="float32", env={"ZERO_HIP_F32_FUSE": "0"})
    out["transformer-bfloat16-head32"] = dict(models=("transformer",), hp={"hidden_size": 96, "embed_size": 96, "num_heads": 3})
    out["ensemble-bfloat16"] = dict(models=("transformer", "transformer_aan"))
    for dt in ("bfloat16", "float32"):           # both encoder forms, weights as tests/test_gpu_rnnsearch_model.py builds them
        for tag, ca in (("", True), ("-caencoder0", False)):
            out["rnnsearch-%s%s" % (dt, tag)] = dict(models=("rnnsearch",), dtype=dt,
                                                    hp={"cell": "atr", "caencoder": ca, "layer_norm": False})
    # the deep recurrent models at the sizes of their model tests, 9 source positions (no padding: a scan is a launch or two per
    # position).  rnnsearch_deepatt: NE = D = 2 takes the forward scan, the reversed and the un-reversed pair
    pad1 = {"ZERO_HIP_DECODE_PAD_LEN": "1"}
    for dt in ("bfloat16", "float32"):
        for c in ("atr", "gru", "lrn", "olrn"):
            out["rnnsearch_deepatt-%s-%s" % (dt, c)] = dict(
                models=("rnnsearch_deepatt",), dtype=dt, env=pad1,
                hp={"cell": c, "embed_size": 64, "num_heads": 1, "num_encoder_layer": 2, "num_decoder_layer": 2,
                    "layer_norm": False})
        # deepnmt_ref.CONFIGS: (A) caencoder, one-to-one layers, dl4mt_redict, x_map + LayerNorm; (B) the plain [x | c] form
        # with the feature gather; (C) gru, use_deep_att, E == H; (A) with olrn: the paired one-launch layers; (B) with lrn
        for tag, config, c in (("A", "A", None), ("B", "B", None), ("C", "C", None), ("A-olrn", "A", "olrn"), ("B-lrn", "B", "lrn")):
            out["deepnmt-%s-%s" % (dt, tag)] = dict(models=("deepnmt",), dtype=dt, env=pad1, deepnmt=(config, c))
    # score_fn: the fp32 scorer of every model that has one and both of its switches, the bf16 scorer of transformer_fixup
    for m in ("transformer", "transformer_aan", "transformer_rpr", "transformer_fuse"):
        out["score-%s-float32" % m] = dict(models=(m,), dtype="float32", score=True)
    out["score-transformer_aan-float32-use_ffn"] = dict(models=("transformer_aan",), dtype="float32", score=True,
                                                        hp={"use_ffn": True})
    out["score-transformer-float32-f32_fuse0"] = dict(models=("transformer",), dtype="float32", score=True,
                                                      env={"ZERO_HIP_F32_FUSE": "0"})
    out["score-transformer_fixup-bfloat16"] = dict(models=("transformer_fixup",), score=True)
    return out


CASES = _cases()


def phases(name):
    """The phases of case ``name``, in the order they are recorded."""
    return ("score",) if CASES[name].get("score") else PHASES


def summary(trace):
    """'<launches per phase> launches[, graph of <n> nodes]' of a trace, for the print lines."""
    text = " + ".join("%d" % len(v) for v in trace.values() if isinstance(v, list)) + " launches"
    return text + (", graph of %d nodes" % trace["graph_nodes"] if "graph_nodes" in trace else "")


def _overrides(case):
    """The hparams a case sets; a deepnmt case names its configuration of tests/deepnmt_ref.py and, maybe, another cell."""
    if "deepnmt" not in case:
        return case.get("hp", {})
    from tests import deepnmt_ref
    config, cell = case["deepnmt"]
    cfg = dict(deepnmt_ref.CONFIGS[config], layer_norm=False, num_heads=1)
    cfg["hidden_size"], cfg["embed_size"] = cfg.pop("H"), cfg.pop("E")
    if cell is not None:
        cfg["cell"] = cell
    return cfg


def _batch(hp, seed):
    from tests.common import make_batch
    return make_batch(np.random.default_rng(seed), 5, 9, 11, hp.src_vocab.size(), hp.tgt_vocab.size())


def _params(hp, model, src, seed):
    """Weights as the model tests of each variant build them (tests/test_gpu_decode_fuse.py::_model)."""
    from oracle import ref_torch as rt
    from tests.common import perturb
    if model == "transformer_l0drop":
        # a source_pruning pair that keeps some but not all positions of every sentence (6, 8, 3, 7 and 2 of them), with
        # the margin make_fixture asserts: 0.61 from the threshold against a bf16-storage error of 0.057
        from tests import l0drop_ref
        Pn = dict(l0drop_ref.make_fixture(hp, src, L0DROP_SEED)["Pn"])
    elif model == "transformer_rela":
        from tests import rela_ref
        Pn = rela_ref.init_params(hp, seed)
    elif model == "transformer_fixup":
        from tests import fixup_ref
        Pn = dict(fixup_ref.init_params(hp, seed))
    elif model == "rnnsearch":
        from tests import rnnsearch_ref
        Pn = rnnsearch_ref.init_params(hp, seed)
    elif model == "rnnsearch_deepatt":
        from tests import deepatt_ref
        Pn = deepatt_ref.init_params(hp, seed)
    elif model == "deepnmt":
        from tests import deepnmt_ref
        Pn = deepnmt_ref.init_params(hp, seed)
    else:
        Pn = perturb(rt.init_params(hp, model, seed=seed + 1), np.random.default_rng(seed))
    Pn["tgt_embedding"] = (Pn["tgt_embedding"] * 6.0).astype(np.float32)
    return Pn


def _argument(ctype, value):
    if ctype is ctypes.c_void_p:
        if value is None or (isinstance(value, int) and value == 0):
            return None
        if isinstance(value, ctypes.c_void_p) and not value.value:
            return None
        return "nonnull"
    if ctype is ctypes.c_float:
        return float(value)
    return int(value)


class Recorder(object):
    """Wraps ``_Lib.call`` (through ``patch.setattr``: a pytest monkeypatch) and files every call under the open phase."""

    def __init__(self, patch):
        from zero_amd import hip
        self.phases = {}
        self.open = None
        inner = hip._Lib.call
        rec = self

        def call(lib, name, *args):
            if rec.open is not None:
                types = lib.protos[name][1]
                assert len(types) == len(args), (name, len(types), len(args))
                rec.phases[rec.open].append([name, [_argument(t, a) for t, a in zip(types, args)]])
            return inner(lib, name, *args)
        patch.setattr(hip._Lib, "call", call)

    def phase(self, name):
        rec = self

        class _Phase(object):
            def __enter__(self):
                rec.phases[name] = []
                rec.open = name

            def __exit__(self, *a):
                rec.open = None
        return _Phase()


def run_case(name, patch):
    """Runs case ``name`` on the device -> its trace.  patch: a pytest monkeypatch (environment and ``_Lib.call``)."""
    import torch
    from tests.common import make_hp
    from zero_amd import search
    from zero_amd.models import model as registry, load_all
    from zero_amd.models._factory import get_core, reset_cores
    load_all()
    case = CASES[name]
    for k in SWITCHES:
        patch.delenv(k, raising=False)
    for k, v in case.get("env", {}).items():
        patch.setenv(k, v)
    models = case["models"]
    hps, Pns = [], []
    for i, m in enumerate(models):
        hp = make_hp(m, beam_size=K, search_mode="cache",
                     **{"score_dtype" if case.get("score") else "decode_dtype": case.get("dtype", "bfloat16")})
        hp.override_from_dict(_overrides(case))
        if i == 0:
            src, tgt = _batch(hp, 21)
        hps.append(hp)
        Pns.append(_params(hp, m, src, 21 + i))
    reset_cores()
    if case.get("score"):
        get_core(hps[0], models[0], Pns[0])
        rec = Recorder(patch)
        with rec.phase("score"):
            registry.get_model(models[0]).score_fn({"source": src, "target": tgt}, hps[0])
        torch.cuda.synchronize()
        reset_cores()
        return dict(rec.phases)
    if len(models) == 1:
        core = get_core(hps[0], models[0], Pns[0])
        enc, dec = registry.get_model(models[0]).infer_fn(hps[0])
        hp0 = hps[0]
    else:
        from zero_amd.models import _ensemble
        core = [get_core(_ensemble.member_params(hp, i), m, Pn) for i, (hp, Pn, m) in enumerate(zip(hps, Pns, models))][0]
        enc, dec, hp0 = _ensemble.make_infer_fns([registry.get_model(m) for m in models], hps)
    rng = np.random.default_rng(5)
    BK = src.shape[0] * K
    toks = [torch.from_numpy(rng.integers(3, hp0.tgt_vocab.size(), size=(BK,)).astype(np.int32)).to(core.eng.device)
            for _ in range(2)]
    ident = torch.arange(BK, dtype=torch.int32, device=core.eng.device)
    rec = Recorder(patch)
    with rec.phase("encode"):
        state = enc(src)
    with rec.phase("step0"):
        _, state = dec(toks[0], state, 0)
    with rec.phase("reorder"):
        state.reorder(ident)
    with rec.phase("step1"):
        _, state = dec(toks[1], state, 1)
    torch.cuda.synchronize()
    core.__dict__.pop("_decode_step_launches", None)
    out = search.beam_search({"source": src}, enc, dec, hp0)
    assert out["steps"] >= 4, out["steps"]           # both parities were captured
    trace = dict(rec.phases)
    trace["graph_nodes"] = int(core.__dict__.get("_decode_step_launches", 0))
    reset_cores()
    return trace


def diff(want, got):
    """-> list of messages, empty if ``got`` reproduces ``want`` exactly: same phases, same entry points in the same
    order, same pointer pattern and same scalar values."""
    msgs = []
    if sorted(want) != sorted(got):
        return ["phases differ: %s against %s" % (sorted(want), sorted(got))]
    for ph in sorted(want):
        a, b = want[ph], got[ph]
        if not isinstance(a, list):
            if a != b:
                msgs.append("%s: %r, recorded %r" % (ph, b, a))
            continue
        if [c[0] for c in a] != [c[0] for c in b]:
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x[0] != y[0]), min(len(a), len(b)))
            msgs.append("%s: launch %d is %s, recorded %s (%d launches, recorded %d)"
                        % (ph, i, b[i][0] if i < len(b) else "missing", a[i][0] if i < len(a) else "nothing", len(b), len(a)))
            continue
        for i, (x, y) in enumerate(zip(a, b)):
            if len(x[1]) != len(y[1]):
                msgs.append("%s: launch %d (%s) has %d arguments, recorded %d" % (ph, i, x[0], len(y[1]), len(x[1])))
                continue
            for j, (u, v) in enumerate(zip(x[1], y[1])):
                if type(u) is not type(v) or u != v:
                    msgs.append("%s: launch %d (%s) argument %d is %r, recorded %r" % (ph, i, x[0], j, v, u))
    return msgs


def dump(traces, path=GOLDEN):
    """One launch per line: the file stays readable in a diff."""
    lines = []
    for name in sorted(traces):
        tr = traces[name]
        body = []
        for ph, launches in tr.items():
            if isinstance(launches, list):
                calls = ",\n".join("   " + json.dumps(c, separators=(",", ":")) for c in launches)
                body.append('  "%s": [\n%s\n  ]' % (ph, calls))
        if "graph_nodes" in tr:
            body.append('  "graph_nodes": %d' % tr["graph_nodes"])
        lines.append('"%s": {\n%s\n }' % (name, ",\n".join(body)))
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")


def load(path=GOLDEN):
    with open(path) as f:
        return json.load(f)
