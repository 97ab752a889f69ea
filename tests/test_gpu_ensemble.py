"""Ensemble decoding on the GPU: the combine kernel against fp64, and the whole search over M members against the
ensemble oracle composed from oracle/ref_torch.py (tests/ensemble_common.py; checked on its own in
tests/test_ensemble_host.py)."""
import copy
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import ref_torch as rt  # noqa: E402
from tests import ensemble_common as ec  # noqa: E402
from zero_amd.models._factory import get_core, reset_cores  # noqa: E402
from zero_amd.models import model as registry, load_all  # noqa: E402

pytestmark = pytest.mark.gpu
load_all()

SET_A = ("transformer", "transformer_aan", "transformer_rpr")
SET_B = ("transformer", "transformer_fuse")
SEEDS = (3, 4, 5)
ROUTES = (("default", {}), ("host_c", {"ZERO_HIP_DECODE_DEVICE_BOOK": "0"}), ("numpy", {"ZERO_HIP_DECODE_HOST_C": "0"}),
          ("eager", {"ZERO_HIP_DECODE_GRAPH": "0"}))
ROUTE_VARS = ("ZERO_HIP_DECODE_DEVICE_BOOK", "ZERO_HIP_DECODE_HOST_C", "ZERO_HIP_DECODE_GRAPH")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------------
def _launch(eng, xs, V, out):
    """zk_ensemble_logprob on cuda tensors xs[m] [rows, ld_m] -> out [rows, ld_out] (columns < V)."""
    M, rows = len(xs), xs[0].shape[0]
    ws = eng.workspace(eng.lib.query("zk_ensemble_logprob_workspace", rows, M, V))
    eng.lib.call("zk_ensemble_logprob", (ctypes.c_void_p * M)(*[x.data_ptr() for x in xs]),
                 (ctypes.c_int * M)(*[x.shape[1] for x in xs]), M, rows, V, out.data_ptr(), out.shape[1], ws.data_ptr(),
                 ws.numel(), eng.stream)


def _check_kernel(tag, x, V, ld):
    """x: CPU fp32 [M, rows, V].  The bound is max(5e-6, 4 * e32): 5e-6 is the project's fp32 bar
    (tests/test_gpu_decode_f32.py), e32 the error fp32 arithmetic itself makes on these inputs -- torch on the CPU in
    fp32 against fp64, the smaller of the literal form log(mean softmax) and of the stable form the kernel evaluates (the
    literal form is -inf in fp32 where every probability underflows; the stable form is what the kernel documents)."""
    from tests.util_gpu import eng
    e = eng()
    M, rows = x.shape[0], x.shape[1]
    want = torch.log(torch.softmax(x.double(), -1).mean(0))
    assert torch.isfinite(want).all(), tag
    lit = torch.log(torch.softmax(x, -1).mean(0)).double()
    stable = (torch.logsumexp(x - torch.logsumexp(x, -1, keepdim=True), 0) - math.log(M)).double()
    e32 = min(float((lit - want).abs().nan_to_num(nan=math.inf).max()), float((stable - want).abs().max()))
    bound = max(5e-6, 4 * e32)
    xs = []
    for m in range(M):
        t = torch.full((rows, ld + 4 * m), 7.0)          # members may have different leading dimensions
        t[:, :V] = x[m]
        xs.append(t.cuda())
    out = torch.full((rows, ld), -77.0, device="cuda")
    _launch(e, xs, V, out)
    torch.cuda.synchronize()
    got = out.cpu()
    assert (got[:, V:] == -77.0).all(), "%s: columns >= V were written" % tag
    err = float((got[:, :V].double() - want).abs().max())
    print("ensemble_logprob %s: err %.3e  e32 %.3e  bound %.3e" % (tag, err, e32, bound))
    assert torch.isfinite(got[:, :V]).all(), tag
    assert err <= bound, (tag, err, bound)
    return xs, out


@pytest.mark.parametrize("V,ld", [(11, 16), (104, 112), (32000, 32064)])
@pytest.mark.parametrize("M", [1, 2, 3, 5])
def test_kernel_against_fp64(M, V, ld):
    g = torch.Generator().manual_seed(100 * M + V)
    for rows in (1, 20, 128):
        for scale in (1.0, 10.0):
            x = torch.randn(M, rows, V, generator=g) * scale
            _check_kernel("M=%d V=%d rows=%d scale=%g" % (M, V, rows, scale), x, V, ld)
            if M == 1:
                # a plain fp32 log-softmax, to the same bound
                from tests.util_gpu import eng
                xs = [torch.zeros(rows, ld)]
                xs[0][:, :V] = x[0]
                out = torch.zeros(rows, ld, device="cuda")
                _launch(eng(), [xs[0].cuda()], V, out)
                ref = torch.log_softmax(x[0].double(), -1)
                e32 = float((torch.log_softmax(x[0], -1).double() - ref).abs().max())
                err = float((out.cpu()[:, :V].double() - ref).abs().max())
                print("  vs log_softmax: err %.3e  e32 %.3e" % (err, e32))
                assert err <= max(5e-6, 4 * e32)


def test_kernel_where_probabilities_underflow():
    g = torch.Generator().manual_seed(7)
    M, rows, V = 3, 20, 104
    # one member's logits shifted by -200 on half of the columns: its probabilities underflow there and the result
    # is the other members' share
    x = torch.randn(M, rows, V, generator=g)
    x[1, :, : V // 2] -= 200.0
    _check_kernel("member 1 underflows on half of the columns", x, V, 112)
    others = torch.log(torch.softmax(x[[0, 2]].double(), -1).sum(0) / M)
    want = torch.log(torch.softmax(x.double(), -1).mean(0))
    assert float((others - want)[:, : V // 2].abs().max()) < 1e-12
    # a column that is very unlikely for ALL members: finite (the reference's literal fp32 form gives -inf here)
    x = torch.randn(M, rows, V, generator=g)
    x[:, :, 17] -= 300.0
    assert torch.isinf(torch.log(torch.softmax(x, -1).mean(0))[:, 17]).all()
    _, out = _check_kernel("column 17 unlikely for every member", x, V, 112)
    assert torch.isfinite(out[:, 17]).all() and float(out[:, 17].max()) < -250.0


def test_kernel_replayed_from_a_graph_equals_the_eager_call():
    from tests.util_gpu import eng
    e = eng()
    g = torch.Generator().manual_seed(11)
    M, rows, V, ld = 3, 128, 32000, 32064
    xs = [(torch.randn(rows, ld, generator=g) * 3).cuda() for _ in range(M)]
    with torch.cuda.stream(e.work_stream):
        eager = torch.zeros(rows, ld, device="cuda")
        _launch(e, xs, V, eager)
        replay = torch.zeros(rows, ld, device="cuda")
        torch.cuda.synchronize()
        exec_ = e.graph_capture(lambda: _launch(e, xs, V, replay))
        assert e.last_graph_nodes == 2
        assert not replay.any(), "capturing must not run the kernel"
        e.graph_launch(exec_)
        torch.cuda.synchronize()
        assert torch.equal(replay[:, :V], eager[:, :V])
        xs[1].mul_(0.5)                      # a replay reads the current contents of the same buffers
        _launch(e, xs, V, eager)
        e.graph_launch(exec_)
        torch.cuda.synchronize()
        assert torch.equal(replay[:, :V], eager[:, :V])
        e.lib.call("zk_graph_destroy", exec_)


def test_kernel_argument_errors():
    from tests.util_gpu import eng
    from zero_amd.hip import ZeroHipError
    e = eng()
    xs = [torch.zeros(4, 16, device="cuda") for _ in range(9)]
    out = torch.zeros(4, 16, device="cuda")
    n = e.lib.ncalls
    with pytest.raises(ZeroHipError, match="out of range"):
        _launch(e, xs, 11, out)
    with pytest.raises(ZeroHipError, match="multiple of 4"):
        _launch(e, [torch.zeros(4, 14, device="cuda")], 11, out)
    assert e.lib.ncalls == n + 2 and int(e.lib.raw("zk_ensemble_max")()) == 8


# ---------------------------------------------------------------------------------------------------------------------
# 2.-7. the search over M members
# ---------------------------------------------------------------------------------------------------------------------
def _install(hps, Pns, models):
    """The members' variables under their ensemble scopes (fresh process state)."""
    from zero_amd.models._ensemble import member_params
    reset_cores()
    for i, (hp, Pn, m) in enumerate(zip(hps, Pns, models)):
        get_core(member_params(hp, i), m, Pn)


def _decode(hps, models, src):
    from zero_amd import search
    from zero_amd.models._ensemble import make_infer_fns
    enc, dec, hp0 = make_infer_fns([registry.get_model(m) for m in models], hps)
    out = search.beam_search({"source": src}, enc, dec, hp0)
    return {"seq": np.asarray(out["seq"]).copy(), "score": np.asarray(out["score"]).copy(), "steps": out["steps"]}


def _same_beams(got, ref):
    L = min(got["seq"].shape[2], ref["seq"].shape[2])
    return np.array_equal(got["seq"][:, :, :L], ref["seq"][:, :, :L]) and not got["seq"][:, :, L:].any() \
        and not ref["seq"][:, :, L:].any()


@pytest.mark.parametrize("models", [SET_A, SET_B])
@pytest.mark.parametrize("K", [1, 4])
def test_fp32_mode_is_token_exact(models, K):
    """decode_dtype = float32: every beam of every sentence equals the composed fp32 oracle, the step counts are equal,
    the scores of finished hypotheses agree to the single model's bound (tests/test_gpu_decode_f32.py)."""
    hps, Pns, src = ec.make_members(models, SEEDS)
    hps = ec.with_beam(hps, K, decode_dtype="float32")
    ref = ec.composed_oracle(hps, Pns, models, src)
    _install(hps, Pns, models)
    got = _decode(hps, models, src)
    assert _same_beams(got, ref), (got["seq"], ref["seq"])
    assert got["steps"] == ref["steps"], (got["steps"], ref["steps"])
    fin = ref["score"] > -1e30
    print("fp32 ensemble %s K=%d: %d steps, score err %.2e" % (models[-1], K, got["steps"],
                                                             np.abs(got["score"][fin] - ref["score"][fin]).max()))
    assert np.allclose(got["score"][fin], ref["score"][fin], rtol=1e-5, atol=1e-6)
    assert get_core(_member_hp(hps, 0), models[0]).__dict__.get("_decode_step_launches", 0) > 0, \
        "the default route must replay a captured step"


def _member_hp(hps, i):
    from zero_amd.models._ensemble import member_params
    return member_params(hps[i], i)


@pytest.mark.parametrize("models", [SET_A, SET_B])
@pytest.mark.parametrize("K", [1, 4])
def test_bf16_mode_best_hypotheses(models, K):
    """The bf16 product path: beam 0 of EVERY sentence equals the fp32 composed oracle.  The batch (seeds 3/4/5) was
    first checked on the CPU -- the check repeated here before the device runs: the composed oracle under the bf16 storage
    model (rt.Cfg.store_bf16 = True; restored in a finally by ensemble_common.composed_oracle) gives the same beam-0
    hypotheses as the fp32 one, i.e. bf16 storage alone does not move this batch's best hypotheses."""
    hps, Pns, src = ec.make_members(models, SEEDS)
    hps = ec.with_beam(hps, K)
    ref = ec.composed_oracle(hps, Pns, models, src)
    ref_bf = ec.composed_oracle(hps, Pns, models, src, store_bf16=True)
    assert rt.Cfg.store_bf16 is False
    want = rt.decode_hypothesis(ref["seq"], hps[0])
    assert rt.decode_hypothesis(ref_bf["seq"], hps[0]) == want, "the seed check of the docstring no longer holds"
    _install(hps, Pns, models)
    got = _decode(hps, models, src)
    from zero_amd.search import decode_hypothesis
    have = decode_hypothesis(got["seq"], hps[0])
    assert len(have) == src.shape[0]
    assert have == want, (have, want)
    assert np.isfinite(got["score"][:, 0]).all()


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_routes_agree(dtype, monkeypatch):
    """Graph + device book (default), host-C bookkeeping, numpy bookkeeping and the eager step: identical seq, score and
    steps, on fresh cores each (tests/test_gpu_model.py test_device_resident_search_equals_host_bookkeeping)."""
    hps, Pns, src = ec.make_members(SET_A, SEEDS)
    hps = ec.with_beam(hps, 4, decode_dtype=dtype)
    outs = {}
    for name, env in ROUTES:
        for k in ROUTE_VARS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _install(hps, Pns, SET_A)
        outs[name] = _decode(hps, SET_A, src)
        launches = get_core(_member_hp(hps, 0), SET_A[0]).__dict__.get("_decode_step_launches", 0)
        assert (launches > 0) == (name != "eager"), (name, launches)
    ref = outs["host_c"]
    assert ref["steps"] > 2
    for name in ("default", "numpy", "eager"):
        o = outs[name]
        assert o["steps"] == ref["steps"], (name, o["steps"], ref["steps"])
        assert np.array_equal(o["seq"], ref["seq"]), name
        assert np.array_equal(o["score"], ref["score"]), name


def test_dev_search_mode_bf16():
    """search_mode = "dev": every member re-runs its training-path decoder on the whole prefix, the same combine, the
    numpy bookkeeping.  The training path is what the oracle's bf16 storage model describes, and on this batch that model
    leaves the beam-0 hypotheses of the fp32 composed oracle unchanged (test_bf16_mode_best_hypotheses): beam 0 equals
    the oracle's."""
    from zero_amd.search import decode_hypothesis
    hps, Pns, src = ec.make_members(SET_A, SEEDS)
    ref = ec.composed_oracle(ec.with_beam(hps, 4), Pns, SET_A, src)      # (the oracle's cache mode: the same mathematics)
    hps = ec.with_beam(hps, 4, search_mode="dev")
    _install(hps, Pns, SET_A)
    dev = _decode(hps, SET_A, src)
    assert np.isfinite(dev["score"][:, 0]).all()
    assert decode_hypothesis(dev["seq"], hps[0]) == rt.decode_hypothesis(ref["seq"], hps[0])


def test_two_identical_members_decode_like_the_single_model():
    """log(mean of two equal distributions) is that distribution: all beams of the single model, fp32 mode."""
    from zero_amd.main import tower_infer_graph
    hps, Pns, src = ec.make_members(("transformer_aan",), (4,))
    hp = ec.with_beam(hps, 4, decode_dtype="float32")[0]
    _install([hp, hp], [Pns[0], Pns[0]], ("transformer_aan",) * 2)
    twin = _decode([hp, hp], ("transformer_aan",) * 2, src)
    get_core(hp, "transformer_aan", Pns[0])
    seqs, scores = tower_infer_graph({"source": src}, registry.get_model("transformer_aan"), hp)
    single = {"seq": np.asarray(seqs), "score": np.asarray(scores)}
    assert _same_beams(twin, single)
    fin = single["score"] > -1e30
    assert np.allclose(twin["score"][fin], single["score"][fin], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_one_member_equals_tower_infer_graph(dtype):
    """M = 1 through tower_ensemble_graph: seq bit for bit; scores within the fp32 bound (the extra log-softmax pass is
    the only difference)."""
    from zero_amd.main import tower_ensemble_graph, tower_infer_graph
    hps, Pns, src = ec.make_members(("transformer",), (3,))
    hp = ec.with_beam(hps, 4, decode_dtype=dtype)[0]
    _install([hp], Pns, ("transformer",))
    g = registry.get_model("transformer")
    seqs1, scores1 = tower_ensemble_graph({"source": src}, [g], [hp])
    get_core(hp, "transformer", Pns[0])
    seqs, scores = tower_infer_graph({"source": src}, g, hp)
    assert np.array_equal(np.asarray(seqs1), np.asarray(seqs))
    fin = np.asarray(scores) > -1e30
    assert np.allclose(np.asarray(scores1)[fin], np.asarray(scores)[fin], rtol=1e-5, atol=1e-6)


def test_single_then_ensemble_then_single_on_one_process():
    """The graph cache and the per-scope cores: a single model, an ensemble that contains its type, the single model again,
    without reset_cores() in between.  First and third are identical; the ensemble's result is what it is on a fresh
    process state."""
    from zero_amd.main import tower_infer_graph
    from zero_amd.models._ensemble import member_params
    hps, Pns, src = ec.make_members(SET_A, SEEDS)
    hps = ec.with_beam(hps, 4)
    _install(hps, Pns, SET_A)
    fresh = _decode(hps, SET_A, src)
    reset_cores()
    g = registry.get_model(SET_A[1])
    get_core(hps[1], SET_A[1], Pns[1])
    first = tower_infer_graph({"source": src}, g, hps[1])
    for i, (hp, Pn, m) in enumerate(zip(hps, Pns, SET_A)):
        get_core(member_params(hp, i), m, Pn)
    ens = _decode(hps, SET_A, src)
    ens2 = _decode(hps, SET_A, src)              # and a second batch on the same cores (graphs captured anew)
    third = tower_infer_graph({"source": src}, g, hps[1])
    assert np.array_equal(np.asarray(first[0]), np.asarray(third[0]))
    assert np.array_equal(np.asarray(first[1]), np.asarray(third[1]))
    for o in (ens, ens2):
        assert np.array_equal(o["seq"], fresh["seq"]) and np.array_equal(o["score"], fresh["score"])
        assert o["steps"] == fresh["steps"]


def test_errors_before_any_launch():
    from tests.util_gpu import eng
    from zero_amd.config import SyntheticVocab
    from zero_amd.hip import ZeroHipError
    from zero_amd.main import tower_ensemble_graph
    hps, Pns, src = ec.make_members(SET_B, SEEDS)
    graphs = [registry.get_model(m) for m in SET_B]
    lib = eng().lib
    n = lib.ncalls
    bad = copy.copy(hps[1])
    bad.tgt_vocab = SyntheticVocab(hps[0].tgt_vocab.size() + 1)
    with pytest.raises(ZeroHipError, match="target vocabulary"):
        tower_ensemble_graph({"source": src}, graphs, [hps[0], bad])
    bad = copy.copy(hps[1])
    bad.decode_dtype = "float32"
    with pytest.raises(ZeroHipError, match="decode_dtype"):
        tower_ensemble_graph({"source": src}, graphs, [hps[0], bad])
    with pytest.raises(ZeroHipError, match="at most 8"):
        tower_ensemble_graph({"source": src}, [graphs[0]] * 9, [hps[0]] * 9)
    with pytest.raises(ZeroHipError, match="at least one"):
        tower_ensemble_graph({"source": src}, [], [])
    assert lib.ncalls == n


def test_cli_ensemble_mode(tmp_path):
    """run.py:322-363 end to end in fresh interpreters: --mode train writes two directories (different model types and
    sizes, one of them with EMA), --mode ensemble --ensemble_dirs "A;B" decodes them together: translations in
    test_output, a BLEU line, and every variable of both members found in its checkpoint."""
    import json
    import subprocess
    rng = np.random.default_rng(3)
    words = ["w%d" % i for i in range(12)]
    (tmp_path / "vocab.txt").write_text("\n".join(words) + "\n")
    lines = [" ".join(rng.choice(words, size=int(rng.integers(2, 7)))) for _ in range(32)]
    for name in ("train.src", "train.tgt", "dev.src", "dev.tgt"):
        (tmp_path / name).write_text("\n".join(lines if name.startswith("train") else lines[:8]) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    common = ("num_heads=2,num_encoder_layer=1,num_decoder_layer=1,batch_or_token=batch,batch_size=16,eval_batch_size=8,"
              "max_training_steps=12,epoches=100,disp_freq=6,save_freq=6,eval_freq=12,warmup_steps=10,lrate=0.3,"
              "lrate_strategy=noam,beam_size=2,decode_length=4,process_num=1,shuffle_batch=False,dropout=0.0,relu_dropout=0.0,"
              "residual_dropout=0.0,attention_dropout=0.0,")
    files = ",".join("%s=%s" % (k, tmp_path / v) for k, v in dict(
        src_vocab_file="vocab.txt", tgt_vocab_file="vocab.txt", src_train_file="train.src", tgt_train_file="train.tgt",
        src_dev_file="dev.src", tgt_dev_file="dev.tgt", src_test_file="dev.src", tgt_test_file="dev.tgt").items())
    base = [sys.executable, "-m", "zero_amd.run"]
    dirs = {"a": "model_name=transformer,hidden_size=32,embed_size=32,filter_size=64,ema_decay=-1.0",
            "b": "model_name=transformer_aan,hidden_size=64,embed_size=64,filter_size=96,ema_decay=0.9"}
    for d, own in dirs.items():
        r = subprocess.run(base + ["--mode", "train", "--parameters", common + own + "," + files + ",output_dir=%s" % (tmp_path / d)],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert (tmp_path / d / "checkpoint").exists()
    out = tmp_path / "ens.trans.txt"
    r = subprocess.run(base + ["--mode", "ensemble", "--ensemble_dirs", "%s;%s" % (tmp_path / "a", tmp_path / "b"),
                               "--parameters", "test_output=%s" % out], env=env, capture_output=True, text=True, timeout=300)
    print("--mode ensemble stdout:\n" + r.stdout[-600:])
    print("--mode ensemble log tail:\n" + "\n".join(r.stderr.splitlines()[-6:]))
    assert r.returncode == 0, r.stderr[-2000:]
    bleu = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["bleu"]
    assert 0.0 <= bleu <= 1.0
    trans = out.read_text().splitlines()
    assert len(trans) == 8
    assert "member 0 (transformer," in r.stderr and "member 1 (transformer_aan," in r.stderr and "--Bad--" not in r.stderr
