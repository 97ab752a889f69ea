"""End-to-end GPU parity of the HIP hot path against the CPU oracle (oracle/ref_torch.py,
fp32).  PARITY NOTE: the oracle is a restatement of the TF1 reference (TF1 cannot run
here); tolerances below are for bf16 MFMA compute with fp32 accumulation:
   loss:      |hip - oracle| / |oracle| < 1e-3   (north-star tolerance)
   gradients: relative L2 error per variable < 1.2e-1 and cosine > 0.99 (bf16 activations:
              ~0.4% rounding per stored tensor, random-walking through ~30 ops each way)
   decode:    token ids of beam_size=1 / 4 equal to the oracle's, cache mode == dev mode
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_torch as rt  # noqa: E402
from tests.common import make_hp, make_batch, perturb  # noqa: E402
from zero_amd.models._factory import get_core, reset_cores  # noqa: E402
from zero_amd.models import model as registry, load_all  # noqa: E402

load_all()
MODELS = ["transformer", "transformer_aan", "transformer_rpr", "transformer_fuse"]
# per-variable gradient error against the oracle under the bf16 storage model (element-wise relative L2 / norm)
# (toy sizes are noisier than the BASELINE sizes of tests/test_gpu_fullsize.py, where every norm is within 1 %:
# measured here <= 7.7e-2 element-wise, <= 3.4e-2 on the norms)
BF16_MODEL_TOL, BF16_MODEL_NORM_TOL = 1e-1, 5e-2


def _setup(model, seed=0, **kw):
    reset_cores()
    rng = np.random.default_rng(seed)
    hp = make_hp(model, **kw)
    Pn = perturb(rt.init_params(hp, model, seed=seed + 1), rng)
    src, tgt = make_batch(rng, 5, 9, 11, hp.src_vocab.size(), hp.tgt_vocab.size())
    return hp, Pn, src, tgt


def _oracle(hp, Pn, src, tgt, model, store_bf16=False):
    """store_bf16: the oracle under the bf16 STORAGE model of the HIP path (oracle/ref_torch.py Cfg.store_bf16:
    same arithmetic in fp32, tensors the HIP path keeps as bf16 rounded at the same points)."""
    P = rt.to_torch(Pn, torch.float32, requires_grad=True)
    rt.Cfg.store_bf16 = store_bf16
    try:
        out = rt.train_fn({"source": torch.tensor(src), "target": torch.tensor(tgt)}, hp, P, model, training=False)
        out["loss"].backward()
    finally:
        rt.Cfg.store_bf16 = False
    G = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in P.items()}
    return float(out["loss"]), out["per_sample_loss"].detach().numpy(), G


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("cfg", ["mfma", "tiny"])
def test_train_loss_and_gradients(model, cfg):
    kw = {} if cfg == "mfma" else dict(H=16, F=32, heads=2, Vs=13, Vt=11)
    hp, Pn, src, tgt = _setup(model, **kw)
    ref_loss, ref_ps, ref_G = _oracle(hp, Pn, src, tgt, model)
    g = registry.get_model(model)
    out = g.train_fn({"source": src, "target": tgt}, hp, initializer=Pn)
    torch.cuda.synchronize()
    loss = float(out["loss"].cpu())
    ps = out["per_sample_loss"].cpu().numpy()
    rel = abs(loss - ref_loss) / abs(ref_loss)
    print("%s/%s loss hip=%.6f oracle=%.6f rel=%.2e" % (model, cfg, loss, ref_loss, rel))
    assert rel < 1e-3 * (1 if cfg == "mfma" else 3), (loss, ref_loss)
    assert np.abs(ps - ref_ps).max() / np.abs(ref_ps).max() < 5e-3
    G = out["store"].export("grad")
    worst = ("", 0.0)
    gmax = max(np.linalg.norm(v) for v in ref_G.values())
    for k, ref in ref_G.items():
        denom = np.linalg.norm(ref)
        if denom < 1e-3 * gmax:
            # analytically (near-)zero gradients, e.g. key biases under softmax shift invariance
            assert np.linalg.norm(G[k]) < 2e-3 * gmax, k
            continue
        err = np.linalg.norm(G[k] - ref) / denom
        cos = float((G[k] * ref).sum() / (np.linalg.norm(G[k]) * denom))
        if err > worst[1]:
            worst = (k, err)
        assert err < 1.2e-1 and cos > 0.99, (k, err, cos)
    print("   worst gradient rel.err: %s %.3e" % worst)
    if cfg == "mfma":
        # against the oracle under the bf16 storage model the element-wise error must be much smaller
        _, _, ref_B = _oracle(hp, Pn, src, tgt, model, store_bf16=True)
        worst_b, worst_n = ("", 0.0), ("", 0.0)
        for k, ref in ref_B.items():
            denom = np.linalg.norm(ref)
            if denom < 1e-3 * gmax:
                continue
            err = np.linalg.norm(G[k] - ref) / denom
            nerr = abs(np.linalg.norm(G[k]) - denom) / denom
            worst_b = max(worst_b, (k, err), key=lambda x: x[1])
            worst_n = max(worst_n, (k, nerr), key=lambda x: x[1])
        print("   vs bf16-storage oracle: worst rel.err %s %.3e; worst norm err %s %.3e" % (worst_b + worst_n))
        assert worst_b[1] < BF16_MODEL_TOL and worst_n[1] < BF16_MODEL_NORM_TOL, (worst_b, worst_n)


@pytest.mark.parametrize("model", MODELS)
def test_naive_and_mfma_paths_agree(model, monkeypatch):
    """The reference HIP kernels and the MFMA kernels must give the same step."""
    hp, Pn, src, tgt = _setup(model)
    res = {}
    for mode in ("naive", "mfma_auto"):
        reset_cores()
        core = get_core(hp, model, Pn)
        core.eng.gemm_impl = 1 if mode == "naive" else 0
        core.eng.attn_impl = 1 if mode == "naive" else 0
        batch = core.upload(src, tgt)
        loss, ps, _ = core.forward(batch, train=True, save=True)
        core.backward()
        torch.cuda.synchronize()
        res[mode] = (float(loss.cpu()), core.store.export("grad"))
    assert abs(res["naive"][0] - res["mfma_auto"][0]) / abs(res["naive"][0]) < 2e-3
    gmax = max(np.linalg.norm(v) for v in res["naive"][1].values())
    for k in res["naive"][1]:
        a, b = res["naive"][1][k], res["mfma_auto"][1][k]
        if np.linalg.norm(a) > 1e-3 * gmax:
            assert np.linalg.norm(a - b) / np.linalg.norm(a) < 1e-1, k


def test_big_layer_shapes_and_long_sequences():
    # Transformer-big widths (H=1024, F=4096, 16 heads of 64: BASELINE config 3) and sequences that
    # need 2-3 attention key tiles; 2 layers keep the CPU oracle fast
    reset_cores()
    rng = np.random.default_rng(9)
    hp = make_hp("transformer", H=1024, F=4096, heads=16, layers=2, Vs=500, Vt=400)
    Pn = perturb(rt.init_params(hp, "transformer", seed=2), rng)
    src, tgt = make_batch(rng, 3, 150, 90, 500, 400)
    ref_loss, ref_ps, ref_G = _oracle(hp, Pn, src, tgt, "transformer")
    out = registry.get_model("transformer").train_fn({"source": src, "target": tgt}, hp, initializer=Pn)
    torch.cuda.synchronize()
    loss = float(out["loss"].cpu())
    print("big-width loss hip=%.6f oracle=%.6f" % (loss, ref_loss))
    assert abs(loss - ref_loss) / abs(ref_loss) < 1e-3
    G = out["store"].export("grad")
    for k in ("encoder/layer_0/self_attention/dot_attention/qkv_map/W_0_0",
              "decoder/layer_1/cross_attention/dot_attention/k_map/W_0_0", "tgt_embedding"):
        err = np.linalg.norm(G[k] - ref_G[k]) / np.linalg.norm(ref_G[k])
        assert err < 1.2e-1, (k, err)


def test_score_fn_matches_oracle():
    hp, Pn, src, tgt = _setup("transformer")
    P = rt.to_torch(Pn)
    ref = rt.score_fn({"source": torch.tensor(src), "target": torch.tensor(tgt)}, hp, P, "transformer")["score"]
    got = registry.get_model("transformer").score_fn({"source": src, "target": tgt}, hp, initializer=Pn)["score"]
    torch.cuda.synchronize()
    assert np.abs(got.cpu().numpy() - ref.numpy()).max() / np.abs(ref.numpy()).max() < 5e-3


def test_dropout_training_step_runs_and_is_reproducible():
    hp, Pn, src, tgt = _setup("transformer", dropout=0.1, relu_dropout=0.1, residual_dropout=0.1,
                              attention_dropout=0.1)
    vals = []
    for _ in range(2):
        reset_cores()
        core = get_core(hp, "transformer", Pn)
        core.eng.set_seed(42)
        batch = core.upload(src, tgt)
        loss, _, _ = core.forward(batch, train=True, save=True)
        core.backward()
        torch.cuda.synchronize()
        vals.append((float(loss.cpu()), core.store.export("grad")["encoder/layer_0/feed_forward/ffn_layer/enlarge/W_0_0"]))
    assert vals[0][0] == vals[1][0] and np.array_equal(vals[0][1], vals[1][1])
    assert np.isfinite(vals[0][0])


def test_adam_update_matches_oracle_given_same_gradients():
    from zero_amd.main import Trainer
    hp, Pn, src, tgt = _setup("transformer", clip_grad_norm=0.5)
    reset_cores()
    tr = Trainer(hp, initializer=Pn)
    tr.micro_step({"source": src, "target": tgt})
    torch.cuda.synchronize()
    G = tr.store.export("grad")
    gnorm, pnorm, skipped = tr.train_op.stats()
    P = rt.to_torch(Pn)
    M = {k: torch.zeros_like(v) for k, v in P.items()}
    V = {k: torch.zeros_like(v) for k, v in P.items()}
    Gt = {k: torch.tensor(G[k]) for k in P}
    ref_gn, ref_pn = rt.adam_step(P, Gt, M, V, 1, rt.noam_lr(0, hp), hp)
    assert not skipped and abs(gnorm - ref_gn) / ref_gn < 1e-4 and abs(pnorm - ref_pn) / ref_pn < 1e-4
    new = tr.store.export("master")
    for k in P:
        assert np.abs(new[k] - P[k].numpy()).max() < 1e-6, k


def test_norm_free_update_equals_norm_first_update_and_counts_bad_steps():
    """zk_adam_step: with clip_grad_norm = 0.0 and no safe_nan (cycle.py:98-101) the gradient norm is accumulated
    inside the Adam pass (norm_free = 1); weights, m, v, shadow, gnorm and pnorm must equal the two-pass form
    (zk_l2norm + zk_adam) bit for bit / to fp32 summation order, the seed must advance by one, and a non-finite
    gradient must show in the per-update flag AND in the sticky counter that a later good update does not clear."""
    from zero_amd.main import Trainer, tower_train_graph
    hp, Pn, src, tgt = _setup("transformer")
    reset_cores()
    tr = Trainer(hp, initializer=Pn)
    assert tr.train_op.can_update_by_range()
    tr.lr.step(0)
    tower_train_graph({"source": src, "target": tgt}, tr.graph, hp, None)
    torch.cuda.synchronize()
    st, top, eng = tr.store, tr.train_op, tr.core.eng
    snap = {k: getattr(st, k).clone() for k in ("master", "grad", "m", "v", "shadow")}
    seed0 = int(eng.seed.cpu()[0])
    scale = top.set_hyper(tr.lr.get_lr(), 1)
    top.launch_update(scale)                      # norm-free single pass
    torch.cuda.synchronize()
    one = {k: getattr(st, k).clone() for k in ("master", "m", "v", "shadow")}
    g1, p1, bad1 = top.stats()
    assert int(eng.seed.cpu()[0]) == seed0 + 1 and not bad1 and top.bad_updates() == 0
    for k, v in snap.items():
        getattr(st, k).copy_(v)
    lib, s = eng.lib, eng.stream
    lib.call("zk_l2norm", st.grad.data_ptr(), st.numel, scale, top.hyper.data_ptr() + 24, top._ws.data_ptr(),
             top._ws.numel(), s)
    lib.call("zk_adam", st.master.data_ptr(), st.grad.data_ptr(), st.m.data_ptr(), st.v.data_ptr(),
             st.shadow.data_ptr(), st.numel, top.hyper.data_ptr(), top.pnorm.data_ptr(), top._ws.data_ptr(),
             top._ws.numel(), s)
    torch.cuda.synchronize()
    g2, p2, bad2 = top.stats()
    for k in one:
        assert torch.equal(one[k], getattr(st, k)), k
    assert abs(g1 - g2) <= 2e-6 * g2 and abs(p1 - p2) <= 2e-6 * p2 and not bad2
    # a NaN gradient: reported for that update and remembered afterwards
    st.grad[5] = float("nan")
    top.launch_update(scale)
    torch.cuda.synchronize()
    assert top.stats()[2] and top.bad_updates() == 1
    for k, v in snap.items():
        getattr(st, k).copy_(v)
    top.launch_update(scale)
    torch.cuda.synchronize()
    assert not top.stats()[2] and top.bad_updates() == 1


def test_hipgraph_replay_equals_eager_steps():
    # the captured step (forward + backward + norm + Adam in one hipGraph) must reproduce the eager
    # launch sequence exactly, update after update
    from zero_amd.main import Trainer
    hp, Pn, src, tgt = _setup("transformer")
    runs = {}
    for mode in ("eager", "graph"):
        reset_cores()
        tr = Trainer(hp, initializer=Pn)
        tr.prepare_static({"source": src, "target": tgt})
        losses = []
        for _ in range(5):
            losses.append(float(tr.step_static(use_graph=(mode == "graph")).cpu()[0]))
        torch.cuda.synchronize()
        runs[mode] = (losses, tr.store.export("master")["decoder/layer_0/feed_forward/ffn_layer/output/W_0_0"],
                      tr.train_op.stats())
    assert runs["eager"][0] == runs["graph"][0], (runs["eager"][0], runs["graph"][0])
    assert np.array_equal(runs["eager"][1], runs["graph"][1])
    assert runs["eager"][0][-1] < runs["eager"][0][0]          # the loss goes down on a repeated batch
    assert abs(runs["eager"][2][0] - runs["graph"][2][0]) < 1e-6 * runs["eager"][2][0]


def test_segmented_graph_step_equals_eager(monkeypatch):
    # the data-parallel step replays hipGraph SEGMENTS cut at every gradient-bucket hand-off
    # (Trainer._step_segmented); with one rank the hand-offs are no-ops and the result must equal
    # the eager launch sequence bit for bit
    from zero_amd.main import Trainer
    hp, Pn, src, tgt = _setup("transformer_aan")
    runs = {}
    for mode in ("eager", "segmented"):
        monkeypatch.setenv("ZERO_HIP_FORCE_SEGMENTED", "1" if mode == "segmented" else "0")
        monkeypatch.setenv("ZERO_HIP_GROUP_LAYERS", "1")          # many hand-offs
        reset_cores()
        tr = Trainer(hp, initializer=Pn)
        tr.prepare_static({"source": src, "target": tgt})
        losses = [float(tr.step_static(use_graph=(mode == "segmented")).cpu()[0]) for _ in range(4)]
        torch.cuda.synchronize()
        runs[mode] = (losses, tr.store.export("master")["encoder/layer_0/feed_forward/ffn_layer/enlarge/W_0_0"])
        if mode == "segmented":
            plan = [v for k, v in tr._graphs.items() if k[0] == "seg"][0]
            kinds = [k for k, _ in plan]
            assert kinds.count("ready") >= 4 and kinds[-1] == "update" and kinds[0] == "graph"
    assert runs["eager"][0] == runs["segmented"][0]
    assert np.array_equal(runs["eager"][1], runs["segmented"][1])


def test_update_cycle_accumulates_like_cycle_py():
    from zero_amd.main import Trainer
    hp, Pn, src, tgt = _setup("transformer", update_cycle=2)
    rng = np.random.default_rng(5)
    src2, tgt2 = make_batch(rng, 5, 9, 11, hp.src_vocab.size(), hp.tgt_vocab.size())
    reset_cores()
    tr = Trainer(hp, initializer=Pn)
    tr.micro_step({"source": src, "target": tgt})
    g1 = tr.store.export("grad")
    tr.micro_step({"source": src2, "target": tgt2})
    torch.cuda.synchronize()
    gsum = tr.store.export("grad")     # after apply(): grad buffer holds g1 + g2
    hp1 = copy.copy(hp); hp1.update_cycle = 1
    reset_cores()
    core = get_core(hp1, "transformer", Pn)
    b = core.upload(src2, tgt2)
    core.forward(b, train=True, save=True); core.backward()
    torch.cuda.synchronize()
    g2 = core.store.export("grad")
    k = "decoder/layer_1/feed_forward/ffn_layer/output/W_0_0"
    assert np.abs(gsum[k] - (g1[k] + g2[k])).max() < 1e-6
    assert tr.global_step == 1 and tr.store.step == 1


# ------------------------------------------------------------------ decode
def _decode_both(model, K, hp, Pn, src):
    hp = copy.copy(hp)
    hp.beam_size = K
    P = rt.to_torch(Pn)
    hp.search_mode = "cache"
    enc, dec = rt.infer_fn(hp, P, model)
    ref = rt.beam_search({"source": torch.tensor(src)}, enc, dec, hp)
    from zero_amd.main import tower_infer_graph
    outs = {}
    for mode in ("cache", "dev"):
        hp.search_mode = mode
        reset_cores()
        get_core(hp, model, Pn)
        seqs, scores = tower_infer_graph({"source": src}, registry.get_model(model), hp)
        outs[mode] = (seqs, scores)
    return ref, outs


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("K", [1, 4])
def test_beam_search_token_ids(model, K):
    hp, Pn, src, tgt = _setup(model, seed=3)
    # sharpen the output distribution so that bf16 noise cannot flip near-ties of a random model
    Pn["tgt_embedding"] = (Pn["tgt_embedding"] * 6.0).astype(np.float32)
    ref, outs = _decode_both(model, K, hp, Pn, src)
    hyp_ref = rt.decode_hypothesis(ref["seq"], hp)
    from zero_amd.search import decode_hypothesis
    for mode in ("cache", "dev"):
        seqs, scores = outs[mode]
        hyp = decode_hypothesis(seqs, hp)
        same = sum(int(a == b) for a, b in zip(hyp, hyp_ref))
        print("%s K=%d %s: %d/%d sentences token-exact; top score diff %.3e" %
              (model, K, mode, same, len(hyp), np.abs(scores[:, 0] - ref["score"][:, 0]).max()))
        assert same == len(hyp), (hyp, hyp_ref)
    if model == "transformer_rpr":
        # cache mode scores single queries with the reference kernels (fp32 table arithmetic), dev mode
        # runs the decomposed MFMA form (bf16 bucket sums): the best hypothesis agrees, lower-ranked beams
        # of this random model sit on near-ties
        L = min(outs["cache"][0].shape[2], outs["dev"][0].shape[2])
        assert np.array_equal(outs["cache"][0][:, 0, :L], outs["dev"][0][:, 0, :L])
    else:
        assert np.array_equal(outs["cache"][0], outs["dev"][0])


@pytest.mark.parametrize("model", ["transformer_aan", "transformer"])
def test_batches_in_flight_on_lanes_equal_the_sequential_loop(model):
    """evalu.decode_many: several decode batches in flight at once, each on its own execution lane (own engine, HIP
    stream, caches, captured graphs; shared variable store), must return exactly what the one-after-the-other loop of
    evalu.py:49-139 returns -- hypotheses, scores, step counts, in the order of the input."""
    from zero_amd.evalu import decode_many
    from zero_amd.search import beam_search
    import threading
    hp, Pn, src, tgt = _setup(model, seed=11, beam_size=4)
    Pn["tgt_embedding"] = (Pn["tgt_embedding"] * 6.0).astype(np.float32)
    hp = copy.copy(hp); hp.search_mode = "cache"
    get_core(hp, model, Pn)
    rng = np.random.default_rng(5)
    batches = []
    for i in range(7):                       # different batch sizes and lengths: every lane re-sizes and re-captures
        s_, _ = make_batch(rng, 3 + (i % 3), 6 + i, 5, hp.src_vocab.size(), hp.tgt_vocab.size())
        batches.append(s_)
    graph = registry.get_model(model)
    tl = threading.local()

    def work(s_):
        if not hasattr(tl, "fns"):
            tl.fns = graph.infer_fn(hp)
        out = beam_search({"source": s_}, tl.fns[0], tl.fns[1], hp)
        return np.asarray(out["seq"]).copy(), np.asarray(out["score"]).copy(), out["steps"]
    seq = decode_many(batches, work, streams=1)
    for n in (2, 3):
        par = decode_many(batches, work, streams=n)
        assert len(par) == len(seq)
        for (a, b, c), (x, y, z) in zip(seq, par):
            assert np.array_equal(a, x) and np.array_equal(b, y) and c == z, n
    # an exception in a lane reaches the caller
    def boom(s_):
        raise ValueError("lane failure")
    with pytest.raises(ValueError):
        decode_many(batches, boom, streams=2)


@pytest.mark.parametrize("model", ["transformer_aan", "transformer"])
def test_step_graphs_are_reused_across_batches_of_one_shape(model, monkeypatch):
    """The two parity graphs of a decode batch are kept per (beam rows, padded source length, cache length) and replayed
    by later batches of that shape; source length and cache length are bucketed to multiples of 8 (masked keys add
    exact zeros).  Same hypotheses, scores and step counts as with a fresh capture per batch on unpadded shapes."""
    from zero_amd.search import beam_search
    hp, Pn, src, tgt = _setup(model, seed=13, beam_size=4)
    Pn["tgt_embedding"] = (Pn["tgt_embedding"] * 6.0).astype(np.float32)
    hp = copy.copy(hp); hp.search_mode = "cache"
    rng = np.random.default_rng(9)
    batches = []
    for ls in (6, 7, 13, 6, 9, 7, 13):        # 6 / 7 and 9 / 13 share a bucket; repeats must hit the cache
        s_, _ = make_batch(rng, 4, ls, 5, hp.src_vocab.size(), hp.tgt_vocab.size())
        batches.append(s_)
    outs = {}
    for name, env in (("fresh", {"ZERO_HIP_DECODE_GRAPH_CACHE": "0", "ZERO_HIP_DECODE_PAD_LEN": "1"}), ("cached", {})):
        for k in ("ZERO_HIP_DECODE_GRAPH_CACHE", "ZERO_HIP_DECODE_PAD_LEN"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        reset_cores()
        core = get_core(hp, model, Pn)
        enc, dec = registry.get_model(model).infer_fn(hp)
        res = []
        for s_ in batches:
            o = beam_search({"source": s_}, enc, dec, hp)
            res.append((np.asarray(o["seq"]).copy(), np.asarray(o["score"]).copy(), o["steps"]))
        outs[name] = (res, core.__dict__.get("_graph_adoptions", 0), len(core.__dict__.get("_step_graph_cache", {})))
    assert outs["fresh"][1] == 0 and outs["cached"][1] >= 3, (outs["fresh"][1:], outs["cached"][1:])
    assert 1 <= outs["cached"][2] <= 3
    for (a, b, c), (x, y, z) in zip(outs["fresh"][0], outs["cached"][0]):
        L = min(a.shape[-1], x.shape[-1])
        assert np.array_equal(a[..., :L], x[..., :L]) and np.array_equal(b, y) and c == z


@pytest.mark.parametrize("model", ["transformer", "transformer_aan", "transformer_rpr"])
def test_output_projection_dgrad_inside_the_attention_backward(model, monkeypatch):
    """ZERO_HIP_ATTN_OPROJ=1 / 0: the o_map dgrad as the prologue of the attention backward launch or as a GEMM launch of
    its own -- same loss (the forward is untouched), gradients equal up to the fp32 summation order inside the
    64 x 64 x H product (bf16 flips of single dO elements), fewer entry-point calls."""
    hp, Pn, src, tgt = _setup(model, seed=21)
    g = registry.get_model(model)
    res = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("ZERO_HIP_ATTN_OPROJ", flag)
        reset_cores()
        core = get_core(hp, model, Pn)
        n0 = core.eng.lib.ncalls
        out = g.train_fn({"source": src, "target": tgt}, hp, initializer=Pn)
        torch.cuda.synchronize()
        res[flag] = (float(out["loss"].cpu()), out["store"].export("grad"), core.eng.lib.ncalls - n0)
    assert res["0"][0] == res["1"][0]
    n_att = hp.num_encoder_layer + (1 if model == "transformer_aan" else 2) * hp.num_decoder_layer
    assert res["0"][2] - res["1"][2] == n_att, (res["0"][2], res["1"][2])
    gmax = max(np.linalg.norm(v) for v in res["0"][1].values())
    for k, ref in res["0"][1].items():
        err = np.linalg.norm(res["1"][1][k] - ref) / max(np.linalg.norm(ref), 1e-3 * gmax)
        assert err < 5e-3, (k, err)


def test_transposed_decode_weights_follow_the_weight_version():
    """The transposed weight copies of the fused decode kernels are made by zk_transpose_bf16 once per weight version:
    reused across batches, refreshed after an optimiser update."""
    from zero_amd.models import _decode
    from zero_amd.main import Trainer
    model = "transformer_aan"
    hp, Pn, src, tgt = _setup(model, seed=2)
    core = get_core(hp, model, Pn)
    name = "decoder/layer_0/%s/dot_attention/q_map/W_0_0" % core.cross
    m1 = _decode._transposed(core, name)
    torch.cuda.synchronize()
    W = core.store.s(name)
    assert torch.equal(m1.t, W.t().contiguous())
    calls = core.eng.lib.ncalls
    assert _decode._transposed(core, name) is m1 and core.eng.lib.ncalls == calls       # same version: no launch
    tr = Trainer(hp)
    assert tr.core is core
    tr.micro_step({"source": src, "target": tgt})
    torch.cuda.synchronize()
    m2 = _decode._transposed(core, name)
    torch.cuda.synchronize()
    assert core.eng.lib.ncalls > calls and torch.equal(m2.t, core.store.s(name).t().contiguous())


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("K", [1, 4, 8])
def test_device_resident_search_equals_host_bookkeeping(model, K, monkeypatch):
    """search.py:85-113,168-228 on the device (zk_beam_dev_prepare / zk_beam_dev_advance inside the step graph,
    stop flag polled every few replays) against the host-C bookkeeping and the numpy statements: all K
    hypotheses, their scores and the step count, bit for bit, whatever the polling interval (replays past the
    stop must not change the frozen state)."""
    from zero_amd.main import tower_infer_graph
    from zero_amd import search
    hp, Pn, src, tgt = _setup(model, seed=5, beam_size=K)
    Pn["tgt_embedding"] = (Pn["tgt_embedding"] * 6.0).astype(np.float32)
    hp = copy.copy(hp); hp.beam_size = K; hp.search_mode = "cache"
    outs = {}
    for name, env in (("numpy", {"ZERO_HIP_DECODE_HOST_C": "0"}),
                      ("host_c", {"ZERO_HIP_DECODE_DEVICE_BOOK": "0"}),
                      ("dev_default", {}), ("dev4", {"ZERO_HIP_DECODE_POLL": "4"}), ("dev7", {"ZERO_HIP_DECODE_POLL": "7"})):
        for k in ("ZERO_HIP_DECODE_HOST_C", "ZERO_HIP_DECODE_DEVICE_BOOK", "ZERO_HIP_DECODE_POLL"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        reset_cores()
        get_core(hp, model, Pn)
        enc, dec = registry.get_model(model).infer_fn(hp)
        outs[name] = search.beam_search({"source": src}, enc, dec, hp)
    ref = outs["host_c"]
    assert ref["steps"] > 2
    for name in ("numpy", "dev_default", "dev4", "dev7"):
        o = outs[name]
        assert o["steps"] == ref["steps"], (name, o["steps"], ref["steps"])
        assert np.array_equal(o["seq"], ref["seq"]), name
        assert np.array_equal(o["score"], ref["score"]), name


@pytest.mark.parametrize("model", ["transformer", "transformer_aan"])
def test_decode_graphs_across_batches_of_changing_shape(model):
    """After the first batch the step graphs are captured without an eager pass (the scratch exists); batches
    that grow a buffer fall back to the eager pass.  A sequence of batches on ONE engine must give exactly
    what each batch gives on a fresh engine."""
    from zero_amd import search
    hp, Pn, _, _ = _setup(model, seed=7, beam_size=4)
    Pn["tgt_embedding"] = (Pn["tgt_embedding"] * 6.0).astype(np.float32)
    hp = copy.copy(hp); hp.beam_size = 4; hp.search_mode = "cache"
    rng = np.random.default_rng(11)
    shapes = [(4, 7), (4, 9), (4, 5), (6, 12), (3, 12), (4, 30), (4, 7)]
    batches = [make_batch(rng, b, l, 3, hp.src_vocab.size(), hp.tgt_vocab.size())[0] for b, l in shapes]

    def run(src):
        enc, dec = registry.get_model(model).infer_fn(hp)
        return search.beam_search({"source": src}, enc, dec, hp)
    fresh = []
    for src in batches:
        reset_cores(); get_core(hp, model, Pn)
        fresh.append(run(src))
    reset_cores(); core = get_core(hp, model, Pn)
    for i, src in enumerate(batches):
        o = run(src)
        assert o["steps"] == fresh[i]["steps"], i
        assert np.array_equal(o["seq"], fresh[i]["seq"]) and np.array_equal(o["score"], fresh[i]["score"]), i
    assert core.__dict__.get("_decode_warm_rows", 0) >= 16


def test_aan_use_ffn_variant():
    """transformer_aan.py:176-183: an FFN between the cumulative average and the gate (use_ffn=True,
    off by default in run.py:119): loss / gradients of the extra ffn_layer variables, beam ids."""
    model = "transformer_aan"
    hp, Pn, src, tgt = _setup(model, seed=2, use_ffn=True, aan_mask=True)
    assert "decoder/layer_0/average_attention/ffn_layer/enlarge/W_0_0" in Pn
    ref_loss, ref_ps, ref_G = _oracle(hp, Pn, src, tgt, model)
    out = registry.get_model(model).train_fn({"source": src, "target": tgt}, hp, initializer=Pn)
    torch.cuda.synchronize()
    assert abs(float(out["loss"].cpu()) - ref_loss) / abs(ref_loss) < 1e-3
    G = out["store"].export("grad")
    gmax = max(np.linalg.norm(v) for v in ref_G.values())
    for k, ref in ref_G.items():
        if np.linalg.norm(ref) < 1e-3 * gmax:
            continue
        err = np.linalg.norm(G[k] - ref) / np.linalg.norm(ref)
        assert err < 1.2e-1, (k, err)
    Pn["tgt_embedding"] = (Pn["tgt_embedding"] * 6.0).astype(np.float32)
    ref, outs = _decode_both(model, 4, hp, Pn, src)
    from zero_amd.search import decode_hypothesis
    assert decode_hypothesis(outs["cache"][0], hp) == rt.decode_hypothesis(ref["seq"], hp)


# ------------------------------------------------------------------ edge cases of the batch shape
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 1), (3, 1, 5), (2, 70, 3), (2, 5, 300), (2, 300, 40)])
def test_ragged_and_extreme_batch_shapes(shape):
    """Single sentence / single token / one side much longer than the other / sequences beyond the
    MFMA attention kernel's 256-key limit (reference kernels take over): loss and gradient norm
    against the oracle."""
    B, Ls, Lt = shape
    model = "transformer"
    reset_cores()
    rng = np.random.default_rng(B * 1000 + Ls * 10 + Lt)
    hp = make_hp(model)
    Pn = perturb(rt.init_params(hp, model, seed=4), rng)
    def rows(n, L, V):                      # lengths 1..L (a row may be just eos), row 0 full length
        ids = np.zeros((n, L), dtype=np.int64)
        for b in range(n):
            ln = L if b == 0 else int(rng.integers(1, L + 1))
            ids[b, :ln - 1] = rng.integers(3, V, ln - 1)
            ids[b, ln - 1] = 2
        return ids
    src, tgt = rows(B, Ls, hp.src_vocab.size()), rows(B, Lt, hp.tgt_vocab.size())
    ref_loss, ref_ps, ref_G = _oracle(hp, Pn, src, tgt, model)
    out = registry.get_model(model).train_fn({"source": src, "target": tgt}, hp, initializer=Pn)
    torch.cuda.synchronize()
    loss = float(out["loss"].cpu())
    # a loss made of ONE target token has no averaging over rows: the bf16 rounding of that single
    # feature row shows directly (|d loss| ~ 1e-2 absolute); batches of >= 15 tokens meet 2e-3
    tol = 5e-3 if B * Lt < 15 else 2e-3
    assert abs(loss - ref_loss) / abs(ref_loss) < tol, (shape, loss, ref_loss)
    G = out["store"].export("grad")
    gn = np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in G.values()))
    rn_ = np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in ref_G.values()))
    assert abs(gn - rn_) / rn_ < 5e-2, (shape, gn, rn_)


def test_empty_batch_and_all_pad_columns():
    """transformer.py:213-216: a batch of zero sentences gives loss 0; remove_invalid_seq
    (util.py:274-287) drops trailing all-pad columns before anything is computed."""
    model = "transformer"
    hp, Pn, src, tgt = _setup(model)
    g = registry.get_model(model)
    out = g.train_fn({"source": src[:0], "target": tgt[:0]}, hp, initializer=Pn)
    assert float(out["loss"].cpu()) == 0.0
    pad_s = np.concatenate([src, np.zeros((src.shape[0], 7), src.dtype)], 1)
    pad_t = np.concatenate([tgt, np.zeros((tgt.shape[0], 3), tgt.dtype)], 1)
    reset_cores()
    a = float(g.train_fn({"source": src, "target": tgt}, hp, initializer=Pn)["loss"].cpu())
    reset_cores()
    b = float(g.train_fn({"source": pad_s, "target": pad_t}, hp, initializer=Pn)["loss"].cpu())
    assert a == b


def test_sequence_longer_than_the_kernel_limit_fails_loudly():
    model = "transformer"
    reset_cores()
    hp = make_hp(model)
    rng = np.random.default_rng(0)
    src, tgt = make_batch(rng, 1, 600, 4, hp.src_vocab.size(), hp.tgt_vocab.size())
    from zero_amd.hip import ZeroHipError
    with pytest.raises(ZeroHipError):
        registry.get_model(model).train_fn({"source": src, "target": tgt}, hp)
        torch.cuda.synchronize()


@pytest.mark.parametrize("graph", ["1", "0"])
def test_noise_beam_search_runs_and_is_seeded(graph, monkeypatch):
    """search.py:143-145 (enable_noise_beam_search): Gumbel-perturbed logits give valid hypotheses,
    reproducible for a fixed seed and different from the noise-free search."""
    monkeypatch.setenv("ZERO_HIP_DECODE_GRAPH", graph)
    from zero_amd.main import tower_infer_graph
    model = "transformer_aan"
    hp, Pn, src, tgt = _setup(model, seed=3, beam_size=4)
    outs = []
    for noise, seed in ((False, 1), (True, 1), (True, 1), (True, 2)):
        hp2 = copy.copy(hp); hp2.enable_noise_beam_search = noise
        reset_cores()
        core = get_core(hp2, model, Pn)
        core.eng.set_seed(seed)
        seqs, scores = tower_infer_graph({"source": src}, registry.get_model(model), hp2)
        assert np.isfinite(scores).all() and seqs.shape[0] == src.shape[0]
        outs.append(seqs)
    assert np.array_equal(outs[1], outs[2])
    assert not np.array_equal(outs[0], outs[1]) or not np.array_equal(outs[1], outs[3])


def test_shape_keyed_graph_cache_matches_eager_and_survives_buffer_growth():
    """Real training feeds batches of varying shape: one captured graph per shape, all dropped when a
    larger shape makes the engine replace a buffer.  Must equal the eager sequence bit for bit."""
    from zero_amd.main import Trainer
    hp, Pn, _, _ = _setup("transformer")
    rng = np.random.default_rng(9)
    shapes = [(3, 5, 6), (4, 9, 7), (3, 5, 6), (6, 12, 11), (4, 9, 7), (3, 5, 6), (6, 12, 11), (4, 9, 7), (3, 5, 6),
              (6, 12, 11), (4, 9, 7), (3, 5, 6)]
    batches = {}
    for sh in set(shapes):
        batches[sh] = make_batch(rng, sh[0], sh[1], sh[2], hp.src_vocab.size(), hp.tgt_vocab.size())
    runs = {}
    for mode in (False, True):
        reset_cores()
        tr = Trainer(hp, initializer=Pn)
        losses = []
        for sh in shapes:
            src, tgt = batches[sh]
            tr.prepare_static({"source": src, "target": tgt})
            losses.append(float(tr.step_static(use_graph=mode).cpu()[0]))
        torch.cuda.synchronize()
        runs[mode] = (losses, tr.store.export("master")["decoder/layer_1/feed_forward/ffn_layer/enlarge/W_0_0"])
        if mode:
            captured = [k for k, g in tr._graphs.items() if not isinstance(g, str)]
            assert len(captured) >= 2, tr._graphs.keys()
    assert runs[False][0] == runs[True][0]
    assert np.array_equal(runs[False][1], runs[True][1])


def test_accumulation_steps_replayed_from_graphs_match_eager():
    """update_cycle=3 over batches of two shapes: Trainer.step (captured 'collect' / final graphs per
    shape) must equal the eager micro_step sequence bit for bit."""
    from zero_amd.main import Trainer
    hp, Pn, _, _ = _setup("transformer", update_cycle=3)
    rng = np.random.default_rng(4)
    shapes = [(3, 5, 6), (4, 9, 7)] * 9
    batches = {sh: make_batch(rng, sh[0], sh[1], sh[2], hp.src_vocab.size(), hp.tgt_vocab.size()) for sh in set(shapes)}
    runs = {}
    for mode in (False, True):
        reset_cores()
        tr = Trainer(hp, initializer=Pn)
        losses = []
        for sh in shapes:
            src, tgt = batches[sh]
            loss = tr.step({"source": src, "target": tgt}, use_graph=mode)
            losses.append(float(loss.reshape(-1)[0].cpu()))
        torch.cuda.synchronize()
        runs[mode] = (losses, tr.store.export("master")["encoder/layer_1/self_attention/dot_attention/o_map/W_0_0"],
                      tr.global_step)
    assert runs[True][2] == runs[False][2] == 6
    assert runs[False][0] == runs[True][0]
    assert np.array_equal(runs[False][1], runs[True][1])


def test_many_shapes_many_replays_match_eager():
    """Stress of the shape-keyed graph cache (scripts/soak_train.py in small): 10 shapes in random order
    for 160 steps, graphs replayed many times each -- loss and gradient norm must equal the eager run at
    every step.  (Found in round 1: hipGraph MEMSET nodes went wrong after a few replays once many graphs
    were alive; zk_zero is a kernel node since.)"""
    from zero_amd.main import Trainer
    hp, Pn, _, _ = _setup("transformer", H=128, F=256)
    rng = np.random.default_rng(12)
    shapes = [(int(rng.integers(2, 9)), int(rng.integers(3, 40)), int(rng.integers(3, 40))) for _ in range(10)]
    order = rng.integers(0, len(shapes), 160)
    data = {sh: make_batch(np.random.default_rng(hash(sh) % 1000), sh[0], sh[1], sh[2], hp.src_vocab.size(),
                           hp.tgt_vocab.size()) for sh in set(shapes)}
    traces = {}
    for mode in (False, True):
        reset_cores()
        tr = Trainer(hp, initializer=Pn)
        out = []
        for i in order:
            src, tgt = data[shapes[i]]
            loss = tr.step({"source": src, "target": tgt}, use_graph=mode)
            g, p, bad = tr.train_op.stats()
            out.append((float(loss.reshape(-1)[0].cpu()), g, bad))
        traces[mode] = out
    assert traces[False] == traces[True]
    assert not any(b for _, _, b in traces[True])


@pytest.mark.parametrize("slots,steps", [(16, 12), (16, 44), (2, 20), (3, 20)])
def test_steps_on_rotating_batches_without_host_syncs_match_eager(slots, steps, monkeypatch):
    """Trainer.step as the training loop calls it: a NEW batch every step, the host never waiting for the device (the
    next batch is uploaded and prepared -- zk_batch_prep -- on a side stream into a staging set while the previous step
    runs, then committed by the first node of the step's graph, whose arguments are rewritten per step).  Steps over 5
    different batches of two shapes, no synchronisation in between, against eager micro steps with a synchronisation after
    every step: same losses, same weights.  44 steps go round the 16 staging sets almost three times; 2 and 3 sets make
    the host wait for the pinned commit word on nearly every step."""
    from zero_amd.main import Trainer
    monkeypatch.setattr(Trainer, "STAGE_SLOTS", slots)
    hp, Pn, _, _ = _setup("transformer", H=128, F=256, lrate=0.5, warmup_steps=10)
    feats = []
    for i in range(5):
        src, tgt = make_batch(np.random.default_rng(100 + i), 6, 12 if i != 3 else 9, 14, hp.src_vocab.size(), hp.tgt_vocab.size())
        src[:, -1], tgt[:, -1] = 2, 2
        feats.append({"source": src, "target": tgt})
    runs = {}
    for mode in ("eager", "pipelined"):
        reset_cores()
        tr = Trainer(hp, initializer=Pn)
        held = []
        for i in range(steps):
            if mode == "eager":
                loss = tr.micro_step(feats[i % 5])
                torch.cuda.synchronize()
                held.append(loss.reshape(-1)[0].clone())
            else:
                loss = tr.step(feats[i % 5])
                held.append(loss.reshape(-1)[0].clone())          # (device-side copy, enqueued behind the step)
        torch.cuda.synchronize()
        runs[mode] = ([float(x.cpu()) for x in held], tr.store.master.cpu().numpy().copy())
    assert runs["eager"][0] == runs["pipelined"][0], (runs["eager"][0], runs["pipelined"][0])
    assert np.array_equal(runs["eager"][1], runs["pipelined"][1])
    assert len(set(runs["eager"][0])) > 5                          # the batches really differ


def test_length_bucketing_leaves_losses_and_updates_unchanged(monkeypatch):
    """ZERO_HIP_PAD_LEN=8 (Trainer.prepare_static: both sides padded to a multiple of 8 so that token-sized batches
    fall into few graph-cache shapes): padded keys are masked, padded target positions follow the real ones and carry
    no loss -- losses and the updated weights equal the unpadded run's up to the order of fp32 sums (dropout 0)."""
    from zero_amd.main import Trainer
    hp, Pn, _, _ = _setup("transformer")
    rng = np.random.default_rng(9)
    batches = [make_batch(rng, 4, ls, lt, hp.src_vocab.size(), hp.tgt_vocab.size()) for ls, lt in ((5, 7), (9, 3), (13, 10))]
    runs = {}
    for pad in ("1", "8"):
        monkeypatch.setenv("ZERO_HIP_PAD_LEN", pad)
        reset_cores()
        tr = Trainer(hp, initializer=Pn)
        losses = []
        for src, tgt in batches * 2:
            loss = tr.step({"source": src, "target": tgt})
            losses.append(float(loss.reshape(-1)[0].cpu()))
        torch.cuda.synchronize()
        if pad == "8":
            assert tr.batch["Ls"] % 8 == 0 and tr.batch["Lt"] % 8 == 0
        runs[pad] = (np.array(losses), tr.store.export("master"))
    assert np.abs(runs["1"][0] - runs["8"][0]).max() < 2e-4 * np.abs(runs["1"][0]).max()
    for k, w in runs["1"][1].items():
        d = np.abs(w - runs["8"][1][k]).max()
        assert d <= 2e-3 * max(np.abs(w).max(), 1e-6), (k, d)


@pytest.mark.parametrize("K", [1, 4])
def test_aan_decode_ln_fusions_are_bit_identical(K, monkeypatch):
    """zk_ln_decode (gate + residual + LayerNorm, and LayerNorm + the next layer's average-attention update, in one
    launch each) against the separate launches: identical hypotheses AND identical scores, replayed graph and eager."""
    from zero_amd import search
    hp, Pn, src, tgt = _setup("transformer_aan", seed=8, beam_size=K)
    hp = copy.copy(hp); hp.beam_size = K; hp.search_mode = "cache"
    outs = {}
    monkeypatch.setenv("ZERO_HIP_DECODE_FUSE_ATT", "0")        # the fused attention sub-layers are not bit-identical
    for fuse in ("0", "1"):
        monkeypatch.setenv("ZERO_HIP_DECODE_FUSE_LN", fuse)
        reset_cores()
        get_core(hp, "transformer_aan", Pn)
        enc, dec = registry.get_model("transformer_aan").infer_fn(hp)
        outs[fuse] = search.beam_search({"source": src}, enc, dec, hp)
    assert outs["0"]["steps"] == outs["1"]["steps"] > 2
    assert np.array_equal(outs["0"]["seq"], outs["1"]["seq"])
    assert np.array_equal(outs["0"]["score"], outs["1"]["score"])
