"""alignment_file / alignment_layer / replace_unk on the host (no GPU): option validation and every refusal text, the pair
helpers, evalu.aligning's batching, the option-off paths, and the kernel's refusals through hip.lib().call."""
import numpy as np
import pytest

from tests.common import make_hp
from zero_amd import align as zalign
from zero_amd import evalu, hip
from zero_amd.models import _align


def test_defaults_are_off():
    hp = make_hp("transformer")
    assert hp.alignment_file == "" and hp.alignment_layer == -1 and hp.replace_unk is False
    assert not zalign.wanted(hp) and zalign.check_opts(hp, "test") is False and zalign.check_opts(hp, "score") is False


def test_option_validation():
    hp = make_hp("transformer", replace_unk=True)
    with pytest.raises(ValueError, match="replace_unk needs alignment_file"):
        zalign.check_opts(hp)
    hp = make_hp("transformer", alignment_file="a.txt", top_beams=2)
    with pytest.raises(ValueError, match="top_beams=2"):
        zalign.check_opts(hp, "test")
    assert zalign.check_opts(hp, "score") is True
    for layer, ok in ((-3, False), (-2, True), (-1, True), (0, True), (1, True), (2, False)):
        hp = make_hp("transformer", alignment_file="a.txt", alignment_layer=layer)
        if ok:
            assert zalign.check_opts(hp) is True and _align.layer_index(hp) == layer % 2
        else:
            with pytest.raises(ValueError, match="alignment_layer=%d is out of range for 2 decoder layers" % layer):
                zalign.check_opts(hp)


@pytest.mark.parametrize("model,why", [("transformer_rpr", "relative-position"), ("transformer_rela", "ReLU"),
                                       ("transformer_l0drop", "compacted"), ("transformer_fixup", "LayerNorm-free"),
                                       ("rnnsearch", "recurrent"), ("rnnsearch_deepatt", "recurrent"), ("deepnmt", "recurrent")])
def test_refused_models_are_named(model, why):
    hp = make_hp(model, alignment_file="a.txt")
    with pytest.raises(NotImplementedError, match="alignment_file is not built for %s: .*%s" % (model, why)):
        zalign.check_opts(hp, "test")
    with pytest.raises(NotImplementedError, match="alignment_file.*" + model):
        zalign.align_fn({"source": np.array([[5, 2]]), "target": np.array([[6, 2]])}, hp, model)
    for m in zalign._align.BUILT:
        _align.check_model(m)


def test_ensemble_mode_is_refused_before_anything_is_read(tmp_path):
    from zero_amd import main as loops
    hp = make_hp("transformer", alignment_file="a.txt", output_dir=str(tmp_path / "nowhere"))
    with pytest.raises(NotImplementedError, match="alignment_file is not built for --mode ensemble"):
        loops.ensemble([hp, hp])


def test_evaluate_and_scorer_refuse_before_the_checkpoint(tmp_path, monkeypatch):
    from zero_amd import main as loops
    monkeypatch.setattr(loops, "_eval_trainer", lambda p: pytest.fail("the checkpoint was read"))
    (tmp_path / "t.src").write_text("a b\n")
    kw = dict(src_test_file=str(tmp_path / "t.src"), tgt_test_file=str(tmp_path / "t.src"))
    with pytest.raises(NotImplementedError, match="alignment_file.*transformer_rela"):
        loops.evaluate(make_hp("transformer_rela", alignment_file="a.txt", **kw))
    with pytest.raises(NotImplementedError, match="alignment_file.*transformer_rpr"):
        loops.scorer(make_hp("transformer_rpr", alignment_file="a.txt", **kw))
    with pytest.raises(ValueError, match="replace_unk needs alignment_file"):
        loops.evaluate(make_hp("transformer", replace_unk=True, **kw))
    with pytest.raises(ValueError, match="top_beams"):
        loops.evaluate(make_hp("transformer", alignment_file="a.txt", top_beams=3, **kw))


def test_hard_pairs_and_format():
    # 4 source words (+ EOS at position 4), 3 hypothesis words (+ its EOS row, + padding rows)
    best = np.array([2, -1, 0, 3, 1, 1])
    pairs = zalign.hard_pairs(best, 4, 3)
    assert pairs == [(2, 0), (0, 2)]                          # the -1 row is skipped, the EOS row (3) and the padding dropped
    assert zalign.format_pairs(pairs) == "2-0 0-2"
    assert zalign.hard_pairs(best, 4, 0) == [] and zalign.format_pairs([]) == ""      # an empty hypothesis: an empty line
    assert zalign.hard_pairs(np.array([4, 5]), 4, 2) == []    # a position behind the source's words is never written
    assert zalign.hard_pairs(np.array([1.0, 3.0]), 4, 2) == [(1, 0), (3, 1)]


def test_eligible_mask_clears_the_source_eos():
    src = np.array([[5, 6, 7, 2, 0], [9, 2, 0, 0, 0], [4, 4, 4, 4, 4], [0, 0, 0, 0, 0]])
    am = _align.eligible_mask(src, 2)
    assert am.tolist() == [[1, 1, 1, 0, 0], [1, 0, 0, 0, 0], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0]]


def test_replace_unk_tokens():
    raw = "Herr Müller wohnt in Zürich".split()
    hyp = ["mr", "<unk>", "lives", "in", "<unk>", "<unk>", "<unk>"]
    pairs = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (7, 5)]      # token 5 points behind the raw tokens, token 6 has no pair
    assert zalign.replace_unk_tokens(hyp, pairs, raw, "<unk>") == ["mr", "Müller", "lives", "in", "Zürich", "<unk>", "<unk>"]
    assert zalign.replace_unk_tokens(["a", "b"], [(0, 0), (1, 1)], raw, "<unk>") == ["a", "b"]     # only UNK tokens change
    assert zalign.replace_unk_tokens([], [], raw, "<unk>") == []
    assert hyp[1] == "<unk>"                                      # the input is not modified


def test_aligning_keeps_file_order_across_batches():
    """A fake align function that answers with the first source id of every row: the answers come back in file order, batches
    of eval_batch_size, sentences with an empty side get no pairs and do not reach the function."""
    hp = make_hp("transformer", eval_batch_size=3)
    seen = []

    def fake(features, graph, params):
        assert graph == "graph" and params is hp
        seen.append(features["source"].shape[0])
        B, Lt = features["target"].shape
        return np.repeat(features["source"][:, :1] - 10, Lt, axis=1)
    pairs = [([10 + i] * (i + 1) + [2], [7] * (1 + i % 3) + [2]) for i in range(7)]
    pairs[4] = ([14, 2], [2])                  # an empty hypothesis
    out = evalu.aligning("graph", pairs, hp, align=fake)
    assert seen == [3, 2, 1]
    assert len(out) == 7 and out[4] == []
    for i, p in enumerate(out):
        if i != 4:
            assert p == [(i, t) for t in range(1 + i % 3)]


def test_dump_alignments(tmp_path):
    evalu.dump_alignments(["0-0 1-1", "", "2-0"], str(tmp_path / "d" / "a.txt"))
    assert (tmp_path / "d" / "a.txt").read_text() == "0-0 1-1\n\n2-0\n"


def test_options_off_call_nothing_new(tmp_path, monkeypatch):
    """evaluate() and scorer() with the options off: decoding / scoring, BLEU and the dump as before -- aligning, align_fn
    and dump_alignments are never reached and no alignment file appears."""
    from zero_amd import main as loops
    import types
    for name in ("aligning", "dump_alignments"):
        monkeypatch.setattr(evalu, name, lambda *a, **k: pytest.fail("evalu.%s was called" % name))
    monkeypatch.setattr(zalign, "align_fn", lambda *a, **k: pytest.fail("align_fn was called"))
    monkeypatch.setattr(loops, "tower_align_graph", lambda *a, **k: pytest.fail("tower_align_graph was called"))
    monkeypatch.setattr(loops, "_eval_trainer", lambda p: types.SimpleNamespace(graph="graph"))
    monkeypatch.setattr(evalu, "decoding", lambda graph, dataset, params, prefixes=None: ([["b"], ["a"]], [0.5, 0.25], [1, 0]))
    monkeypatch.setattr(evalu, "scoring", lambda graph, dataset, params: ([0.5, 0.25], 1.5))
    (tmp_path / "t.src").write_text("x\ny\n")
    (tmp_path / "t.tgt").write_text("a\nb\n")
    hp = make_hp("transformer", src_test_file=str(tmp_path / "t.src"), tgt_test_file=str(tmp_path / "t.tgt"),
                 test_output=str(tmp_path / "out.txt"))
    loops.evaluate(hp)
    assert (tmp_path / "out.txt").read_text() == "a\nb\n"
    assert loops.scorer(hp) == 0.375
    assert sorted(p.name for p in tmp_path.iterdir()) == ["out.txt", "t.src", "t.tgt"]


def test_evaluate_with_the_option_aligns_in_file_order(tmp_path, monkeypatch):
    """evaluate() with alignment_file and replace_unk on fakes: hypotheses come back in decode order, the alignment file and
    the replaced translations are in file order, BLEU sees the replaced text."""
    from zero_amd import main as loops
    import types
    vocab = "\n".join(["a", "b", "c"]) + "\n"
    (tmp_path / "v.txt").write_text(vocab)
    (tmp_path / "t.src").write_text("a Zürich\nb\n")
    (tmp_path / "t.tgt").write_text("a Zürich\nb\n")
    hp = make_hp("transformer", src_test_file=str(tmp_path / "t.src"), tgt_test_file=str(tmp_path / "t.tgt"),
                 test_output=str(tmp_path / "out.txt"), alignment_file=str(tmp_path / "ali.txt"), replace_unk=True)
    from zero_amd.vocab import Vocab
    hp.src_vocab = hp.tgt_vocab = Vocab(str(tmp_path / "v.txt"))
    monkeypatch.setattr(loops, "_eval_trainer", lambda p: types.SimpleNamespace(graph="graph"))
    monkeypatch.setattr(evalu, "decoding", lambda graph, dataset, params, prefixes=None:
                        ([["b"], ["a", "<unk>"]], [0.5, 0.25], [1, 0]))
    monkeypatch.setattr(loops, "tower_align_graph", lambda feats, graph, params:
                        np.tile(np.arange(feats["target"].shape[1]), (feats["target"].shape[0], 1)))
    seen = {}
    real = evalu.eval_metric
    monkeypatch.setattr(evalu, "eval_metric", lambda trans, f, indices=None: seen.update(trans=trans, indices=indices) or 1.0)
    assert loops.evaluate(hp) == 1.0
    assert (tmp_path / "ali.txt").read_text() == "0-0 1-1\n0-0\n"
    assert (tmp_path / "out.txt").read_text() == "a Zürich\nb\n"
    assert seen["trans"] == [["a", "Zürich"], ["b"]] and seen["indices"] is None and real is not None


def test_kernel_refusals_need_no_gpu():
    lib = hip.lib()
    limit = lib.raw("zk_align_max_lk")()
    assert limit >= 1024
    P = 1 << 12          # any non-NULL, 16-byte aligned address: nothing is dereferenced, nothing is launched
    #       q, ldq, bsq, k, ldk, bsk, kmask, ldmask, amask, probs, ldp, bsp, best, B, nh, Lq, Lk, d, scale, inf, stream
    ok = [P, 64, 640, P, 64, 640, None, 0, None, P, 10, 100, P, 1, 2, 10, 10, 32, 0.17, 1e8, None]

    def with_(**kw):
        names = "q ldq bsq k ldk bsk kmask ldmask amask probs ldp bsp best B nh Lq Lk d scale inf stream".split()
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a
    for name, args, text in [
            ("zk_align_probs", with_(d=40, nh=1), r"zk_align_probs: head size d=40 \(a multiple of 32 up to 128"),
            ("zk_align_probs", with_(ldk=63), "zk_align_probs: row strides ldq=64 ldk=63 are shorter than nh \\* d = 64"),
            ("zk_f32_align_probs", with_(ldk=60), "zk_f32_align_probs: row strides .* shorter than nh"),
            ("zk_align_probs", with_(probs=None, best=None), "zk_align_probs: neither probs nor best is given"),
            ("zk_f32_align_probs", with_(probs=None, best=None), "zk_f32_align_probs: neither probs nor best"),
            ("zk_align_probs", with_(Lk=limit + 1, ldp=limit + 1, bsp=10 * (limit + 1)),
             "zk_align_probs: Lk=%d keys \\(at most %d" % (limit + 1, limit)),
            ("zk_f32_align_probs", with_(Lk=limit + 1, ldp=limit + 1, bsp=10 * (limit + 1)), "at most %d" % limit),
            ("zk_f32_align_probs", with_(d=130, nh=1, ldq=130, ldk=132), "head size d=130"),
            ("zk_align_probs", with_(ldq=68), "16-byte aligned rows"),
            ("zk_align_probs", with_(kmask=P, ldmask=9), "ldmask=9 elements are shorter than Lk=10"),
            ("zk_align_probs", with_(ldp=9), "ldp=9")]:
        with pytest.raises(hip.ZeroHipError, match=text):
            lib.call(name, *args)
