"""tgt_prefix_file on the CPU: the HParam, what is refused (without a core, before the encoder pass), the file loader, the graph
key, and the batch of empty prefixes."""
import numpy as np
import pytest

from tests.common import make_hp
from zero_amd.config import SyntheticVocab, default_params
from zero_amd.models import _decode


# ---------------------------------------------------------------------------------------------- the HParam
def test_hparam_default_and_parse():
    hp = default_params()
    assert hp.tgt_prefix_file == "" and _decode.prefix_file(hp) == ""
    hp.parse("tgt_prefix_file=/tmp/p.txt,beam_size=2")
    assert hp.tgt_prefix_file == "/tmp/p.txt" and _decode.prefix_file(hp) == "/tmp/p.txt"
    bare = make_hp("transformer")
    bare.del_hparam("tgt_prefix_file")
    assert _decode.prefix_file(bare) == ""
    _decode.check_prefix_opts(bare)
    _decode.check_prefix_opts(default_params())


@pytest.mark.parametrize("model", ["transformer", "transformer_aan", "rnnsearch"])      # (the models a shortlist is built for)
def test_a_shortlist_is_refused_before_a_core_is_built(model, monkeypatch, tmp_path):
    from zero_amd.models import _factory, model as registry, load_all
    load_all()

    def no_core(*a, **k):
        raise AssertionError("a core was asked for")
    monkeypatch.setattr(_factory, "get_core", no_core)
    monkeypatch.setattr(_decode, "get_core", no_core)
    hp = make_hp(model, search_mode="cache", tgt_prefix_file=str(tmp_path / "p.txt"), shortlist_file=str(tmp_path / "lex.txt"))
    with pytest.raises(NotImplementedError, match=r"tgt_prefix_file=.*p\.txt with shortlist_file=.*lex\.txt"):
        registry.get_model(model).infer_fn(hp)
    with pytest.raises(NotImplementedError, match=r"tgt_prefix_file.*shortlist_file"):
        _decode.check_prefix_opts(hp)
    hp.shortlist_file = ""
    _decode.check_prefix_opts(hp)
    registry.get_model(model).infer_fn(hp)             # the option alone is taken, and still no core


# ---------------------------------------------------------------------------------------------- a batch's prefixes
SRC_LEN = np.array([6, 3, 4])
ARGS = dict(B=3, V=20, eos_id=2, src_len=SRC_LEN, decode_length=5)
BAD = [
    (np.array([[3, 4], [5, 0]]), r"shape \(2, 2\).*\[3, P\]"),                                        # a row count other than B
    (np.array([3, 4, 5]), r"shape \(3,\)"),
    (np.array([[3, 0], [20, 0], [0, 0]]), r"sentence 1: id 20 at position 0 is outside \[1, 20\)"),
    (np.array([[3, 0], [4, 0], [5, -1]]), r"sentence 2: id -1 at position 1 is outside \[1, 20\)"),
    (np.array([[3, 2], [4, 0], [0, 0]]), r"sentence 0: position 1 holds the end-of-sentence id 2"),
    (np.array([[3, 0, 0], [4, 0, 7], [0, 0, 0]]), r"sentence 1: position 1 is 0 \(padding\) and position 2 holds id 7"),
    (np.array([[3] * 8, [4] * 8, [0] * 8]), r"sentence 1: 8 tokens, .* 3 \+ 5 = 8 tokens"),
    (np.array([[3.0, 0.0], [4.0, 0.0], [0.0, 0.0]]), r"float64 values"),
]


@pytest.mark.parametrize("prefix, text", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_prefixes_are_refused_by_name(prefix, text):
    with pytest.raises(ValueError, match=text):
        _decode.check_prefix(prefix, **ARGS)


def test_good_prefixes_are_taken():
    assert _decode.check_prefix(None, **ARGS) == (None, None)
    p, n = _decode.check_prefix(np.array([[3, 4, 0, 0], [0, 0, 0, 0], [19, 1, 5, 0]]), **ARGS)
    assert p.dtype == np.int32 and p.tolist() == [[3, 4, 0], [0, 0, 0], [19, 1, 5]] and n.tolist() == [2, 0, 3]
    p, n = _decode.check_prefix(np.zeros((3, 2), dtype=np.int64), **ARGS)
    assert p.shape == (3, 1) and not p.any() and n.tolist() == [0, 0, 0]
    # one token short of the length at which the search cuts the sentence off
    p, n = _decode.check_prefix(np.array([[3] * 7, [4] * 7, [0] * 7]), **ARGS)
    assert n.tolist() == [7, 7, 0]
    import torch
    p, n = _decode.check_prefix(torch.tensor([[3, 4], [0, 0], [5, 0]]), **ARGS)
    assert p.tolist() == [[3, 4], [0, 0], [5, 0]]


@pytest.mark.parametrize("mode", ["cache", "dev"])
def test_the_search_refuses_before_the_encoder_pass(mode, monkeypatch):
    from zero_amd import search
    from zero_amd.models import _factory

    def no_core(*a, **k):
        raise AssertionError("a core was asked for")
    monkeypatch.setattr(_factory, "get_core", no_core)

    def encoding_fn(*a, **k):
        raise AssertionError("encoding_fn was called")
    hp = make_hp("transformer", search_mode=mode, beam_size=2)
    src = np.array([[5, 6, 7, 2], [5, 2, 0, 0]])
    V = hp.tgt_vocab.size()
    for prefix, text in [(np.array([[3, 0]]), r"\[2, P\]"), (np.array([[3, 0], [V, 0]]), r"sentence 1: id %d" % V),
                         (np.array([[3, 2], [0, 0]]), r"end-of-sentence id 2"), (np.array([[0, 3], [0, 0]]), r"right-padded"),
                         (np.array([[3] * (4 + hp.decode_length), [0] * (4 + hp.decode_length)]), r"could not end")]:
        with pytest.raises(ValueError, match=text):
            search._beam_search_body({"source": src, "prefix": prefix}, encoding_fn, None, hp, [])
    # with the n-gram ban, a prefix that holds an n-gram twice (the ban would take the forced token: tests/prefix_ref.py)
    hp.no_repeat_ngram_size = 2
    with pytest.raises(ValueError, match=r"sentence 0 with no_repeat_ngram_size=2: the 2-gram \(5, 6\) at position 2"):
        search._beam_search_body({"source": src, "prefix": np.array([[5, 6, 5, 6], [0, 0, 0, 0]])}, encoding_fn, None, hp, [])
    hp.no_repeat_ngram_size = 0
    hp.shortlist_file = "lex.txt"
    with pytest.raises(NotImplementedError, match=r"features\['prefix'\] with shortlist_file=lex\.txt"):
        search._beam_search_body({"source": src, "prefix": np.array([[3, 0], [0, 0]])}, encoding_fn, None, hp, [])


# ---------------------------------------------------------------------------------------------- the step graphs
def test_graph_key():
    """Without a table -- no key "prefix" in the state, or None: a batch of empty prefixes -- the key of a step is the tuple
    it was before the option existed; with one it has one more entry."""
    state = {"B": 4, "K": 4, "Ls": 16, "Tmax": 24, "f32": True}
    args = (None, 1.0, 1e8, False, 0)
    before = (4, 4, 16, 24, False, 1.0, 1e8, False, 0, True)
    assert _decode.graph_key(state, *args) == before
    assert _decode.graph_key(dict(state, prefix=None), *args) == before
    with_table = dict(state, prefix=(0x7f0000001000, 24))
    assert _decode.graph_key(with_table, *args) == before + (("prefix",),)
    assert _decode.graph_key(with_table, *args, 3, (10, 0.9), (2, 0.5, 2)) == \
        before + (("ngram", 3), ("sample", 10, 0x3f666666), ("diverse", 2, 0x3f000000), ("prefix",))


def test_graph_pointers_carry_the_table():
    class Own(dict):
        def graph_pointers(self):
            return (11, 12)
    st = Own(prefix=None)
    assert _decode._graph_pointers(st, (1, 2)) == (11, 12, 1, 2)
    st["prefix"] = (77, 24)
    assert _decode._graph_pointers(st, (1, 2)) == (11, 12, 1, 2, 77, 24)
    assert _decode._graph_pointers(st, None) == (11, 12, 77, 24)
    st["ngram_hist"] = (55, 26)
    assert _decode._graph_pointers(st, None) == (11, 12, 55, 26, 77, 24)


class _NoCore(object):
    def __getattr__(self, name):
        raise AssertionError("the core was touched (%s)" % name)


def test_a_batch_of_empty_prefixes_has_no_table():
    state = {"_core": _NoCore(), "B": 3, "Tmax": 16}
    assert _decode.prefix_table(state, None, 2) is None and state["prefix"] is None
    assert _decode.prefix_table(state, np.zeros((3, 4), dtype=np.int32), 2) is None and state["prefix"] is None
    assert "prefix_eos" not in state
    state["prefix"] = (1, 2)                      # a stale entry does not survive either
    _decode.prefix_table(state, np.zeros((3, 1), dtype=np.int32), 2)
    assert state["prefix"] is None
    with pytest.raises(AssertionError, match="the core was touched"):
        _decode.prefix_table(state, np.array([[3], [0], [0]], dtype=np.int32), 2)


# ---------------------------------------------------------------------------------------------- the file loader
def _files(tmp_path, src_lines, prefix_lines):
    (tmp_path / "test.src").write_text("".join(l + "\n" for l in src_lines))
    (tmp_path / "prefix.txt").write_text("".join(l + "\n" for l in prefix_lines))
    return str(tmp_path / "test.src"), str(tmp_path / "prefix.txt")


def test_loader_skips_the_lines_the_dataset_skips(tmp_path):
    """A source file with blank lines: Dataset.load_data skips them and numbers what is left; the loader's list is indexed by
    those numbers, whatever order a batch has them in."""
    from zero_amd import evalu
    from zero_amd.data import Dataset
    vocab = SyntheticVocab(30)
    vocab.to_id = lambda toks, append_eos=True: [vocab.find(t) if vocab.find(t) is not None else vocab.unk() for t in toks] + \
        ([vocab.eos()] if append_eos else [])
    src_lines = ["5 6 7", "", "8 9", "10 11 12 13", "   ", "14"]
    prefix_lines = ["20 21", "22", "", "23 zzz 24", "25", "26"]
    src, pre = _files(tmp_path, src_lines, prefix_lines)
    prefixes = evalu.load_prefixes(src, pre, vocab)
    assert prefixes == [[20, 21], [], [23, 1, 24], [26]]          # the lines beside blank source lines are gone; zzz is UNK
    ds = Dataset(src, src, vocab, vocab, 100, batch_or_token="batch")
    rows = list(ds.load_data())
    assert len(rows) == len(prefixes)
    seen = []
    for data in ds.batcher(3, shuffle=False, train=False):
        m = evalu.prefix_matrix(prefixes, data["index"])
        assert m.dtype == np.int32 and m.shape[0] == len(data["index"])
        for b, i in enumerate(data["index"]):
            assert [int(v) for v in m[b] if v] == prefixes[i]
            assert data["src"][b, 0] == rows[i][0][0]               # the source row the prefix travels with
            assert not m[b, len(prefixes[i]):].any()
            seen.append(i)
    assert sorted(seen) == [0, 1, 2, 3] and seen != sorted(seen)       # (sorted by length: a permuted index)
    assert evalu.prefix_matrix(prefixes, [1]).tolist() == [[0]]
    assert evalu.load_prefixes(src, pre, vocab, max_len=2)[2] == [23, 1]


def test_loader_refuses_another_line_count(tmp_path):
    from zero_amd import evalu
    src, pre = _files(tmp_path, ["5 6", "7"], ["20"])
    with pytest.raises(ValueError, match=r"prefix\.txt has 1 lines, src_test_file .*test\.src has 2"):
        evalu.load_prefixes(src, pre, SyntheticVocab(30))


def test_decoding_adds_the_prefix_feature(tmp_path):
    """evalu.decoding with prefixes: every batch's features carry the rows of its index; without: no such key."""
    from zero_amd import evalu
    from zero_amd.data import Dataset
    vocab = SyntheticVocab(30)
    vocab.to_id = lambda toks, append_eos=True: [int(t) for t in toks] + ([2] if append_eos else [])
    vocab.to_tokens = lambda ids: [str(i) for i in ids]
    src, pre = _files(tmp_path, ["5 6 7", "8 9", "10 11 12 13"], ["20 21", "", "22"])
    prefixes = evalu.load_prefixes(src, pre, vocab)
    hp = make_hp("transformer", search_mode="cache", eval_batch_size=2)
    hp.tgt_vocab = vocab
    got = []

    def infer(features, graph, params):
        got.append(features)
        B = features["source"].shape[0]
        return np.full((B, 1, 2), 7), np.zeros((B, 1))
    for p in (prefixes, None):
        del got[:]
        ds = Dataset(src, src, vocab, vocab, 100, batch_or_token="batch")
        _, _, indices = evalu.decoding(None, ds, hp, infer=infer, streams=1, prefixes=p)
        assert sorted(indices) == [0, 1, 2]
        if p is None:
            assert all("prefix" not in f for f in got)
        else:
            rows = [r for f in got for r in f["prefix"].tolist()]
            assert [[v for v in r if v] for r in rows] == [prefixes[i] for i in indices]
