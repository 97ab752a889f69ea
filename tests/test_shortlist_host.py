"""Lexical shortlist decoding on the CPU: the new HParams, the loader of the table file, the numpy reference of the set
construction (tests/shortlist_ref.py) against a plain set-based restatement, the refusals, and the check of the kernel test
(tests/test_gpu_shortlist_kernels.py: exact equality of ids and count) shown to reject planted defects.

Planted (tests/shortlist_ref.DEFECTS), each must differ from the reference on at least one case of shortlist_ref.product():
    fill_from_top   the fill takes the highest missing ids          pad_counts     source id 0 (pad) looked up
    best_ignored    whole table rows taken                          unsorted       the set not ascending
    not_rounded     Vs = n                                          not_capped     Vs beyond V
    tail_zero       ids[Vs .. cap) = 0 instead of -1
"""
import numpy as np
import pytest

from tests import shortlist_ref as SR
from tests.common import make_hp
from zero_amd import shortlist
from zero_amd.config import SyntheticVocab, default_params


def test_new_hparams_and_their_defaults():
    hp = default_params()
    assert (hp.shortlist_file, hp.shortlist_first, hp.shortlist_best, hp.shortlist_round) == ("", 100, 100, 1024)
    assert hp.shortlist_round % 8 == 0 and not shortlist.wanted(hp)
    shortlist.check(hp, "deepnmt")                   # off: nothing is refused
    hp.parse("shortlist_file=lex.txt,shortlist_first=50,shortlist_best=20,shortlist_round=512")
    assert shortlist.wanted(hp) and (hp.shortlist_first, hp.shortlist_best, hp.shortlist_round) == (50, 20, 512)


def _vocab(tmp_path, name, tokens):
    from zero_amd.vocab import Vocab
    p = tmp_path / name
    p.write_text("".join(t + "\n" for t in tokens))
    return Vocab(str(p))


LINES = """haus house 0.6
das the 0.5
die the 0.7
der the 0.5
heim house 0.6
xyzzy house 0.9
haus plugh 0.9
gruen green 0.25
malformed line
katze cat notanumber
"""


def test_loader_on_an_inline_file(tmp_path):
    """Unknown tokens on either side, unsorted probabilities, a tie (file order kept) and source rows without entries."""
    src = _vocab(tmp_path, "src.txt", ["<pad>", "<unk>", "<eos>", "the", "house", "cat", "green"])
    tgt = _vocab(tmp_path, "tgt.txt", ["<pad>", "<unk>", "<eos>", "der", "die", "das", "haus", "heim", "gruen", "katze"])
    f = tmp_path / "lex.txt"
    f.write_text(LINES)
    t = shortlist.load_table(str(f), src, tgt)
    assert t.off.dtype == np.int32 and t.ids.dtype == np.int32 and len(t.off) == src.size() + 1
    the, house, cat, green = (src.find(w) for w in ("the", "house", "cat", "green"))
    assert list(t.row(the)) == [tgt.find("die"), tgt.find("das"), tgt.find("der")]          # 0.7, then the 0.5 tie in file order
    assert list(t.row(house)) == [tgt.find("haus"), tgt.find("heim")]                         # the tie again; xyzzy dropped
    assert list(t.row(cat)) == [] and list(t.row(green)) == [tgt.find("gruen")]
    assert all(len(t.row(s)) == 0 for s in range(3)) and t.off[-1] == len(t.ids) == 6
    assert shortlist.load_table(str(f), src, tgt) is t                                        # cached per (path, vocabularies)
    assert shortlist.load_table(str(f), src, _vocab(tmp_path, "tgt2.txt", ["<pad>", "<unk>", "<eos>", "haus"])) is not t
    # synthetic vocabularies spell a token as its decimal id
    s = shortlist.parse_table(["5 3 0.5", "6 3 0.7", "8 3 0.9", "4 12 0.1", "x 3 1"], SyntheticVocab(10), SyntheticVocab(8))
    assert list(s.row(3)) == [6, 5] and s.off[-1] == 2


def _by_sets(src, off, lex, first, best, V, round_to):
    S = set(range(min(first, V)))
    for s in np.asarray(src).reshape(-1):
        if 0 < s < len(off) - 1:
            S |= {int(t) for t in lex[off[s]:off[s + 1]][:best] if 0 <= t < V}
    n = len(S)
    Vs = min(V, (n + round_to - 1) // round_to * round_to)
    i = 0
    while len(S) < Vs:
        S.add(i)
        i += 1
    return sorted(S), n, Vs


def test_reference_equals_a_set_restatement_and_the_cases_cover_the_edges():
    cases = SR.product()
    assert 30 <= len(cases) <= 80
    seen = {"exact": False, "capped": False, "filled": False, "pad_row": False}
    for case in cases:
        V, name, best, first, rnd = case
        src, off, lex = SR.case_inputs(case)
        ids, (n, Vs) = SR.build(src, off, lex, first, best, V, rnd, V + 5)
        S, n2, Vs2 = _by_sets(src, off, lex, first, best, V, rnd)
        assert (n, Vs) == (n2, Vs2) and list(ids[:Vs]) == S and (ids[Vs:] == -1).all(), case
        assert (np.diff(ids[:Vs]) > 0).all() and 3 <= n <= Vs <= V and (Vs % rnd == 0 or Vs == V)
        seen["exact"] |= n == Vs and n % rnd == 0 and Vs < V
        seen["capped"] |= Vs == V and -(-n // rnd) * rnd > V
        seen["filled"] |= n < Vs < V
        seen["pad_row"] |= bool((np.asarray(src) == 0).all(axis=1).any())
    assert all(seen.values()), seen
    # every value of every factor occurs
    assert {c[0] for c in cases} == set(SR.VOCABS)
    triples = set()
    for V in SR.VOCABS:                                          # every V meets every value of every factor
        mine = [c for c in cases if c[0] == V]
        assert {c[1] for c in mine} == set(SR.sources()) and {c[2] for c in mine} == set(SR.BESTS)
        assert {c[3] for c in mine} >= set(SR.firsts(V)) and {c[4] for c in mine} == set(SR.ROUNDS)
        triples |= {(c[2], SR.firsts(V).index(c[3]), c[4]) for c in mine if c[3] in SR.firsts(V)}
    assert len(triples) == len(SR.BESTS) * 3 * len(SR.ROUNDS)    # and every (best, first, round) triple runs at some V


@pytest.mark.parametrize("defect", SR.DEFECTS)
def test_each_planted_defect_fails_on_a_listed_case(defect):
    caught = []
    for case in SR.product():
        V, name, best, first, rnd = case
        src, off, lex = SR.case_inputs(case)
        ref = SR.build(src, off, lex, first, best, V, rnd, V + 5)
        bad = SR.build(src, off, lex, first, best, V, rnd, V + 5, defect=defect)
        if not (np.array_equal(ref[0], bad[0]) and ref[1] == bad[1]):
            caught.append(case)
    print("%s: caught on %d of %d cases" % (defect, len(caught), len(SR.product())))
    assert caught


# ---------------------------------------------------------------------------------------------- refusals
def _with_file(model, **kw):
    return make_hp(model, search_mode="cache", shortlist_file="lex.txt", shortlist_first=5, shortlist_round=8, **kw)


@pytest.mark.parametrize("model", ["transformer_l0drop", "transformer_rela", "transformer_fixup", "rnnsearch_deepatt",
                                   "deepnmt"])
def test_other_models_refuse_before_a_core_is_built(model):
    from zero_amd.models import model as registry, load_all
    load_all()
    kw = dict(cell="atr", layer_norm=False) if model in ("rnnsearch_deepatt", "deepnmt") else {}
    with pytest.raises(NotImplementedError, match="shortlist_file"):
        registry.get_model(model).infer_fn(_with_file(model, **kw))


@pytest.mark.parametrize("model", ["transformer", "rnnsearch"])
def test_other_search_modes_and_ensembles_refuse(model):
    from zero_amd.models import _ensemble, model as registry, load_all
    load_all()
    kw = dict(cell="atr", layer_norm=False, caencoder=True) if model == "rnnsearch" else {}
    hp = _with_file(model, **kw)
    hp.search_mode = "dev"
    with pytest.raises(NotImplementedError, match="shortlist_file"):
        registry.get_model(model).infer_fn(hp)
    hp.search_mode = "cache"
    registry.get_model(model).infer_fn(hp)            # the required models build their closures (no core, no file read yet)
    with pytest.raises(NotImplementedError, match="shortlist_file"):
        _ensemble.make_infer_fns([registry.get_model("transformer")] * 2, [make_hp("transformer"), _with_file("transformer")])


@pytest.mark.parametrize("kw, word", [(dict(shortlist_first=2), "shortlist_first"), (dict(shortlist_round=12), "shortlist_round"),
                                      (dict(shortlist_round=0), "shortlist_round"), (dict(shortlist_best=-1), "shortlist_best")])
def test_bad_shortlist_parameters_are_named(kw, word):
    hp = _with_file("transformer")
    hp.override_from_dict(kw)
    with pytest.raises(ValueError, match=word):
        shortlist.check(hp, "transformer")
