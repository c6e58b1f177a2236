"""tests/phrase_oracle.py, the numpy restatement of ocr_lexicon_phrase_match's rule, held to the enumeration of every segmentation
and to hand-worked cases.  No GPU: nothing is skipped, every case compares every array."""
import numpy as np
import pytest

from tests import phrase_oracle as PO

KEYS = ("line_word_offsets", "word_offsets", "entries", "word_costs", "line_costs", "raw_costs", "line_flags")


def _one(text, words, bound=None, join=None, **prm):
    r = PO.phrase_match(PO.costs_for_text(text), [0, len(text)], words, bound, join, **prm)
    assert set(r) == set(KEYS)
    return r


def _read(r, text, words):
    o = r["word_offsets"].tolist()
    return [(text[o[k]:o[k + 1]], words[e] if e >= 0 else None) for k, e in enumerate(r["entries"].tolist())]


def _enum_case(seed, G, n_entries, integer, gaps, prm):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, min(G, 4) + 1, n_entries)
    # few classes, so that entries hit each other's letters and equal values are common when the costs are whole numbers
    words = ["".join(PO.ALPHABET[c] for c in rng.integers(0, 3, int(m))) for m in lens]
    cost = PO.make_costs(rng, G, integer=integer)
    bound = join = None
    if gaps:
        bound = rng.integers(0, 3, G).astype(np.float32) if integer else (rng.random(G) * 2).astype(np.float32)
        join = rng.integers(0, 3, G).astype(np.float32) if integer else (rng.random(G) * 2).astype(np.float32)
    got = PO.phrase_match(cost, [0, G], words, bound, join, **prm)
    lens_e, ents_e, costs_e, total_e = PO.enumerate_line(cost, words, bound, join, **prm)
    assert np.diff(got["word_offsets"]).tolist() == lens_e, (seed, G)
    assert got["entries"].tolist() == ents_e, (seed, G)
    assert np.array_equal(got["word_costs"].view(np.uint64), np.array(costs_e, np.float64).view(np.uint64)), (seed, G)
    assert np.array_equal(got["line_costs"].view(np.uint64), np.array([total_e], np.float64).view(np.uint64)), (seed, G)
    assert got["line_word_offsets"].tolist() == [0, len(lens_e)] and got["line_flags"].tolist() == [0]
    acc = np.float64(0.0)
    for g in range(G):
        acc = acc + np.float64(cost[g].min())
    assert got["raw_costs"][0] == acc
    return got


ENUM_PARAMS = [dict(), dict(word_cost=0.0, oov_word_cost=0.0, oov_glyph_cost=0.0), dict(word_cost=2.0, oov_word_cost=1.0, fold_case=0),
               dict(oov_word_cost=3.0, oov_glyph_cost=0.0)]


@pytest.mark.parametrize("integer", [False, True], ids=["f32", "integer"])
def test_oracle_equals_enumeration(integer):
    """Every segmentation (2^(G-1) compositions x {every entry of that length, OOV} per part) for G <= 6, lexicons of at most 12
    entries: once with random f32 costs, once with costs from {0, 1, 2, 3}, where ties abound and every tie rule decides somewhere."""
    seed = 100 if integer else 200
    oov, lex, multi = 0, 0, 0
    for G in (1, 2, 3, 4, 5, 6):
        for rep in range(4 if G < 6 else 2):
            for gaps in (False, True):
                seed += 1
                n_entries = 12 if G < 6 else 9
                got = _enum_case(seed, G, n_entries, integer, gaps, ENUM_PARAMS[(rep + G) % len(ENUM_PARAMS)])
                oov += int(np.count_nonzero(got["entries"] < 0))
                lex += int(np.count_nonzero(got["entries"] >= 0))
                multi += int(len(got["entries"]) > 1)
    assert oov > 0 and lex > 0 and multi > 0, (oov, lex, multi)   # both kinds of word and real segmentations were compared


def test_integer_enumeration_has_ties():
    """The integer cases really tie: with whole-number costs and all parameters whole numbers some line has two different
    segmentations of the minimal value, so the (v, kind, M) order decided."""
    rng = np.random.default_rng(7)
    cost = rng.integers(0, 4, size=(4, 62)).astype(np.float32)
    words = ["A", "B", "AB", "BA", "ABA"]
    # all parameters zero: every segmentation into lexicon words of zero-cost letters and every OOV reading costs raw: ties everywhere
    r = PO.phrase_match(cost, [0, 4], words, word_cost=0.0, oov_word_cost=0.0, oov_glyph_cost=0.0)
    lens_e, ents_e, _, total_e = PO.enumerate_line(cost, words, word_cost=0.0, oov_word_cost=0.0, oov_glyph_cost=0.0)
    assert np.diff(r["word_offsets"]).tolist() == lens_e and r["entries"].tolist() == ents_e and r["line_costs"][0] == total_e
    # OOV alone reaches the greedy sum with any cut: the minimum is shared by at least the 8 compositions
    assert r["line_costs"][0] == r["raw_costs"][0]


def test_inthebox_tie_rule_and_word_cost():
    words = ["in", "the", "box", "int", "he"]
    # both "in the box" and "int he box" are three exact words: at glyph 5 `the` behind `in` ties with `he` behind `int`, and the
    # shorter word wins the tie.  Hand-worked: B = [0, 7, 1, 1, 8, 2, 9, 10, 3].
    r = _one("inthebox", words)
    assert _read(r, "inthebox", words) == [("int", "int"), ("he", "he"), ("box", "box")]
    assert r["word_costs"].tolist() == [1.0, 1.0, 1.0] and r["line_costs"].tolist() == [3.0] and r["raw_costs"].tolist() == [0.0]
    r0 = _one("inthebox", words, word_cost=0.0)
    assert _read(r0, "inthebox", words) == [("int", "int"), ("he", "he"), ("box", "box")] and r0["line_costs"].tolist() == [0.0]
    # without `int` there is one exact reading
    r3 = _one("inthebox", words[:3])
    assert _read(r3, "inthebox", words) == [("in", "in"), ("the", "the"), ("box", "box")] and r3["line_costs"].tolist() == [3.0]
    # what word_cost is for: with every letter an entry of its own, a free word falls apart into letters (shorter wins the ties) ...
    letters = words[:3] + list("inthebox")
    rl0 = _one("inthebox", letters, word_cost=0.0)
    assert np.diff(rl0["word_offsets"]).tolist() == [1] * 8 and rl0["line_costs"].tolist() == [0.0]
    # ... and a paid word keeps the three words: 3.0 against 8.0
    rl1 = _one("inthebox", letters)
    assert _read(rl1, "inthebox", letters) == [("in", "in"), ("the", "the"), ("box", "box")] and rl1["line_costs"].tolist() == [3.0]


def test_oov_word_between_two_entries():
    words = ["the", "box"]
    r = _one("theQZXbox", words)
    assert _read(r, "theQZXbox", words) == [("the", "the"), ("QZX", None), ("box", "box")]
    assert r["entries"].tolist() == [0, -1, 1]
    assert r["word_costs"].tolist() == [1.0, 9.0, 1.0] and r["line_costs"].tolist() == [11.0]   # OOV: 6 + 3 * (0 + 1)
    assert r["line_word_offsets"].tolist() == [0, 3] and r["line_flags"].tolist() == [0]


def test_no_entry_fits_cuts_every_32_glyphs():
    text = "a" * 70
    r = _one(text, ["Z9"], fold_case=0)
    # three OOV words is the least (M <= 32): every split 70 = a + b + c costs 18 + 70; the walk back takes the shortest last word
    # that still leaves two words of 32
    assert np.diff(r["word_offsets"]).tolist() == [32, 32, 6] and r["entries"].tolist() == [-1, -1, -1]
    assert r["word_costs"].tolist() == [38.0, 38.0, 12.0] and r["line_costs"].tolist() == [88.0]


def test_gap_costs_flip_one_boundary_by_one_unit():
    words = ["a", "b", "ab"]
    z = np.zeros(2, np.float32)
    one = np.array([0, 1], np.float32)
    # `ab` costs 1 + join[1], `a b` costs 2 + bound[1]
    r = _one("ab", words, z, z)
    assert np.diff(r["word_offsets"]).tolist() == [2] and r["entries"].tolist() == [2] and r["line_costs"].tolist() == [1.0]
    r = _one("ab", words, z, one)         # 2 against 2: the shorter word wins the tie
    assert np.diff(r["word_offsets"]).tolist() == [1, 1] and r["entries"].tolist() == [0, 1] and r["line_costs"].tolist() == [2.0]
    assert r["word_costs"].tolist() == [1.0, 1.0]
    r = _one("ab", words, one, one)       # 3 against 2
    assert np.diff(r["word_offsets"]).tolist() == [2] and r["word_costs"].tolist() == [2.0] and r["line_costs"].tolist() == [2.0]
    r = _one("ab", words, one, 2 * one)   # 3 against 3: the tie again
    assert np.diff(r["word_offsets"]).tolist() == [1, 1] and r["line_costs"].tolist() == [3.0]
    # the first glyph's bound and join are never paid
    r = _one("ab", words, np.array([5, 0], np.float32), np.array([5, 0], np.float32))
    assert np.diff(r["word_offsets"]).tolist() == [2] and r["line_costs"].tolist() == [1.0]


def test_flagged_lines_keep_the_tiling():
    cost = np.concatenate([PO.costs_for_text("a" * 257, hit=1.0), PO.costs_for_text("box")])
    r = PO.phrase_match(cost, [0, 0, 257, 257, 260], ["box"])
    assert r["line_flags"].tolist() == [1, 2, 1, 0]
    assert r["line_word_offsets"].tolist() == [0, 1, 2, 3, 4] and r["word_offsets"].tolist() == [0, 0, 257, 257, 260]
    assert r["entries"].tolist() == [-1, -1, -1, 0]
    assert r["word_costs"].tolist() == [0.0, np.inf, 0.0, 1.0] and r["line_costs"].tolist() == [0.0, np.inf, 0.0, 1.0]
    assert r["raw_costs"].tolist() == [0.0, 257.0, 0.0, 0.0]   # a flagged line is summed like any other


def test_fold_case_and_duplicates():
    words = ["BOX", "box", "box"]
    r = _one("bOx", words)                       # folded: all three cost 0, the lowest index wins
    assert r["entries"].tolist() == [0] and r["line_costs"].tolist() == [1.0]
    r = _one("bOx", words, fold_case=0)          # unfolded: box misses one letter (6 + 1), BOX two; OOV costs 6 + 3
    assert r["entries"].tolist() == [1] and r["line_costs"].tolist() == [7.0]


def test_arguments_are_checked():
    c = PO.costs_for_text("ab")
    with pytest.raises(ValueError):
        PO.phrase_match(c, [0, 1], ["a"])
    with pytest.raises(ValueError):
        PO.phrase_match(c, [0, 2], ["a"], bound_cost=np.zeros(2, np.float32))
    with pytest.raises(ValueError):
        PO.phrase_match(c, [0, 2], ["a"], word_cost=-1.0)
    with pytest.raises(ValueError):
        PO.phrase_match(c, [0, 2], ["a" * 33])
    bad = c.copy()
    bad[1, 3] = np.nan
    with pytest.raises(ValueError):
        PO.phrase_match(bad, [0, 2], ["a"])


def test_gap_costs_restatement():
    bound, join = PO.gap_costs([0, 2, 3, 3, 5], 5, break_penalty=1.5, join_penalty=0.5)
    assert bound.tolist() == [0.0, 1.5, 0.0, 0.0, 1.5] and join.tolist() == [0.5, 0.0, 0.5, 0.5, 0.0]
