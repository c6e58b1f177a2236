"""The character language model's oracle (tests/char_lm_oracle.py) against enumeration of every path, on hand cases and on the cases
whose ties tests/test_gpu_char_lm.py relies on, and capi.char_lm_table.  No GPU."""
import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from tests import char_lm_oracle as LM
from tests import lexicon_oracle as LX


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("G", [1, 2, 3])
def test_k_best_equals_enumeration_of_all_paths(G, integer):
    rng = np.random.default_rng(100 + G + 10 * integer)
    cost = LM.make_costs(rng, G, integer=integer)
    T = LM.make_model(rng, integer=integer)
    all_cost, paths = LM.enumerate_paths(cost, T)
    assert len(all_cost) == 62 ** G
    want = np.sort(all_cost, kind="stable")
    for K in (1, 8):
        got = LM.decode(cost, [0, G], T, top_k=K)
        assert np.array_equal(_u64(got["costs"][0]), _u64(want[:K]))
        seen = set()
        for k in range(K):
            path = got["labels"][k]
            assert path.min() >= 0 and path.max() < 62
            assert _u64(LM.path_cost(cost, T, path)) == _u64(got["costs"][0, k])     # the path's own left-to-right cost
            seen.add(tuple(path.tolist()))
        assert len(seen) == K                                                        # distinct strings
        assert got["costs"][0, 0] <= got["raw_costs"][0]
    if integer:
        assert np.count_nonzero(want[:9][1:] == want[:9][:-1]) > 0                   # whole numbers: the enumeration itself has ties


def _read(cost, T, K=1):
    got = LM.decode(cost, [0, cost.shape[0]], T, top_k=K)
    return [LM.text_of(got["labels"][k]) for k in range(K)], got


def test_c0de_reads_code_under_a_letter_model_and_c0de_under_the_zero_model():
    # the glyph 0 beats o by a little: alone it reads c0de
    cost = LM.costs_for_text("c0de", confusions={1: {"o": 1.0}})
    T = capi.char_lm_table(["code", "node", "mode", "coda", "cone", "dome", "come"])
    assert _read(cost, T)[0] == ["code"]
    texts, got = _read(cost, LM.zero_model())
    assert texts == ["c0de"] and got["costs"][0, 0] == 0.0 == got["raw_costs"][0]
    # and the second reading under the zero model is the o
    assert _read(cost, LM.zero_model(), 2)[0] == ["c0de", "code"]


def test_l_I_1_at_a_word_start():
    # the first glyph is l, I or 1 at the same cost: the first minimum is I (class 8); a model from capitalised words keeps I,
    # one from numbers reads 1, one from lower-case words reads l
    cost = LM.costs_for_text("Ion", confusions={0: {"l": 0.0, "1": 0.0}})
    assert _read(cost, LM.zero_model())[0] == ["Ion"]
    assert _read(cost, capi.char_lm_table(["Ion", "Iron", "Inn"]))[0] == ["Ion"]
    assert _read(cost, capi.char_lm_table(["lon", "lion", "loan", "long"]))[0] == ["lon"]
    cost = LM.costs_for_text("I00", confusions={0: {"l": 0.0, "1": 0.0}})
    assert _read(cost, capi.char_lm_table(["100", "1000", "10", "12"]))[0] == ["100"]


def test_begin_and_end_costs_each_change_the_winner():
    cost = LM.costs_for_text("ab", hit=1.0, confusions={0: {"x": 1.5}, 1: {"y": 1.5}})
    T = LM.zero_model()
    assert _read(cost, T)[0] == ["ab"]
    Tb = T.copy()
    Tb[LM.BEGIN, LM.CLASS_OF["a"]] = 1.0           # a may not start a word: x does
    assert _read(cost, Tb)[0] == ["xb"]
    Te = T.copy()
    Te[LM.CLASS_OF["b"], LM.END] = 1.0             # b may not end one: y does
    assert _read(cost, Te)[0] == ["ay"]
    both = np.maximum(Tb, Te)
    texts, got = _read(cost, both)
    assert texts == ["xy"] and got["costs"][0, 0] == 3.0 and got["raw_costs"][0] == 4.0


def test_hand_tie_order():
    """AA, BA and BB cost 0 and are ordered by (last class, rank), the rank by (first class); then the six cheapest of the paths of
    cost 1 are those that end in A - C, D, E, F, G in front - and AB, which also costs 1, comes behind every one of them."""
    cost, off, T = LM.hand_tie_case()
    got = LM.decode(cost, off, T, top_k=8)
    assert [LM.text_of(got["labels"][k]) for k in range(8)] == ["AA", "BA", "BB", "CA", "DA", "EA", "FA", "GA"]
    assert got["costs"][0].tolist() == [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    assert got["ties"] == 7                        # every rank ties with the next but 2 | 3
    assert [LM.text_of(LM.decode(cost, off, T, top_k=2)["labels"][k]) for k in range(2)] == ["AA", "BA"]


def test_seeded_tie_case_has_ties_and_every_cut_is_a_prefix():
    cost, off, T = LM.tie_case()
    got = LM.decode(cost, off, T, top_k=8)
    assert got["ties"] >= 20
    assert np.all(np.diff(got["costs"], axis=1) >= 0)
    for K in (1, 2, 5):                            # the lists cut at K are the prefixes of the lists cut at 8
        cut = LM.decode(cost, off, T, top_k=K)
        assert np.array_equal(_u64(cut["costs"]), _u64(got["costs"][:, :K])) and np.array_equal(cut["labels"], got["labels"][:K])
    for w in range(len(off) - 1):
        rows = cost[off[w]:off[w + 1]]
        paths = {tuple(got["labels"][k, off[w]:off[w + 1]].tolist()) for k in range(8)}
        assert len(paths) == 8
        for k in range(8):
            assert LM.path_cost(rows, T, got["labels"][k, off[w]:off[w + 1]]) == got["costs"][w, k]


def test_flags_and_words_that_are_not_decoded():
    rng = np.random.default_rng(5)
    off = LM.offsets([0, 33, 2, 0, 32])
    cost = LM.make_costs(rng, int(off[-1]))
    T = LM.make_model(rng)
    got = LM.decode(cost, off, T, top_k=2)
    assert got["word_flags"].tolist() == [1, 2, 0, 1, 0]
    assert np.all(np.isinf(got["costs"][[0, 1, 3]])) and np.all(np.isfinite(got["costs"][[2, 4]]))
    assert np.all(got["labels"][:, 0:33] == -1) and np.all(got["labels"][:, 33:] >= 0)
    assert got["raw_costs"][0] == 0.0 and got["raw_costs"][1] > 0 and np.all(got["costs"][[2, 4], 0] <= got["raw_costs"][[2, 4]])


def test_zero_model_is_the_greedy_reading_and_the_lexicon_raw_cost():
    rng = np.random.default_rng(9)
    off = LM.offsets([1, 2, 5, 12, 32, 0, 40])
    cost = LX.make_costs(rng, int(off[-1]))
    cost[3, 7] = cost[3, 20] = cost[3].min()       # a doubled minimum: the first one is read
    got = LM.decode(cost, off, LM.zero_model(), top_k=1)
    first = cost.argmin(axis=1)
    dec = np.repeat(np.arange(len(off) - 1), np.diff(off))
    keep = np.isin(dec, [0, 1, 2, 3, 4])
    assert np.array_equal(got["labels"][0][keep], first[keep]) and np.all(got["labels"][0][~keep] == -1)
    assert np.array_equal(_u64(got["costs"][:5, 0]), _u64(got["raw_costs"][:5]))
    lex = LX.match(cost, off, ["A"], top_k=1)
    assert np.array_equal(_u64(got["raw_costs"]), _u64(lex["raw_costs"]))             # x + 0.0 is exact


def test_bad_inputs_raise():
    T = LM.zero_model()
    for bad in (np.nan, np.inf, -1.0):
        Tb = T.copy()
        Tb[3, 4] = bad
        with pytest.raises(ValueError):
            LM.check_model(Tb)
    for cell in ((63, 0), (0, 63), (62, 62)):
        Tb = T.copy()
        Tb[cell] = 1.0
        with pytest.raises(ValueError):
            LM.check_model(Tb)
    with pytest.raises(ValueError):
        LM.decode(np.full((1, 62), np.nan, np.float32), [0, 1], T)
    with pytest.raises(ValueError):
        LM.decode(np.zeros((1, 62), np.float32), [0, 2], T)


def test_char_lm_table_rows_are_distributions():
    words = ["code", "Code9", "a", "zz", "HELLO", "world", "x1y2"]
    for weight in (1.0, 2.5):
        t = capi.char_lm_table(words, alpha=0.5, weight=weight)
        assert t.shape == (64, 64) and t.dtype == np.float32
        LM.check_model(t)
        p = np.exp(-t.astype(np.float64) / weight)
        assert np.all(np.abs(p[:62, :63].sum(axis=1) - 1.0) < 1e-6)                   # 62 classes and end-of-word
        assert abs(p[62, :62].sum() - 1.0) < 1e-6                                     # begin-of-word: 62 classes
        assert not t[63].any() and not t[:, 63].any() and t[62, 62] == 0


def test_char_lm_table_counts_weight_the_words():
    a = capi.char_lm_table(["ab", "ac"], counts=[3, 1])
    b = capi.char_lm_table(["ab", "ab", "ab", "ac"])
    assert np.array_equal(a, b)
    ia, ib, ic = (LM.CLASS_OF[ch] for ch in "abc")
    assert a[ia, ib] < a[ia, ic] < a[ia, ia]
    want = -np.log((3 + 0.5) / (4 + 63 * 0.5))
    assert a[ia, ib] == np.float32(want)
    assert capi.char_lm_table(["ab"], weight=2.0)[ia, ib] == np.float32(2.0 * -np.log(1.5 / (1 + 63 * 0.5)))


def test_char_lm_table_refuses_a_character_outside_the_alphabet():
    with pytest.raises(capi.OcrError):
        capi.char_lm_table(["ok", "not ok"])
    with pytest.raises(capi.OcrError):
        capi.char_lm_table(["café"])
    with pytest.raises(capi.OcrError):
        capi.char_lm_table(["ab"], counts=[1, 2])
