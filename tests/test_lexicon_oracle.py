"""The lexicon oracle (tests/lexicon_oracle.py) against a brute force that shares none of its code, and the hand cases of the rule
(include/ocr_amd.h, ocr_lexicon_match) with what each must give.  No GPU."""
import functools
import itertools

import numpy as np
import pytest

from tests import lexicon_oracle as LX


def brute(cost, word, ins, dele, fold):
    """D[G][M] by the memoised recursion over the last step of an alignment, in Python floats (IEEE f64, one rounding per operation)."""
    cls = [LX.CLASS_OF[ch] for ch in word]
    G, M = cost.shape[0], len(cls)

    def s(i, j):
        v = float(cost[i, cls[j]])
        if fold and cls[j] < 52:
            v = min(v, float(cost[i, cls[j] + 26 if cls[j] < 26 else cls[j] - 26]))
        return v

    @functools.lru_cache(maxsize=None)
    def D(i, j):
        if i == 0 and j == 0:
            return 0.0
        if j == 0:
            return D(i - 1, 0) + dele
        if i == 0:
            return D(0, j - 1) + ins
        return min(D(i - 1, j - 1) + s(i - 1, j - 1), min(D(i - 1, j) + dele, D(i, j - 1) + ins))
    return D(G, M)


def all_alignments(cost, word, ins, dele):
    """The minimum over every monotone alignment, enumerated: for whole-number costs every sum is exact, so the order does not matter."""
    cls = [LX.CLASS_OF[ch] for ch in word]
    G, M = cost.shape[0], len(cls)
    best = np.inf
    for k in range(min(G, M) + 1):           # k substituted pairs
        for gi in itertools.combinations(range(G), k):
            for mj in itertools.combinations(range(M), k):
                tot = (G - k) * dele + (M - k) * ins + sum(float(cost[i, cls[j]]) for i, j in zip(gi, mj))
                best = min(best, tot)
    return best


@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("fold", [0, 1])
def test_oracle_against_brute_force(integer, fold):
    rng = np.random.default_rng(11 + 2 * fold + integer)
    words = LX.random_words(rng, 40, 1, 5)
    Gs = [1, 2, 3, 4, 5, 3, 2]
    off = np.concatenate([[0], np.cumsum(Gs)])
    cost = LX.make_costs(rng, int(off[-1]), integer=integer)
    ins, dele = (2.0, 3.0) if integer else (1.75, 0.6)
    got = LX.match(cost, off, words, ins_cost=ins, del_cost=dele, max_len_diff=8, fold_case=fold, top_k=8)
    assert got["n_candidates"].tolist() == [40] * len(Gs)
    for w, G in enumerate(Gs):
        want = sorted((brute(cost[off[w]:off[w + 1]], words[k], ins, dele, fold), k) for k in range(40))[:8]
        assert got["entries"][w].tolist() == [k for _, k in want]
        assert np.array_equal(got["costs"][w].view(np.uint64), np.array([c for c, _ in want]).view(np.uint64))
        if integer and not fold:
            for r in range(3):
                k = int(got["entries"][w, r])
                if G <= 4 and len(words[k]) <= 4:
                    assert got["costs"][w, r] == all_alignments(cost[off[w]:off[w + 1]], words[k], ins, dele)
    if integer:
        assert got["ties"] > 0


CASES = LX.hand_cases()


def run(name):
    cost, off, words, params = CASES[name]
    return LX.match(cost, off, words, **params), words


def test_greedy_reading_in_the_list():
    r, _ = run("greedy_in_list")
    assert r["entries"][0].tolist() == [0, 2] and r["raw_costs"][0] == 5.0
    assert r["costs"][0, 0].view(np.uint64) == r["raw_costs"][0].view(np.uint64)
    assert r["costs"][0, 1] == 3.0 + 6.0 + 6.0


def test_missed_and_spurious_glyph():
    r, _ = run("missed_glyph")
    assert r["entries"][0].tolist() == [1, 0, 2] and r["costs"][0].tolist() == [r["raw_costs"][0] + 4.0, 6.0, 8.0]
    r, _ = run("spurious_glyph")
    assert r["entries"][0].tolist() == [0, 1] and r["costs"][0].tolist() == [r["raw_costs"][0] + 3.0, 3.0 + 6.0]


def test_fold_case():
    on, _ = run("fold_on")
    off, _ = run("fold_off")
    assert on["entries"][0].tolist() == [0, 1] and on["costs"][0].tolist() == [0.0, 12.0]
    assert off["entries"][0].tolist() == [1, 0] and off["costs"][0].tolist() == [12.0, 24.0]


def test_max_len_diff():
    r0, _ = run("len_diff_0")
    r2, _ = run("len_diff_2")
    assert r0["n_candidates"].tolist() == [0] and r0["word_flags"].tolist() == [4] and r0["entries"].tolist() == [[-1]] and np.isinf(r0["costs"][0, 0])
    assert r2["n_candidates"].tolist() == [2] and r2["word_flags"].tolist() == [0] and r2["entries"].tolist() == [[0]] and r2["costs"][0, 0] == 4.0


def test_duplicates_and_equal_costs_by_index():
    r, _ = run("duplicates")
    assert r["entries"][0].tolist() == [0, 1, 3] and r["costs"][0].tolist() == [0.0, 0.0, 0.0] and r["ties"] >= 2
    r, _ = run("equal_costs")
    assert r["entries"][0].tolist() == [2, 0, 1] and r["costs"][0].tolist() == [4.0, 6.0, 6.0] and r["ties"] == 1


def test_top_k_past_the_candidates():
    r, _ = run("top_k_past_candidates")
    assert r["entries"][0].tolist() == [0, 1] + [-1] * 6 and r["costs"][0, :2].tolist() == [0.0, 4.0] and np.all(np.isposinf(r["costs"][0, 2:]))
    assert r["n_candidates"].tolist() == [2]


def test_flags():
    r, _ = run("flags")
    assert r["word_flags"].tolist() == [1, 2, 4, 1] and r["n_candidates"].tolist() == [0, 0, 0, 0]
    assert r["raw_costs"].tolist() == [0.0, 0.0, 0.0, 0.0] and np.all(r["entries"] == -1) and np.all(np.isposinf(r["costs"]))
    cost = LX.costs_for_text("A" * 33, hit=1.0)
    assert LX.match(cost, [0, 33], ["A"])["raw_costs"].tolist() == [33.0]     # a word of more than 32 glyphs is summed like any other


def test_invalid_inputs_raise():
    c = LX.costs_for_text("AB")
    for bad in (np.nan, np.inf, -1.0):
        d = c.copy()
        d[1, 3] = bad
        with pytest.raises(ValueError):
            LX.match(d, [0, 2], ["AB"])
    with pytest.raises(ValueError):
        LX.match(c, [0, 1], ["AB"])
    with pytest.raises(ValueError):
        LX.match(c, [0, 2], ["A" * 33])


def test_glyph_costs_restated():
    lg = (np.random.default_rng(5).standard_normal((50, 62)) * 8).astype(np.float32)
    c = LX.glyph_costs(lg)
    p = np.exp(-c.astype(np.float64))
    assert c.dtype == np.float32 and np.all(c >= 0) and np.allclose(p.sum(axis=1), 1.0, atol=1e-5)
    lg[0] = 0
    lg[0, 7] = 60
    assert LX.glyph_costs(lg)[0, 7] == 0.0


@pytest.mark.parametrize("name", sorted(LX.TIE_CASES))
def test_seeded_cases_have_the_tie_counts_the_gpu_tests_claim(name):
    fa, params, want_ties = LX.TIE_CASES[name]
    cost, off, words = LX.fuzz(**fa)
    r = LX.match(cost, off, words, **params)
    assert (r["ties"] > 0) if want_ties else (r["ties"] == 0)
    assert np.all(r["n_candidates"] >= params["top_k"])      # full rows: every rank is a real candidate
