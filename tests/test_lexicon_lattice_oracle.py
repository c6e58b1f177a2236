"""The oracle of the joint lexicon and lattice search (tests/lexicon_lattice_oracle.py) held to the enumeration of every alignment
path, to the lexicon oracle at M = 1, to the length rule at its edges and to hand cases with every number written out.  No GPU."""
import numpy as np
import pytest

from tests import lexicon_lattice_oracle as O
from tests import lexicon_oracle as LX

u64 = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


def _path_sum_integer(res, po, w, k, G, so_w, cost, words, M, ins, dele, sc, fold):
    """the alignment's cost from its arrays: exact for whole-number costs, where the order of the summation does not matter"""
    sub = O._fold(cost, fold)
    cls = LX.classes(words[int(res["entries"][w, k])])
    p0 = int(po[w])
    total = float(res["n_ins"][w, k]) * ins
    covered = 0
    for p in range(p0, p0 + G):
        m = int(res["seg_len"][k, p])
        if m > 0:
            i = p - p0
            total += sc[m - 1] + sub[so_w + O.row_of(i + m, m, M), cls[int(res["seg_char"][k, p])]]
            covered += m
        elif m == -1:
            total += dele
            covered += 1
    assert covered == G
    return total


# 2 x 3 x 50 = 300 random cases, G <= 4, L <= 3, M <= 3: the oracle's cost is the minimum over every alignment path, in every bit
@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("M", [1, 2, 3])
def test_cost_equals_the_full_enumeration(M, integer):
    rng = np.random.default_rng(500 + M + 10 * integer)
    for case in range(50):
        G = int(rng.integers(1, 5))
        words = LX.random_words(rng, 6, 1, 3)
        po = O.offsets([G])
        so = O.span_offsets(po, M)
        cost = LX.make_costs(rng, int(so[-1]), integer=integer)
        ins, dele = (float(rng.integers(0, 4)), float(rng.integers(0, 4))) if integer else (float(rng.uniform(0, 3)), float(rng.uniform(0, 3)))
        sc = [float(x) for x in (rng.integers(0, 3, 4) if integer else rng.uniform(0, 1.5, 4))]
        fold = int(rng.integers(0, 2))
        res = O.match(cost, so, po, words, M, ins, dele, sc, 8, fold, 8)
        assert res["n_candidates"][0] == 6 and np.all(res["entries"][0, :6] >= 0) and np.all(res["entries"][0, 6:] == -1)
        sub = O._fold(cost, fold)
        want = sorted((O.brute_force(sub, LX.classes(wd), G, M, ins, dele, sc), k) for k, wd in enumerate(words))
        assert np.array_equal(u64(res["costs"][0, :6]), u64([c for c, _ in want])), (case, G)
        assert res["entries"][0, :6].tolist() == [k for _, k in want]
        if integer:
            for k in range(6):
                assert _path_sum_integer(res, po, 0, k, G, 0, cost, words, M, ins, dele, sc, fold) == res["costs"][0, k]
                assert res["n_ins"][0, k] + np.count_nonzero(res["seg_len"][k] > 0) == len(words[int(res["entries"][0, k])])


# M = 1 with zero span_cost is tests/lexicon_oracle.match in every output: 5 seeds x 6 words x 200 entries
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_m1_is_the_lexicon_oracle(seed):
    cost, off, words = LX.fuzz(seed, 200, [0, 1, 3, 6, 9, 33], min_len=1, max_len=12, integer=seed == 5)
    prm = dict(ins_cost=3.25, del_cost=2.5, max_len_diff=seed % 3, fold_case=seed % 2, top_k=1 + 7 * (seed % 2))
    want = LX.match(cost, off, words, **prm)
    got = O.match(cost, O.span_offsets(off, 1), off, words, max_span=1, **prm)
    assert np.array_equal(off, O.span_offsets(off, 1))
    for name in ("entries", "n_candidates", "word_flags"):
        assert np.array_equal(got[name], want[name]), name
    for name in O.F64_ARRAYS:
        assert np.array_equal(u64(got[name]), u64(want[name])), name
    assert got["ties"] == want["ties"] and set(want["word_flags"].tolist()) >= {0, 1, 2}
    assert np.all(np.isin(got["seg_len"], (-1, 0, 1)))


@pytest.mark.parametrize("M", [1, 2, 4])
def test_prefix_property(M):
    cost, so, po, words = O.fuzz(31 + M, 150, [1, 2, 4, 7], M, 1, 9, integer=True, high=3)
    full = O.match(cost, so, po, words, M, top_k=8, span_cost=[1.0, 0.0, 0.0, 2.0])
    for k in range(1, 8):
        part = O.match(cost, so, po, words, M, top_k=k, span_cost=[1.0, 0.0, 0.0, 2.0])
        assert np.array_equal(part["entries"], full["entries"][:, :k]) and np.array_equal(u64(part["costs"]), u64(full["costs"][:, :k]))
        assert np.array_equal(part["seg_len"], full["seg_len"][:k]) and np.array_equal(part["seg_char"], full["seg_char"][:k])
        assert np.array_equal(part["n_ins"], full["n_ins"][:, :k]) and np.array_equal(u64(part["raw_costs"]), u64(full["raw_costs"]))


def _one_per_length(lo, hi):
    return ["a" * L for L in range(lo, hi + 1)]


def test_length_rule_edges():
    words = _one_per_length(1, 32)                       # entry k has k + 1 characters
    def admitted(G, M, d):
        po = O.offsets([G])
        so = O.span_offsets(po, M)
        res = O.match(np.ones((int(so[-1]), 62), np.float32), so, po, words, M, max_len_diff=d, top_k=8)
        assert O.len_range(G, M, d) == (max(1, -(-G // M) - d), min(32, G + d))
        return int(res["n_candidates"][0]), O.len_range(G, M, d)
    assert admitted(8, 4, 0) == (7, (2, 8))              # ceil(8 / 4) = 2 .. 8
    assert admitted(1, 4, 2) == (3, (1, 3))              # G = 1: the lower edge stops at 1
    assert admitted(1, 1, 0) == (1, (1, 1))
    assert admitted(32, 1, 2) == (3, (30, 32))           # L = 32: the upper edge stops at 32
    assert admitted(32, 4, 0) == (25, (8, 32))
    assert admitted(31, 2, 8) == (25, (8, 32))
    # the entries of a word at the edges are exactly the admitted lengths
    po = O.offsets([8])
    so = O.span_offsets(po, 4)
    res = O.match(np.ones((int(so[-1]), 62), np.float32), so, po, words, 4, max_len_diff=0, top_k=8)
    assert sorted(res["entries"][0].tolist()) == [-1, 1, 2, 3, 4, 5, 6, 7]
    # no admissible length: flag 4, no candidates, the raw cost still summed
    res = O.match(np.ones((int(so[-1]), 62), np.float32), so, po, ["a"], 4, max_len_diff=0)
    assert res["word_flags"].tolist() == [4] and res["n_candidates"].tolist() == [0] and res["entries"].tolist() == [[-1]]
    assert res["costs"].tolist() == [[np.inf]] and res["raw_costs"].tolist() == [2.0] and not res["seg_len"].any()


def test_flags_and_raw_costs_of_words_that_are_not_matched():
    gs, M = [0, 33, 2], 2
    po = O.offsets(gs)
    so = O.span_offsets(po, M)
    cost = np.full((int(so[-1]), 62), 2.0, np.float32)
    cost[::2, 7] = 0.5
    res = O.match(cost, so, po, ["ab", "abc"], M, top_k=2, span_cost=[0.25, 0.0])
    assert res["word_flags"].tolist() == [1, 2, 0] and res["n_candidates"].tolist() == [0, 0, 2]
    assert res["raw_costs"][0] == 0.0 and res["raw_costs"][1] > 0 and np.all(res["entries"][:2] == -1) and np.all(np.isinf(res["costs"][:2]))
    assert not res["seg_len"][:, :33].any() and np.all(res["seg_char"][:, :33] == -1)


HAND = O.hand_cases()


def _run(name):
    cost, so, po, words, prm = HAND[name]
    return O.match(cost, so, po, words, **prm)


def test_hand_rn_reads_as_com_over_the_span():
    # pieces c o r n; r and n cost 1.0 each (a cut m), the span of both reads m at 0.5: com = 0 + 0 + 0.5, corn = 0 + 0 + 1 + 1
    r = _run("rn_span")
    assert r["entries"].tolist() == [[1, 0]] and r["costs"].tolist() == [[0.5, 2.0]] and r["raw_costs"].tolist() == [0.5]
    assert r["seg_len"].tolist() == [[1, 1, 2, 0], [1, 1, 1, 1]] and r["seg_char"].tolist() == [[0, 1, 2, -1], [0, 1, 2, 3]]
    assert r["n_ins"].tolist() == [[0, 0]] and r["n_candidates"].tolist() == [2]
    assert O.segments(r, [0, 4], 0, 0) == [(0, 1, 0), (1, 1, 1), (2, 2, 2)]


def test_hand_rn_reads_as_corn_with_the_span_cost_raised():
    # span_cost[1] = 3.0 on the two-piece span: com = 0 + 0 + (3 + 0.5), corn stays 2.0, and the free segmentation is the singles
    r = _run("rn_span_cost")
    assert r["entries"].tolist() == [[0, 1]] and r["costs"].tolist() == [[2.0, 3.5]] and r["raw_costs"].tolist() == [2.0]
    assert r["seg_len"].tolist() == [[1, 1, 1, 1], [1, 1, 2, 0]]


def test_hand_m1_needs_a_deletion_or_an_insertion():
    # the same pieces without spans: com pays a substitution (6) and a deleted piece (4); the walk takes n as the m and deletes r
    r = _run("rn_m1")
    assert r["entries"].tolist() == [[0, 1]] and r["costs"].tolist() == [[2.0, 10.0]]
    assert r["seg_len"][1].tolist() == [1, 1, -1, 1] and r["seg_char"][1].tolist() == [0, 1, -1, 2] and r["n_ins"].tolist() == [[0, 0]]
    # the converse: three pieces c o m against corn pay a substitution (6) and an inserted character (4)
    r = _run("m_cut_m1")
    assert r["entries"].tolist() == [[1, 0]] and r["costs"].tolist() == [[0.0, 10.0]]
    assert r["seg_len"][1].tolist() == [1, 1, 1] and r["seg_char"][1].tolist() == [0, 1, 3] and r["n_ins"].tolist() == [[0, 1]]


def test_hand_inserted_character():
    # pieces c m against com: the o has no piece, 4.0; the greedy pieces cost nothing
    r = _run("inserted")
    assert r["costs"].tolist() == [[4.0]] and r["raw_costs"].tolist() == [0.0]
    assert r["seg_len"].tolist() == [[1, 1]] and r["seg_char"].tolist() == [[0, 2]] and r["n_ins"].tolist() == [[1]]


def test_hand_fold_on_and_off():
    # pieces C o m: folded, com costs 0 and Cam one miss (6); unfolded, com misses the C (6) and ties with Cam, the lower index first
    on, off = _run("fold_on"), _run("fold_off")
    assert on["entries"].tolist() == [[0, 1]] and on["costs"].tolist() == [[0.0, 6.0]] and on["ties"] == 0
    assert off["entries"].tolist() == [[0, 1]] and off["costs"].tolist() == [[6.0, 6.0]] and off["ties"] == 1


def test_hand_trace_tie_takes_the_one_piece_segment():
    # two pieces against "a": piece 2 reads a at 0 behind a deleted piece 1 (4 + 0), the span of both reads a at 4 (0 + 4): both 4.0;
    # the walk tries m = 1 first, so piece 2 is the a and piece 1 is deleted
    r = _run("trace_tie")
    assert r["costs"].tolist() == [[4.0]] and r["trace_ties"] == 1
    assert r["seg_len"].tolist() == [[-1, 1]] and r["seg_char"].tolist() == [[-1, 0]] and r["n_ins"].tolist() == [[0]]


def test_seeded_tie_case_holds_rank_ties_and_trace_ties():
    fz, prm = O.TIE_CASE
    cost, so, po, words = O.fuzz(**fz)
    res = O.match(cost, so, po, words, **prm)
    assert res["ties"] >= 20, res["ties"]
    assert res["trace_ties"] >= 1, res["trace_ties"]
    assert np.all(res["costs"] == np.floor(res["costs"]))       # whole numbers: the equal costs are exact


def test_refusals():
    cost, so, po, words, _ = HAND["rn_span"]
    for bad in (dict(max_span=0), dict(max_span=5), dict(top_k=0), dict(top_k=9), dict(max_len_diff=9), dict(fold_case=2),
                dict(ins_cost=-1.0), dict(del_cost=np.nan), dict(span_cost=[0.0, -1.0]), dict(span_cost=[np.inf])):
        with pytest.raises(ValueError):
            O.match(cost, so, po, words, **{"max_span": 2, **bad})
    with pytest.raises(ValueError):
        O.match(cost, so, po, words, max_span=3)                # the span count of M = 2
    neg = cost.copy()
    neg[3, 5] = -1.0
    with pytest.raises(ValueError):
        O.match(neg, so, po, words, max_span=2)
