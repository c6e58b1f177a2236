"""The segmentation lattice's oracle (tests/lattice_oracle.py) held to the enumeration of every (segmentation, classes) pair, to the
character model's oracle at M = 1, and to hand cases; ocr_glyph_spans (host only, through ctypes) against the oracle's span table.  No
GPU."""
import numpy as np
import pytest

from ocr_rs_amd import capi
from tests import char_lm_oracle as CL
from tests import lattice_oracle as LO

u64 = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check_against_enumeration(res, cost, so, po, T, M, K, sc=None, classes=None):
    for w in range(len(po) - 1):
        G = int(po[w + 1] - po[w])
        rows = cost[so[w]:so[w + 1]]
        all_costs, pairs = LO.enumerate_paths(rows, T, G, M, sc, classes)
        want = np.sort(all_costs, kind="stable")[:K]
        assert np.array_equal(u64(res["costs"][w]), u64(want)), (w, G, M, K)
        seen = set()
        for k in range(K):
            seg, cls = LO.hypothesis(res, po, w, k)
            assert sum(seg) == G and len(seg) == len(cls) == res["n_chars"][w, k] and max(seg) <= M
            assert u64(LO.path_cost(rows, T, M, seg, cls, sc)) == u64(res["costs"][w, k]), (w, k, seg, cls)
            seen.add((seg, cls))
        assert len(seen) == K


@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("M", [1, 2, 3])
def test_enumeration_g_1_2_3(M, integer):
    rng = np.random.default_rng(100 + M + 10 * integer)
    cost, so, po, T = LO.make_case(rng, [1, 2, 3], M, integer=integer)
    sc = [0.0, 1.0, 2.0, 0.0] if integer else [0.25, 0.0, 1.5, 0.0]
    for K in (1, 8):
        res = LO.decode(cost, so, po, T, M, K, sc)
        _check_against_enumeration(res, cost, so, po, T, M, K, sc)
        assert np.all(res["costs"][:, 0] <= res["raw_costs"])


def test_enumeration_g4_m4_three_classes():
    rng = np.random.default_rng(7)
    cost, so, po, T = LO.make_case(rng, [4], 4)
    keep = np.array([3, 30, 61])
    big = np.full_like(cost, 1e30)
    big[:, keep] = cost[:, keep]
    for K in (1, 8):
        res = LO.decode(big, so, po, T, 4, K, [0.5, 0.0, 0.25, 1.0])
        _check_against_enumeration(res, big, so, po, T, 4, K, [0.5, 0.0, 0.25, 1.0], classes=keep)
        assert np.all(res["costs"] < 1e29)   # 3 + 2*9 + 9 + 3*27 + 81 pairs avoid the 1e30 classes: more than 8


@pytest.mark.parametrize("K", [1, 2, 8])
def test_m1_is_the_character_model(K):
    rng = np.random.default_rng(11)
    gs = [0, 1, 2, 3, 5, 9, 32, 33]
    off = CL.offsets(gs)
    cost, T = CL.make_costs(rng, int(off[-1])), CL.make_model(rng)
    want = CL.decode(cost, off, T, K)
    got = LO.decode(cost, LO.span_offsets(off, 1), off, T, 1, K)
    assert np.array_equal(off, LO.span_offsets(off, 1))
    assert np.array_equal(u64(got["costs"]), u64(want["costs"])) and np.array_equal(u64(got["raw_costs"]), u64(want["raw_costs"]))
    assert np.array_equal(got["labels"], want["labels"]) and np.array_equal(got["word_flags"], want["word_flags"])
    decoded = np.repeat(want["word_flags"] == 0, gs)
    assert np.all(got["seg_len"][:, decoded] == 1) and np.all(got["seg_len"][:, ~decoded] == 0)
    assert np.array_equal(got["n_chars"][:, 0], np.where(want["word_flags"] == 0, gs, 0))


@pytest.mark.parametrize("M", [1, 2, 4])
def test_prefix_property(M):
    rng = np.random.default_rng(21 + M)
    cost, so, po, T = LO.make_case(rng, [1, 2, 4, 7], M, integer=True, high=3)
    full = LO.decode(cost, so, po, T, M, 8, [1.0, 0.0, 0.0, 2.0])
    for k in range(1, 8):
        part = LO.decode(cost, so, po, T, M, k, [1.0, 0.0, 0.0, 2.0])
        assert np.array_equal(u64(part["costs"]), u64(full["costs"][:, :k]))
        assert np.array_equal(part["labels"], full["labels"][:k]) and np.array_equal(part["seg_len"], full["seg_len"][:k])


def test_seeded_tie_case():
    cost, so, po, T, M = LO.tie_case()
    res = LO.decode(cost, so, po, T, M, 8)
    assert res["ties"] >= 20, res["ties"]
    _check_against_enumeration(res, cost, so[:4], po[:4], T, M, 8)


def test_hand_tie_across_two_segmentations():
    cost, so, po, T, M = LO.hand_tie_case()
    res = LO.decode(cost, so, po, T, M, 8)
    assert res["costs"][0].tolist() == [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    got = [LO.hypothesis(res, po, 0, k) for k in range(8)]
    assert got == [((1, 1), (0, 0)), ((2,), (0,)), ((2,), (1,)),                       # AA in two segments, then A and B merged
                   ((1, 1), (1, 0)), ((1, 1), (2, 0)), ((1, 1), (3, 0)), ((1, 1), (4, 0)), ((1, 1), (5, 0))]   # BA, CA, DA, EA, FA
    assert res["labels"][0].tolist() == [0, 0] and res["labels"][1].tolist() == [0, -1] and res["seg_len"][1].tolist() == [2, 0]


WORDS = ["come", "home", "time", "some", "name", "game", "more", "make", "mine", "moon"]


def test_rn_reads_m_under_a_model_and_rn_with_a_span_cost():
    rows, so, po = LO.rn_case()
    T = capi.char_lm_table(WORDS)
    res = LO.decode(rows, so, po, T, 2, 2)
    assert LO.text(res, po, 0, 0) == "m" and LO.hypothesis(res, po, 0, 0)[0] == (2,)
    assert LO.text(res, po, 0, 1) == "rn"
    res = LO.decode(rows, so, po, T, 2, 2, [0.0, 20.0])
    assert LO.text(res, po, 0, 0) == "rn" and LO.hypothesis(res, po, 0, 0)[0] == (1, 1)
    assert u64(res["costs"][0, 0]) == u64(res["raw_costs"][0])


def test_a_wide_piece_cut_in_two_reads_as_two_letters():
    # the converse: the halves read r and n well, the merged span reads m only fairly; a model of -rn words keeps the cut
    rows, so, po = LO.rn_case()
    rows[2, CL.CLASS_OF["m"]] = 2.0
    T = capi.char_lm_table(["corn", "born", "horn", "torn", "worn", "burn", "turn", "barn"])
    res = LO.decode(rows, so, po, T, 2, 1)
    assert LO.text(res, po, 0) == "rn"
    assert LO.text(LO.decode(rows[:2], LO.span_offsets(po, 1), po, T, 1, 1), po, 0) == "rn"   # M = 1 has no merged span at all


def _piece_block(rng, gs):
    off = CL.offsets(gs)
    n = int(off[-1])
    x0, y0 = rng.integers(0, 50, n), rng.integers(0, 20, n)
    boxes = np.stack([x0, y0, x0 + rng.integers(1, 9, n), y0 + rng.integers(1, 9, n)], axis=1).astype(np.int32)
    nw = len(gs)
    info = np.stack([np.zeros(nw), np.full(nw, 100), np.ones(nw), np.zeros(nw)], axis=1).astype(np.int32)
    levels = rng.uniform(0, 255, (nw, 2)).astype(np.float32)
    return capi.GlyphSet([0, nw], off, info, levels, boxes)


@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_glyph_spans_counts_order_and_boxes(M):
    gs = [0, 1, 2, 5]
    pieces = _piece_block(np.random.default_rng(5), gs)
    sp, tab = capi.glyph_spans(pieces, M)
    want = LO.spans(pieces.word_offsets, pieces.boxes, M)
    assert np.diff(sp.word_offsets).tolist() == [sum(min(M, e) for e in range(1, g + 1)) for g in gs]
    assert np.array_equal(sp.word_offsets, want["span_offsets"]) and np.array_equal(sp.boxes, want["boxes"])
    assert np.array_equal(tab.span_word, want["span_word"]) and np.array_equal(tab.span_end, want["span_end"])
    assert np.array_equal(tab.span_len, want["span_len"]) and np.array_equal(tab.piece_offsets, pieces.word_offsets)
    assert np.array_equal(tab.span_offsets, LO.span_offsets(pieces.word_offsets, M)) and tab.max_span == M
    assert np.array_equal(sp.word_info, pieces.word_info) and np.array_equal(sp.img_offsets, pieces.img_offsets)
    assert np.array_equal(sp.word_levels.view(np.uint32), pieces.word_levels.view(np.uint32))
    if M == 1:   # the piece block array for array
        assert np.array_equal(sp.boxes, pieces.boxes) and np.array_equal(sp.word_offsets, pieces.word_offsets)


def test_glyph_spans_errors():
    pieces = _piece_block(np.random.default_rng(6), [2, 3])
    for M in (0, 5, -1):
        with pytest.raises(capi.OcrError):
            capi.glyph_spans(pieces, M)
    pieces.word_offsets[1] = 4   # decreases behind it
    pieces.word_offsets[2] = 3
    with pytest.raises(capi.OcrError):
        capi.glyph_spans(pieces, 2)
    assert capi.glyph_spans(_piece_block(np.random.default_rng(6), []), 2)[1].n_spans == 0
