"""tests/word_break_oracle.py (the plain-Python restatement of ocr_break_words' rule) pinned to hand-worked answers.  No GPU.  The
expected breaks are spelled out; the fixed mode is also held to a second, vectorised restatement on seeded random words."""
import os
import re

import numpy as np

from tests import word_break_oracle as WB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def row(gaps, h=20, w=10, x=0, y=0):
    """glyphs of width w and height h on one baseline with the given gaps between neighbours"""
    boxes = [[x, y, x + w, y + h]]
    for g in gaps:
        x = boxes[-1][2] + g
        boxes.append([x, y, x + w, y + h])
    return boxes


def breaks_at(boxes, params=None):
    brk, pct, info = WB.break_source(boxes, params)
    return [i for i, b in enumerate(brk) if b], info


def test_one_wide_gap_among_narrow_ones_is_the_adaptive_split():
    # sorted gaps 2 2 2 3 3 9: the best cut is in front of the 9 (c = 5, L = 3, T = 9); 900 >= 25 * 20 and 900 >= 200 * 3
    at, info = breaks_at(row([2, 3, 2, 9, 2, 3, 2]))
    assert at == [4] and info == (20, 2, 9, 0)
    brk, pct, _ = WB.break_source(row([2, 3, 2, 9, 2, 3, 2]))
    assert pct[4] == 9 * 100 // 20
    # the fixed rule on the same word: 9 * 100 >= 35 * 20 = 700, 3 * 100 < 700; the threshold is ceil(700 / 100) = 7
    at, info = breaks_at(row([2, 3, 2, 9, 2, 3, 2]), {"mode": 0})
    assert at == [4] and info == (20, 1, 7, 0)


def test_fixed_threshold_hit_exactly_and_missed_by_one_pixel():
    # hw 20, space_pct 35: gap * 100 >= 700, so 7 breaks and 6 does not
    assert breaks_at(row([7, 6], h=20), {"mode": 0}) == ([1], (20, 1, 7, 0))
    # hw 21: 735 / 100 -> the smallest breaking gap is 8 (800 >= 735, 700 < 735)
    assert breaks_at(row([7, 8], h=21), {"mode": 0}) == ([2], (21, 1, 8, 0))


def test_separation_passed_exactly_and_missed_by_one():
    # L = 5: T = 10 passes sep_pct 200 exactly (1000 >= 1000), T = 9 misses (900 < 1000) and the fixed rule decides: 9 and 10 both
    # break at hw 20 (>= 7), 5 does not
    assert breaks_at(row([5, 5, 10, 5])) == ([3], (20, 2, 10, 0))
    assert breaks_at(row([5, 5, 9, 5])) == ([3], (20, 1, 7, 0))
    # missed with a tall word: the fixed rule breaks nowhere (hw 40: 14 px)
    assert breaks_at(row([5, 5, 9, 5], h=40)) == ([], (40, 1, 14, 0))
    # min_space_pct: T = 4 at hw 20 is 400 < 500, refused although it is 4 x L
    assert breaks_at(row([1, 1, 4, 1])) == ([], (20, 1, 7, 0))
    assert breaks_at(row([1, 1, 5, 1])) == ([3], (20, 2, 5, 0))


def test_all_gaps_equal_have_no_valid_cut():
    assert breaks_at(row([3, 3, 3, 3, 3])) == ([], (20, 1, 7, 0))
    # ... and letter-spaced: every gap is above the fixed share, a break at every letter (named out of scope in the header)
    assert breaks_at(row([9, 9, 9, 9]))[0] == [1, 2, 3, 4]


def test_letter_spaced_text_is_read_by_the_adaptive_rule():
    # letter gaps 8 > 7 px: the fixed rule would break everywhere; the adaptive rule cuts at the 20s only
    gaps = [8, 8, 8, 20, 8, 8, 20, 8]
    assert breaks_at(row(gaps)) == ([4, 7], (20, 2, 20, 0))
    assert breaks_at(row(gaps), {"mode": 0})[0] == list(range(1, 9))


def test_prefix_maximum_with_nested_and_overlapping_boxes():
    # glyph 1 is nested in glyph 0, glyph 2 starts 4 px after glyph 0's right edge but 24 after glyph 1's
    boxes = [[0, 0, 30, 20], [5, 5, 10, 15], [34, 0, 44, 20], [40, 0, 60, 20], [75, 0, 85, 20]]
    assert WB.gaps_of(boxes) == [0, 0, 4, 0, 15]
    at, info = breaks_at(boxes)
    # sorted gaps 0 0 4 15: c = 3 wins (T = 15, L = 4), accepted; heights 20 10 20 20 20 -> hw 20
    assert at == [4] and info == (20, 2, 15, 0)
    # boxes in any order: a glyph left of everything before it has gap 0
    assert WB.gaps_of([[50, 0, 60, 20], [0, 0, 10, 20], [70, 0, 80, 20]]) == [0, 0, 10]


def test_height_tie_at_the_upper_median():
    # heights 10 10 30 30: index 2 of the sorted list is 30; 10 10 10 30: 10
    def h_of(hs):
        return WB.break_source([[12 * i, 0, 12 * i + 10, h] for i, h in enumerate(hs)], {"mode": 0})[2][0]
    assert h_of([30, 10, 10, 30]) == 30 and h_of([10, 30, 10, 10]) == 10 and h_of([10, 30]) == 30 and h_of([7]) == 7
    assert h_of([5, 9, 7]) == 7


def test_smallest_words():
    assert WB.break_source([]) == ([], [], (0, 0, 0, 0))
    assert breaks_at(row([])) == ([], (20, 1, 7, 0))
    assert breaks_at(row([30])) == ([1], (20, 1, 7, 0))
    # G = 3: two gaps are below min_gaps 3, the fixed rule decides although the split would be clean
    assert breaks_at(row([2, 6])) == ([], (20, 1, 7, 0))
    assert breaks_at(row([2, 30])) == ([2], (20, 1, 7, 0))
    # G = 4: the first where the adaptive rule applies at the default - 6 is no fixed break (600 < 700) and is an adaptive one
    assert breaks_at(row([2, 6, 2])) == ([2], (20, 2, 6, 0))
    assert breaks_at(row([2, 6, 2]), {"min_gaps": 4}) == ([], (20, 1, 7, 0))


def test_too_many_glyphs_are_flagged_and_not_broken():
    boxes = row([30] * 256)
    assert len(boxes) == 257
    brk, pct, info = WB.break_source(boxes)
    assert not any(brk) and info == (0, 0, 0, 2)
    assert sum(WB.break_source(boxes[:256])[0]) == 255


def test_score_tie_goes_to_the_smaller_cut():
    # gaps 0 1 2: c = 1 scores (3*1 - 0*2)^2 / 2 = 4.5, c = 2 scores (2*2 - 1*1)^2 / 2 = 4.5: c = 1 wins, T = 1, L = 0
    s, c = WB.adaptive_split([2, 0, 1], 3)
    assert s == [0, 1, 2] and c == 1
    at, info = breaks_at(row([2, 0, 1], h=4))   # 100 >= 25 * 4 and 100 >= 200 * 0
    assert at == [1, 3] and info == (4, 2, 1, 0)


def test_gap_pct_divides_with_truncation_and_uses_int64():
    big = 1 << 22
    boxes = [[0, 0, 1, 1], [big - 1, 0, big, 1]]
    brk, pct, info = WB.break_source(boxes, {"mode": 0})
    assert brk == [False, True] and pct[1] == (big - 2) * 100 and info == (1, 1, 1, 0)
    assert WB.break_source(row([7], h=3), {"mode": 0})[1][1] == 233


def _fixed_vectorised(boxes, off, space_pct):
    """the fixed mode once more, without loops over glyphs: -> break flag per glyph"""
    boxes = np.asarray(boxes, np.int64)
    out = np.zeros(len(boxes), bool)
    for k in range(len(off) - 1):
        b = boxes[off[k]:off[k + 1]]
        if len(b) < 2 or len(b) > 256:
            continue
        hw = np.sort(b[:, 3] - b[:, 1])[len(b) // 2]
        reach = np.maximum.accumulate(b[:, 2])[:-1]
        gap = np.maximum(0, b[1:, 0] - reach)
        out[off[k] + 1:off[k + 1]] = gap * 100 >= space_pct * hw
    return out


def random_block(rng, lengths, coord=400, n_images=None):
    """a glyph block of len(lengths) words with boxes drawn left to right with jitter, overlaps and a few wide gaps"""
    boxes = []
    for G in lengths:
        x = int(rng.integers(0, coord))
        for _ in range(G):
            w, h = int(rng.integers(1, 30)), int(rng.integers(4, 40))
            y = int(rng.integers(0, 50))
            boxes.append([x, y, x + w, y + h])
            x = max(0, x + w + int(rng.choice([-8, 0, 1, 2, 3, 3, 4, 12, 25])))
    nw = len(lengths)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    if n_images is None:
        n_images = 1
    cuts = np.sort(rng.integers(0, nw + 1, n_images - 1)) if n_images > 1 else np.zeros(0, np.int64)
    img = np.concatenate([[0], cuts, [nw]]).astype(np.int32)
    info = np.stack([np.searchsorted(img[1:], np.arange(nw), side="right"), rng.integers(0, 255, nw), rng.integers(1, 3, nw), np.zeros(nw, np.int64)],
                    axis=1).astype(np.int32) if nw else np.zeros((0, 4), np.int32)
    levels = rng.random((nw, 2)).astype(np.float32)
    return {"img_offsets": img, "word_offsets": off, "word_info": info, "word_levels": levels,
            "boxes": np.asarray(boxes, np.int32).reshape(-1, 4)}


def test_fixed_mode_against_a_vectorised_restatement():
    rng = np.random.default_rng(5)
    lengths = rng.integers(0, 12, 3000).tolist()
    blk = random_block(rng, lengths)
    counts = {}
    for pct in (35, 1, 1000):
        words, breaks = WB.break_words(blk, {"mode": 0, "space_pct": pct})
        got = np.zeros(len(blk["boxes"]), bool)
        got[words["word_offsets"][:-1][words["word_offsets"][:-1] < len(got)]] = True
        got[blk["word_offsets"][:-1][blk["word_offsets"][:-1] < len(got)]] = False     # a source word's first glyph is no break
        want = _fixed_vectorised(blk["boxes"], blk["word_offsets"], pct)
        assert np.array_equal(got, want), pct
        counts[pct] = int(want.sum())
    assert counts[1] > counts[35] > 100 and counts[35] > counts[1000]


def test_glyphs_are_conserved_and_the_block_is_ordinary():
    rng = np.random.default_rng(6)
    lengths = rng.integers(0, 20, 400).tolist() + [257, 256, 0]
    blk = random_block(rng, lengths, n_images=5)
    for params in (None, {"mode": 0}):
        words, breaks = WB.break_words(blk, params)
        wo, so = words["word_offsets"], breaks["sub_offsets"]
        assert wo[0] == 0 and wo[-1] == len(blk["boxes"]) and (np.diff(wo) >= 0).all()
        assert np.array_equal(words["boxes"], blk["boxes"])
        assert len(so) == len(lengths) + 1 and (np.diff(so) >= 1).all() and so[-1] == len(wo) - 1
        for k in range(len(lengths)):
            # the sub-words of source word k tile its glyph range, in order
            assert wo[so[k]] == blk["word_offsets"][k] and wo[so[k + 1]] == blk["word_offsets"][k + 1]
            assert (breaks["source"][so[k]:so[k + 1]] == k).all() and breaks["gap_pct"][so[k]] == 0
            if lengths[k] > 0:
                assert (np.diff(wo[so[k]:so[k + 1] + 1]) >= 1).all()
        assert np.array_equal(words["word_info"], blk["word_info"][breaks["source"]])
        assert np.array_equal(words["word_levels"], blk["word_levels"][breaks["source"]])
        assert np.array_equal(words["img_offsets"], so[blk["img_offsets"]])
        assert breaks["source_info"][-3].tolist() == [0, 0, 0, 2] and breaks["source_info"][-1].tolist() == [0, 0, 0, 0]
    assert len(wo) - 1 > len(lengths)


def test_the_header_declares_the_call():
    hdr = open(os.path.join(ROOT, "include", "ocr_amd.h")).read()
    declared = set(re.findall(r"\b(ocr_[a-z0-9_]+)\s*\(", hdr))
    assert {"ocr_break_default_params", "ocr_break_words", "ocr_word_breaks_free"} <= declared
    assert re.search(r"#define OCR_BREAK_MAX_GLYPHS %d\b" % WB.MAX_GLYPHS, hdr)
    from ocr_rs_amd import capi
    assert capi.BREAK_MAX_GLYPHS == WB.MAX_GLYPHS and {n for n, _ in capi.BreakParams._fields_} == set(WB.DEFAULTS) | {"reserved"}
