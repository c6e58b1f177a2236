"""tests/column_oracle.py (the numpy restatement of ocr_group_columns' rule) held to what the rule is for: two-column pages come out
as heading, left column, right column, footer.  No GPU.  The hand cases are built by `cases()` and shared with
tests/test_gpu_columns.py, which holds the device to the oracle on every one of them.

The page generator (column_oracle.columns_page): 5 words a row, word heights 16..18, row pitch 30, ragged right edges, the last row
of each column half length, words shuffled; a heading or footer spans the page and stands two row pitches from the columns.  Two
pitches, not one: at one pitch a full-width line is within block_reach of both columns' nearest lines and joins whichever is nearer
by the jitter (the documented consequence of the rule, pinned by test_a_heading_at_one_pitch_joins_a_column)."""
import itertools

import numpy as np
import pytest

from tests import column_oracle as CO
from tests import line_oracle as LO

Q = LO.quad
GUTTERS, ANGLES = (2, 3, 5), (0.0, 0.1, -0.3, 0.6)
ROWS, EXTRAS, SEEDS = ((8, 8), (8, 5), (4, 9), (3, 3)), (0, 1, 2), (1, 2, 3)


def reading(res, labels, b=0):
    """the labels of image b's words in the order the result reads them"""
    return [[[labels[k] for k in line] for line in block] for block in CO.blocks_of(res, b)]


def flat(blocks):
    return [lab for block in blocks for line in block for lab in line]


def grid_rows(rows, h=12.0):
    """rows of (y, [(x0, x1), ...]) on integers -> quads, in the order given"""
    return np.array([Q((x0 + x1) / 2, y, x1 - x0, h) for y, spans in rows for x0, x1 in spans])


def tie_down():
    # row 0: two words 60 apart (5 heights: a wide gap, and eligible); row 1: three words 20 apart (eligible, not wide).  The gap of
    # row 0 has both gaps of row 1 below it at a = 24 (a tie of next), and the line of row 1 has both lines of row 0 above it at
    # a = 24 (a tie of prev)
    return grid_rows([(0, [(0, 40), (100, 140)]), (24, [(0, 40), (60, 80), (100, 140)])])


def tie_up():
    # the same upside down: the ties are of prev among the gaps and of next among the lines
    return grid_rows([(0, [(0, 40), (60, 80), (100, 140)]), (24, [(0, 40), (100, 140)])])


def narrow_gutter():
    # two columns of four rows, two words a row each, the gutter 30 px = 2.5 heights: eligible (>= 1.5), not wide (<= 3)
    return grid_rows([(24 * r, [(0, 40), (50, 90), (120, 160), (170, 210)]) for r in range(4)])


def cases():
    """name -> (quads, img_offsets, params): every hand case, as the GPU test runs them"""
    out = {"tie_down": (tie_down(), [0, 5], None), "tie_up": (tie_up(), [0, 5], None),
           "narrow_gutter": (narrow_gutter(), [0, 16], None), "narrow_gutter_min_rows_5": (narrow_gutter(), [0, 16], dict(min_rows=5)),
           "ring": (LO.ring(), [0, 24], None), "two_sections": (CO.two_sections()[0], [0, len(CO.two_sections()[0])], None),
           "three_columns": (CO.columns_page(3, 0.1, (6, 6, 6), 0, 1, n_cols=3)[0], [0, 84], None),
           "degenerate": (np.array([Q(50, 100, 50, 18), Q(120, 100, 0, 18), Q(125, 100, 50, 0), Q(150, 100, 50, 18), [7.0] * 8]), [0, 5], None),
           "no_words": (np.zeros((0, 8)), [0, 0, 0], None)}
    q = CO.columns_page(2, 0.1, (4, 4), 2, 1)[0]
    out["empty_between"] = (np.concatenate([q, tie_down()]), [0, len(q), len(q), len(q) + 5], None)
    for ang in (0.0, 0.35, -0.35, 0.6):
        out[f"page_{ang:+.2f}"] = (LO.page(6, 8, ang, 7, pitch_x=60)[0], [0, 48], None)
    return out


@pytest.mark.parametrize("gutter,angle", list(itertools.product(GUTTERS, ANGLES)))
def test_two_column_pages_read_heading_left_right_footer(gutter, angle):
    """36 of the 432 pages per case: every combination of rows, heading / footer and seed"""
    n = 0
    for rows, extras, seed in itertools.product(ROWS, EXTRAS, SEEDS):
        q, labels = CO.columns_page(gutter, angle, rows, extras, seed)
        res = CO.group(q, [0, len(q)])
        blocks = reading(res, labels)
        assert flat(blocks) == sorted(labels), (rows, extras, seed)
        # heading, left column, right column and footer are a block each, every row a line
        assert [sorted({lab[0] for line in block for lab in line}) for block in blocks] == [[p] for p in sorted({lab[0] for lab in labels})]
        assert all(len({lab[1] for lab in line}) == 1 for block in blocks for line in block)
        assert sum(len(block) for block in blocks) == sum(rows) + extras
        assert sorted(res["order"].tolist()) == list(range(len(q)))
        n += 1
    assert n == 36


def test_the_line_rule_alone_merges_or_interleaves_these_pages():
    q, labels = CO.columns_page(2, 0.0, (8, 8), 0, 1)
    got = [labels[k] for k in LO.group(q, [0, len(q)])["order"]]
    assert got != sorted(labels)
    q, labels = CO.columns_page(5, 0.0, (8, 8), 0, 1)
    got = [labels[k] for k in LO.group(q, [0, len(q)])["order"]]
    assert got != sorted(labels)


@pytest.mark.parametrize("angle", [0.0, 0.35, -0.35, 0.6])
def test_a_single_column_page_keeps_the_lines_of_the_line_rule_in_one_block(angle):
    for seed in range(5):
        q = LO.page(6, 8, angle, seed, pitch_x=60)[0]
        res, want = CO.group(q, [0, 48]), LO.group(q, [0, 48])
        assert res["order"].tolist() == want["order"].tolist() and res["line_offsets"].tolist() == want["line_offsets"].tolist()
        assert res["block_offsets"].tolist() == [0, 6] and res["img_offsets"].tolist() == [0, 1] and res["block_levels"].tolist() == [0]
        assert np.array_equal(res["gaps"], want["gaps"]) and not res["word_flags"].any() and not res["line_flags"].any()


def test_two_sections_with_a_heading_between_them_read_section_by_section():
    q, labels = CO.two_sections()
    res = CO.group(q, [0, len(q)])
    blocks = reading(res, labels)
    assert flat(blocks) == sorted(labels)
    assert [sorted({lab[0] for line in block for lab in line}) for block in blocks] == [[1], [2], [3], [4], [5]]   # L1 R1 heading L2 R2
    assert res["block_levels"].tolist() == [0, 1, 2, 3, 4]


def test_three_columns_read_left_to_right():
    q, labels = CO.columns_page(3, 0.1, (6, 6, 6), 0, 1, n_cols=3)
    res = CO.group(q, [0, len(q)])
    assert flat(reading(res, labels)) == sorted(labels) and res["block_levels"].tolist() == [0, 1, 2]
    assert (res["word_flags"] == 4).sum() == 12         # two gutters of six rows


def test_a_heading_at_one_pitch_joins_a_column():
    """the documented consequence: within block_reach, a full-width heading is the head line of one of the columns' blocks"""
    q, labels = CO.columns_page(3, 0.0, (4, 4), 0, 1)
    top = min(q[:, 1::2].min(axis=1))
    x0, x1 = q[:, 0::2].min(), q[:, 0::2].max()
    heading = np.array([Q(x, top - 30.0 + 8.5, 36.0, 17.0) for x in np.arange(x0 + 18, x1 - 18, 44.0)])
    res = CO.group(np.concatenate([heading, q]), [0, len(heading) + len(q)])
    blocks = CO.blocks_of(res, 0)
    assert len(blocks) == 2 and sorted(len(b) for b in blocks) == [4, 5]
    assert [b for b in blocks if len(b) == 5][0][0] == list(range(len(heading)))


def test_the_ring_is_one_line_in_one_block():
    res = CO.group(LO.ring(), [0, 24])
    assert CO.blocks_of(res, 0) == [[list(range(24))]]
    assert res["word_flags"].tolist() == [2] + [0] * 23 and res["block_levels"].tolist() == [0] and res["line_flags"].tolist() == [0]


def test_ties_of_next_and_prev_go_to_the_smaller_index():
    down = CO.group(tie_down(), [0, 5])
    # words 0 1 / 2 3 4.  Gaps by right word: 1 (wide), 3 and 4.  next[gap 1] ties between gaps 3 and 4; prev[line 2] between lines 0, 1
    assert down["ties"][1] == 1 and down["ties"][2] == 1
    assert CO.blocks_of(down, 0) == [[[0], [2, 3, 4]], [[1]]]          # line 2 went to the smaller index, line 0
    assert down["word_flags"].tolist() == [0] * 5                       # (the cut in front of word 1 is a wide one: no flag)
    assert down["gaps"].tolist() == [0.0, 0.0, 20 / 12, 20 / 12, 0.0]
    assert down["block_levels"].tolist() == [0, 0]                      # word 1 lies inside block 0's box: TL.y ties, TL.x decides
    up = CO.group(tie_up(), [0, 5])
    assert up["ties"][1] == 1 and up["ties"][2] == 1
    assert CO.blocks_of(up, 0) == [[[0, 1, 2], [3]], [[4]]]


def test_min_rows_above_the_row_count_leaves_only_the_wide_cuts():
    q = narrow_gutter()
    res = CO.group(q, [0, 16])
    assert (res["word_flags"] == 4).nonzero()[0].tolist() == [2, 6, 10, 14]
    assert CO.blocks_of(res, 0) == [[[4 * r, 4 * r + 1] for r in range(4)], [[4 * r + 2, 4 * r + 3] for r in range(4)]]
    assert res["block_levels"].tolist() == [0, 1]
    off = CO.group(q, [0, 16], dict(min_rows=5))
    assert not off["word_flags"].any() and CO.blocks_of(off, 0) == [[[4 * r + k for k in range(4)] for r in range(4)]]
    # a 50 px gutter is wide (> 3 heights): cut whatever min_rows says
    wide = grid_rows([(24 * r, [(0, 40), (50, 90), (140, 180), (190, 230)]) for r in range(2)])
    res = CO.group(wide, [0, 8], dict(min_rows=5))
    assert not res["word_flags"].any() and CO.blocks_of(res, 0) == [[[0, 1], [4, 5]], [[2, 3], [6, 7]]]


def test_isolated_words_are_blocks_of_their_bounding_box():
    q, off, _ = cases()["degenerate"]
    res = CO.group(q, off)
    assert res["word_flags"].tolist() == [0, 1, 1, 0, 1]
    k = [b[0][0] for b in CO.blocks_of(res, 0)].index(1)                # the block of word 1: zero width, 18 high at x = 120
    assert res["block_quads"].reshape(-1, 8)[k].tolist() == [120, 91, 120, 91, 120, 109, 120, 109]


def test_an_empty_image_between_two_full_ones_and_no_words_at_all():
    q, off, _ = cases()["empty_between"]
    res = CO.group(q, off)
    assert res["img_offsets"].tolist()[1] == res["img_offsets"].tolist()[2]
    alone = CO.group(q[off[2]:], [0, 5])
    assert (alone["order"] + off[2]).tolist() == res["order"][off[2]:].tolist()
    none = CO.group(np.zeros((0, 8)), [0, 0, 0])
    assert none["img_offsets"].tolist() == [0, 0, 0] and none["block_offsets"].tolist() == [0] and none["line_offsets"].tolist() == [0]
    assert all(none[k].size == 0 for k in ("order", "gaps", "word_flags", "line_flags", "block_levels", "block_quads"))


def test_integer_grid_fuzz_has_ties_in_every_stage_and_fuzz_reaches_the_level_cap():
    res = CO.group(CO.grid_fuzz(257, seed=7), [0, 257])
    assert all(t > 0 for t in res["ties"]) and (res["word_flags"] & 4).any()
    assert CO.group(LO.fuzz(1025, seed=1125), [0, 1025])["block_levels"].max() == 63
