"""tests/line_oracle.py (the numpy restatement of ocr_group_lines' rule) pinned to hand-worked answers.  No GPU.  The cases are
built by `cases()` and shared with tests/test_gpu_lines.py, which holds the device to the oracle on every one of them."""
import time

import numpy as np
import pytest

from tests import line_oracle as LO

Q = LO.quad


def two_lines_shuffled():
    # line A at y = 100: words at x = 50, 120, 190; line B at y = 140: x = 60, 130, 200; all 50 x 18; given in shuffled order
    words = {"A0": Q(50, 100, 50, 18), "A1": Q(120, 100, 50, 18), "A2": Q(190, 100, 50, 18),
             "B0": Q(60, 140, 50, 18), "B1": Q(130, 140, 50, 18), "B2": Q(200, 140, 50, 18)}
    names = ["B1", "A2", "B0", "A0", "B2", "A1"]
    return np.array([words[n] for n in names]), names


def two_columns():
    # two columns of three rows, two words a row in each; the columns' inner edges are 300 px apart (16.7 heights: beyond max_gap)
    rows, names = [], []
    for r in range(3):
        for col, x0 in enumerate((100.0, 100.0 + 60 + 50 + 300)):
            for k in range(2):
                rows.append(Q(x0 + 60 * k, 100 + 30 * r, 50, 18))
                names.append((r, col, k))
    return np.array(rows), names


def cases():
    """name -> (quads, img_offsets): every hand case, as the GPU test runs them"""
    out = {}
    q, _ = two_lines_shuffled()
    out["two_lines"] = (q, [0, 6])
    for ang in (0.0, 0.35, -0.35, 0.6):
        out[f"page_{ang:+.2f}"] = (LO.page(6, 8, ang, seed=7)[0], [0, 48])
    q, _ = two_columns()
    out["two_columns"] = (q, [0, len(q)])
    out["tall_at_ratio"] = (np.array([Q(50, 100, 50, 16), Q(120, 100, 50, 32), Q(190, 100, 50, 16)]), [0, 3])
    out["tall_over_ratio"] = (np.array([Q(50, 100, 50, 16), Q(120, 100, 50, 32.5), Q(190, 100, 50, 16)]), [0, 3])
    out["subscript"] = (np.array([Q(50, 100, 50, 20), Q(100, 112, 20, 10), Q(150, 100, 50, 20)]), [0, 3])
    out["ring"] = (LO.ring(), [0, 24])
    out["identical"] = (np.array([Q(50, 100, 40, 16), Q(120, 100, 40, 16), Q(120, 100, 40, 16), Q(190, 100, 40, 16)]), [0, 4])
    out["degenerate"] = (np.array([Q(50, 100, 50, 18), Q(120, 100, 0, 18), Q(125, 100, 50, 0), Q(150, 100, 50, 18), [7.0] * 8]), [0, 5])
    q, _ = two_lines_shuffled()
    out["empty_between"] = (np.concatenate([q, LO.page(2, 3, 0.1, seed=3)[0]]), [0, 6, 6, 12])
    out["no_words"] = (np.zeros((0, 8)), [0, 0, 0])
    return out


def test_two_lines_of_three_words_in_shuffled_order():
    q, names = two_lines_shuffled()
    res = LO.group(q, [0, 6])
    assert [[names[k] for k in line] for line in LO.lines_of(res, 0)] == [["A0", "A1", "A2"], ["B0", "B1", "B2"]]
    assert res["img_offsets"].tolist() == [0, 2] and res["line_offsets"].tolist() == [0, 3, 6] and not res["word_flags"].any()
    # centres 70 apart, widths 50: g = 20, heights 18 -> 20 / 18; heads carry 0
    assert res["gaps"].tolist() == [0.0, 20 / 18, 20 / 18] * 2


@pytest.mark.parametrize("angle", [0.0, 0.35, -0.35, 0.6])
def test_tilted_page_comes_out_as_its_rows_in_order(angle):
    q, row, col = LO.page(6, 8, angle, seed=7)
    res = LO.group(q, [0, 48])
    lines = LO.lines_of(res, 0)
    assert len(lines) == 6
    rows_seen = []
    for line in lines:
        assert len(line) == 8 and len({int(row[k]) for k in line}) == 1 and [int(col[k]) for k in line] == list(range(8))
        rows_seen.append(int(row[line[0]]))
    assert rows_seen == list(range(6))      # heads by (Cy, Cx): the left margin descends row by row at any tilt below a right angle
    assert not res["word_flags"].any() and sorted(res["order"].tolist()) == list(range(48))


def test_two_columns_300_px_apart_stay_two_lines_a_row():
    q, names = two_columns()
    res = LO.group(q, [0, len(q)])
    got = [[names[k] for k in line] for line in LO.lines_of(res, 0)]
    # rows interleave by height: left column's line, then the right column's, row by row (out of scope: column detection)
    want = [[(r, col, 0), (r, col, 1)] for r in range(3) for col in range(2)]
    assert got == want


def test_a_word_twice_the_height_links_at_the_ratio_and_not_just_over_it():
    c = cases()
    at = LO.group(*c["tall_at_ratio"])
    assert LO.lines_of(at, 0) == [[0, 1, 2]]
    assert at["gaps"].tolist() == [0.0, 20 / 32, 20 / 32]       # g over the taller of the two heights
    over = LO.group(*c["tall_over_ratio"])
    # 32.5 > 2 * 16: the tall word links to nobody, and the small ones do not reach past it (g = 140 - 50 = 90 > 3 * 16)
    assert LO.lines_of(over, 0) == [[0], [1], [2]] and over["gaps"].tolist() == [0.0, 0.0, 0.0]


def test_a_subscript_off_the_line_is_a_line_of_its_own():
    res = LO.group(*cases()["subscript"])
    # |b| = 12 against line_tol * hmin = 5: the subscript links to nobody; its neighbours are 100 apart, g = 50 <= 3 * 20
    assert LO.lines_of(res, 0) == [[0, 2], [1]]
    assert res["gaps"].tolist() == [0.0, 2.5, 0.0]


def test_twenty_four_words_on_a_circle_are_one_line_cut_at_word_0():
    res = LO.group(*cases()["ring"])
    assert LO.lines_of(res, 0) == [list(range(24))]
    assert res["word_flags"].tolist() == [2] + [0] * 23
    assert res["gaps"][0] == 0.0 and np.all(res["gaps"][1:] > 0)


def test_identical_quads_break_ties_by_index():
    res = LO.group(*cases()["identical"])
    # words 1 and 2 coincide: 0's right is the smaller index 1, 3's left is the smaller index 1; neither of 1 and 2 is right of the
    # other (a = 0), so 2 is alone and sorts behind the line by index only after (Cy, Cx): its centre is to the right of word 0's
    assert LO.lines_of(res, 0) == [[0, 1, 3], [2]]
    assert res["ties"] >= 2


def test_zero_width_and_zero_height_quads_are_isolated():
    res = LO.group(*cases()["degenerate"])
    assert res["word_flags"].tolist() == [0, 1, 1, 0, 1]
    assert LO.lines_of(res, 0) == [[4], [0, 3], [1], [2]]        # the point (7, 7) first, then by (Cy, Cx): x = 50, 120, 125
    assert res["gaps"].tolist() == [0.0, 0.0, 50 / 18, 0.0, 0.0]


def test_an_empty_image_between_two_full_ones():
    q, off = cases()["empty_between"]
    res = LO.group(q, off)
    assert res["img_offsets"].tolist() == [0, 2, 2, 4]
    assert [sorted(sum(LO.lines_of(res, b), [])) for b in range(3)] == [list(range(6)), [], list(range(6, 12))]
    alone = LO.group(q[6:], [0, 6])
    assert (alone["order"] + 6).tolist() == res["order"][6:].tolist() and alone["gaps"].tolist() == res["gaps"][6:].tolist()


def test_a_batch_with_no_words():
    res = LO.group(*cases()["no_words"])
    assert res["img_offsets"].tolist() == [0, 0, 0] and res["line_offsets"].tolist() == [0]
    assert res["order"].size == 0 and res["gaps"].size == 0 and res["word_flags"].size == 0


def test_integer_grid_fuzz_has_ties():
    assert LO.group(LO.fuzz(257, seed=11, grid=True), [0, 257])["ties"] > 0


def test_4096_words_take_about_a_second():
    t0 = time.perf_counter()
    res = LO.group(LO.fuzz(4096, seed=5), [0, 4096])
    assert sorted(res["order"].tolist()) == list(range(4096))
    assert time.perf_counter() - t0 < 20.0      # (about 1.5 s on one core; the bound only catches a quadratic Python loop)
