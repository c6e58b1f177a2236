"""The split oracle (tests/glyph_split_oracle.py) on its drawn frames, with every expected number written out by hand, and the fuzz
generator's coverage.  No GPU."""
import numpy as np
import pytest

from tests import glyph_cc_oracle as GC
from tests import glyph_oracle as GO
from tests import glyph_split_oracle as SO

CASES = {c[0]: c for c in SO.drawn_cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_drawn_case(name):
    _, frames, blk, prm, want, bits = CASES[name]
    got = SO.split(frames, blk, prm)
    assert got["boxes"].tolist() == want and got["word_info"][:, 3].tolist() == bits
    assert np.array_equal(got["word_info"][:, :3], blk["word_info"][:, :3]) and np.array_equal(got["img_offsets"], blk["img_offsets"])
    assert got["word_offsets"][-1] == len(want) == len(got["map"])


def test_the_bridge_is_one_component_and_is_cut_at_column_13():
    _, frames, blk, _, want, _ = CASES["bridge"]
    cc = GC.segment_cc(frames, [[[(0, 0), (39, 23)]]], np.ones((1, 2)))
    assert cc["boxes"].tolist() == blk["boxes"].tolist() == [[4, 6, 22, 18]] and cc["word_info"][0, 2] == 1
    got = SO.split(frames, cc)
    assert got["boxes"].tolist() == want and got["boxes"][0, 2] == 13 and got["map"].tolist() == [[0, 0], [0, 1]]
    # the tie rule: all five columns of the window [11, 15] hold one ink pixel; the distance to c = 13 decides, then the smaller x
    assert SO.cuts_of(np.ones(18, np.int64), 4, 22, 2) == [13]
    cnt = np.ones(18, np.int64)
    cnt[13 - 4] = 2
    assert SO.cuts_of(cnt, 4, 22, 2) == [12]   # 12 and 14 tie in count and distance: the smaller x


def test_pass_through_and_asked_counts():
    _, frames, blk, prm, _, _ = CASES["clip"]
    got = SO.split(frames, blk, prm)
    assert got["asked"].tolist() == [4, 1]
    assert SO.split(frames, blk, dict(aspect_pct=25, max_pieces=1))["boxes"].tolist() == blk["boxes"].tolist()


def test_window_clamps_of_the_rule():
    """With min_piece_w >= 3 no window reaches x0 + 1 or x1 - 1 (c_1 - r >= x0 + 2, c_(n-1) + r <= x1 - 2), so the clamps cannot be met
    through the call; cuts_of applies them all the same, and this holds them on widths the call never passes."""
    assert SO.cuts_of(np.array([0, 5, 1]), 10, 13, 2) == [12]    # c = 11, r = 1: [10, 12] clipped to [11, 12]
    assert SO.cuts_of(np.array([5, 1]), 10, 12, 2) == [11]       # c = 11, r = 1: [10, 12] clipped to [11, 11]
    for gw in range(3, 200):
        for n in range(2, min(4, gw // 3) + 1):
            r = max(1, gw // (4 * n))
            assert (gw // n) - r >= 2 and ((n - 1) * gw) // n + r <= gw - 2


def test_the_fuzz_generator_covers_every_piece_count():
    frames, polys, adj = SO.fuzz_case()
    col = GO.segment(frames, polys, adj, dict(polarity=1))
    cc = GC.segment_cc(frames, polys, adj, dict(polarity=1))
    assert len(col["word_offsets"]) - 1 == 64 and frames.shape == (2, 1, 96, 160)
    widths = np.concatenate([b["boxes"][:, 2] - b["boxes"][:, 0] for b in (col, cc)])
    assert widths.min() <= 3 and widths.max() == 60
    for blk in (col, cc):
        asked = SO.split(frames, blk, dict(max_pieces=4))["asked"]
        assert set(asked.tolist()) == {1, 2, 3, 4}
    assert SO.split(frames, col, dict(max_pieces=1))["boxes"].tolist() == col["boxes"].tolist()
