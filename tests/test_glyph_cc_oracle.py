"""The connected-component glyph oracle (tests/glyph_cc_oracle.py) held to facts that do not come from itself: scipy's labelling, words
whose glyph boxes are known by construction, kerned letters that the column rule fuses, the two limits against the column rule, words
drawn with a real font and the transcriptions of the reference pages.  CPU only; the kernel is held to this oracle bit for bit in
tests/test_gpu_glyphs_cc.py."""
import numpy as np
import pytest

from tests import glyph_cc_oracle as CC
from tests import glyph_oracle as G
from tests.test_glyph_oracle import PIL_WORDS, _blocks_frame, draw_word

BG, INK = 200.0, 40.0


def _label_image(mask):
    """The oracle's components painted into an image: 0 background, k + 1 for the component of the k-th anchor."""
    runs, comps = CC.components(mask)
    lab = CC.label_runs(runs)
    order = {int(r): k + 1 for k, r in enumerate(np.unique(lab))}
    out = np.zeros(mask.shape, np.int64)
    for (y, a0, a1), r in zip(runs.tolist(), lab.tolist()):
        out[y, a0:a1] = order[r]
    return out, comps


def _same_partition(a, b):
    """Two label images describe the same components (labels may be numbered differently)."""
    if not np.array_equal(a > 0, b > 0):
        return False
    pairs = np.unique(np.stack([a[a > 0], b[b > 0]], axis=1), axis=0)
    return len(pairs) == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1]))


@pytest.mark.parametrize("density", [0.05, 0.3, 0.5, 0.7, 0.95])
def test_components_equal_scipy_label_on_random_masks(density):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(int(density * 100))
    for shape in ((1, 1), (1, 70), (33, 1), (17, 64), (40, 129), (64, 65)):
        mask = rng.random(shape) < density
        want, n = ndi.label(mask, structure=np.ones((3, 3), int))
        got, comps = _label_image(mask)
        assert len(comps) == n and _same_partition(got, want)
        for k, c in enumerate(comps):                       # boxes, counts and anchors by the definition
            ys, xs = np.nonzero(got == k + 1)
            assert (c["x0"], c["y0"], c["x1"], c["y1"], c["s"]) == (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1, len(xs))
            assert c["anchor"] == int((ys * shape[1] + xs).min())
        assert [c["anchor"] for c in comps] == sorted(c["anchor"] for c in comps)


def test_components_equal_scipy_label_on_font_words():
    ndi = pytest.importorskip("scipy.ndimage")
    for word in PIL_WORDS:
        img, _, _ = draw_word(word)
        for thr in (64, 128, 250):
            mask = img < thr
            want, n = ndi.label(mask, structure=np.ones((3, 3), int))
            got, comps = _label_image(mask)
            assert len(comps) == n and _same_partition(got, want)


def test_runs_are_in_raster_order_and_touch_diagonally():
    mask = np.array([[1, 1, 0, 0, 1], [0, 0, 1, 1, 0], [1, 0, 0, 0, 1]], bool)
    assert CC.runs_of(mask).tolist() == [[0, 0, 2], [0, 4, 5], [1, 2, 4], [2, 0, 1], [2, 4, 5]]
    _, comps = CC.components(mask)                              # a zigzag held together by corners only, and one pixel two columns off
    assert [(c["x0"], c["y0"], c["x1"], c["y1"], c["s"], c["anchor"]) for c in comps] == [(0, 0, 5, 3, 6, 0), (0, 2, 1, 3, 1, 10)]


def test_block_glyphs_are_recovered_box_for_box():
    blocks = [(12, 8, 17, 20), (19, 10, 22, 19), (25, 8, 33, 21), (36, 14, 37, 16), (40, 9, 46, 20)]
    img = _blocks_frame(30, 60, blocks)
    t, pol, flags, bg, ink, boxes = CC.segment_word_cc(img, 10, 5, 50, 25)
    assert pol == 1 and flags == 0 and (bg, ink) == (np.float32(200), np.float32(40))
    assert boxes == blocks[:3] + blocks[4:]                  # the 1 x 2 speck has 2 ink pixels < min_glyph_pixels = 4
    _, _, _, _, _, boxes = CC.segment_word_cc(img, 10, 5, 50, 25, dict(min_glyph_pixels=2), dict(min_height_pct=0))
    assert boxes == blocks
    _, _, _, _, _, boxes = CC.segment_word_cc(img, 10, 5, 50, 25, dict(min_glyph_pixels=2))   # 2 rows of a 20-row box: under 25 %
    assert boxes == blocks[:3] + blocks[4:]
    assert CC.segment_word_cc(np.full((10, 10), 93.0, np.float32), 1, 1, 9, 9) == (-1, 0, 0, np.float32(0), np.float32(0), [])


def kerned_pair(h=32, w=40):
    """'/' beside '\\' whose column ranges overlap although no pixel of one touches the other -> (frame, the box of each stroke)."""
    img = np.full((h, w), BG, np.float32)
    a = [(y, 16 - (y - 2) // 2 + d) for y in range(2, 22) for d in (0, 1)]        # '/': columns 7 .. 17
    b = [(y, 17 + (y - 8) // 2 + d) for y in range(8, 28) for d in (0, 1)]        # '\': columns 17 .. 27, tucked under the top of '/'
    for y, x in a + b:
        img[y, x] = INK
    boxes = [(min(x for _, x in s), min(y for y, _ in s), max(x for _, x in s) + 1, max(y for y, _ in s) + 1) for s in (a, b)]
    assert boxes[0][2] > boxes[1][0]                                              # the column ranges do overlap
    assert min(max(abs(ya - yb), abs(xa - xb)) for ya, xa in a for yb, xb in b) >= 2   # ... and no pixel touches
    return img, boxes


def test_kerned_pair_is_one_glyph_by_columns_and_two_by_components():
    img, boxes = kerned_pair()
    h, w = img.shape
    assert len(G.segment_word(img, 0, 0, w, h)[5]) == 1
    t, pol, flags, _, _, got = CC.segment_word_cc(img, 0, 0, w, h)
    assert flags == 0 and got == boxes
    # parallel strokes '//' lean over each other the same way
    img2 = np.full((30, 40), BG, np.float32)
    for y in range(4, 26):
        img2[y, 20 - y // 2], img2[y, 26 - y // 2] = INK, INK
    assert len(G.segment_word(img2, 0, 0, 40, 30)[5]) == 1 and len(CC.segment_word_cc(img2, 0, 0, 40, 30)[5]) == 2


def dotted_i(h=30, w=24):
    """An 'i' (stem and dot, columns 10 .. 12) and an 'l' beside it."""
    return _blocks_frame(h, w, [(10, 5, 13, 8), (10, 10, 13, 25), (17, 4, 19, 25)])


def test_i_dot_merges_at_50_and_not_at_0():
    img = dotted_i()
    h, w = img.shape
    assert CC.segment_word_cc(img, 0, 0, w, h)[5] == [(10, 5, 13, 25), (17, 4, 19, 25)]
    assert CC.segment_word_cc(img, 0, 0, w, h, None, dict(merge_overlap_pct=100))[5] == [(10, 5, 13, 25), (17, 4, 19, 25)]
    # never merged: the dot (3 of 30 rows) falls to the height filter; without the filter it is a glyph of its own, before its stem
    assert CC.segment_word_cc(img, 0, 0, w, h, None, dict(merge_overlap_pct=0))[5] == [(10, 10, 13, 25), (17, 4, 19, 25)]
    assert CC.segment_word_cc(img, 0, 0, w, h, None, dict(merge_overlap_pct=0, min_height_pct=0))[5] == \
        [(10, 5, 13, 8), (10, 10, 13, 25), (17, 4, 19, 25)]
    # a partial overlap: 2 of the narrower 4 columns is 50 %, 1 of 4 is not; the group's accumulated range is what counts
    img = _blocks_frame(30, 30, [(5, 5, 9, 12), (7, 14, 15, 25), (13, 3, 17, 12)])
    assert CC.segment_word_cc(img, 0, 0, 30, 30, None, dict(min_height_pct=0))[5] == [(5, 3, 17, 25)]
    assert CC.segment_word_cc(img, 0, 0, 30, 30, None, dict(min_height_pct=0, merge_overlap_pct=51))[5] == \
        [(5, 5, 9, 12), (7, 14, 15, 25), (13, 3, 17, 12)]
    img = _blocks_frame(30, 30, [(5, 5, 9, 12), (7, 14, 15, 25), (14, 3, 18, 12)])
    assert CC.segment_word_cc(img, 0, 0, 30, 30, None, dict(min_height_pct=0))[5] == [(5, 5, 15, 25), (14, 3, 18, 12)]


def test_height_filter():
    blocks = [(2, 2, 6, 22), (8, 10, 12, 15), (14, 10, 18, 16), (20, 21, 24, 22)]       # heights 20, 5, 6, 1 in a 24-row box
    img = _blocks_frame(24, 30, blocks)
    assert CC.segment_word_cc(img, 0, 0, 30, 24)[5] == [blocks[0], blocks[2]]            # 25 % of 24 rows is 6
    assert CC.segment_word_cc(img, 0, 0, 30, 24, None, dict(min_height_pct=0))[5] == blocks
    assert CC.segment_word_cc(img, 0, 0, 30, 24, None, dict(min_height_pct=1))[5] == blocks
    assert CC.segment_word_cc(img, 0, 0, 30, 24, None, dict(min_height_pct=84))[5] == []  # 20 * 100 < 84 * 24
    assert CC.segment_word_cc(img, 0, 0, 30, 24, None, dict(min_height_pct=83))[5] == [blocks[0]]
    assert CC.segment_word_cc(img, 0, 0, 30, 24, None, dict(min_height_pct=100))[5] == []


def test_truncation_at_max_glyphs():
    blocks = [(2 + 4 * k, 2, 4 + 4 * k, 8) for k in range(10)]
    img = _blocks_frame(10, 44, blocks)
    _, _, flags, _, _, boxes = CC.segment_word_cc(img, 0, 0, 44, 10, dict(max_glyphs=4))
    assert flags == CC.FLAG_TRUNCATED and boxes == blocks[:4]
    _, _, flags, _, _, boxes = CC.segment_word_cc(img, 0, 0, 44, 10, dict(max_glyphs=10))
    assert flags == 0 and boxes == blocks
    img[2:3, 42] = INK                                          # a dropped component beyond the cap does not count as truncation
    _, _, flags, _, _, boxes = CC.segment_word_cc(img, 0, 0, 44, 10, dict(max_glyphs=10))
    assert flags == 0 and boxes == blocks


def noise_word(h=64, w=600, seed=7):
    """More than 8192 runs."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((h, w)) < 0.5, INK, BG).astype(np.float32)


def lattice_word(h=50, w=100):
    """Isolated pixels on every second row and column: 1250 components of one run each."""
    img = np.full((h, w), BG, np.float32)
    img[::2, ::2] = INK
    return img


def test_both_limits_fall_back_to_the_column_rule():
    for img, params in ((noise_word(), None), (lattice_word(), None), (lattice_word(), dict(max_glyphs=256, min_glyph_pixels=0))):
        h, w = img.shape
        st = {}
        t, pol, flags, bg, ink, boxes = CC.segment_word_cc(img, 0, 0, w, h, params, None, st)
        ct, cpol, ctrunc, cbg, cink, cboxes = G.segment_word(img, 0, 0, w, h, params)
        assert (t, pol, bg, ink, boxes) == (ct, cpol, cbg, cink, cboxes) and flags == (ctrunc | CC.FLAG_FALLBACK)
        assert st["runs"] > CC.MAX_RUNS or st["components"] > CC.MAX_COMPONENTS
    st = {}
    CC.segment_word_cc(noise_word(), 0, 0, 600, 64, None, None, st)
    assert st["runs"] > 8192
    CC.segment_word_cc(lattice_word(), 0, 0, 100, 50, None, None, st)
    assert st["runs"] <= 8192 and st["components"] == 1250
    assert CC.segment_word_cc(lattice_word(), 0, 0, 100, 50)[2] == 3       # 50 one-column spans: truncated at 32, and the fallback
    # exactly at the limits the component rule still holds: 1024 isolated pixels
    img = np.full((64, 64), BG, np.float32)
    img[::2, ::2] = INK
    CC.segment_word_cc(img, 0, 0, 64, 64, None, None, st)
    assert st["components"] == 1024 and CC.segment_word_cc(img, 0, 0, 64, 64)[2] == 0


@pytest.mark.parametrize("dark", [True, False])
@pytest.mark.parametrize("word", PIL_WORDS)
def test_font_words_split_into_one_glyph_per_character(word, dark):
    img, bbs, solid = draw_word(word, dark)
    t, pol, flags, _, _, boxes = CC.segment_word_cc(img, 5, 5, bbs[-1][2] + 5, 43)
    assert pol == (1 if dark else 2) and flags == 0
    assert len(boxes) == len(word)
    for (bx0, by0, bx1, by1), (gx0, gy0, gx1, gy1), (sx0, sy0, sx1, sy1) in zip(boxes, bbs, solid):
        assert bx0 <= sx0 and by0 <= sy0 and bx1 >= sx1 and by1 >= sy1
        assert gx0 <= bx0 and gy0 <= by0 and bx1 <= gx1 and by1 <= gy1


def test_segment_batch_layout_and_empty_lists():
    img = _blocks_frame(20, 30, [(5, 5, 9, 15), (12, 5, 20, 15)])
    frames = np.stack([img, np.full_like(img, 7.0), img])[:, None]
    rect = [(2, 2), (24, 2), (24, 17), (2, 17)]
    polys = [[rect], [], [rect, [(0, 0), (2, 0), (2, 2), (0, 2)]]]
    seg = CC.segment_cc(frames, polys, [[1.0, 1.0]] * 3)
    assert seg["img_offsets"].tolist() == [0, 1, 1, 3] and seg["word_offsets"].tolist() == [0, 2, 4, 4]
    assert seg["boxes"].tolist() == [[5, 5, 9, 15], [12, 5, 20, 15]] * 2
    assert np.array_equal(seg["word_info"], G.segment(frames, polys, [[1.0, 1.0]] * 3)["word_info"])
    empty = CC.segment_cc(frames[:1], [[]], [[1.0, 1.0]])
    assert empty["word_offsets"].tolist() == [0] and empty["boxes"].shape == (0, 4)


# glyphs per word on the reference pages (ground-truth polygons, in file order; '###' is an unreadable word the count skips)
PAGE_WORDS = ["ENFORCER", "DETROIT", "FIRE", "DEPARTMENT", "BODA", "FURNITURE", "COM", "ISTANBUL", "HOUSE", "###", "LIBERTY", "HARBOUR", "MARINA"]
AXIS_COUNTS = [2, 7, 4, 10, 4, 1, 3, 4, 1, 6, 3, 1, 4]
STRIP_COUNTS = [1, 7, 4, 10, 4, 1, 3, 5, 1, 8, 1, 1, 6]


def _hits(words, counts):
    return sum(len(w) == c for w, c in zip(words, counts) if w != "###")


def test_reference_pages_split_more_words_than_the_column_rule(golden_dir):
    from tests import strip_oracle as S
    from tests.test_gpu_glyphs import load_pages
    frames, polys, adj, words = load_pages(golden_dir)
    flat = [w for page in words for w in page]
    assert flat == PAGE_WORDS
    plan = S.plan(polys, adj)                                      # strips of height 32
    atlas = S.extract(frames, plan)[None, None]
    rects = S.strip_polygons(plan)
    for name, (fr, pl, ad), want in (("axis-aligned", (frames, polys, adj), AXIS_COUNTS), ("strips", (atlas, rects, [[1.0, 1.0]]), STRIP_COUNTS)):
        st = []
        seg = CC.segment_cc(fr, pl, ad, stats=st)
        col = np.diff(G.segment(fr, pl, ad)["word_offsets"]).tolist()
        got = np.diff(seg["word_offsets"]).tolist()
        print(f"\n{name}: (word, column rule, component rule)", list(zip(flat, col, got)),
              f"hits {_hits(flat, col)} -> {_hits(flat, got)} of 12; most runs {max(s['runs'] for s in st)}, components {max(s['components'] for s in st)}")
        assert got == want
        assert _hits(flat, col) == 2 and _hits(flat, got) > 2
        assert not seg["word_info"][:, 3].any()                    # no word truncated, none at a limit
        assert max(s["runs"] for s in st) <= CC.MAX_RUNS and max(s["components"] for s in st) <= CC.MAX_COMPONENTS
    assert _hits(flat, AXIS_COUNTS) == 5 and _hits(flat, STRIP_COUNTS) == 6


def test_params_defaults():
    assert CC.CC_DEFAULTS == dict(merge_overlap_pct=50, min_height_pct=25)
    assert CC.cc_params_with(dict(min_height_pct=3)) == dict(merge_overlap_pct=50, min_height_pct=3)
    assert (CC.MAX_RUNS, CC.MAX_COMPONENTS) == (8192, 1024)
