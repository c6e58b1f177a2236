"""The glyph segmentation oracle (tests/glyph_oracle.py) held to facts that do not come from itself: Otsu's definition evaluated exactly,
synthetic words whose glyph boxes are known by construction, and words drawn glyph by glyph with a real font.  CPU only; the kernels
are held to this oracle bit for bit in tests/test_gpu_glyphs.py."""
from fractions import Fraction

import numpy as np
import pytest

from tests import glyph_oracle as G


def _otsu_exact(hist):
    """Otsu by the definition, exact rationals: argmax over valid t of W0*W1*(mu1 - mu0)^2, ties to the smaller t."""
    best, bt = None, -1
    for t in range(255):
        w0, w1 = sum(hist[: t + 1]), sum(hist[t + 1:])
        if w0 == 0 or w1 == 0:
            continue
        mu0 = Fraction(sum(q * h for q, h in enumerate(hist[: t + 1])), w0)
        mu1 = Fraction(sum(q * h for q, h in enumerate(hist[t + 1:], start=t + 1)), w1)
        sc = w0 * w1 * (mu1 - mu0) ** 2
        if best is None or sc > best:
            best, bt = sc, t
    return bt, best


def _random_hist(rng, kind):
    h = np.zeros(256, np.int64)
    if kind == "sparse":
        idx = rng.choice(256, size=int(rng.integers(2, 8)), replace=False)
        h[idx] = rng.integers(1, 50, size=len(idx))
    elif kind == "bimodal":
        q = np.concatenate([rng.normal(rng.uniform(20, 100), 12, 300), rng.normal(rng.uniform(150, 235), 15, int(rng.integers(20, 600)))])
        h = np.bincount(np.clip(q, 0, 255).astype(np.int64), minlength=256)
    else:
        h = rng.integers(0, 4, size=256)
    return h


@pytest.mark.parametrize("kind", ["sparse", "bimodal", "dense"])
def test_otsu_equals_the_exact_definition(kind):
    rng = np.random.default_rng({"sparse": 1, "bimodal": 2, "dense": 3}[kind])
    for _ in range(40):
        h = _random_hist(rng, kind)
        t, W0, S0, W1, S1 = G.otsu(h)
        et, best = _otsu_exact(h.tolist())
        assert t == et, (t, et)
        assert W0 == int(h[: t + 1].sum()) and W1 == int(h[t + 1:].sum())
        assert S0 == int((h[: t + 1] * np.arange(t + 1)).sum()) and S1 == int((h * np.arange(256)).sum()) - S0


def test_otsu_ties_go_to_the_smaller_threshold_and_flat_histograms_have_none():
    h = np.zeros(256, np.int64)
    h[10], h[200] = 7, 7              # every t in 10..199 splits the same way: same score
    assert G.otsu(h)[0] == 10
    h = np.zeros(256, np.int64)
    h[0], h[255] = 3, 3               # the same at the ends of the range
    assert G.otsu(h)[0] == 0
    for v in (0, 17, 255):
        h = np.zeros(256, np.int64)
        h[v] = 100
        assert G.otsu(h)[0] == -1


def test_quantise_truncates_and_maps_nan_to_zero():
    v = np.array([-1.0, -0.0, 0.5, 1.99, 254.9, 255.0, 300.0, np.nan, np.inf, -np.inf], np.float32)
    assert G.quantise(v).tolist() == [0, 0, 0, 1, 254, 255, 255, 0, 255, 0]


def _rect(x0, y0, x1, y1):
    """A polygon (original pixels, adjust 1) whose crop box is exactly [x0, x1) x [y0, y1)."""
    return [(x0, y0), (x1 - 1, y0), (x1 - 1, y1 - 1), (x0, y1 - 1)]


def _blocks_frame(h, w, blocks, bg=200.0, ink=40.0):
    img = np.full((h, w), bg, np.float32)
    for x0, y0, x1, y1 in blocks:
        img[y0:y1, x0:x1] = ink
    return img


def test_word_box_is_the_crop_box_rounded_outwards():
    polys = [[[(3, 4), (10, 4), (10, 9), (3, 9)]]]
    assert G.word_boxes(polys, [[1.0, 1.0]], 50, 60) == [(0, 3, 4, 11, 10)]
    assert G.word_boxes(polys, [[1.5, 0.5]], 50, 60) == [(0, 4, 2, 16, 6)]     # x 4.5 .. 16.0, y 2.0 .. 5.5
    assert G.word_boxes([[[(0, 0), (100, 100)]]], [[1.0, 1.0]], 20, 30) == [(0, 0, 0, 30, 20)]   # clamped to the frame
    with pytest.raises(ValueError):
        G.word_boxes([[[(0, 0), (4096, 1024)]]], [[1.0, 1.0]], 1100, 5000)     # 4097 x 1025 pixels > 2^22


def test_synthetic_blocks_are_recovered_box_for_box():
    blocks = [(12, 8, 17, 20), (19, 10, 22, 19), (25, 8, 33, 21), (36, 14, 37, 16), (40, 9, 46, 20)]
    img = _blocks_frame(30, 60, blocks)
    t, pol, trunc, bg, ink, boxes = G.segment_word(img, 10, 5, 50, 25)
    assert pol == 1 and trunc == 0 and 40 <= t < 200
    assert (bg, ink) == (np.float32(200), np.float32(40))
    assert boxes == blocks[:3] + blocks[4:]      # the 1 x 2 speck has 2 ink pixels < min_glyph_pixels = 4
    _, _, _, _, _, boxes = G.segment_word(img, 10, 5, 50, 25, dict(min_glyph_pixels=2))
    assert boxes == blocks
    _, _, _, _, _, boxes = G.segment_word(img, 10, 5, 50, 25, dict(min_col_ink=10))   # only columns with >= 10 ink pixels count
    assert boxes == [(12, 8, 17, 20), (25, 8, 33, 21), (40, 9, 46, 20)]


def test_inverted_word_auto_picks_light_ink_and_forced_polarity_obeys():
    blocks = [(5, 5, 9, 15), (12, 5, 20, 15)]
    img = 255.0 - _blocks_frame(20, 30, blocks)
    t, pol, _, bg, ink, boxes = G.segment_word(img, 0, 0, 30, 20)
    assert pol == 2 and boxes == blocks and (bg, ink) == (np.float32(55), np.float32(215))
    t, pol, _, bg, ink, boxes = G.segment_word(img, 0, 0, 30, 20, dict(polarity=1))   # dark ink forced: the background is the "glyph"
    assert pol == 1 and (bg, ink) == (np.float32(215), np.float32(55)) and boxes == [(0, 0, 30, 20)]


def test_auto_polarity_tie_takes_dark_ink():
    img = np.full((4, 8), 10.0, np.float32)
    img[:, 4:] = 250.0                # 16 dark, 16 light pixels
    _, pol, _, bg, ink, boxes = G.segment_word(img, 0, 0, 8, 4)
    assert pol == 1 and (bg, ink) == (np.float32(250), np.float32(10)) and boxes == [(0, 0, 4, 4)]


@pytest.mark.parametrize("value", [0.0, 93.7, 255.0, 400.0, np.nan])
def test_flat_box_has_no_threshold_and_no_glyphs(value):
    img = np.full((10, 10), value, np.float32)
    assert G.segment_word(img, 1, 1, 9, 9) == (-1, 0, 0, np.float32(0), np.float32(0), [])


def test_truncation_at_max_glyphs():
    blocks = [(2 + 4 * k, 2, 4 + 4 * k, 8) for k in range(10)]
    img = _blocks_frame(10, 44, blocks)
    _, _, trunc, _, _, boxes = G.segment_word(img, 0, 0, 44, 10, dict(max_glyphs=4))
    assert trunc == 1 and boxes == blocks[:4]
    _, _, trunc, _, _, boxes = G.segment_word(img, 0, 0, 44, 10, dict(max_glyphs=10))
    assert trunc == 0 and boxes == blocks
    # a dropped span beyond the cap does not count as truncation
    img[2:3, 42] = 40.0
    _, _, trunc, _, _, boxes = G.segment_word(img, 0, 0, 44, 10, dict(max_glyphs=10))
    assert trunc == 0 and boxes == blocks


def _font():
    from PIL import features, ImageFont
    if not features.check("freetype2"):
        pytest.skip("PIL without FreeType")
    return ImageFont.load_default(size=22)


def draw_word(word, dark_on_light=True, gap=3, x=10, y=10, size=(300, 48)):
    """word drawn glyph by glyph (PIL's built-in FreeType font, `gap` pixels between glyph boxes) -> (H x W f32 frame, the
    getbbox of every glyph in frame pixels, the solid-ink box (value < 64 on the dark-on-light image) of every glyph)."""
    from PIL import Image, ImageDraw
    font = _font()
    img = Image.new("L", size, 255)
    d = ImageDraw.Draw(img)
    bbs, solid = [], []
    for ch in word:
        l, t, r, b = font.getbbox(ch)
        one = Image.new("L", size, 255)
        ImageDraw.Draw(one).text((x - l, y), ch, font=font, fill=0)
        d.text((x - l, y), ch, font=font, fill=0)
        ys, xs = np.nonzero(np.asarray(one) < 64)
        solid.append((int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1))
        bbs.append((x, y + t, x + (r - l), y + b))
        x += (r - l) + gap
    a = np.asarray(img, np.float32)
    return (a if dark_on_light else 255.0 - a), bbs, solid


PIL_WORDS = ["HOUSE", "Istanbul", "ocr2026", "Wm8gQ"]


@pytest.mark.parametrize("dark", [True, False])
@pytest.mark.parametrize("word", PIL_WORDS)
def test_font_words_split_into_one_glyph_per_character(word, dark):
    img, bbs, solid = draw_word(word, dark)
    t, pol, trunc, _, _, boxes = G.segment_word(img, 5, 5, bbs[-1][2] + 5, 43)
    assert pol == (1 if dark else 2) and trunc == 0
    assert len(boxes) == len(word)
    for (bx0, by0, bx1, by1), (gx0, gy0, gx1, gy1), (sx0, sy0, sx1, sy1) in zip(boxes, bbs, solid):
        # the glyph box holds the character's solid ink and lies inside its font box (getbbox counts the side bearings too)
        assert bx0 <= sx0 and by0 <= sy0 and bx1 >= sx1 and by1 >= sy1
        assert gx0 <= bx0 and gy0 <= by0 and bx1 <= gx1 and by1 <= gy1


def test_segment_batch_layout_and_empty_lists():
    img = _blocks_frame(20, 30, [(5, 5, 9, 15), (12, 5, 20, 15)])
    frames = np.stack([img, np.full_like(img, 7.0), img])[:, None]
    polys = [[_rect(2, 2, 25, 18)], [], [_rect(2, 2, 25, 18), _rect(0, 0, 3, 3)]]
    seg = G.segment(frames, polys, [[1.0, 1.0]] * 3)
    assert seg["img_offsets"].tolist() == [0, 1, 1, 3]
    assert seg["word_offsets"].tolist() == [0, 2, 4, 4]
    assert seg["word_info"].tolist() == [[0, seg["word_info"][0, 1], 1, 0], [2, seg["word_info"][0, 1], 1, 0], [2, -1, 0, 0]]
    assert seg["boxes"].tolist() == [[5, 5, 9, 15], [12, 5, 20, 15]] * 2
    empty = G.segment(frames[:1], [[]], [[1.0, 1.0]])
    assert empty["word_offsets"].tolist() == [0] and empty["boxes"].shape == (0, 4) and G.glyph_crops(frames[:1], empty).shape == (0, 784)


def test_glyph_crop_is_centred_aspect_preserving_and_inverts():
    img = _blocks_frame(40, 40, [(10, 5, 20, 35)])          # a 10 x 30 bar: s = 30 / 20 = 1.5
    frames = img[None, None]
    seg = G.segment(frames, [[_rect(5, 2, 30, 38)]], [[1.0, 1.0]])
    assert seg["boxes"].tolist() == [[10, 5, 20, 35]]
    crop = G.glyph_crops(frames, seg).reshape(28, 28)
    assert crop.min() == 0.0 and crop.max() == 1.0
    assert np.array_equal(crop, crop[:, ::-1]) and np.array_equal(crop, crop[::-1, :])   # centred both ways
    rows, cols = np.nonzero(crop > 0.5)
    assert rows.min() == 4 and rows.max() == 23 and cols.min() == 11 and cols.max() == 16   # 20 rows tall, ~6.7 columns wide
    inv = G.glyph_crops(frames, seg, dict(ink_high=0)).reshape(28, 28)
    assert np.array_equal(inv, (np.float32(1) - crop).astype(np.float32))
    big = G.glyph_crops(frames, seg, dict(glyph_box=28)).reshape(28, 28)
    assert np.count_nonzero(big > 0.5) > np.count_nonzero(crop > 0.5)


def test_glyph_crop_reads_only_inside_the_glyph_box():
    img = _blocks_frame(30, 30, [(10, 10, 14, 20)])
    img[0:30, 15:30] = 40.0                                  # ink right next to the glyph box must not leak in
    frames = img[None, None]
    seg = dict(img_offsets=np.array([0, 1], np.int32), word_offsets=np.array([0, 1], np.int32),
               word_info=np.array([[0, 100, 1, 0]], np.int32), word_levels=np.array([[200.0, 40.0]], np.float32),
               boxes=np.array([[10, 10, 14, 20]], np.int32))
    a = G.glyph_crops(frames, seg)
    img2 = _blocks_frame(30, 30, [(10, 10, 14, 20)])
    b = G.glyph_crops(img2[None, None], seg)
    assert np.array_equal(a, b)
    # values beyond the levels clamp to [0, 1]; NaN reads as background
    img3 = img2.copy()
    img3[10:20, 10:14] = -50.0
    img3[12, 11] = np.nan
    c = G.glyph_crops(img3[None, None], seg)
    assert c.min() == 0.0 and c.max() == 1.0 and not np.isnan(c).any()


def test_params_defaults():
    assert G.DEFAULTS == dict(polarity=0, min_col_ink=1, min_glyph_pixels=4, max_glyphs=32, glyph_box=20, ink_high=1)
    assert G.params_with(dict(max_glyphs=3)) == dict(G.DEFAULTS, max_glyphs=3)
