"""ORACLE (test infrastructure) for the BUILD-DEFINED glyph segmentation rule: detected word -> glyph boxes -> 28 x 28 glyph crops.

The reference lists "Character Segmentation" in its pipeline (README.md:20-26, pipeline.png) but never built it, so there is no
reference behaviour to match: this file restates the rule of include/ocr_amd.h (ocr_segment_glyphs, ocr_extract_glyph_crops) and
ocr-rs_amd/csrc/glyphs.hip must equal it bit for bit.  Kept in tests/ (like tests/ctc_beam_oracle.py) because oracle/ is frozen;
the word box comes from oracle/crop_oracle.py, read-only.

For every polygon of the batch, in polygon order (a polygon is a word):
  1. word box: crop_boxes() of oracle/crop_oracle.py (f32 frame coordinates) -> X0 = floor(x0), X1 = ceil(x1), Y0 = floor(y0),
     Y1 = ceil(y1), clamped to the frame, half-open; more than 2^22 pixels is an error;
  2. q = (int)min(max(v, 0), 255) (truncation; NaN -> 0) of the raw 0..255 f32 frame value v;
  3. Otsu on the 256-bin histogram of q over the box: for t in 0..254 class 0 is q <= t (count W0, int64 sum S0), class 1 the rest;
     t is valid when both classes are non-empty and scores d*d / ((double)W0 * (double)W1), d = (double)(S1*W0 - S0*W1) (exact
     int64); the highest score wins, ties to the smaller t; no valid t (a flat box) -> t = -1 and no glyphs;
  4. polarity 0 (auto): ink is the smaller class, dark on a tie; 1 forces dark ink (q <= t), 2 light ink (q > t);
  5. mu0 = (float)((double)S0 / W0), mu1 likewise; bg = the non-ink class's mean, ink = the ink class's mean;
  6. cnt[x] = ink pixels of column x over [Y0, Y1); a column is ink when cnt[x] >= min_col_ink; each maximal run of ink columns is a
     span, left to right; a span with fewer than min_glyph_pixels ink pixels is dropped;
  7. a glyph box is [xs, xe) x [first ink row of the span, last ink row + 1);
  8. at most max_glyphs spans per word are kept; a word that had more is flagged truncated.
Glyph crop, 28 x 28 f32 (ink high), aspect-preserving and centred: s = (float)max(gw, gh) / (float)glyph_box,
cx = (float)(x0 + x1) * 0.5f, sx = (cx + (((float)j + 0.5f) - 14.0f) * s) - 0.5f (sy with i), bilinear taps at floor(sx), floor(sy)
with crops.hip's operation order; a tap reads g = clamp((v - bg) / (ink - bg), 0, 1) (r > 0 ? min(r, 1) : +0, so NaN -> 0) inside the
glyph box and 0 outside it; ink_high = 0 writes 1 - o.  Every f32 operation is separately rounded.
"""
from __future__ import annotations

import math

import numpy as np

from oracle.crop_oracle import crop_boxes

F = np.float32
MAX_WORD_PIXELS = 1 << 22
DEFAULTS = dict(polarity=0, min_col_ink=1, min_glyph_pixels=4, max_glyphs=32, glyph_box=20, ink_high=1)


def params_with(params=None) -> dict:
    p = dict(DEFAULTS)
    if params:
        p.update(params)
    return p


def word_boxes(polys, adj, h, w):
    """Per polygon: (frame, X0, Y0, X1, Y1) integer pixels, half-open, clamped to the frame."""
    out = []
    for b, x0, y0, x1, y1 in crop_boxes(polys, adj, h, w):
        X0 = min(max(math.floor(float(x0)), 0), w)
        X1 = min(max(math.ceil(float(x1)), 0), w)
        Y0 = min(max(math.floor(float(y0)), 0), h)
        Y1 = min(max(math.ceil(float(y1)), 0), h)
        if (X1 - X0) * (Y1 - Y0) > MAX_WORD_PIXELS:
            raise ValueError(f"word box of {(X1 - X0) * (Y1 - Y0)} pixels (limit 2^22)")
        out.append((b, X0, Y0, X1, Y1))
    return out


def quantise(v: np.ndarray) -> np.ndarray:
    v = np.asarray(v, np.float32)
    v = np.where(np.isnan(v), F(0), v)
    return np.clip(v, F(0), F(255)).astype(np.int64)    # non-negative: astype truncates toward zero


def otsu(hist: np.ndarray):
    """hist: 256 counts -> (t, W0, S0, W1, S1) of the winning threshold, or (-1, 0, 0, 0, 0) when no t is valid."""
    hist = np.asarray(hist, np.int64)
    W0 = np.cumsum(hist)[:255]
    S0 = np.cumsum(hist * np.arange(256, dtype=np.int64))[:255]
    Wt, St = int(hist.sum()), int((hist * np.arange(256)).sum())
    W1, S1 = Wt - W0, St - S0
    valid = (W0 > 0) & (W1 > 0)
    d = (S1 * W0 - S0 * W1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        score = np.where(valid, (d * d) / (W0.astype(np.float64) * W1.astype(np.float64)), -1.0)
    t = int(np.argmax(score))            # the first maximum: ties go to the smaller t
    if score[t] < 0:
        return -1, 0, 0, 0, 0
    return t, int(W0[t]), int(S0[t]), int(W1[t]), int(S1[t])


def segment_word(img: np.ndarray, X0, Y0, X1, Y1, params=None):
    """img: H x W f32 frame.  Returns (t, polarity used, truncated, bg, ink, [(x0, y0, x1, y1), ...])."""
    p = params_with(params)
    q = quantise(img[Y0:Y1, X0:X1])
    t, W0, S0, W1, S1 = otsu(np.bincount(q.ravel(), minlength=256))
    if t < 0:
        return -1, 0, 0, F(0), F(0), []
    pol = p["polarity"]
    if pol == 0:
        pol = 1 if W0 <= W1 else 2
    mu0, mu1 = F(S0 / W0), F(S1 / W1)    # Python's int / int is the correctly rounded quotient, as (double)S0 / W0 is here
    bg, ink = (mu1, mu0) if pol == 1 else (mu0, mu1)
    inkpx = (q <= t) if pol == 1 else (q > t)
    cnt = inkpx.sum(axis=0)
    col = cnt >= p["min_col_ink"]
    boxes, truncated = [], 0
    x = 0
    wb = X1 - X0
    while x < wb:
        if not col[x]:
            x += 1
            continue
        xs = x
        while x < wb and col[x]:
            x += 1
        if int(cnt[xs:x].sum()) < p["min_glyph_pixels"]:
            continue
        if len(boxes) == p["max_glyphs"]:
            truncated = 1
            break
        rows = np.nonzero(inkpx[:, xs:x].any(axis=1))[0]
        boxes.append((X0 + xs, Y0 + int(rows[0]), X0 + x, Y0 + int(rows[-1]) + 1))
    return t, pol, truncated, bg, ink, boxes


def segment(frames: np.ndarray, polys, adj, params=None) -> dict:
    """frames: N x 1 x H x W f32 (raw 0..255); polys: per image the polygons in original-image pixels (ocr_polygons_t);
    adj: N x 2.  Returns the arrays of ocr_glyphs_t."""
    n, _, h, w = frames.shape
    words = word_boxes(polys, adj, h, w)
    info, levels, boxes, woff = [], [], [], [0]
    for b, X0, Y0, X1, Y1 in words:
        t, pol, trunc, bg, ink, bx = segment_word(frames[b, 0], X0, Y0, X1, Y1, params)
        info.append((b, t, pol, trunc))
        levels.append((bg, ink))
        boxes.extend(bx)
        woff.append(len(boxes))
    return dict(img_offsets=np.cumsum([0] + [len(p) for p in polys]).astype(np.int32),
                word_offsets=np.asarray(woff, np.int32),
                word_info=np.asarray(info, np.int32).reshape(-1, 4),
                word_levels=np.asarray(levels, np.float32).reshape(-1, 2),
                boxes=np.asarray(boxes, np.int32).reshape(-1, 4))


def glyph_crops(frames: np.ndarray, seg: dict, params=None) -> np.ndarray:
    """The 28 x 28 crop of every glyph of `seg` (segment()'s arrays): n_glyphs x 784 f32."""
    p = params_with(params)
    n, _, h, w = frames.shape
    woff = seg["word_offsets"]
    G = int(woff[-1])
    if G == 0:
        return np.zeros((0, 784), np.float32)
    word_of = np.repeat(np.arange(len(woff) - 1), np.diff(woff))
    fr = seg["word_info"][word_of, 0].astype(np.int64)[:, None]
    bg = seg["word_levels"][word_of, 0][:, None]
    ink = seg["word_levels"][word_of, 1][:, None]
    x0, y0, x1, y1 = (seg["boxes"][:, k].astype(np.int64)[:, None] for k in range(4))
    s = (np.maximum(x1 - x0, y1 - y0).astype(np.float32) / F(p["glyph_box"])).astype(np.float32)
    cx = (x0 + x1).astype(np.float32) * F(0.5)
    cy = (y0 + y1).astype(np.float32) * F(0.5)
    o = np.arange(784)
    ii, jj = (o // 28).astype(np.float32)[None, :], (o % 28).astype(np.float32)[None, :]
    sx = (cx + ((jj + F(0.5)) - F(14)) * s) - F(0.5)
    sy = (cy + ((ii + F(0.5)) - F(14)) * s) - F(0.5)
    ix0 = np.floor(sx).astype(np.int64)
    iy0 = np.floor(sy).astype(np.int64)
    fx = sx - ix0.astype(np.float32)
    fy = sy - iy0.astype(np.float32)
    flat = frames.reshape(n, h * w)
    den = ink - bg

    def tap(ix, iy):
        inside = (ix >= x0) & (ix < x1) & (iy >= y0) & (iy < y1)
        v = flat[np.broadcast_to(fr, ix.shape), np.where(inside, iy * w + ix, 0)]
        with np.errstate(invalid="ignore"):
            r = (v - bg) / den
            g = np.where(r > F(0), np.where(r < F(1), r, F(1)), F(0)).astype(np.float32)
        return np.where(inside, g, F(0)).astype(np.float32)

    a, b = tap(ix0, iy0), tap(ix0 + 1, iy0)
    c, d = tap(ix0, iy0 + 1), tap(ix0 + 1, iy0 + 1)
    top = a + fx * (b - a)
    bot = c + fx * (d - c)
    out = (top + fy * (bot - top)).astype(np.float32)
    if not p["ink_high"]:
        out = (F(1) - out).astype(np.float32)
    return out
