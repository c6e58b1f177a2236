"""Numpy restatement of ocr_split_glyphs (include/ocr_amd.h; kernel csrc/glyph_split.hip): wide glyphs cut into pieces at ink minima.
BUILD-DEFINED: the reference has no counterpart, nothing here is read from it.  All integer.

For word k, hw = the largest y1 - y0 of its glyphs; ink is q <= t (polarity 1) or q > t (polarity 2) with the word's t and polarity from
word_info and q of tests/glyph_oracle.py.  For glyph g with box [x0, x1) x [y0, y1), gw = x1 - x0:
    n = (200*gw + hw*aspect_pct) // (2*hw*aspect_pct);  n = max(1, min(n, max_pieces, gw // min_piece_w))
n = 1: one piece, the box unchanged.  Otherwise cnt[x] = ink of column x over [y0, y1), r = max(1, gw // (4n)), c_j = x0 + (j*gw)//n
and cut j is the x in [max(c_j - r, x0 + 1), min(c_j + r, x1 - 1)] that minimises (cnt[x], |x - c_j|, x).  Piece i covers
[cut_i, cut_(i+1)) with its y range first ink row .. last ink row + 1; a piece without ink is dropped.  A word with more than
max_word_pieces pieces (after the drops) passes through unsplit and word_info[k][3] gains bit 4.
"""
from __future__ import annotations

import numpy as np

from tests import glyph_oracle as GO

DEFAULTS = dict(aspect_pct=100, max_pieces=3, min_piece_w=3, max_word_pieces=32)


def params_with(params=None) -> dict:
    p = dict(DEFAULTS)
    p.update(params or {})
    return p


def pieces_asked(gw: int, hw: int, p: dict) -> int:
    n = (200 * gw + hw * p["aspect_pct"]) // (2 * hw * p["aspect_pct"])
    return max(1, min(n, p["max_pieces"], gw // p["min_piece_w"]))


def cuts_of(cnt: np.ndarray, x0: int, x1: int, n: int) -> list:
    """cnt indexed by frame column - x0 -> the n - 1 cut columns (frame coordinates)"""
    gw = x1 - x0
    r = max(1, gw // (4 * n))
    out = []
    for j in range(1, n):
        c = x0 + (j * gw) // n
        lo, hi = max(c - r, x0 + 1), min(c + r, x1 - 1)
        out.append(min(range(lo, hi + 1), key=lambda x: (int(cnt[x - x0]), abs(x - c), x)))
    return out


def split(frames: np.ndarray, glyphs: dict, params=None) -> dict:
    """glyphs: the arrays of an ocr_glyphs_t (tests/glyph_oracle.py's dict, or a capi.GlyphSet's attributes as a dict) -> the piece
    block's arrays, `map` (n_pieces x 2: source glyph, rank) and `asked` (n per input glyph)."""
    p = params_with(params)
    off = np.asarray(glyphs["word_offsets"], np.int64)
    info = np.array(glyphs["word_info"], np.int32).reshape(-1, 4)
    boxes = np.asarray(glyphs["boxes"], np.int32).reshape(-1, 4)
    out_boxes, out_map, woff, asked = [], [], [0], []
    for k in range(len(off) - 1):
        g0, g1 = int(off[k]), int(off[k + 1])
        word, wmap = [], []
        if g1 > g0:
            fr, t, pol = int(info[k, 0]), int(info[k, 1]), int(info[k, 2])
            hw = int((boxes[g0:g1, 3] - boxes[g0:g1, 1]).max())
        for g in range(g0, g1):
            x0, y0, x1, y1 = (int(v) for v in boxes[g])
            n = pieces_asked(x1 - x0, hw, p)
            asked.append(n)
            if n == 1:
                word.append((x0, y0, x1, y1))
                wmap.append((g, 0))
                continue
            q = GO.quantise(frames[fr, 0, y0:y1, x0:x1])
            ink = (q <= t) if pol == 1 else (q > t)
            edges = [x0] + cuts_of(ink.sum(axis=0), x0, x1, n) + [x1]
            assert all(b > a for a, b in zip(edges, edges[1:])), edges   # the windows are disjoint: the cuts increase strictly
            rank = 0
            for xa, xb in zip(edges, edges[1:]):
                rows = np.nonzero(ink[:, xa - x0:xb - x0].any(axis=1))[0]
                if len(rows) == 0:
                    continue
                word.append((xa, y0 + int(rows[0]), xb, y0 + int(rows[-1]) + 1))
                wmap.append((g, rank))
                rank += 1
        if len(word) > p["max_word_pieces"]:
            word = [tuple(int(v) for v in boxes[g]) for g in range(g0, g1)]
            wmap = [(g, 0) for g in range(g0, g1)]
            info[k, 3] |= 4
        out_boxes += word
        out_map += wmap
        woff.append(len(out_boxes))
    return dict(img_offsets=np.asarray(glyphs["img_offsets"], np.int32), word_offsets=np.asarray(woff, np.int32), word_info=info,
                word_levels=np.asarray(glyphs["word_levels"], np.float32).reshape(-1, 2),
                boxes=np.asarray(out_boxes, np.int32).reshape(-1, 4), map=np.asarray(out_map, np.int32).reshape(-1, 2),
                asked=np.asarray(asked, np.int32))


def block(frame_of_word, t, pol, boxes_per_word) -> dict:
    """a glyph block written by hand: per word its frame and a list of boxes; one threshold and polarity for all"""
    nw = len(boxes_per_word)
    off = np.concatenate([[0], np.cumsum([len(b) for b in boxes_per_word])]).astype(np.int32)
    n_img = (max(frame_of_word) + 1) if nw else 1
    per_img = np.bincount(np.asarray(frame_of_word, np.int64), minlength=n_img) if nw else np.zeros(1, np.int64)
    assert list(frame_of_word) == sorted(frame_of_word)
    return dict(img_offsets=np.concatenate([[0], np.cumsum(per_img)]).astype(np.int32), word_offsets=off,
                word_info=np.array([[f, t, pol, 0] for f in frame_of_word], np.int32).reshape(-1, 4),
                word_levels=np.tile(np.array([[210.0, 30.0]], np.float32), (nw, 1)),
                boxes=np.array([b for bs in boxes_per_word for b in bs], np.int32).reshape(-1, 4))


PAPER, INK, T_HAND = 210.0, 30.0, 120


def drawn_cases():
    """-> [(name, frames 1 x 1 x H x W, glyph block, params, expected piece boxes or None, expected bit 4 per word)].  Dark ink on
    light paper, polarity 1, t = 120.
      bridge   two bars of 12 rows, columns [4, 10) and [16, 22), joined by a one-row bridge over [10, 16): one glyph [4, 22) x [6, 18),
               gw = 18, hw = 12: n = (3600 + 1200) // 2400 = 2, r = max(1, 18 // 8) = 2, c_1 = 4 + 9 = 13, window [11, 15]: every column
               of it holds 1 ink pixel, so |x - c| decides: the cut is column 13.
      narrow   a glyph of 8 x 12: n = (1600 + 1200) // 2400 = 1, passed through with its box (which is wider than its ink).
      clip     aspect_pct 25, max_pieces 4 on a solid glyph of 13 columns [3, 16), hw = 12: n = (2600 + 300) // 600 = 4, r = 1,
               c = 6, 9, 12, every count equal: the cuts are the centres.  A second glyph of 3 columns: gw // min_piece_w = 1 keeps it
               whole.  (With min_piece_w >= 3 a window never reaches x0 + 1 or x1 - 1 - c_1 - r >= x0 + 2 and c_(n-1) + r <= x1 - 2 -
               so the two clamps of the rule are guards; tests/test_glyph_split_oracle.py meets them on cuts_of directly.)
      empty    a glyph box [4, 28) x [6, 18), n = 3 (aspect 67: (4800 + 804) // 1608 = 3), ink only in [4, 10) and [22, 28): the
               middle piece [12, 20) has no ink and is dropped; the cuts sit at the first zero column nearest c (12 and 20).
      many     max_word_pieces 3 over a word of two bridge glyphs (4 pieces): passes through, bit 4 set; a second word of one bridge
               glyph (2 pieces) is split.
    """
    cases = []
    f = np.full((1, 1, 24, 40), PAPER, np.float32)
    f[0, 0, 6:18, 4:10] = INK
    f[0, 0, 6:18, 16:22] = INK
    f[0, 0, 11, 10:16] = INK
    cases.append(("bridge", f, block([0], T_HAND, 1, [[(4, 6, 22, 18)]]), None, [[4, 6, 13, 18], [13, 6, 22, 18]], [0]))

    f = np.full((1, 1, 24, 40), PAPER, np.float32)
    f[0, 0, 6:18, 5:11] = INK
    cases.append(("narrow", f, block([0], T_HAND, 1, [[(4, 6, 12, 18)]]), None, [[4, 6, 12, 18]], [0]))

    f = np.full((1, 1, 24, 40), PAPER, np.float32)
    f[0, 0, 6:18, 3:16] = INK
    f[0, 0, 6:18, 20:23] = INK
    cases.append(("clip", f, block([0], T_HAND, 1, [[(3, 6, 16, 18), (20, 6, 23, 18)]]), dict(aspect_pct=25, max_pieces=4),
                  [[3, 6, 6, 18], [6, 6, 9, 18], [9, 6, 12, 18], [12, 6, 16, 18], [20, 6, 23, 18]], [0]))

    f = np.full((1, 1, 24, 40), PAPER, np.float32)
    f[0, 0, 6:18, 4:10] = INK
    f[0, 0, 8:15, 22:28] = INK
    cases.append(("empty", f, block([0], T_HAND, 1, [[(4, 6, 28, 18)]]), dict(aspect_pct=67),
                  [[4, 6, 12, 18], [20, 8, 28, 15]], [0]))

    f = np.full((1, 1, 24, 96), PAPER, np.float32)
    for x in (4, 30, 60):
        f[0, 0, 6:18, x:x + 6] = INK
        f[0, 0, 6:18, x + 12:x + 18] = INK
        f[0, 0, 11, x + 6:x + 12] = INK
    cases.append(("many", f, block([0, 0], T_HAND, 1, [[(4, 6, 22, 18), (30, 6, 48, 18)], [(60, 6, 78, 18)]]), dict(max_word_pieces=3),
                  [[4, 6, 22, 18], [30, 6, 48, 18], [60, 6, 69, 18], [69, 6, 78, 18]], [4, 0]))
    return cases


def fuzz_case(seed: int = 77):
    """Two 96 x 160 frames of uniform noise (about 40 % of the pixels are ink at t = 120, dark ink), 32 words a frame as rectangles
    of width 3 to 60 (both ends forced) and height 6 to 11, packed first-fit into 8 rows a frame.  The column rule makes nearly every
    word one glyph as wide as the word, the component rule breaks it into blobs.  -> (frames, polys, adj)"""
    rng = np.random.default_rng(seed)
    frames = rng.uniform(0.0, 300.0, (2, 1, 96, 160)).astype(np.float32)
    polys = []
    for fr in range(2):
        widths = np.sort(np.concatenate([[3, 60], rng.integers(3, 61, 30)]))[::-1]
        used, words = [2] * 8, []
        for gw in widths:
            row = next(r for r in range(8) if used[r] + int(gw) <= 158)
            h = int(rng.integers(6, 12))
            x, y = used[row], 12 * row
            words.append([(x, y), (x + int(gw) - 1, y + h - 1)])
            used[row] += int(gw) + 2
        polys.append(words)
    return frames, polys, np.ones((2, 2))
