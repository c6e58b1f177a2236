"""Numpy restatement of ocr_split_glyphs (include/ocr_amd.h; kernel csrc/glyph_split.hip): wide glyphs cut into pieces at ink minima.
BUILD-DEFINED: the reference has no counterpart, nothing here is read from it.  All integer.

For word k, hw = the largest y1 - y0 of its glyphs; ink is q <= t (polarity 1) or q > t (polarity 2) with the word's t and polarity from
word_info and q of tests/glyph_oracle.py.  For glyph g with box [x0, x1) x [y0, y1), gw = x1 - x0:
    n = (200*gw + hw*aspect_pct) // (2*hw*aspect_pct);  n = max(1, min(n, max_pieces, gw // min_piece_w))
n = 1: one piece, the box unchanged.  Otherwise cnt[x] = ink of column x over [y0, y1), r = max(1, gw // (4n)), c_j = x0 + (j*gw)//n
and cut j is the x in [max(c_j - r, x0 + 1), min(c_j + r, x1 - 1)] that minimises (cnt[x], |x - c_j|, x).  Piece i covers
[cut_i, cut_(i+1)) with its y range first ink row .. last ink row + 1; a piece without ink is dropped.  A word with more than
max_word_pieces pieces (after the drops) passes through unsplit and word_info[k][3] gains bit 4.

Cases: drawn_cases and fuzz_case (glyphs up to 60 columns), wide_drawn_cases and wide_fuzz_case (up to 1201 columns, both polarities);
reach() counts what a case reaches of the sizes at which the kernel's loops over columns take further steps.
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
    word one glyph as wide as the word, the component rule breaks it into blobs.  -> (frames, polys, adj)
    What it does not reach: the widest window is 2 * (60 // 8) + 1 = 15 columns and no piece is 64 columns wide, so neither of the
    kernel's loops over columns takes a second step of 64; no piece is dropped (at 40 % ink every piece holds some); and every word is
    polarity 1.  wide_fuzz_case and wide_drawn_cases are there for those; reach() counts what a case reaches."""
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


REACH_KEYS = ("win_gt64", "win_gt128", "cut_ge64", "cut_ge128", "count_ties", "dist_ties", "piece_gt64", "piece_gt128", "dropped", "far_rows")


def reach(frames: np.ndarray, glyphs: dict, params=None) -> dict:
    """What a case reaches, counted from the oracle's own quantities (64 is the kernel's step over columns, one wave):
      win_gt64, win_gt128      search windows [lo, hi] of more than 64 / 128 columns
      cut_ge64, cut_ge128      cuts whose index in their window, cut - lo, is >= 64 / >= 128
      count_ties               cuts whose ink count is held by more than one column of the window
      dist_ties                of those, cuts whose (count, |x - c|) is held by two columns: the smaller x decided
      piece_gt64, piece_gt128  pieces [cut_i, cut_(i+1)) of a cut glyph wider than 64 / 128 columns, dropped ones included
      dropped                  pieces without ink
      far_rows                 kept pieces wider than 64 whose first or last ink row is not that of their first 64 columns, or whose
                               first 64 columns hold no ink
      asked                    {n: glyphs that ask for n pieces}"""
    p = params_with(params)
    off = np.asarray(glyphs["word_offsets"], np.int64)
    info = np.array(glyphs["word_info"], np.int32).reshape(-1, 4)
    boxes = np.asarray(glyphs["boxes"], np.int32).reshape(-1, 4)
    out = dict.fromkeys(REACH_KEYS, 0)
    out["asked"] = {}
    for k in range(len(off) - 1):
        g0, g1 = int(off[k]), int(off[k + 1])
        if g1 == g0:
            continue
        fr, t, pol = int(info[k, 0]), int(info[k, 1]), int(info[k, 2])
        hw = int((boxes[g0:g1, 3] - boxes[g0:g1, 1]).max())
        for g in range(g0, g1):
            x0, y0, x1, y1 = (int(v) for v in boxes[g])
            gw = x1 - x0
            n = pieces_asked(gw, hw, p)
            out["asked"][n] = out["asked"].get(n, 0) + 1
            if n == 1:
                continue
            q = GO.quantise(frames[fr, 0, y0:y1, x0:x1])
            ink = (q <= t) if pol == 1 else (q > t)
            cnt = ink.sum(axis=0)
            r = max(1, gw // (4 * n))
            cuts = cuts_of(cnt, x0, x1, n)
            for j, cut in zip(range(1, n), cuts):
                c = x0 + (j * gw) // n
                lo, hi = max(c - r, x0 + 1), min(c + r, x1 - 1)
                out["win_gt64"] += hi - lo + 1 > 64
                out["win_gt128"] += hi - lo + 1 > 128
                out["cut_ge64"] += cut - lo >= 64
                out["cut_ge128"] += cut - lo >= 128
                same = [x for x in range(lo, hi + 1) if cnt[x - x0] == cnt[cut - x0]]
                out["count_ties"] += len(same) > 1
                out["dist_ties"] += sum(abs(x - c) == abs(cut - c) for x in same) > 1
            edges = [x0] + cuts + [x1]
            for xa, xb in zip(edges, edges[1:]):
                out["piece_gt64"] += xb - xa > 64
                out["piece_gt128"] += xb - xa > 128
                rows = np.nonzero(ink[:, xa - x0:xb - x0].any(axis=1))[0]
                if len(rows) == 0:
                    out["dropped"] += 1
                elif xb - xa > 64:
                    first = np.nonzero(ink[:, xa - x0:xa - x0 + 64].any(axis=1))[0]
                    out["far_rows"] += len(first) == 0 or (first[0], first[-1]) != (rows[0], rows[-1])
    return {k: (v if k == "asked" else int(v)) for k, v in out.items()}


def add_reach(a: dict, b: dict) -> dict:
    """the counters of two cases, added"""
    out = {k: a[k] + b[k] for k in REACH_KEYS}
    out["asked"] = {n: a["asked"].get(n, 0) + b["asked"].get(n, 0) for n in sorted(set(a["asked"]) | set(b["asked"]))}
    return out


WIDE_BOX = (10, 2, 610, 14)


def _inverted(case):
    """the same drawing light on dark at polarity 2: 210 <-> 30 (levels mirrored about 120), every expected number unchanged"""
    name, frames, blk, prm, want, bits = case
    info = blk["word_info"].copy()
    info[:, 2] = 2
    return (name, (PAPER + INK - frames).astype(np.float32), dict(blk, word_info=info), prm, want, bits)


def wide_drawn_cases():
    """-> [(name + "-p1" | "-p2", frames, glyph block, params, expected piece boxes, expected bit 4 per word)]: drawn cases past one
    wave's 64 columns, each at polarity 1 (dark on light, as drawn below) and as the same drawing inverted at polarity 2; t = 120.
    All but tall_wide: a 16 x 700 frame per glyph, the glyph [10, 610) x [2, 14) (gw = 600, hw = 12, the rule asks for (120000 + 1200)
    // 2400 = 50 pieces) and max_pieces = 2: n = 2, r = 600 // 8 = 75, c = 10 + 300 = 310, the window is [235, 385] (151 columns; a lane
    that starts at 235 + l meets 235 + l, 299 + l, 363 + l: index 64 is column 299, index 128 is column 363).
      far_min       a solid bar over the glyph with column 380 blank: the only zero count lies in the third step (index 145): the cut
                    is 380, the pieces [10, 380) and [380, 610), both with all 12 rows.
      far_tie       frame 0: the bar with columns 250 and 370 blank, both at distance 60 from c, in steps 0 and 2: the smaller x wins,
                    the cut is 250.  Frame 1: columns 250 and 300 blank: 300 is nearer (10 against 60) and wins although it is the
                    larger x.
      far_rows      ink [10, 14) x [6, 9) and [320, 324) x [6, 9), one pixel at (x 200, y 2) and one at (x 290, y 13).  In the window
                    column 290 counts 1, 320..323 count 3, the rest 0: the cut is c = 310.  Piece 0 = [10, 310) has rows 2 (x 200),
                    6..8 and 13 (x 290): [10, 2, 310, 14], both extremes beyond its first 64 columns.  Piece 1 = [310, 6, 610, 9].
      far_only      ink [10, 14) x [6, 9) and one pixel at (x 600, y 7); the window is blank, the cut is 310.  Piece 1 = [310, 610)
                    holds only that pixel, 290 columns in: [310, 7, 610, 8], kept.
      far_only3     the same drawing at max_pieces = 3: n = 3, r = 600 // 12 = 50, c = 210 and 410, both windows blank: cuts 210 and
                    410.  The middle piece [210, 410) has no ink and is dropped: [10, 6, 210, 9] and [410, 7, 610, 8].
      at_threshold  not an inversion: the two polarities share the drawing and differ in what the levels A = 120.0, B = 120.9 (both
                    q = 120 = t) and C = 121.0 (q = 121) are.  Rows 6 and 7 are solid ink over [10, 610) (30 at polarity 1, 210 at
                    polarity 2, the paper the other of the two), except column 305 = A, column 300 = B, column 290 = C in both rows;
                    single pixels (x 100, y 2) = A, (x 100, y 3) = C, (x 500, y 13) = B, (x 500, y 12) = C.
                    Polarity 1 (ink is q <= 120: A and B are ink, C is not): column 290 counts 0, every other 2: the cut is 290.
                    Piece 0 = [10, 290) has rows 2 (A), 6, 7: [10, 2, 290, 8].  Piece 1 has rows 6, 7 and 13 (B): [290, 6, 610, 14].
                    Polarity 2 (ink is q > 120: C is ink, A and B are not): columns 300 and 305 count 0, 305 is nearer to 310: the cut
                    is 305.  Piece 0 = [10, 305) has rows 3 (C), 6, 7: [10, 3, 305, 8].  Piece 1 has rows 6, 7 and 12 (C):
                    [305, 6, 610, 13].  (Were q = t ink at polarity 2 every column would count 2 and the cut would be 310.)
      tall_wide     a 1006 x 608 frame, one glyph [4, 604) x [3, 1003) (gw = 600, hw = 1000), aspect_pct 25: n = (120000 + 25000) //
                    50000 = 2, r = 75, c = 304, window [229, 379].  Ink only over the window's columns [229, 380), all 1000 rows, but
                    for the pixel (x 370, y 500): column 370 counts 999, every other 1000 - four digits in the key's high field -
                    and the cut is 370 (index 141).  Pieces [4, 3, 370, 1003] and [370, 3, 604, 1003].
    """
    two = dict(max_pieces=2)
    paper = lambda n=1, h=16, w=700: np.full((n, 1, h, w), PAPER, np.float32)
    x0, y0, x1, y1 = WIDE_BOX
    one = lambda pol=1: block([0], T_HAND, pol, [[WIDE_BOX]])
    cases = []

    f = paper()
    f[0, 0, y0:y1, x0:x1] = INK
    f[0, 0, :, 380] = PAPER
    cases.append(("far_min", f, one(), two, [[10, 2, 380, 14], [380, 2, 610, 14]], [0]))

    f = paper(2)
    f[:, 0, y0:y1, x0:x1] = INK
    f[0, 0, :, [250, 370]] = PAPER
    f[1, 0, :, [250, 300]] = PAPER
    cases.append(("far_tie", f, block([0, 1], T_HAND, 1, [[WIDE_BOX], [WIDE_BOX]]), two,
                  [[10, 2, 250, 14], [250, 2, 610, 14], [10, 2, 300, 14], [300, 2, 610, 14]], [0, 0]))

    f = paper()
    f[0, 0, 6:9, 10:14] = INK
    f[0, 0, 6:9, 320:324] = INK
    f[0, 0, 2, 200] = INK
    f[0, 0, 13, 290] = INK
    cases.append(("far_rows", f, one(), two, [[10, 2, 310, 14], [310, 6, 610, 9]], [0]))

    f = paper()
    f[0, 0, 6:9, 10:14] = INK
    f[0, 0, 7, 600] = INK
    cases.append(("far_only", f, one(), two, [[10, 6, 310, 9], [310, 7, 610, 8]], [0]))
    cases.append(("far_only3", f, one(), dict(max_pieces=3), [[10, 6, 210, 9], [410, 7, 610, 8]], [0]))

    f = paper(1, 1006, 608)
    f[0, 0, 3:1003, 229:380] = INK
    f[0, 0, 500, 370] = PAPER
    cases.append(("tall_wide", f, block([0], T_HAND, 1, [[(4, 3, 604, 1003)]]), dict(aspect_pct=25),
                  [[4, 3, 370, 1003], [370, 3, 604, 1003]], [0]))

    out = []
    for c in cases:
        out.append((c[0] + "-p1",) + c[1:])
        out.append((c[0] + "-p2",) + _inverted(c)[1:])

    A, B, Cl = T_HAND + 0.0, T_HAND + 0.9, T_HAND + 1.0
    for pol, want in ((1, [[10, 2, 290, 8], [290, 6, 610, 14]]), (2, [[10, 3, 305, 8], [305, 6, 610, 13]])):
        f = np.full((1, 1, 16, 700), PAPER if pol == 1 else INK, np.float32)
        f[0, 0, 6:8, x0:x1] = INK if pol == 1 else PAPER
        f[0, 0, 6:8, 305] = A
        f[0, 0, 6:8, 300] = B
        f[0, 0, 6:8, 290] = Cl
        f[0, 0, 2, 100], f[0, 0, 3, 100] = A, Cl
        f[0, 0, 13, 500], f[0, 0, 12, 500] = B, Cl
        out.append((f"at_threshold-p{pol}", f, one(pol), two, want, [0]))
    return out


WIDE_H, WIDE_W = 48, 1201
# the parameter sets of the wide fuzz, on the CPU and on the GPU: max_pieces 1..4, aspect_pct 25 / 100 / 400, min_piece_w 3 / 64, and a
# max_word_pieces that lets single glyphs through and stops the words of many
WIDE_PARAMS = (dict(max_pieces=1), dict(max_pieces=2), dict(max_pieces=3), dict(max_pieces=4),
               dict(max_pieces=2, aspect_pct=25), dict(max_pieces=4, aspect_pct=25), dict(max_pieces=3, aspect_pct=400),
               dict(max_pieces=4, aspect_pct=400), dict(max_pieces=2, min_piece_w=64), dict(max_pieces=4, aspect_pct=25, min_piece_w=64),
               dict(max_pieces=4, max_word_pieces=6))


def wide_fuzz_case(seed: int = 11, polarity: int = 1):
    """Two 48 x 1201 frames, eight bands of six rows a frame, a band one word of glyphs side by side (so hw is often a neighbour's
    height).  Widths 3, 65, 129, 257, 513 and the whole 1201 columns plus random ones up to 1100, heights 3 to 6; the glyphs of width 3
    ask for one piece whatever the parameters, so waves that return at once share workgroups with waves that cut.  Boxes touch x = 0,
    x = W, y = 0 and y = H.  Ink is sparse and patchy: a (row, 64-column chunk) cell is blank with probability 1/2 and otherwise 24 %
    ink, about 12 % overall, so columns without ink are common, pieces lose all their ink, and a piece's first and last ink row often
    lie past its first 64 columns.  Levels are k + j/10, ink 0..120.9 and paper 121..255.9 at polarity 1, swapped at polarity 2, t = 120:
    pixels with q = t occur.  -> (frames 2 x 1 x 48 x 1201, glyph block)"""
    rng = np.random.default_rng([seed, polarity])
    H, W = WIDE_H, WIDE_W
    cells = rng.random((2, H, (W + 63) // 64)) < 0.5
    ink = rng.random((2, H, W)) < np.repeat(cells, 64, axis=2)[:, :, :W] * 0.24
    low = rng.integers(0, 121, (2, H, W)) + rng.integers(0, 10, (2, H, W)) / 10.0
    high = rng.integers(121, 256, (2, H, W)) + rng.integers(0, 10, (2, H, W)) / 10.0
    frames = np.where(ink == (polarity == 1), low, high).astype(np.float32)[:, None]
    R = lambda a, b: int(rng.integers(a, b + 1))
    bands = [[[W], [513, 3, 257, 3, 65, 129, 3, R(6, 12)], [R(600, 1100), 3, R(6, 12)], [65, 3, 65, 129, 3, 257, R(3, 60), R(3, 60)],
              [R(600, 1100)], [R(3, 150) for _ in range(6)], [R(900, 1100), 3], [513, 3, 513]],
             [[R(600, 1100), 3, 65], [129, 3, R(6, 12), 513, R(6, 12), 257, 3], [R(900, 1100)], [R(3, 150) for _ in range(6)],
              [257, 3, 129, 65, 3, 513], [R(600, 1100), R(6, 12), 3], [R(3, 300) for _ in range(4)], [W]]]
    frame_of_word, words = [], []
    for fr in range(2):
        for b, widths in enumerate(bands[fr]):
            gaps = [R(0, 2) for _ in widths]
            x = 0 if b % 2 == 0 else W - (sum(widths) + sum(gaps[1:]))     # even bands start at x = 0, odd bands end at x = W
            assert x >= 0 and sum(widths) + sum(gaps[1:]) <= W
            word = []
            for i, gw in enumerate(widths):
                x += gaps[i] if i else 0
                h = 6 if i == 0 and b in (0, 7) else R(3, 6)
                y = 6 * b + R(0, 6 - h)
                word.append((x, y, x + gw, y + h))
                x += gw
            frame_of_word.append(fr)
            words.append(word)
    return frames, block(frame_of_word, T_HAND, polarity, words)
