"""Plain-Python restatement of the word-break rule of ocr_break_words (include/ocr_amd.h; kernel csrc/word_breaks.hip).

Loops over Python integers (exact, so every int64 product of the rule is what the device computes as long as the inputs are inside
the call's limits), and the one f64 score through separate numpy operations: a conversion, two multiplications and a division, each
rounded on its own.  The device result must equal this bit for bit.

    break_source(boxes, params)     one source word: G x 4 boxes -> (break flags per glyph, gap_pct per glyph, info)
    break_words(glyphs, params)     a glyph block (dict of the arrays of an ocr_glyphs_t) -> (block of the sub-words, breaks dict)
"""
import numpy as np

MAX_GLYPHS = 256
INT32_MAX = 2 ** 31 - 1
DEFAULTS = {"mode": 1, "space_pct": 35, "min_space_pct": 25, "sep_pct": 200, "min_gaps": 3}


def params_of(params=None):
    p = dict(DEFAULTS)
    p.update(params or {})
    assert set(p) == set(DEFAULTS), p
    return p


def gaps_of(boxes):
    """gap_i for i = 1..G-1 against the prefix maximum of x1 (index 0 is 0 and stands for nothing)"""
    gaps, reach = [0], None
    for i in range(len(boxes)):
        if i >= 1:
            gaps.append(max(0, int(boxes[i][0]) - reach))
        x1 = int(boxes[i][2])
        reach = x1 if reach is None else max(reach, x1)
    return gaps


def adaptive_split(gaps, n):
    """the sorted gaps s and the best c (0: no valid c) by the Otsu score, ties to the smaller c"""
    s = sorted(gaps)
    best, best_c = None, 0
    for c in range(1, n):
        if not s[c - 1] < s[c]:
            continue
        n0, n1 = c, n - c
        S0, S1 = sum(s[:c]), sum(s[c:])
        d = np.float64(S1 * n0 - S0 * n1)
        dd = np.multiply(d, d)
        den = np.multiply(np.float64(n0), np.float64(n1))
        score = np.divide(dd, den)
        if best is None or score > best:
            best, best_c = score, c
    return s, best_c


def break_source(boxes, params=None):
    """-> (brk [G] bool, gap_pct [G] int (meaningful where brk), (hw, rule, threshold, flags))"""
    p = params_of(params)
    G = len(boxes)
    if G == 0:
        return [], [], (0, 0, 0, 0)
    if G > MAX_GLYPHS:
        return [False] * G, [0] * G, (0, 0, 0, 2)
    heights = sorted(int(b[3]) - int(b[1]) for b in boxes)
    hw = heights[G // 2]
    gaps = gaps_of(boxes)
    n = G - 1
    fixed_lim = p["space_pct"] * hw
    rule, thr = 1, -(-fixed_lim // 100)
    if p["mode"] == 1 and n >= p["min_gaps"]:
        s, c = adaptive_split(gaps[1:], n)
        if c:
            L, T = s[c - 1], s[c]
            if T * 100 >= p["min_space_pct"] * hw and T * 100 >= p["sep_pct"] * L:
                rule, thr = 2, T
    brk, pct = [False], [0]
    for i in range(1, G):
        brk.append(gaps[i] >= thr if rule == 2 else gaps[i] * 100 >= fixed_lim)
        pct.append(min(gaps[i] * 100 // hw, INT32_MAX))
    return brk, pct, (hw, rule, thr, 0)


def break_words(glyphs, params=None):
    """glyphs: dict with img_offsets, word_offsets, word_info (n x 4), word_levels (n x 2), boxes (g x 4).  -> (words, breaks): words the
    same dict for the sub-words, breaks a dict with source, sub_offsets, gap_pct, source_info (n_source x 4)."""
    img_off = np.asarray(glyphs["img_offsets"], np.int64)
    off = np.asarray(glyphs["word_offsets"], np.int64)
    info = np.asarray(glyphs["word_info"], np.int32).reshape(-1, 4)
    levels = np.asarray(glyphs["word_levels"], np.float32).reshape(-1, 2)
    boxes = np.asarray(glyphs["boxes"], np.int32).reshape(-1, 4)
    nw = len(off) - 1
    starts, source, gap_pct, sub_off, src_info = [], [], [], [0], []
    for k in range(nw):
        g0, g1 = int(off[k]), int(off[k + 1])
        brk, pct, inf = break_source(boxes[g0:g1].tolist(), params)
        src_info.append(inf)
        starts.append(g0)
        source.append(k)
        gap_pct.append(0)
        for i in range(1, g1 - g0):
            if brk[i]:
                starts.append(g0 + i)
                source.append(k)
                gap_pct.append(pct[i])
        sub_off.append(len(source))
    source = np.asarray(source, np.int32).reshape(-1)
    sub_off = np.asarray(sub_off, np.int32)
    words = {
        "img_offsets": sub_off[img_off].astype(np.int32),
        "word_offsets": np.asarray(starts + [int(off[-1])], np.int32),
        "word_info": info[source].reshape(-1, 4),
        "word_levels": levels[source].reshape(-1, 2),
        "boxes": boxes.copy(),
    }
    breaks = {"source": source, "sub_offsets": sub_off, "gap_pct": np.asarray(gap_pct, np.int32).reshape(-1),
              "source_info": np.asarray(src_info, np.int32).reshape(-1, 4)}
    return words, breaks
