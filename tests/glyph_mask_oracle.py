"""ORACLE (test infrastructure) for the BUILD-DEFINED label planes and masked glyph crops (include/ocr_amd.h,
ocr_segment_glyphs_cc_labelled and ocr_extract_glyph_crops_masked): numpy only; segment_cc_labelled_kernel (csrc/glyph_cc.hip) and
glyph_crop_masked_kernel (csrc/glyphs.hip) must equal it element for element, bit for bit.  The components, the limits and steps 1-5
are tests/glyph_cc_oracle.py's, the sampling is tests/glyph_oracle.py's; this file restates the grouping walk with membership and
the crop with the masked tap.  Kept in tests/ because oracle/ is frozen.

Label planes.  Word k with the box [X0, X1) x [Y0, Y1) owns a plane of bh x bw uint16, row-major, at element offset plane_offsets[k].
After steps 1-11 of the component rule it holds
  0       where the pixel is not ink, and everywhere when the word is flat or fell back to the column rule (flag 2);
  g + 1   for an ink pixel of a component in the group that became glyph g of the word;
  0xFFFF  for every other ink pixel: a component dropped at step 6 (s < min_glyph_pixels), a component of a group dropped at step 9
          (height), a component of a group past the first max_glyphs (step 10).
Masked tap of glyph g of word k, m = g + 1, L(x, y) the plane value inside the word box and 0 outside it:
  1. outside the glyph box: 0;
  2. l = L(x, y); l != 0 and l != m: 0;
  3. l == 0 and halo == 1: foreign = some of the eight neighbours has L not in {0, m}, own = some has L == m; foreign and not own: 0;
  4. otherwise glyph_oracle's value g = r > 0 ? min(r, 1) : 0, r = (v - bg) / (ink - bg).
Everything else of the crop (sample positions, the order of the bilinear blend, ink_high) is glyph_oracle.glyph_crops'.
"""
from __future__ import annotations

import numpy as np

from tests import glyph_cc_oracle as CC
from tests import glyph_oracle as G

F = np.float32
NO_GLYPH = 0xFFFF
MASK_DEFAULTS = dict(halo=1)


def mask_params_with(mask=None) -> dict:
    p = dict(MASK_DEFAULTS)
    if mask:
        p.update(mask)
    return p


def group_membership(comps, bh, params, cc):
    """Steps 6-10 of the component rule with membership: (label of every component of `comps`, the kept groups' boxes).  A label is
    g + 1 for a component of the group that became glyph g, NO_GLYPH for every other one."""
    order = sorted((k for k, c in enumerate(comps) if c["s"] >= params["min_glyph_pixels"]), key=lambda k: (comps[k]["x0"], comps[k]["anchor"]))
    pct = cc["merge_overlap_pct"]
    groups = []                                      # [box as a list x0, y0, x1, y1, members]
    for k in order:
        c = comps[k]
        if groups:
            a = groups[-1][0]
            ov = min(a[2], c["x1"]) - max(a[0], c["x0"])
            nar = min(a[2] - a[0], c["x1"] - c["x0"])
            if pct > 0 and ov > 0 and ov * 100 >= nar * pct:
                groups[-1][0] = [min(a[0], c["x0"]), min(a[1], c["y0"]), max(a[2], c["x1"]), max(a[3], c["y1"])]
                groups[-1][1].append(k)
                continue
        groups.append([[c["x0"], c["y0"], c["x1"], c["y1"]], [k]])
    labels = np.full(len(comps), NO_GLYPH, np.int64)
    boxes = []
    for box, members in groups:
        if (box[3] - box[1]) * 100 < cc["min_height_pct"] * bh or len(boxes) == params["max_glyphs"]:
            continue
        boxes.append(tuple(box))
        labels[members] = len(boxes)
    return labels, boxes


def word_plane(img: np.ndarray, X0, Y0, X1, Y1, params=None, cc=None) -> np.ndarray:
    """The bh x bw uint16 label plane of one word of the frame `img`."""
    p, c = G.params_with(params), CC.cc_params_with(cc)
    plane = np.zeros((Y1 - Y0, X1 - X0), np.uint16)
    _, _, _, _, ink = CC.word_ink(img, X0, Y0, X1, Y1, p)
    if ink is None:
        return plane                                             # flat
    runs = CC.runs_of(ink)
    if len(runs) > CC.MAX_RUNS:
        return plane                                             # the column rule read this word: not masked
    _, comps = CC.components(ink)
    if len(comps) > CC.MAX_COMPONENTS:
        return plane
    labels, boxes = group_membership(comps, Y1 - Y0, p, c)
    assert boxes == CC.group_components(comps, Y1 - Y0, p, c)[1]  # membership changes no box
    lab = CC.label_runs(runs)
    slot = {int(r): k for k, r in enumerate(np.unique(lab))}     # ascending root = ascending anchor = the order of `comps`
    for (y, a0, a1), r in zip(runs.tolist(), lab.tolist()):
        plane[y, a0:a1] = labels[slot[r]]
    return plane


def label_planes(frames: np.ndarray, polys, adj, params=None, cc=None) -> dict:
    """frames, polys, adj as glyph_cc_oracle.segment_cc.  Returns the arrays of ocr_glyph_labels_t: word_boxes n_words x 4 int32 (X0, Y0,
    X1, Y1), plane_offsets [n_words + 1] int64, planes [plane_offsets[-1]] uint16."""
    n, _, h, w = frames.shape
    boxes, off, planes = [], [0], []
    for b, X0, Y0, X1, Y1 in G.word_boxes(polys, adj, h, w):
        boxes.append((X0, Y0, X1, Y1))
        planes.append(word_plane(frames[b, 0], X0, Y0, X1, Y1, params, cc).ravel())
        off.append(off[-1] + (X1 - X0) * (Y1 - Y0))
    return dict(word_boxes=np.asarray(boxes, np.int32).reshape(-1, 4), plane_offsets=np.asarray(off, np.int64),
                planes=np.concatenate(planes) if planes else np.zeros(0, np.uint16))


def plane_of(planes: dict, k: int) -> np.ndarray:
    """Word k's bh x bw view of label_planes()' result."""
    x0, y0, x1, y1 = (int(v) for v in planes["word_boxes"][k])
    return planes["planes"][int(planes["plane_offsets"][k]):int(planes["plane_offsets"][k + 1])].reshape(y1 - y0, x1 - x0)


def masked_glyph_crops(frames: np.ndarray, seg: dict, planes: dict, params=None, mask=None) -> np.ndarray:
    """glyph_oracle.glyph_crops with the masked tap: seg is glyph_cc_oracle.segment_cc's, planes label_planes()' (or any arrays of that
    layout) for the same words.  n_glyphs x 784 f32."""
    p, mk = G.params_with(params), mask_params_with(mask)
    n, _, h, w = frames.shape
    woff = seg["word_offsets"]
    ng = int(woff[-1])
    if ng == 0:
        return np.zeros((0, 784), np.float32)
    word_of = np.repeat(np.arange(len(woff) - 1), np.diff(woff))
    m = (np.arange(ng) - woff[word_of] + 1).astype(np.int64)[:, None]
    fr = seg["word_info"][word_of, 0].astype(np.int64)[:, None]
    bg = seg["word_levels"][word_of, 0][:, None]
    ink = seg["word_levels"][word_of, 1][:, None]
    x0, y0, x1, y1 = (seg["boxes"][:, k].astype(np.int64)[:, None] for k in range(4))
    wx0, wy0, wx1, wy1 = (planes["word_boxes"][word_of, k].astype(np.int64)[:, None] for k in range(4))
    poff = planes["plane_offsets"][word_of].astype(np.int64)[:, None]
    flat_l = np.concatenate([planes["planes"].astype(np.int64), np.zeros(1, np.int64)])     # the last element serves every read outside
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

    def label_at(ix, iy):
        inw = (ix >= wx0) & (ix < wx1) & (iy >= wy0) & (iy < wy1)
        return flat_l[np.where(inw, poff + (iy - wy0) * (wx1 - wx0) + (ix - wx0), len(flat_l) - 1)]

    def tap(ix, iy):
        inside = (ix >= x0) & (ix < x1) & (iy >= y0) & (iy < y1)
        v = flat[np.broadcast_to(fr, ix.shape), np.where(inside, iy * w + ix, 0)]
        with np.errstate(invalid="ignore"):
            r = (v - bg) / den
            g = np.where(r > F(0), np.where(r < F(1), r, F(1)), F(0)).astype(np.float32)
        lab = label_at(ix, iy)
        keep = inside & ((lab == 0) | (lab == m))
        if mk["halo"]:
            foreign = np.zeros(ix.shape, bool)
            own = np.zeros(ix.shape, bool)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dx or dy:
                        nb = label_at(ix + dx, iy + dy)
                        foreign |= (nb != 0) & (nb != m)
                        own |= nb == m
            keep &= ~((lab == 0) & foreign & ~own)
        return np.where(keep, g, F(0)).astype(np.float32)

    a, b = tap(ix0, iy0), tap(ix0 + 1, iy0)
    c, d = tap(ix0, iy0 + 1), tap(ix0 + 1, iy0 + 1)
    top = a + fx * (b - a)
    bot = c + fx * (d - c)
    out = (top + fy * (bot - top)).astype(np.float32)
    if not p["ink_high"]:
        out = (F(1) - out).astype(np.float32)
    return out
