"""ORACLE (test infrastructure) for the BUILD-DEFINED connected-component glyph rule (include/ocr_amd.h, ocr_segment_glyphs_cc):
numpy only; ocr-rs_amd/csrc/glyph_cc.hip must equal it array for array, bit for bit.  Steps 1-5 (box, quantise, Otsu, polarity,
levels) and the column fallback are tests/glyph_oracle.py's.  Kept in tests/ because oracle/ is frozen.

Per word, after steps 1-5 (a flat word gives no glyphs):
  2. a run is a maximal horizontal sequence of ink pixels in one row of the box, [a0, a1) in box columns;
  3. a component is an 8-connected set of ink pixels: runs [a0, a1) and [b0, b1) of adjacent rows are connected when a0 <= b1 and
     b0 <= a1;
  4. a component carries its half-open bounding box, its pixel count s and its anchor, the smallest raster index
     (y - Y0) * (X1 - X0) + (x - X0) of its pixels;
  5. more than MAX_RUNS runs, or more than MAX_COMPONENTS components before any filter: the word is segmented by the column rule
     (glyph_oracle.segment_word) and flag 2 is set;
  6. components with s < min_glyph_pixels are dropped;
  7. the rest is sorted by (x0, anchor);
  8. grouping walk: the first component opens a group; every next component c is compared with the last group a over the group's
     accumulated x range: ov = min(a.x1, c.x1) - max(a.x0, c.x0), nar = min(a.x1 - a.x0, c.x1 - c.x0); c joins a (boxes united,
     counts added) when merge_overlap_pct > 0 and ov > 0 and ov * 100 >= nar * merge_overlap_pct, else c opens a new group;
  9. groups with (y1 - y0) * 100 < min_height_pct * (Y1 - Y0) are dropped;
 10. the first max_glyphs groups are kept; more -> flag 1;
 11. a glyph box is the group's box in frame pixels; boxes come out ordered by x0.
word_info[:, 3] is a bit set here: 1 truncated, 2 column fallback.
"""
from __future__ import annotations

import numpy as np

from tests import glyph_oracle as G

F = np.float32
MAX_RUNS = 8192
MAX_COMPONENTS = 1024
CC_DEFAULTS = dict(merge_overlap_pct=50, min_height_pct=25)
FLAG_TRUNCATED, FLAG_FALLBACK = 1, 2


def cc_params_with(cc=None) -> dict:
    p = dict(CC_DEFAULTS)
    if cc:
        p.update(cc)
    return p


def runs_of(ink: np.ndarray) -> np.ndarray:
    """ink: bh x bw bool -> the runs in raster order, n x 3 int64 (row, a0, a1)."""
    bh, bw = ink.shape
    pad = np.zeros((bh, bw + 2), np.int8)
    pad[:, 1:-1] = ink
    d = np.diff(pad, axis=1)                   # d[:, x] = ink[x] - ink[x - 1]
    ys, a0 = np.nonzero(d == 1)                # nonzero walks row by row: raster order
    _, a1 = np.nonzero(d == -1)
    return np.stack([ys, a0, a1], axis=1).astype(np.int64).reshape(-1, 3)


def label_runs(runs: np.ndarray) -> np.ndarray:
    """The component of every run as the index of the component's first run (union-find over runs of adjacent rows)."""
    n = len(runs)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    row_start = {}
    for i, (y, _, _) in enumerate(runs.tolist()):
        row_start.setdefault(y, i)
    rl = runs.tolist()
    for i, (y, a0, a1) in enumerate(rl):
        j = row_start.get(y - 1)
        if j is None:
            continue
        while j < n and rl[j][0] == y - 1:
            b0, b1 = rl[j][1], rl[j][2]
            if a0 <= b1 and b0 <= a1:
                ri, rj = find(i), find(j)
                if ri != rj:
                    parent[max(ri, rj)] = min(ri, rj)
            j += 1
    return np.asarray([find(i) for i in range(n)], np.int64)


def components(ink: np.ndarray):
    """ink: bh x bw bool -> (runs, per component in anchor order: dict x0, y0, x1, y1 (box columns / rows, half-open), s, anchor)."""
    bw = ink.shape[1]
    runs = runs_of(ink)
    lab = label_runs(runs)
    comps = []
    for root in np.unique(lab):                # ascending root index = ascending anchor
        r = runs[lab == root]
        comps.append(dict(x0=int(r[:, 1].min()), y0=int(r[:, 0].min()), x1=int(r[:, 2].max()), y1=int(r[:, 0].max()) + 1,
                          s=int((r[:, 2] - r[:, 1]).sum()), anchor=int(runs[root, 0]) * bw + int(runs[root, 1])))
    return runs, comps


def group_components(comps, bh, params, cc):
    """Steps 6-10 on box-relative components -> (flags, [(x0, y0, x1, y1)] box-relative)."""
    kept = sorted((c for c in comps if c["s"] >= params["min_glyph_pixels"]), key=lambda c: (c["x0"], c["anchor"]))
    pct = cc["merge_overlap_pct"]
    groups = []
    for c in kept:
        if groups:
            a = groups[-1]
            ov = min(a["x1"], c["x1"]) - max(a["x0"], c["x0"])
            nar = min(a["x1"] - a["x0"], c["x1"] - c["x0"])
            if pct > 0 and ov > 0 and ov * 100 >= nar * pct:
                a["x0"], a["y0"] = min(a["x0"], c["x0"]), min(a["y0"], c["y0"])
                a["x1"], a["y1"] = max(a["x1"], c["x1"]), max(a["y1"], c["y1"])
                a["s"] += c["s"]
                continue
        groups.append(dict(c))
    groups = [g for g in groups if (g["y1"] - g["y0"]) * 100 >= cc["min_height_pct"] * bh]
    flags = FLAG_TRUNCATED if len(groups) > params["max_glyphs"] else 0
    return flags, [(g["x0"], g["y0"], g["x1"], g["y1"]) for g in groups[: params["max_glyphs"]]]


def word_ink(img: np.ndarray, X0, Y0, X1, Y1, params=None):
    """Steps 1-5 with glyph_oracle's pieces -> (t, polarity used, bg, ink, ink mask or None for a flat word)."""
    p = G.params_with(params)
    q = G.quantise(img[Y0:Y1, X0:X1])
    t, W0, S0, W1, S1 = G.otsu(np.bincount(q.ravel(), minlength=256))
    if t < 0:
        return -1, 0, F(0), F(0), None
    pol = p["polarity"]
    if pol == 0:
        pol = 1 if W0 <= W1 else 2
    mu0, mu1 = F(S0 / W0), F(S1 / W1)
    bg, ink = (mu1, mu0) if pol == 1 else (mu0, mu1)
    return t, pol, bg, ink, ((q <= t) if pol == 1 else (q > t))


def segment_word_cc(img: np.ndarray, X0, Y0, X1, Y1, params=None, cc=None, stats=None):
    """img: H x W f32 frame.  Returns (t, polarity used, flags, bg, ink, [(x0, y0, x1, y1), ...]); stats (a dict) receives the word's
    run and component counts."""
    p, c = G.params_with(params), cc_params_with(cc)
    t, pol, bg, ink, mask = word_ink(img, X0, Y0, X1, Y1, p)
    if mask is None:
        return -1, 0, 0, F(0), F(0), []
    n_runs = len(runs_of(mask))
    n_comps = -1
    if n_runs <= MAX_RUNS:
        _, comps = components(mask)
        n_comps = len(comps)
    if stats is not None:
        stats.update(runs=n_runs, components=n_comps)
    if n_runs > MAX_RUNS or n_comps > MAX_COMPONENTS:
        t2, pol2, trunc, bg2, ink2, boxes = G.segment_word(img, X0, Y0, X1, Y1, p)
        assert (t2, pol2) == (t, pol) and bg2 == bg and ink2 == ink
        return t, pol, trunc | FLAG_FALLBACK, bg, ink, boxes
    flags, rel = group_components(comps, Y1 - Y0, p, c)
    return t, pol, flags, bg, ink, [(X0 + a, Y0 + b, X0 + cc_, Y0 + d) for a, b, cc_, d in rel]


def segment_cc(frames: np.ndarray, polys, adj, params=None, cc=None, stats=None) -> dict:
    """frames: N x 1 x H x W f32 (raw 0..255); polys, adj as glyph_oracle.segment.  Returns the arrays of ocr_glyphs_t; stats (a list)
    receives one dict per word."""
    n, _, h, w = frames.shape
    info, levels, boxes, woff = [], [], [], [0]
    for b, X0, Y0, X1, Y1 in G.word_boxes(polys, adj, h, w):
        st = {}
        t, pol, flags, bg, ink, bx = segment_word_cc(frames[b, 0], X0, Y0, X1, Y1, params, cc, st)
        if stats is not None:
            stats.append(st)
        info.append((b, t, pol, flags))
        levels.append((bg, ink))
        boxes.extend(bx)
        woff.append(len(boxes))
    return dict(img_offsets=np.cumsum([0] + [len(p) for p in polys]).astype(np.int32),
                word_offsets=np.asarray(woff, np.int32),
                word_info=np.asarray(info, np.int32).reshape(-1, 4),
                word_levels=np.asarray(levels, np.float32).reshape(-1, 2),
                boxes=np.asarray(boxes, np.int32).reshape(-1, 4))
