"""ORACLE (test infrastructure) for the BUILD-DEFINED word strip rule: detected word (polygon, possibly rotated) -> minimum-area rectangle
-> upright strip of strip_height rows, all strips of a batch side by side in one atlas.

The reference never built this step; this file restates the rule of include/ocr_amd.h (ocr_plan_word_strips, ocr_extract_word_strips)
and ocr-rs_amd/csrc/word_strips.cpp / strips.hip must equal it bit for bit.  Frame coordinates are continuous (pixel p spans [p, p + 1));
a vertex (x, y) is the point (x * adj_x, y * adj_y).  Geometry in Python floats (IEEE f64, every operation separately rounded, as the C++
is compiled without FMA contraction); math.sqrt is correctly rounded, as std::sqrt is.  Per polygon:
  1. convex hull of the integer vertices, exact (Andrew's monotone chain): repeated vertices merged, collinear points dropped,
     counter-clockwise in the x-right / y-up sense, starting at the smallest (x, y); a coordinate >= 2^24 or no vertex is an error;
     m < 3 hull vertices flags the word degenerate; hull vertices mapped to (x * adj_x, y * adj_y);
  2. per hull edge i (m >= 3: all m edges; m = 2: edge 0; m = 1: e = (1, 0) from P_0): a = dx*ex + dy*ey, b = dy*ex - dx*ey over the
     hull vertices, area = ((a1 - a0) * (b1 - b0)) / ee; the smallest area wins, ties to the smaller i; corners R0 = (a0, b0),
     R1 = (a1, b0), R2 = (a1, b1), R3 = (a0, b1) at (P_ix + (a*ex - b*ey) / ee, P_iy + (a*ey + b*ex) / ee);
  3. u = the one of +e, +e' = (-ey, ex), -e, -e' with the largest x, ties to the smaller y; TL, TR, BR, BL = R shifted cyclically by the
     index of u in that list; v = (-u_y, u_x);
  4. U = TR - TL, V = BL - TL; a side under 1 is widened to 1 about the centre (U first, then V; lengths taken again after each);
  5. Ws = floor((Hs * |U|) / |V| + 0.5) clamped to [1, max_width] (above: squeezed);
  6. map (f32): TL, U / Ws, V / Hs.
Sampling, f32: sx = ((ox + (c + 0.5) * ux) + (i + 0.5) * vx) - 0.5 (sy likewise), clamped with fminf / fmaxf semantics (NaN -> 0), bilinear
taps in oracle/crop_oracle.py's operation order, raw values.
"""
from __future__ import annotations

import math

import numpy as np

F = np.float32
DEFAULTS = dict(strip_height=32, max_width=1024)
COORD_LIMIT = 1 << 24
MAX_ATLAS = 1 << 31
SQUEEZED, DEGENERATE = 1, 2


def params_with(params=None) -> dict:
    p = dict(DEFAULTS)
    if params:
        p.update(params)
    return p


def convex_hull(pts):
    """Integer points -> hull vertices (counter-clockwise with y up, collinear dropped, from the smallest (x, y))."""
    pts = sorted(set((int(x), int(y)) for x, y in pts))
    if len(pts) < 2:
        return pts

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    h = []
    for p in pts:
        while len(h) >= 2 and cross(h[-2], h[-1], p) <= 0:
            h.pop()
        h.append(p)
    lower = len(h)
    for p in reversed(pts[:-1]):
        while len(h) > lower and cross(h[-2], h[-1], p) <= 0:
            h.pop()
        h.append(p)
    h.pop()
    return h


def _widen(C, lo, hi, length, ux, uy):
    h = (1.0 - length) * 0.5
    s = math.sqrt(ux * ux + uy * uy)
    dx, dy = h * (ux / s), h * (uy / s)
    for k in lo:
        C[k] = (C[k][0] - dx, C[k][1] - dy)
    for k in hi:
        C[k] = (C[k][0] + dx, C[k][1] + dy)


def plan_word(poly, ax: float, ay: float, hs: int, max_width: int):
    """One polygon -> (quad [(x, y)] * 4 as TL, TR, BR, BL, map (6 f32), Ws, flags)."""
    if len(poly) == 0:
        raise ValueError("polygon without vertices")
    for x, y in poly:
        if not (0 <= x < COORD_LIMIT and 0 <= y < COORD_LIMIT):
            raise ValueError(f"vertex ({x}, {y}) beyond 2^24")
    hull = convex_hull(poly)
    m = len(hull)
    P = [(float(x) * ax, float(y) * ay) for x, y in hull]
    best = None
    for i in range(m if m >= 3 else 1):
        ex, ey = (P[(i + 1) % m][0] - P[i][0], P[(i + 1) % m][1] - P[i][1]) if m >= 2 else (1.0, 0.0)
        ee = ex * ex + ey * ey
        a_s, b_s = [], []
        for qx, qy in P:
            dx, dy = qx - P[i][0], qy - P[i][1]
            a_s.append(dx * ex + dy * ey)
            b_s.append(dy * ex - dx * ey)
        a0, a1, b0, b1 = min(a_s), max(a_s), min(b_s), max(b_s)
        area = ((a1 - a0) * (b1 - b0)) / ee
        if best is None or area < best[0]:
            best = (area, i, a0, a1, b0, b1, ex, ey)
    _, i, a0, a1, b0, b1, ex, ey = best
    ee = ex * ex + ey * ey
    px, py = P[i]

    def corner(a, b):
        return (px + (a * ex - b * ey) / ee, py + (a * ey + b * ex) / ee)
    R = [corner(a0, b0), corner(a1, b0), corner(a1, b1), corner(a0, b1)]
    cand = [(ex, ey), (-ey, ex), (-ex, -ey), (ey, -ex)]
    d = min(range(4), key=lambda c: (-cand[c][0], cand[c][1]))
    ux, uy = cand[d]
    vx, vy = -uy, ux
    C = [R[(c + d) % 4] for c in range(4)]

    def sides():
        U = (C[1][0] - C[0][0], C[1][1] - C[0][1])
        V = (C[3][0] - C[0][0], C[3][1] - C[0][1])
        return U, V, math.sqrt(U[0] * U[0] + U[1] * U[1]), math.sqrt(V[0] * V[0] + V[1] * V[1])
    U, V, lu, lv = sides()
    if lu < 1.0:
        _widen(C, (0, 3), (1, 2), lu, ux, uy)
        U, V, lu, lv = sides()
    if lv < 1.0:
        _widen(C, (0, 1), (3, 2), lv, vx, vy)
        U, V, lu, lv = sides()
    wd = math.floor((float(hs) * lu) / lv + 0.5)
    flags = DEGENERATE if m < 3 else 0
    if wd > max_width:
        ws = max_width
        flags |= SQUEEZED
    else:
        ws = max(int(wd), 1)
    mp = np.array([C[0][0], C[0][1], U[0] / ws, U[1] / ws, V[0] / hs, V[1] / hs], np.float64).astype(np.float32)
    return C, mp, ws, flags


def plan(polys, adj, scores=None, params=None) -> dict:
    """polys: per image the polygons in original-image pixels; adj: N x 2.  Returns the arrays of ocr_word_strips_t."""
    p = params_with(params)
    hs, mw = p["strip_height"], p["max_width"]
    info, quads, maps, cols = [], [], [], [0]
    for b, plist in enumerate(polys):
        ax, ay = float(adj[b][0]), float(adj[b][1])
        if not (math.isfinite(ax) and ax > 0 and math.isfinite(ay) and ay > 0):
            raise ValueError(f"adjust values ({ax}, {ay})")
        for poly in plist:
            C, mp, ws, flags = plan_word(poly, ax, ay, hs, mw)
            info.append((b, flags))
            quads.append([c for xy in C for c in xy])
            maps.append(mp)
            cols.append(cols[-1] + ws)
            if cols[-1] * hs > MAX_ATLAS:
                raise ValueError("atlas of more than 2^31 elements")
    nw = len(info)
    sc = [s for ss in scores for s in ss] if scores is not None else [0.0] * nw
    return dict(img_offsets=np.cumsum([0] + [len(pl) for pl in polys]).astype(np.int32), col_offsets=np.asarray(cols, np.int32),
                word_info=np.asarray(info, np.int32).reshape(-1, 2), quads=np.asarray(quads, np.float64).reshape(-1, 8),
                maps=np.asarray(maps, np.float32).reshape(-1, 6), scores=np.asarray(sc, np.float64), height=hs, total_width=int(cols[-1]))


def extract(frames: np.ndarray, strips: dict) -> np.ndarray:
    """frames: N x 1 x H x W f32 (raw 0..255) -> the atlas, height x total_width f32."""
    n, _, h, w = frames.shape
    hs, tw = strips["height"], strips["total_width"]
    if tw == 0:
        return np.zeros((hs, 0), np.float32)
    cols = strips["col_offsets"]
    word = np.repeat(np.arange(len(cols) - 1), np.diff(cols))
    mp = strips["maps"][word]                                           # tw x 6
    fr = strips["word_info"][word, 0].astype(np.int64)[None, :]
    fc = ((np.arange(tw) - cols[word]).astype(np.float32) + F(0.5))[None, :]
    fi = (np.arange(hs).astype(np.float32) + F(0.5))[:, None]
    ox, oy, ux, uy, vx, vy = (mp[:, k][None, :] for k in range(6))
    sx = ((ox + fc * ux) + fi * vx) - F(0.5)
    sy = ((oy + fc * uy) + fi * vy) - F(0.5)
    sx = np.fmin(np.fmax(sx, F(0)), F(w - 1))                          # fminf / fmaxf: NaN -> the other operand
    sy = np.fmin(np.fmax(sy, F(0)), F(h - 1))
    ix0 = np.floor(sx).astype(np.int64)
    iy0 = np.floor(sy).astype(np.int64)
    ix1 = np.minimum(ix0 + 1, w - 1)
    iy1 = np.minimum(iy0 + 1, h - 1)
    fx = sx - ix0.astype(np.float32)
    fy = sy - iy0.astype(np.float32)
    flat = frames.reshape(n, h * w)
    fr = np.broadcast_to(fr, sx.shape)
    a, b = flat[fr, iy0 * w + ix0], flat[fr, iy0 * w + ix1]
    c, d = flat[fr, iy1 * w + ix0], flat[fr, iy1 * w + ix1]
    with np.errstate(invalid="ignore"):          # inf - inf in a tap: NaN, as on the device
        top = a + fx * (b - a)
        bot = c + fx * (d - c)
        return (top + fy * (bot - top)).astype(np.float32)


def strip_polygons(strips: dict):
    """ocr_word_strip_polygons: one image, per word the rectangle (c0, 0), (c1 - 1, 0), (c1 - 1, Hs - 1), (c0, Hs - 1)."""
    cols, y1 = strips["col_offsets"], strips["height"] - 1
    return [[[(int(cols[k]), 0), (int(cols[k + 1]) - 1, 0), (int(cols[k + 1]) - 1, y1), (int(cols[k]), y1)] for k in range(len(cols) - 1)]]


def glyph_quads(strips: dict, word: int, boxes: np.ndarray) -> np.ndarray:
    """Glyph boxes (x0, y0, x1, y1 half-open atlas pixels) of word `word` -> k x 4 x 2 f64 frame coordinates of the corners (x0, y0),
    (x1, y0), (x1, y1), (x0, y1), mapped through the word's quad: TL + cs * (U / Ws) + is * (V / Hs), in that order."""
    q = strips["quads"][word]
    hs = float(strips["height"])
    c0 = int(strips["col_offsets"][word])
    ws = float(strips["col_offsets"][word + 1] - c0)
    tlx, tly = q[0], q[1]
    cux, cuy = (q[2] - q[0]) / ws, (q[3] - q[1]) / ws
    rvx, rvy = (q[6] - q[0]) / hs, (q[7] - q[1]) / hs
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    cs = np.stack([b[:, 0], b[:, 2], b[:, 2], b[:, 0]], axis=1).astype(np.float64) - float(c0)
    rs = np.stack([b[:, 1], b[:, 1], b[:, 3], b[:, 3]], axis=1).astype(np.float64)
    return np.stack([(tlx + cs * cux) + rs * rvx, (tly + cs * cuy) + rs * rvy], axis=2)
