"""Polygons for the box-score rasteriser (box_score.hip) and a copy of the oracle's draw_polygon with SWITCHABLE rules.

box_score.hip evaluates imageproc's draw_polygon_mut in closed form per pixel; each closed form has one subtle way to be wrong that a
blind fuzz hardly notices, because the outline covers most one-pixel shifts of the fill:

    intersections   f32 divide, multiply, add, each rounded on its own, then round half away from zero ("spec").  Wrong variants:
                    "fma"   a fused multiply-add (the product is not rounded): what a compiler does when it contracts a*b + c
                    "even"  round half to even (rintf instead of roundf)
                    "f64"   the intersection in f64 (or exact) arithmetic
    outline         BresenhamLineIter steps y when its error is < 0 ("lt").  Wrong variant: "le", <= 0, which moves the step at a tie
                    (2*k*dy == dx (mod 2*dx): the closed form's floor((2*k*dy + dx - 1) / (2*dx)) with the -1 dropped)

draw_polygon_rules is the oracle's draw_polygon with those two switches; tests/test_box_score_cases.py holds it to the oracle itself
on every polygon below, so the copy cannot drift.  PINNED is a fixed list of polygons whose MASK changes under a wrong rule, found by
search_rule_sensitive (seeded; `python -m tests.box_score_cases` prints the list): every wrong rule changes at least 24 of them, so a
kernel with that defect fails tests/test_gpu_box_score_kernel.py on every run, not on one in a thousand.

The generators are deterministic: the CPU test and the GPU test see the same polygons."""
import math
import sys
import time

import numpy as np

from oracle import postproc_oracle as O

INTER_RULES = ("spec", "fma", "even", "f64")
TIE_RULES = ("lt", "le")
MUTANTS = (("fma", "lt"), ("even", "lt"), ("f64", "lt"), ("spec", "le"))   # (intersection rule, outline tie rule)


# ---------------------------------------------------------------------------------------------------------------- the switchable copy
def _round_half_away(f: float) -> int:
    return int(math.floor(f + 0.5)) if f >= 0 else -int(math.floor(-f + 0.5))


def _intersection(p0, p1, y: int, rule: str) -> int:
    if rule == "f64":
        return _round_half_away(p0[0] + (y - p0[1]) / (p1[1] - p0[1]) * (p1[0] - p0[0]))
    frac = np.float32(y - p0[1]) / np.float32(p1[1] - p0[1])
    d = np.float32(p1[0] - p0[0])
    if rule == "fma":   # the f32 x f32 product is exact in f64; one rounding, of the sum
        v = np.float32(np.float64(p0[0]) + np.float64(frac) * np.float64(d))
    else:
        v = np.float32(p0[0]) + np.float32(frac * d)
    if rule == "even":
        return int(np.rint(np.float64(v)))
    return _round_half_away(float(v))


def _bresenham_rules(canvas: np.ndarray, s, e, tie: str) -> None:
    hh, ww = canvas.shape
    x0, y0, x1, y1 = float(s[0]), float(s[1]), float(e[0]), float(e[1])
    steep = abs(y1 - y0) > abs(x1 - x0)
    if steep:
        x0, y0, x1, y1 = y0, x0, y1, x1
    if x0 > x1:
        x0, x1, y0, y1 = x1, x0, y1, y0
    dx = np.float32(x1 - x0)
    dy = np.float32(abs(y1 - y0))
    err = np.float32(dx / np.float32(2))
    ystep = 1 if y0 < y1 else -1
    x, y, endx = int(x0), int(y0), int(x1)
    while x <= endx:
        px, py = (y, x) if steep else (x, y)
        if 0 <= px < ww and 0 <= py < hh:
            canvas[py, px] = 255
        x += 1
        err = np.float32(err - dy)
        if (err <= 0) if tie == "le" else (err < 0):
            y += ystep
            err = np.float32(err + dx)


def draw_polygon_rules(canvas: np.ndarray, poly, inter: str = "spec", tie: str = "lt") -> None:
    """O.draw_polygon with the intersection rule and the outline's tie rule switchable; ("spec", "lt") is the oracle."""
    assert inter in INTER_RULES and tie in TIE_RULES
    if not poly:
        return
    if poly[0] == poly[-1]:
        raise ValueError("First point == last point")
    hh, ww = canvas.shape
    ys = [p[1] for p in poly]
    y_min = max(0, min(min(ys), hh - 1))
    y_max = max(0, min(max(ys), hh - 1))
    closed = list(poly) + [poly[0]]
    for y in range(y_min, y_max + 1):
        xs = []
        for i in range(len(closed) - 1):
            p0, p1 = closed[i], closed[i + 1]
            if (p0[1] <= y <= p1[1]) or (p1[1] <= y <= p0[1]):
                if p0[1] == p1[1]:
                    xs.append(p0[0])
                    xs.append(p1[0])
                elif p0[1] == y or p1[1] == y:
                    if p1[1] > y:
                        xs.append(p0[0])
                    if p0[1] > y:
                        xs.append(p1[0])
                else:
                    xs.append(_intersection(p0, p1, y, inter))
        xs.sort()
        for k in range(0, len(xs) - 1, 2):
            frm = min(xs[k], ww)
            to = min(xs[k + 1], ww - 1)
            if frm < ww and to >= 0:
                frm = max(0, frm)
                to = max(0, to)
                if to >= frm:
                    canvas[y, frm:to + 1] = 255
    for i in range(len(closed) - 1):
        _bresenham_rules(canvas, closed[i], closed[i + 1], tie)


# ---------------------------------------------------------------------------------------------------------------- boxes and references
def job_box(pts, h: int, w: int):
    """the mask canvas of box_score_fast on an h x w map as (min_x, min_y, bw, bh): x clamped by H, y by W (metrics.rs:151-166)"""
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    cl = lambda v, hi: min(max(v, 0), hi - 1)   # noqa: E731
    x0, x1, y0, y1 = cl(min(xs), h), cl(max(xs), h), cl(min(ys), w), cl(max(ys), w)
    return (x0, y0, x1 - x0 + 1, y1 - y0 + 1)


def extent(pts):
    """the polygon's own bounding box, same layout"""
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    return (min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1)


def fits(pts, h: int, w: int) -> bool:
    """whether the clamped box lies on the map (where it does not, the reference fails in narrow() and the library refuses the map)"""
    x0, y0, bw, bh = job_box(pts, h, w)
    return x0 + bw <= w and y0 + bh <= h


def mask_on_map(pts, h: int, w: int, inter: str = "spec", tie: str = "lt", draw=None):
    """(box, bool mask of the box) as box_score_fast draws it on an h x w map; draw=O.draw_polygon takes the oracle itself"""
    x0, y0, bw, bh = job_box(pts, h, w)
    canvas = np.zeros((bh, bw), np.uint8)
    moved = [(p[0] - x0, p[1] - y0) for p in pts]
    if draw is not None:
        draw(canvas, moved)
    else:
        draw_polygon_rules(canvas, moved, inter, tie)
    return (x0, y0, bw, bh), canvas > 0


def oracle_sum_count(pred: np.ndarray, pts):
    """(sum, count, box) of box_score_fast's mask over pred (H x W, f32), through O.draw_polygon: the values summed in f64, in the
    oracle's own expression, so that sum / count IS O.box_score_fast(pred, pts)"""
    h, w = pred.shape
    (x0, y0, bw, bh), m = mask_on_map(pts, h, w, draw=O.draw_polygon)
    part = pred[y0:y0 + bh, x0:x0 + bw]
    m8 = m.astype(np.uint8)
    return float(np.sum((part * m8).astype(np.float64))), int(np.sum(m8, dtype=np.float64)), (x0, y0, bw, bh)


def as_poly(p):
    return [(int(x), int(y)) for x, y in p]


# ---------------------------------------------------------------------------------------------------------------- octants and ties
OCTANT_MAP = (64, 64)


def octant_polys():
    """Every edge direction (dx, dy) with |dx|, |dy| <= 9 as a thin quadrilateral, in both orientations: all eight octants, the axes and
    the diagonals, the outline's ties (2*k*dy == dx: (2,1), (4,2), (6,1), (6,3), (8,4) ...) and the fill's (dy == 2, dx odd: the middle row
    crosses at k + 0.5).  Then longer edges of both tie kinds as triangles and quadrilaterals."""
    out = []
    a = (12, 12)
    for dx in range(-9, 10):
        for dy in range(-9, 10):
            if dx == 0 and dy == 0:
                continue
            b = (a[0] + dx, a[1] + dy)
            off = (0, 2) if abs(dx) >= abs(dy) else (2, 0)
            quad = [a, b, (b[0] + off[0], b[1] + off[1]), (a[0] + off[0], a[1] + off[1])]
            out.append(quad)
            out.append(quad[::-1])
    for dx, dy in ((2, 1), (6, 1), (10, 1), (6, 3), (10, 5), (14, 7), (18, 9), (20, 2), (30, 3), (30, 5), (26, 13)):   # outline ties
        for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
            for ex, ey in ((dx, dy), (dy, dx)):
                p0 = (32, 32)
                p1 = (32 + sx * ex, 32 + sy * ey)
                out.append([p0, p1, (p0[0] - sy * 3, p0[1] + sx * 3)])
                out.append([p0, (p0[0] - sy * 3, p0[1] + sx * 3), p1])
    for dx, dy in ((1, 2), (3, 2), (5, 2), (7, 2), (21, 2), (2, 4), (6, 4), (10, 4), (22, 4), (3, 6), (9, 6), (15, 6), (13, 26), (29, 2)):   # fill ties: k + 0.5
        for sx in (1, -1):
            for sy in (1, -1):
                p0 = (32, 32)
                p1 = (32 + sx * dx, 32 + sy * dy)
                out.append([p0, p1, (p1[0], p1[1] + sy * 4), (p0[0], p0[1] + sy * 4)])
                out.append([p0, (p0[0] - sx * 15, p0[1] + sy * dy), p1])
    return [as_poly(p) for p in out]


# ---------------------------------------------------------------------------------------------------------------- scanline rules
SCANLINE_MAP = (64, 64)


def _star(cx, cy, r, n, step):
    return [(int(round(cx + r * math.sin(2 * math.pi * ((i * step) % n) / n))), int(round(cy - r * math.cos(2 * math.pi * ((i * step) % n) / n))))
            for i in range(n)]


def scanline_polys():
    """(name, polygon) on a 64 x 64 map: what the scanline rules of draw_polygon_mut decide"""
    cases = [
        ("vertices as local extrema (W)", [(10, 10), (20, 30), (30, 10), (40, 30), (50, 10), (50, 40), (10, 40)]),
        ("vertices as local extrema (M)", [(10, 40), (20, 20), (30, 40), (40, 20), (50, 40), (50, 8), (10, 8)]),
        ("extrema inside a row of other crossings", [(5, 5), (58, 5), (58, 50), (45, 25), (32, 50), (20, 25), (5, 50)]),
        ("monotone pass-through vertices", [(10, 5), (20, 15), (25, 25), (15, 35), (5, 20)]),
        ("pass-through on both chains", [(30, 2), (40, 12), (44, 22), (40, 32), (30, 42), (20, 32), (16, 22), (20, 12)]),
        ("horizontal edges top, middle, bottom", [(10, 10), (30, 10), (30, 20), (40, 20), (40, 30), (5, 30), (5, 20), (10, 20)]),
        ("horizontal edge in the middle, reversed", [(10, 20), (5, 20), (5, 30), (40, 30), (40, 20), (30, 20), (30, 10), (10, 10)]),
        ("horizontal notch from below", [(5, 5), (55, 5), (55, 40), (40, 40), (40, 25), (20, 25), (20, 40), (5, 40)]),
        ("repeated points", [(10, 10), (10, 10), (30, 12), (30, 12), (30, 12), (20, 30)]),
        ("collinear points", [(5, 5), (15, 5), (25, 5), (25, 15), (25, 25), (15, 15)]),
        ("collinear on a slanted edge", [(5, 5), (15, 10), (25, 15), (35, 20), (10, 40)]),
        ("zero-area line, slanted", [(36, 36), (34, 38), (34, 39), (34, 38)]),
        ("zero-area line, horizontal", [(5, 50), (30, 50), (17, 50)]),
        ("zero-area line, vertical", [(50, 5), (50, 30), (50, 17)]),
        ("zero-area line, diagonal", [(3, 3), (20, 20), (10, 10)]),
        ("zero-area line, shallow", [(3, 60), (40, 55), (3, 60), (40, 55), (21, 57)]),
        ("two points", [(7, 7), (20, 12)]),
        ("pentagram", _star(32, 32, 28, 5, 2)),
        ("heptagram 7/3", _star(32, 32, 30, 7, 3)),
        ("heptagram 7/2", _star(30, 33, 27, 7, 2)),
        ("bow-tie", [(10, 10), (50, 40), (50, 10), (10, 40)]),
        ("bow-tie, upright", [(10, 10), (40, 10), (10, 50), (40, 50)]),
        ("bow-tie crossing at a pixel centre", [(10, 10), (30, 30), (30, 10), (10, 30)]),
        ("self-touching", [(5, 30), (30, 31), (29, 50), (6, 63), (5, 40), (20, 42)]),
        ("zig-zag sliver", [(60, 5), (61, 30), (62, 5), (63, 30)]),
        ("zig-zag sliver, long", [(10 + 3 * i, 5 if i % 2 == 0 else 45) for i in range(12)]),
        ("zig-zag sliver, sideways", [(5 if i % 2 == 0 else 55, 8 + 2 * i) for i in range(15)]),
        ("comb", [(4, 60), (4, 10), (8, 60), (12, 10), (16, 60), (20, 10), (24, 60), (28, 10), (32, 60)]),
    ]
    return [(n, as_poly(p)) for n, p in cases]


# ---------------------------------------------------------------------------------------------------------------- random fuzz
FUZZ_MAPS = ((96, 96), (48, 160), (160, 48))
FUZZ_PER_MAP = 520


def fuzz_polys(seed: int = 20260):
    """[(map index, polygon)]: FUZZ_PER_MAP tries per map of 3..12 points with spans 3 / 8 / 40 / 160.  On an H x W map the mask canvas
    lies inside the min(H, W) square (x is clamped by H, y by W), and a coordinate that would put the box off the map is not allowed:
    that axis is capped at the map's edge, the other one is free, and the polygon's origin is drawn from a little before 0 to a little
    past the square's far side - so that whole polygons (unclipped), partly clipped ones and ones wholly outside (empty mask) all occur."""
    rng = np.random.default_rng(seed)
    out = []
    for mi, (h, w) in enumerate(FUZZ_MAPS):
        side = min(h, w)
        cap_x = w - 1 if h > w else None    # max x must stay < W where the clamp by H does not see to it
        cap_y = h - 1 if w > h else None
        for _ in range(FUZZ_PER_MAP):
            k = int(rng.integers(3, 13))
            span = int(rng.choice([3, 8, 40, 160]))
            ox = int(rng.integers(-(span // 3) - 2, side + 3))
            oy = int(rng.integers(-(span // 3) - 2, side + 3))
            pts = []
            for _i in range(k):
                x = ox + int(rng.integers(0, span))
                y = oy + int(rng.integers(0, span))
                if cap_x is not None:
                    x = min(x, cap_x)
                if cap_y is not None:
                    y = min(y, cap_y)
                pts.append((x, y))
            if pts[0] == pts[-1]:   # imageproc panics
                continue
            assert fits(pts, h, w)
            out.append((mi, pts))
    return out


def clip_class(pts, h: int, w: int, count: int) -> str:
    """"empty" (no mask pixel), "unclipped" (the canvas is the polygon's extent) or "clipped" (non-empty on a smaller canvas)"""
    if count == 0:
        return "empty"
    return "unclipped" if job_box(pts, h, w) == extent(pts) else "clipped"


# ---------------------------------------------------------------------------------------------------------------- many vertices
MANY_MAP = (224, 224)


def many_vertex_poly(n: int, seed: int = 7):
    """a jittered ellipse of about 200 x 40 px with exactly n points (consecutive points repeat: the perimeter is far shorter than n)"""
    rng = np.random.default_rng(seed + n)
    pts = []
    for i in range(n):
        t = 2 * math.pi * i / n
        pts.append((int(round(110 + (98 + rng.uniform(-2, 2)) * math.cos(t))), int(round(100 + (18 + rng.uniform(-2, 2)) * math.sin(t)))))
    if pts[0] == pts[-1]:
        pts[-1] = (pts[-1][0], pts[-1][1] - 1)
    return pts


# ---------------------------------------------------------------------------------------------------------------- row bands
BAND_MAP = (1024, 1024)
TALL_MAP = (4128, 4128)


def band_polys():
    """(name, polygon) on a 1024 x 1024 map.  The kernel keeps 8192 mask words in LDS and walks the canvas in bands of 8192 / wpr rows
    (wpr = words per row): 256 rows at bw = 1024, 910 at wpr = 9, 744 at wpr = 11."""
    cases = [
        ("bw 1024: vertices and horizontal edges on rows 255 / 256 / 511 / 512",
         [(0, 10), (1023, 255), (600, 255), (600, 256), (1023, 256), (1023, 511), (300, 511), (300, 512), (1023, 512), (1023, 1000), (0, 1023),
          (0, 512), (200, 511), (0, 256), (100, 255), (0, 0)]),
        ("bw 1024: outline across band edges, shallow and steep", [(500, 0), (0, 250), (1023, 260), (510, 1023), (490, 1023)]),
        ("bw 1024: shallow slivers on the band edges", [(0, 255), (1023, 256), (0, 511), (1023, 512), (0, 767), (1023, 768), (1023, 0), (1000, 1023)]),
        ("bw 33, few points", [(100, 0), (132, 500), (110, 1023), (105, 400)]),
        ("bw 97, few points", [(200, 5), (296, 300), (250, 1020), (210, 600)]),
        ("bw 260 (wpr 9, 910.2 rows per band): vertices on rows 909 / 910", [(300, 0), (559, 400), (400, 1023), (310, 909), (300, 910)]),
        ("bw 330 (wpr 11, 744.7 rows per band): horizontal edges on rows 743 / 744", [(600, 0), (929, 743), (700, 743), (700, 744), (929, 744), (929, 1023), (600, 1023)]),
        ("bw 1", [(7, 3), (7, 900), (7, 500)]),
        ("bh 1", [(3, 7), (1000, 7), (500, 7)]),
        ("1 x 1 at the origin, one pixel", [(0, 0), (-5, -2), (-3, -6)]),
        ("1 x 1 at the origin, empty", [(-5, -5), (-1, -9), (-8, -2)]),
        ("1 x 1 at the far corner, empty", [(1030, 1040), (1100, 1030), (1050, 1100)]),
        ("1 x 1 at the far corner, one pixel", [(1023, 1023), (1100, 1030), (1050, 1100)]),
    ]
    return [(n, as_poly(p)) for n, p in cases]


def tall_band_polys():
    """(name, polygon) on a 4128 x 4128 map: canvases of bw 33 (wpr 2, 4096 rows per band) and bw 97 (wpr 4, 2048) taller than one band"""
    cases = [
        ("bw 33, bh 4101: vertices on rows 4095 / 4096", [(50, 0), (82, 2000), (60, 4100), (55, 4095), (52, 4096)]),
        ("bw 97, bh 4101: horizontal edge on rows 2047 / 2048 of the canvas", [(200, 10), (296, 2057), (230, 2057), (230, 2058), (296, 2058), (296, 4110), (200, 4105)]),
    ]
    return [(n, as_poly(p)) for n, p in cases]


# ---------------------------------------------------------------------------------------------------------------- rule-sensitive polygons
def pinned_map(pts):
    """the square map just large enough for a pinned polygon: its box is the polygon's extent"""
    side = max(max(p[0] for p in pts), max(p[1] for p in pts)) + 1
    return (side, side)


def pinned_pred(k: int) -> np.ndarray:
    """the probability map the GPU test scores PINNED[k] on"""
    return np.random.default_rng(1000 + k).random(pinned_map(PINNED[k]), dtype=np.float32)


def sum_count_under(pred: np.ndarray, pts, inter: str, tie: str):
    """(sum, count) of the mask drawn with the given rules"""
    h, w = pred.shape
    (x0, y0, bw, bh), m = mask_on_map(pts, h, w, inter, tie)
    return float(pred[y0:y0 + bh, x0:x0 + bw][m].astype(np.float64).sum()), int(m.sum())


def mutants_changing(pts):
    """the wrong rules (entries of MUTANTS) that change this polygon's mask on its pinned map"""
    h, w = pinned_map(pts)
    _, base = mask_on_map(pts, h, w)
    return [mu for mu in MUTANTS if not np.array_equal(mask_on_map(pts, h, w, *mu)[1], base)]


def search_rule_sensitive(seed: int = 5, per_rule: int = 28, seconds: float = 240.0):
    """Random 3..6-gons with coordinates below 200 (spans 16 / 64 / 200), kept while some wrong rule that still has fewer than per_rule
    polygons changes their mask.  Returns (polygons, {rule: count}, polygons tried)."""
    rng = np.random.default_rng(seed)
    hits = {mu: 0 for mu in MUTANTS}
    kept, tried, t0 = [], 0, time.time()
    while min(hits.values()) < per_rule and time.time() - t0 < seconds:
        span = int(rng.choice([16, 64, 200]))
        k = int(rng.integers(3, 7))
        pts = [(int(rng.integers(0, span)), int(rng.integers(0, span))) for _ in range(k)]
        if pts[0] == pts[-1]:
            continue
        tried += 1
        ch = mutants_changing(pts)
        if any(hits[mu] < per_rule for mu in ch):
            kept.append(tuple(pts))
            for mu in ch:
                hits[mu] += 1
    return kept, hits, tried


# 98 polygons kept of 7297 tried (46 s); masks changed: fma 30, even 74, f64 28, outline tie 89
PINNED = (
    ((4, 161), (93, 103), (126, 57), (195, 10), (55, 76), (114, 81)),
    ((11, 4), (23, 43), (7, 55), (21, 14), (34, 57), (56, 55)),
    ((12, 11), (12, 0), (0, 8)),
    ((59, 13), (33, 20), (18, 51), (9, 20)),
    ((4, 11), (9, 7), (2, 12)),
    ((11, 63), (29, 159), (103, 101)),
    ((15, 3), (12, 0), (5, 14), (13, 1), (13, 13)),
    ((62, 60), (43, 25), (13, 59), (17, 35)),
    ((63, 148), (39, 134), (188, 136)),
    ((61, 14), (22, 41), (41, 6), (10, 44)),
    ((186, 75), (65, 159), (8, 38), (38, 78), (31, 159)),
    ((5, 142), (21, 122), (34, 188), (135, 198)),
    ((24, 51), (7, 9), (23, 45), (31, 54), (60, 25)),
    ((41, 30), (38, 61), (46, 20), (27, 25), (9, 0)),
    ((70, 126), (112, 186), (123, 184), (115, 65)),
    ((9, 3), (13, 13), (0, 2), (11, 6), (5, 1), (3, 13)),
    ((114, 27), (64, 105), (199, 51), (109, 98), (100, 110), (140, 21)),
    ((153, 55), (88, 89), (61, 11), (148, 0), (152, 39), (128, 68)),
    ((8, 6), (14, 9), (15, 11), (9, 8), (3, 11), (12, 11)),
    ((47, 2), (51, 9), (19, 13)),
    ((16, 3), (62, 13), (12, 38)),
    ((12, 5), (6, 5), (11, 6), (4, 10), (2, 12), (6, 15)),
    ((20, 101), (73, 145), (185, 106), (149, 63), (115, 98), (146, 10)),
    ((15, 8), (7, 7), (0, 13)),
    ((124, 111), (76, 98), (176, 119)),
    ((44, 33), (53, 36), (39, 31), (37, 39), (57, 15)),
    ((21, 43), (52, 12), (3, 63), (32, 47), (48, 61)),
    ((3, 35), (11, 29), (7, 17), (26, 31), (1, 59)),
    ((113, 12), (4, 42), (144, 83)),
    ((47, 30), (19, 24), (12, 60), (1, 23), (4, 56), (41, 26)),
    ((13, 8), (14, 8), (14, 9), (5, 9), (11, 12), (15, 4)),
    ((9, 14), (14, 7), (0, 15), (3, 2)),
    ((7, 15), (0, 10), (4, 3), (10, 10), (12, 3), (13, 5)),
    ((167, 48), (88, 165), (162, 1), (133, 11), (126, 12), (115, 186)),
    ((18, 0), (33, 59), (46, 14), (16, 16), (36, 37), (38, 13)),
    ((7, 3), (4, 10), (14, 13)),
    ((0, 0), (13, 3), (12, 6), (9, 8), (8, 12), (11, 8)),
    ((14, 45), (56, 52), (38, 0)),
    ((61, 18), (44, 61), (73, 97), (68, 84), (74, 43), (123, 145)),
    ((9, 14), (10, 10), (18, 33), (13, 9), (0, 60), (19, 54)),
    ((18, 33), (33, 6), (46, 36), (30, 63), (15, 46)),
    ((114, 162), (194, 90), (161, 19), (115, 70)),
    ((191, 137), (141, 14), (179, 196), (198, 111), (60, 120), (158, 51)),
    ((21, 9), (50, 53), (3, 31), (35, 38), (37, 42)),
    ((11, 5), (0, 13), (3, 8), (6, 12), (11, 13), (0, 13)),
    ((11, 7), (4, 11), (12, 15), (3, 5), (9, 1)),
    ((12, 1), (11, 2), (2, 5), (0, 13), (13, 7), (8, 8)),
    ((61, 30), (35, 30), (37, 14), (61, 59), (47, 17)),
    ((79, 8), (75, 21), (57, 1), (96, 158)),
    ((32, 40), (7, 8), (22, 51), (25, 62)),
    ((34, 44), (4, 84), (79, 70), (87, 133), (2, 103)),
    ((6, 9), (5, 11), (15, 0), (5, 10), (1, 14), (2, 2)),
    ((7, 0), (7, 2), (1, 14), (3, 10), (11, 13), (13, 0)),
    ((56, 2), (26, 62), (63, 0)),
    ((36, 58), (19, 3), (16, 1), (34, 11), (16, 35)),
    ((117, 12), (105, 28), (194, 37), (48, 162), (18, 30), (30, 187)),
    ((141, 24), (27, 176), (164, 86)),
    ((46, 60), (23, 14), (11, 44)),
    ((114, 128), (177, 105), (131, 13)),
    ((118, 49), (46, 109), (1, 181)),
    ((9, 190), (92, 24), (45, 114), (138, 39), (34, 158), (116, 132)),
    ((6, 0), (0, 12), (15, 10), (4, 10), (4, 11)),
    ((175, 32), (150, 1), (9, 189), (156, 10), (191, 7), (140, 158)),
    ((137, 184), (57, 190), (103, 98)),
    ((43, 8), (32, 30), (44, 28), (35, 52)),
    ((26, 58), (53, 51), (56, 31), (55, 1), (33, 45)),
    ((109, 162), (58, 49), (6, 182), (55, 169), (167, 186), (44, 22)),
    ((57, 57), (33, 9), (40, 56), (33, 46)),
    ((138, 131), (124, 159), (199, 99)),
    ((152, 23), (47, 191), (80, 155), (48, 161), (130, 103)),
    ((29, 115), (6, 161), (150, 192)),
    ((34, 61), (34, 3), (9, 53)),
    ((34, 2), (13, 58), (50, 58)),
    ((36, 195), (49, 130), (154, 192), (135, 51)),
    ((32, 186), (174, 197), (123, 46)),
    ((8, 1), (2, 13), (13, 0), (3, 7), (6, 7), (6, 2)),
    ((167, 143), (158, 188), (113, 47)),
    ((68, 121), (14, 130), (41, 52), (173, 184), (12, 9)),
    ((37, 186), (76, 4), (47, 158)),
    ((7, 14), (1, 2), (2, 15)),
    ((142, 112), (117, 22), (75, 70)),
    ((88, 171), (138, 70), (166, 192), (85, 12)),
    ((21, 9), (26, 14), (19, 5), (13, 41), (43, 20), (26, 30)),
    ((25, 28), (35, 192), (131, 95), (131, 191), (32, 37)),
    ((45, 77), (62, 116), (51, 136), (172, 21), (79, 9)),
    ((163, 4), (159, 8), (64, 160)),
    ((10, 45), (50, 43), (17, 50), (48, 50), (42, 54), (12, 6)),
    ((151, 44), (52, 110), (133, 2), (71, 80)),
    ((18, 5), (4, 33), (32, 23), (59, 21), (36, 33), (44, 17)),
    ((156, 161), (72, 41), (118, 194), (159, 194), (143, 11)),
    ((5, 61), (33, 5), (42, 31), (32, 15)),
    ((96, 44), (92, 156), (27, 77), (2, 127)),
    ((196, 2), (188, 33), (142, 86)),
    ((117, 153), (11, 26), (165, 194), (113, 99)),
    ((30, 36), (50, 4), (59, 42), (33, 19), (11, 63)),
    ((6, 57), (28, 13), (50, 21), (22, 11), (11, 34), (25, 50)),
    ((152, 143), (146, 27), (58, 1), (9, 141)),
    ((3, 47), (48, 59), (1, 1), (20, 18), (17, 7), (26, 1)),
)


if __name__ == "__main__":
    t0 = time.time()
    polys, hits, tried = search_rule_sensitive()
    print(f"# {len(polys)} polygons kept of {tried} tried in {time.time() - t0:.0f} s; masks changed per rule: {hits}", file=sys.stderr)
    print("PINNED = (")
    for p in polys:
        print(f"    {p},")
    print(")")
