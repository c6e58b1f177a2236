"""Hand-written cases for the word-crop rule (crops.hip crop_kernel, api.hip crop_boxes; oracle oracle/crop_oracle.py) and two
restatements of that rule which the CPU test tests/test_crop_cases.py holds against the oracle:

    trace_boxes / trace_samples   the oracle's own f32 operations, vectorised, RETURNING their intermediates (which clamp acted, whether
                                  a box was widened, the taps of every sample), so that a case can be shown to reach what it was written
                                  for.  Like the kernel it reads a flat frame block by offset, here with a NaN guard behind it: a tap one
                                  past the last column of the last row would show as a NaN crop.
    extract_crops_f64             the same boxes, f64 positions, f64 bilinear blend, / 255 - written on its own (separable weights and
                                  np.clip, no operation-order mirroring), with f64_bar() the derived bound on |oracle - f64|.

A case is (name, frames N x 1 x H x W f32, polygons per image, adj N x 2 f64); names are "group/part", the group is the row of the table
in tests/test_crop_cases.py.  Polygon coordinates are u32 (ocr_polygons_t), so a polygon left of or above the frame exists only under a
NEGATIVE adjust value, and none can straddle the left or the top border (all products of an axis share a sign): the nearest is one that
starts at 0.  Frame values are integers 0..255 as f32 unless the case says otherwise.  Everything is deterministic: the CPU test and
tests/test_gpu_crops.py see the same arrays."""
import numpy as np

F = np.float32
U = 2.0 ** -24    # unit roundoff of f32


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def point(x, y):
    return [(x, y)] * 4


def _frames(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 1, h, w)).astype(np.float32)


def _random_rects(seed, count, h, w):
    r = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        x0, y0 = int(r.integers(0, w)), int(r.integers(0, h))
        out.append(rect(x0, y0, int(r.integers(x0, w + 8)), int(r.integers(y0, h + 8))))   # some run past the right / bottom border
    return out


def cases():
    out = []
    ones = lambda n: np.ones((n, 2), np.float64)
    # ---- borders: 37 x 53
    h, w = 37, 53
    out.append(("borders/37x53", _frames(1, 1, h, w), [[
        rect(0, 10, 12, 20), rect(15, 0, 30, 8), rect(40, 12, w - 1, 25), rect(10, 28, 30, h - 1),            # left, top, right, bottom
        rect(0, 0, 6, 5), rect(46, 0, w - 1, 6), rect(0, 30, 7, h - 1), rect(45, 29, w - 1, h - 1),           # the four corners
        rect(0, 0, w - 1, h - 1),                                                                             # the whole frame
        rect(w - 1, 5, w - 1, 30), rect(4, h - 1, 40, h - 1),                                                 # the last column, the last row
    ]], ones(1)))
    # ---- one pixel: 23 x 31; image 1 (adjust values -1) puts coincident vertices left of and above the frame
    h, w = 23, 31
    out.append(("one pixel/23x31", _frames(2, 2, h, w), [
        [point(10, 10), point(0, 0), point(w - 1, h - 1), point(w + 3, h + 2), rect(5, 3, 5, 20), rect(4, 7, 25, 7)],
        [point(3, 4), point(0, 0)],
    ], np.array([[1.0, 1.0], [-1.0, -1.0]])))
    # ---- outside: 29 x 41; image 1 mirrors x, image 2 mirrors y
    h, w = 29, 41
    out.append(("outside/29x41", _frames(3, 3, h, w), [
        [rect(50, 5, 60, 15), rect(5, 40, 20, 50), rect(35, 5, 50, 15), rect(5, 20, 15, 40), rect(45, 35, 50, 40), rect(30, 20, 60, 50)],
        [rect(3, 5, 10, 15), rect(0, 5, 10, 15), rect(3, 35, 10, 45)],      # left of; from 0 leftwards; left of and below
        [rect(5, 3, 20, 10), rect(5, 0, 20, 9), rect(45, 2, 50, 9)],        # above; from 0 upwards; above and right of
    ], np.array([[1.0, 1.0], [-1.0, 1.0], [1.0, -1.0]])))
    # ---- fractional: the same polygons under three adjust values on 120 x 160 frames
    h, w = 120, 160
    pl = [rect(3, 2, 40, 30), rect(10, 10, 14, 13), rect(1, 1, 7, 44), rect(20, 5, 58, 9), rect(0, 0, 59, 44), rect(33, 17, 33, 17)]
    out.append(("fractional/120x160", _frames(4, 3, h, w), [pl, pl, pl], np.array([[800 / 300, 533 / 200], [0.37, 1.9], [1.0, 1.0]])))
    # ---- tiny frames
    for i, (h, w) in enumerate(((1, 1), (1, 40), (40, 1), (2, 2))):
        out.append((f"tiny frames/{h}x{w}", _frames(10 + i, 1, h, w),
                    [[point(0, 0), rect(0, 0, w - 1, h - 1), rect(5, 5, 50, 50), rect(0, 0, 50, 50)]], ones(1)))
    # ---- wide and tall
    h, w = 8, 2048
    out.append(("wide and tall/8x2048", _frames(20, 1, h, w),
                [[rect(2000, 1, 2047, 6), rect(2040, 0, 2047, 7), rect(1900, 2, 1930, 5), rect(0, 0, 2047, 7), rect(2047, 3, 2047, 3)]], ones(1)))
    h, w = 1024, 8
    out.append(("wide and tall/1024x8", _frames(21, 1, h, w),
                [[rect(1, 990, 6, 1023), rect(0, 1016, 7, 1023), rect(2, 900, 5, 950), rect(0, 0, 7, 1023), rect(3, 1023, 3, 1023)]], ones(1)))
    # ---- batch: images 0 and 2 empty, image 3 holds image 1's polygons
    h, w = 24, 32
    pl = [rect(2, 3, 20, 12), rect(25, 15, 31, 23), rect(0, 0, 31, 23), rect(10, 10, 11, 11)]
    out.append(("batch/4 x 24x32", _frames(30, 4, h, w), [[], pl, [], pl], np.array([[3.0, 0.5], [1.0, 1.0], [0.25, 7.0], [1.0, 1.0]])))
    # ---- counts: the grid (one workgroup per box) on one 64 x 96 frame
    fr = _frames(40, 1, 64, 96)
    for cnt in (1, 255, 256, 257, 1025):
        out.append((f"counts/{cnt}", fr, [_random_rects(400 + cnt, cnt, 64, 96)], ones(1)))
    # ---- constant and ramps: 19 x 27
    h, w = 19, 27
    pl = [rect(0, 0, w - 1, h - 1), rect(3, 4, 9, 8), rect(20, 10, 40, 30), rect(0, 0, 2, 2), point(13, 9), rect(1, 2, 25, 3), rect(5, 1, 6, 17)]
    out.append(("constant and ramp/constant 137", np.full((1, 1, h, w), 137.0, np.float32), [pl], ones(1)))
    out.append(("constant and ramp/v = x", np.broadcast_to(np.arange(w, dtype=np.float32), (1, 1, h, w)).copy(), [pl], ones(1)))
    out.append(("constant and ramp/v = y", np.broadcast_to(np.arange(h, dtype=np.float32)[:, None], (1, 1, h, w)).copy(), [pl], ones(1)))
    return [(name, np.ascontiguousarray(fr), polys, np.ascontiguousarray(adj, dtype=np.float64)) for name, fr, polys, adj in out]


def group(name):
    return name.split("/")[0]


_CASES = None
_ORACLE = {}


def all_cases():
    """cases(), built once per process"""
    global _CASES
    if _CASES is None:
        _CASES = cases()
    return _CASES


def case_names():
    return [c[0] for c in all_cases()]


def case(name):
    return next(c for c in all_cases() if c[0] == name)


def oracle_crops(name):
    """oracle.crop_oracle.extract_crops of a case: computed once per process (about 6 ms a box), shared by the CPU and the GPU tests
    and handed out read-only"""
    from oracle import crop_oracle as CR
    if name not in _ORACLE:
        _, fr, polys, adj = case(name)
        want = CR.extract_crops(fr, polys, adj)
        want.setflags(write=False)
        _ORACLE[name] = want
    return _ORACLE[name]


def nonfinite_cases():
    """Adjust values that are not finite: (name, frames, polygons, adj, the boxes (frame, x0, y0, x1, y1) the header promises).  A NaN
    product takes no part in an extreme; an axis with nothing but NaN products is the last pixel; +-inf clamps like any value."""
    h, w = 11, 17
    fr = _frames(50, 1, h, w)
    inf, nan = float("inf"), float("nan")
    pl = [rect(2, 3, 9, 7), rect(0, 3, 9, 7), rect(2, 0, 9, 7), rect(0, 0, 0, 0)]
    last_x, last_y = (w - 1.0, float(w)), (h - 1.0, float(h))
    out = []
    for name, adj, bx in (
        ("NaN, 1", (nan, 1.0), [last_x + (3, 8), last_x + (3, 8), last_x + (0, 8), last_x + (0, 1)]),
        ("1, NaN", (1.0, nan), [(2, 10) + last_y, (0, 10) + last_y, (2, 10) + last_y, (0, 1) + last_y]),
        ("NaN, NaN", (nan, nan), [last_x + last_y] * 4),
        # +inf: x * inf = +inf where x > 0 (min stays at its sentinel, clamped to W - 1), 0 * inf = NaN is skipped
        ("+inf, 1", (inf, 1.0), [last_x + (3, 8), last_x + (3, 8), last_x + (0, 8), last_x + (0, 1)]),
        # -inf: the minimum is -inf -> x0 = 0; the maximum is -inf (or the sentinel) -> widened to one pixel
        ("-inf, 1", (-inf, 1.0), [(0, 1, 3, 8), (0, 1, 3, 8), (0, 1, 0, 8), last_x + (0, 1)]),
        ("1, -inf", (1.0, -inf), [(2, 10, 0, 1), (0, 10, 0, 1), (2, 10, 0, 1), (0, 1) + last_y]),
    ):
        boxes = [(0, F(x0), F(y0), F(x1), F(y1)) for (x0, x1, y0, y1) in bx]
        out.append((name, fr, [pl], np.array([adj], np.float64), boxes))
    return out


# ------------------------------------------------------------------------------------------------- the oracle's rule with its intermediates
def trace_boxes(polys, adj, h, w):
    """api.hip's crop_boxes step by step: per polygon a dict with the f32 box and what acted on it"""
    out = []
    for b, plist in enumerate(polys):
        ax, ay = float(adj[b][0]), float(adj[b][1])
        for poly in plist:
            mn = [1e300, 1e300]
            mx = [-1e300, -1e300]
            for p in poly:
                for a, v in enumerate((p[0] * ax, p[1] * ay)):
                    if v < mn[a]:
                        mn[a] = v
                    if v > mx[a]:
                        mx[a] = v
            rec = {"frame": b}
            for a, (name, size) in enumerate((("x", w), ("y", h))):
                lo = max(mn[a], 0.0)
                p0 = min(lo, size - 1.0)
                want1 = mx[a] + 1.0
                wide = max(want1, p0 + 1.0)
                p1 = min(wide, float(size))
                rec.update({name + "0": p0, name + "1": p1,
                            name + "0_low": mn[a] < 0.0, name + "0_high": lo > size - 1.0, name + "1_high": wide > size,
                            name + "_widened": want1 < p0 + 1.0, name + "_one": p1 - p0 == 1.0,
                            name + "_inexact": float(F(p0)) != p0 or float(F(p1)) != p1,
                            name + "_up": float(F(p1)) - float(F(p0)) < 28.0, name + "_down": float(F(p1)) - float(F(p0)) > 28.0})
            rec["box"] = (b, F(rec["x0"]), F(rec["y0"]), F(rec["x1"]), F(rec["y1"]))
            out.append(rec)
    return out


def _trace_axis(p0, p1, size):
    k = np.arange(28, dtype=np.float32)
    step = F(p1 - p0) / F(28)
    raw = (p0 + (k + F(0.5)) * step) - F(0.5)
    s = np.minimum(np.maximum(raw, F(0)), F(size - 1))
    i0 = np.floor(s).astype(np.int64)
    i1 = np.minimum(i0 + 1, size - 1)
    return {"raw": raw, "s": s, "i0": i0, "i1": i1, "f": s - i0.astype(np.float32)}


def trace_samples(frames, box):
    """The sample loop of oracle/crop_oracle.py extract_crops for one box, all 784 samples at once, with its intermediates.  The taps
    are read from the flat frame block by offset, as the kernel reads them; behind the block stands a NaN guard."""
    n, _, h, w = frames.shape
    b, x0, y0, x1, y1 = box
    flat = np.concatenate([np.ascontiguousarray(frames, np.float32).ravel(), np.full(w + 2, np.nan, np.float32)])
    X, Y = _trace_axis(x0, x1, w), _trace_axis(y0, y1, h)
    base = b * h * w
    tap = lambda iy, ix: flat[base + iy[:, None] * w + ix[None, :]]
    a, bb, c, d = tap(Y["i0"], X["i0"]), tap(Y["i0"], X["i1"]), tap(Y["i1"], X["i0"]), tap(Y["i1"], X["i1"])
    fx, fy = X["f"][None, :], Y["f"][:, None]
    top = a + fx * (bb - a)
    bot = c + fx * (d - c)
    crop = (top + fy * (bot - top)) / F(255)
    assert crop.dtype == np.float32
    return {"x": X, "y": Y, "crop": crop.reshape(784)}


def extract_crops_traced(frames, polys, adj):
    """(crops P x 784 f32, hit counts) - the crops must equal oracle.crop_oracle.extract_crops bit for bit"""
    n, _, h, w = frames.shape
    boxes = trace_boxes(polys, adj, h, w)
    crops = np.zeros((len(boxes), 784), np.float32)
    hits = {k: 0 for k in (
        "boxes", "widened", "one_pixel", "box_low", "box0_high", "box1_high", "inexact", "up", "down",
        "sx_low", "sx_high", "ix_same", "sy_low", "sy_high", "iy_same", "all_taps_same", "far", "taps_outside")}
    frames_used = set()
    for k, rec in enumerate(boxes):
        t = trace_samples(frames, rec["box"])
        crops[k] = t["crop"]
        X, Y = t["x"], t["y"]
        hits["boxes"] += 1
        frames_used.add(rec["frame"])
        for key, flag in (("widened", "_widened"), ("one_pixel", "_one"), ("box_low", "0_low"), ("box0_high", "0_high"),
                          ("box1_high", "1_high"), ("inexact", "_inexact"), ("up", "_up"), ("down", "_down")):
            hits[key] += int(rec["x" + flag]) + int(rec["y" + flag])
        hits["sx_low"] += int((X["raw"] < 0).sum())
        hits["sx_high"] += int((X["raw"] > w - 1).sum())
        hits["ix_same"] += int((X["i1"] == X["i0"]).sum())
        hits["sy_low"] += int((Y["raw"] < 0).sum())
        hits["sy_high"] += int((Y["raw"] > h - 1).sum())
        hits["iy_same"] += int((Y["i1"] == Y["i0"]).sum())
        hits["all_taps_same"] += int((X["i1"] == X["i0"]).all() and (Y["i1"] == Y["i0"]).all())
        hits["far"] += int((X["s"] >= 1000).sum()) + int((Y["s"] >= 1000).sum())
        for A, size in ((X, w), (Y, h)):
            hits["taps_outside"] += int(((A["i0"] < 0) | (A["i0"] > size - 1) | (A["i1"] < 0) | (A["i1"] > size - 1)).sum())
    hits["frames_used"] = len(frames_used)
    return crops, hits


# what each group of cases must reach (hit counts summed over its parts, each > 0)
REQUIRED = {
    "borders": ("sx_low", "sx_high", "sy_low", "sy_high", "ix_same", "iy_same"),
    "one pixel": ("widened", "one_pixel", "box0_high", "box1_high", "box_low"),
    "outside": ("box_low", "box0_high", "box1_high", "widened"),
    "fractional": ("inexact", "up", "down"),
    "tiny frames": ("all_taps_same", "sx_low", "sx_high", "sy_low", "sy_high"),
    "wide and tall": ("far", "sx_high", "sy_high"),
    "batch": ("boxes",),
    "counts": ("boxes",),
    "constant and ramp": ("boxes", "sx_low", "sy_high"),
}


# ------------------------------------------------------------------------------------------------------------- the f64 restatement
def _weights_f64(p0, p1, size):
    """28 sample positions of one axis in f64 -> a 28 x size matrix of interpolation weights (each row sums to 1)"""
    s = np.clip(p0 + (np.arange(28) + 0.5) * ((p1 - p0) / 28.0) - 0.5, 0.0, size - 1.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), size - 1)
    i1 = np.minimum(i0 + 1, size - 1)
    m = np.zeros((28, size))
    np.add.at(m, (np.arange(28), i0), 1.0 - (s - i0))
    np.add.at(m, (np.arange(28), i1), s - i0)
    return m


def extract_crops_f64(frames, boxes):
    """boxes: oracle.crop_oracle.crop_boxes' tuples.  P x 784 f64."""
    n, _, h, w = frames.shape
    out = np.zeros((len(boxes), 784))
    for k, (b, x0, y0, x1, y1) in enumerate(boxes):
        wy, wx = _weights_f64(float(y0), float(y1), h), _weights_f64(float(x0), float(x1), w)
        out[k] = (wy @ frames[b, 0].astype(np.float64) @ wx.T).reshape(784) / 255.0
    return out


def f64_bar(frame):
    """Bound on |oracle - extract_crops_f64| for one H x W frame, u = 2^-24.

    The clamped bilinear interpolant is continuous and, per unit of x, changes by at most Dx = the largest difference of two
    horizontal neighbours (Dy likewise), so a position off by dx moves it by at most Dx dx, whichever cell either side lands in.
      position  sx = fl(fl(x0 + fl((j + 0.5) fl(fl(x1 - x0) / 28))) - 0.5): five roundings ((j + 0.5) is exact), each of a value of
                magnitude <= W (0 <= x0, x1 <= W): |dx| <= 5 u W; |dy| <= 5 u H.           ->  5 u (W Dx + H Dy)
      blend     fx = sx - ix0 is exact.  top = fl(a + fl(fx fl(b - a))): the difference and the product are off by <= u Dx each, the
                sum (magnitude <= M = max |v|) by <= u M; bot the same, and fy blends the two errors with weights summing to 1:
                <= u M + 2 u Dx.  fl(top + fl(fy fl(bot - top))): <= 2 u Dy + u M more.      ->  u (2 M + 2 Dx + 2 Dy)
      / 255     one rounding of a value <= M / 255.                                         ->  u M / 255
    Second-order terms and the f64 side's own 2^-53 roundings go into the factor 1.001."""
    fr = frame.astype(np.float64)
    h, w = fr.shape
    dx = float(np.abs(np.diff(fr, axis=1)).max()) if w > 1 else 0.0
    dy = float(np.abs(np.diff(fr, axis=0)).max()) if h > 1 else 0.0
    m = float(np.abs(fr).max())
    return 1.001 * U * (5.0 * (w * dx + h * dy) + 3.0 * m + 2.0 * dx + 2.0 * dy) / 255.0
