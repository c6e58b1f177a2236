"""Bit maps for the device contour tracer at its size limits (tests/test_contour_forms.py, tests/test_gpu_large_maps.py), and a
restatement of its plausible starts (contours.hip row_starts), so that a test knows K - the count the parallel form reports and
on which its three outcomes turn - without a GPU.

text_page  - word-like rectangles over the WHOLE map (row 0 to row h-1, column 1 to column w-1), some hollow (hole borders), a few
             nested rings, one-pixel runs and a line in column w-1, thin lines across every 64-row band edge; column 0 clear
dot_field  - small dots on a grid: one outer start each, so K is set by the grid
"""
import numpy as np

BAND_ROWS = 64        # contours.hip kBandRows: the parallel form's scan streams the bit image through a band of this many rows
KEY_CACHE = 1024      # contours.hip kKeyCache: the scan reads the first 1024 plausible starts from LDS, later ones from global memory
MAX_STARTS = 8192     # contours.hip kMaxStarts: more plausible starts than this and the parallel form reports status 1


def parallel_words(h: int, w: int) -> int:
    """LDS words of the parallel form for an h x w map (contours.hip parallel_words): the bit plane, one word, the band buffer."""
    return (h * w + 31) // 32 + 1 + BAND_ROWS * (w // 32)


def row_starts(bm: np.ndarray, y: int):
    """The plausible starts of row y in raster order, as keys 2 * (y * w + x) + type (0 outer, 1 hole): the last pixel of a run whose
    gap to the next run is all foreground in the row above (the top row of a hole), and the first pixel of a run at x > 0 with
    nothing of the row above within one pixel of it."""
    h, w = bm.shape
    row = bm[y].astype(bool)
    up = bm[y - 1].astype(bool) if y > 0 else None
    d = np.diff(np.concatenate(([0], row.view(np.int8), [0])))
    x0s, x1s = np.flatnonzero(d == 1), np.flatnonzero(d == -1) - 1
    keys, prev_x1 = [], -1
    for x0, x1 in zip(x0s.tolist(), x1s.tolist()):
        if prev_x1 >= 0 and up is not None and up[prev_x1 + 1:x0].all():
            keys.append(2 * (y * w + prev_x1) + 1)
        if x0 > 0 and (up is None or not up[max(x0 - 1, 0):min(x1 + 1, w - 1) + 1].any()):
            keys.append(2 * (y * w + x0))
        prev_x1 = x1
    return keys


def plausible_starts(bm: np.ndarray):
    """Every plausible start of the map in raster order (the parallel form's list before it checks kMaxStarts)."""
    out = []
    for y in range(bm.shape[0]):
        out += row_starts(bm, y)
    return out


POOL = 1 << 17        # contours.hip kContourPool: points of all speculative walks of an image; more and the parallel form reports status 1
_DX = (-1, -1, 0, 1, 1, 1, 0, -1)   # directions W NW N NE E SE S SW (clockwise, y down), contours.hip ddx / ddy
_DY = (0, -1, -1, -1, 0, 1, 1, 1)


def walk_length(bm: np.ndarray, key: int) -> int:
    """Points of the border the parallel form walks from plausible start `key` (contours.hip walk_border): the first foreground
    neighbour clockwise from W (outer start) or E (hole start), then Suzuki-Abe steps counter-clockwise until the walk is back at
    its start with the first neighbour next."""
    h, w = bm.shape
    y, x = divmod(key >> 1, w)
    start = 4 if key & 1 else 0

    def nz(xx, yy):
        return 0 <= xx < w and 0 <= yy < h and bm[yy, xx] != 0

    for k in range(8):
        d = (start + k) & 7
        if nz(x + _DX[d], y + _DY[d]):
            p1x, p1y, base = x + _DX[d], y + _DY[d], d
            break
    else:
        return 1
    p3x, p3y, n = x, y, 0
    while True:
        for k in range(1, 9):
            dn = (base - k) & 7
            if nz(p3x + _DX[dn], p3y + _DY[dn]):
                break
        n += 1
        p4x, p4y = p3x + _DX[dn], p3y + _DY[dn]
        if p4x == x and p4y == y and p3x == p1x and p3y == p1y:
            return n
        p3x, p3y, base = p4x, p4y, (dn + 4) & 7


def walked_points(bm: np.ndarray) -> int:
    """Points of all the parallel form's speculative walks (one per plausible start): what must fit its pool of POOL points."""
    return sum(walk_length(bm, k) for k in plausible_starts(bm))


def text_page(h: int, w: int, seed: int, fill: float = None, hollow: float = 0.3) -> np.ndarray:
    """A 0/1 map with content everywhere a large map can go wrong: lines of word-like boxes from row 0 to row h-1 (the last line is
    cut by the bottom edge) whose last box ends at column w-1, a share of them hollow, nested rings, one-pixel runs and a line
    in column w-1, vertical and diagonal one-pixel lines across every 64-row band edge.  Column 0 stays clear.  fill: the share of
    box slots filled (default: about 30 000 border points whatever the size, well inside the parallel form's pool of walked points)."""
    if fill is None:
        fill = 0.55 * min(1.0, 640 * 640 / (h * w))
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    y = 0
    while y < h:
        lh = int(rng.integers(7, 15))
        x = 1 + int(rng.integers(0, 24))
        while x < w - 4:
            bw = int(rng.integers(10, 70))
            x1 = min(x + bw, w) if rng.random() < 0.8 else w      # (lines often run into the right edge)
            if rng.random() < fill:
                y1 = min(y + lh, h)
                m[y:y1, x:x1] = 1
                if rng.random() < hollow and lh >= 7 and x1 - x >= 6:
                    m[y + 2:y1 - 2, x + 2:x1 - 2] = 0                 # a hole border (open at the bottom edge where the line is cut)
            x = x1 + int(rng.integers(3, 14))
        y += lh + int(rng.integers(2, 10))
    m[h - 1, 1:w:7] = 1                                               # the last row: one-pixel runs, the last one at column w-1
    m[h - 1, w - 1] = 1
    # nested rings: outer border, hole border, outer border of the inner ring, its hole border
    for cy, cx in ((h // 3, w // 3), (2 * h // 3, 2 * w // 3), (h - 30, w - 40)):
        for r, v in ((14, 1), (12, 0), (8, 1), (6, 0), (2, 1)):
            m[max(cy - r, 0):cy + r, max(cx - r, 1):min(cx + r, w)] = v
    # thin lines across the band edges (one pixel wide: outer and hole walks share every pixel), both ways
    for b in range(BAND_ROWS, h, BAND_ROWS):
        xa = 1 + (37 * b) % (w - 8)
        m[b - 3:min(b + 3, h), xa] = 1
        for k in range(6):
            if b - 3 + k < h and xa + 2 + k < w:
                m[b - 3 + k, xa + 2 + k] = 1
    # column w-1: isolated pixels (one-pixel runs), a vertical line crossing a band edge
    m[3:h:11, w - 1] = 1
    m[3:h:11, w - 2] = 0
    m[BAND_ROWS - 5:min(BAND_ROWS + 9, h), w - 1] = 1
    m[:, 0] = 0
    return m


def dot_field(h: int, w: int, dy: int, dx: int, size: int = 2) -> np.ndarray:
    """size x size dots every dy rows and dx columns from (1, 1): one outer start (and one short border) per dot."""
    m = np.zeros((h, w), np.uint8)
    for s0 in range(size):
        for s1 in range(size):
            m[1 + s0:h:dy, 1 + s1:w - 1:dx] = 1
    return m
