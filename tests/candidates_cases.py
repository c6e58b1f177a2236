"""Batches for the candidates chain (candidates.hip: dp_kernel, cand_count_kernel, cand_fill_kernel), an iterative oracle of what the
three kernels must leave, and a copy of that oracle with SWITCHABLE rules.

The chain turns the device tracer's contours into the job and point lists that box_score.hip and unclip.hip walk by count; the product
hands an image or a batch back to the host whenever the chain reports -1 or an overflow, so a chain that wrongly gives up, or that
reports a wrong total and then falls back, still produces the right polygons.  tests/test_gpu_candidates_kernel.py therefore reads the
chain's RAW outputs (capi.device_candidates_batch) and holds them to expected_chain() word for word.

    dp_indices            Douglas-Peucker without recursion: the kept indices in increasing order.  The arithmetic is
                          O.approximate_polygon_dp's - f64, the line through the two ends, the strict > scan, NaN when both ends
                          coincide - and tests/test_candidates_cases.py proves the two equal.
    candidate_rules       metrics.rs:86-98 (epsilon = 0.01 * arc length or 0.01, Douglas-Peucker, pop a repeated end point, >= 4 points)
                          with four switches, each one way the kernel could plausibly be wrong:
        tie    "first"    the spec: the first index attaining the maximum wins
               "last"     >= instead of >
               "stride"   64 lanes scan i = lo + 1 + lane + 64 k and keep their LAST maximum (>= inside the lane); the reduction is right
               "lane"     64 lanes scan i = lo + 1 + lane + 64 k and keep their first maximum; the reduction takes the operand of the
                          HIGHER lane among equal distances (the reduction without its index clause)
        dist   "line"     the spec: distance to the infinite line
               "segment"  distance to the segment, clamped at its ends
        close  "spec"
               "no_closing_segment"   the arc length without P[0] - P[L-1]
               "keep_repeat"          a repeated end point is not dropped
        eps0   "spec"     epsilon == 0 becomes 0.01
               "zero"     no substitution
    MUTANTS lists the seven single-switch deviations.  PINNED is a fixed list of lattice contours whose candidate changes under a wrong
    rule, found by search_rule_sensitive (seeded; `python -m tests.candidates_cases` prints it): every observable mutant changes at
    least 8 of them, so a kernel with that defect fails the GPU test on every run.

One of them, eps0 = "zero", is EQUIVALENT: no input can show it.  The arc length is 0 only when all points are one point; then
every range has coinciding ends, every distance is 0 / 0 = NaN, no scan finds a maximum above 0, and neither 0 > 0 nor 0 > 0.01 holds.
The all-identical contours below run the substitution's branch all the same; the CPU test asserts that the mutant changes nothing.

Deliberately NOT pinned:
  * the order of the f64 arc-length sum.  Coordinates stay below 2^16, so every product and sum in the numerator and under the square
    roots is an exact integer and contraction cannot matter; the summation order can only flip a decision when dmax sits within an ulp
    of 0.01 * len, which no search finds in reasonable time.  No case is faked for it.
  * a candidate of more than kBoxScoreMaxPts (2048) kept points.  A kept point must deviate by more than 1 % of the perimeter, so this
    appears unreachable: the largest kept count any case or search contour here produced is 14.  That branch stays untested.

The generators are deterministic: the CPU test and the GPU test see the same batches."""
import math
import sys
import time

import numpy as np

from oracle import postproc_oracle as O

K_KEEP_CAP = 32768          # contour points dp_kernel holds (32 * kKeepWords)
K_MAX_PTS = 2048            # kBoxScoreMaxPts
POISON = 0x5A5AC3C3
POISON_I32 = int(np.array([POISON], np.uint32).view(np.int32)[0])

MUTANTS = (("tie", "last"), ("tie", "stride"), ("tie", "lane"), ("dist", "segment"), ("close", "no_closing_segment"), ("close", "keep_repeat"), ("eps0", "zero"))
EQUIVALENT_MUTANTS = (("eps0", "zero"),)   # see the module docstring


# ---------------------------------------------------------------------------------------------------------------- the iterative oracle
def dp_indices(c, eps: float):
    """approximate_polygon_dp(c, eps, closed = False) as indices: 0, L - 1 and every split point, increasing.  len(c) >= 1."""
    L = len(c)
    if L == 1:
        return [0, 0]
    keep = {0, L - 1}
    stack = [(0, L - 1)]
    while stack:
        lo, hi = stack.pop()
        x0, y0 = float(c[lo][0]), float(c[lo][1])
        x1, y1 = float(c[hi][0]), float(c[hi][1])
        a = y0 - y1
        b = x1 - x0
        cc = x0 * y1 - x1 * y0
        norm = math.sqrt(a * a + b * b)
        dmax, index = 0.0, lo
        for i in range(lo + 1, hi + 1):
            num = abs(a * float(c[i][0]) + b * float(c[i][1]) + cc)
            d = num / norm if norm != 0.0 else float("nan")
            if d > dmax:
                index, dmax = i, d
        if dmax > eps:
            keep.add(index)
            stack.append((lo, index))
            stack.append((index, hi))
    return sorted(keep)


def candidate(c):
    """metrics.rs:86-98 on one contour: the candidate polygon (a list of points) or None.  Fewer than 4 contour points cannot leave 4."""
    if len(c) < 4:
        return None
    eps = 0.01 * O.arc_length(c, True)
    if eps == 0.0:
        eps = 0.01
    idx = dp_indices(c, eps)
    idx.pop()   # closed
    pts = [(int(c[i][0]), int(c[i][1])) for i in idx]
    if len(pts) > 1 and pts[0] == pts[-1]:
        pts.pop()
    return pts if len(pts) >= 4 else None


# ---------------------------------------------------------------------------------------------------------------- the switchable copy
def _scan_rules(c, lo, hi, tie, dist):
    """(index, dmax, indices attaining dmax) over lo < i < hi (the end point itself is at distance 0 or NaN: never greater)"""
    x0, y0 = float(c[lo][0]), float(c[lo][1])
    x1, y1 = float(c[hi][0]), float(c[hi][1])
    a = y0 - y1
    b = x1 - x0
    cc = x0 * y1 - x1 * y0
    n2 = a * a + b * b
    norm = math.sqrt(n2)
    ds = []
    for i in range(lo + 1, hi):
        x, y = float(c[i][0]), float(c[i][1])
        d = abs(a * x + b * y + cc) / norm if norm != 0.0 else float("nan")
        if dist == "segment":
            t = ((x - x0) * (x1 - x0) + (y - y0) * (y1 - y0)) / n2 if n2 != 0.0 else -1.0
            if t < 0.0:
                d = math.sqrt((x - x0) ** 2 + (y - y0) ** 2)
            elif t > 1.0:
                d = math.sqrt((x - x1) ** 2 + (y - y1) ** 2)
        ds.append(d)
    dmax, index = 0.0, lo
    if tie in ("lane", "stride"):
        best = [(0.0, lo)] * 64
        for k, d in enumerate(ds):
            if (d >= best[k & 63][0] and d > 0.0) if tie == "stride" else (d > best[k & 63][0]):
                best[k & 63] = (d, lo + 1 + k)
        for d, i in best:   # lanes 0 .. 63
            if tie == "lane" and d >= dmax and d > 0.0:        # the higher lane wins among equals
                dmax, index = d, i
            elif tie == "stride" and (d > dmax or (d == dmax and d > 0.0 and i < index)):   # the smaller index wins, as it should
                dmax, index = d, i
    else:
        for k, d in enumerate(ds):
            if (d >= dmax and d > 0.0) if tie == "last" else (d > dmax):
                dmax, index = d, lo + 1 + k
    tied = [lo + 1 + k for k, d in enumerate(ds) if d == dmax] if dmax > 0.0 else []
    return index, dmax, tied


def candidate_rules(c, tie="first", dist="line", close="spec", eps0="spec", stats=None):
    """candidate() with switchable rules; stats (a list) receives (lo, hi, first tied index, a tie 64 k apart, a tie not 64 k apart) of
    every DECISIVE scan (dmax > epsilon) whose maximum is attained more than once, and afterwards ("kept", count)."""
    L = len(c)
    if L < 4:
        return None
    length = 0.0
    for i in range(L - 1):
        length += O._dist(c[i], c[i + 1])
    if L > 2 and close != "no_closing_segment":
        length += O._dist(c[0], c[L - 1])
    eps = 0.01 * length
    if eps == 0.0 and eps0 == "spec":
        eps = 0.01
    keep = {0, L - 1}
    stack = [(0, L - 1)]
    while stack:
        lo, hi = stack.pop()
        if hi - lo < 2:
            continue
        index, dmax, tied = _scan_rules(c, lo, hi, tie, dist)
        if dmax > eps:
            if stats is not None and len(tied) > 1:
                stats.append((lo, hi, tied[0], any((j - tied[0]) % 64 == 0 for j in tied[1:]), any((j - tied[0]) % 64 != 0 for j in tied[1:])))
            keep.add(index)
            stack.append((lo, index))
            stack.append((index, hi))
    idx = sorted(keep)
    idx.pop()
    pts = [(int(c[i][0]), int(c[i][1])) for i in idx]
    if stats is not None:
        stats.append(("kept", len(pts)))
    if close != "keep_repeat" and len(pts) > 1 and pts[0] == pts[-1]:
        pts.pop()
    return pts if len(pts) >= 4 else None


def mutants_changing(c):
    """the entries of MUTANTS under which this contour's candidate differs from the spec's"""
    base = candidate_rules(c)
    return [mu for mu in MUTANTS if candidate_rules(c, **{mu[0]: mu[1]}) != base]


# ---------------------------------------------------------------------------------------------------------------- what the chain leaves
def job_box(pts, h: int, w: int):
    """(min_x, min_y, bw, bh): x clamped by H, y by W (metrics.rs:151-166), as _box of tests/test_gpu_device_chain.py"""
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    cl = lambda v, hi: min(max(v, 0), hi - 1)   # noqa: E731
    x0, x1, y0, y1 = cl(min(xs), h), cl(max(xs), h), cl(min(ys), w), cl(max(ys), w)
    return (x0, y0, x1 - x0 + 1, y1 - y0 + 1)


def expected_chain(images, h: int, w: int, max_jobs: int, max_pts: int):
    """What dp_kernel + cand_count_kernel + cand_fill_kernel must leave for images = [(status, contours)]:
        tot      per image (candidates, points), or (-1, -1) where the host must take it: status != 0, a contour longer than 32768
                 points, a candidate of more than 2048 points
        totals   (jobs, points, 0), or (0, 0, 1) when either list overflows
        jobs     [(image, pt_offset, n_pts, min_x, min_y, bw, bh)] in image and contour order; None on overflow (no statement then about
                 what lies below the guards)
        points   [(x, y)]; None on overflow"""
    tot, jobs, points = [], [], []
    for b, (status, contours) in enumerate(images):
        if status != 0 or any(len(c) > K_KEEP_CAP for c in contours):
            tot.append((-1, -1))
            continue
        cands = [p for p in (candidate(c) for c in contours) if p is not None]
        if any(len(p) > K_MAX_PTS for p in cands):
            tot.append((-1, -1))
            continue
        tot.append((len(cands), sum(len(p) for p in cands)))
        for p in cands:
            jobs.append((b, len(points), len(p)) + job_box(p, h, w))
            points.extend(p)
    if len(jobs) > max_jobs or len(points) > max_pts:
        return {"tot": tot, "totals": (0, 0, 1), "jobs": None, "points": None}
    return {"tot": tot, "totals": (len(jobs), len(points), 0), "jobs": jobs, "points": points}


# ---------------------------------------------------------------------------------------------------------------- lattice shapes
def walk(start, moves):
    """the closed lattice curve from start along moves [(dx, dy, steps)]; the last step returns to start, which is not repeated"""
    pts = [tuple(start)]
    for dx, dy, n in moves:
        for _ in range(n):
            pts.append((pts[-1][0] + dx, pts[-1][1] + dy))
    assert pts[-1] == pts[0], (pts[0], pts[-1])
    pts.pop()
    return pts


def rotate(c, k: int):
    k %= max(len(c), 1)
    return list(c[k:]) + list(c[:k])


def rect_outline(x0: int, y0: int, a: int, b: int):
    """every boundary point of a rectangle of a x b points, clockwise from its top-left corner: 2 a + 2 b - 4 points"""
    return walk((x0, y0), [(1, 0, a - 1), (0, 1, b - 1), (-1, 0, a - 1), (0, -1, b - 1)])


def ell_outline(x0: int, y0: int, a: int, b: int):
    """an L-shape of a x b points with a quarter cut out of its top-right corner"""
    return walk((x0, y0), [(1, 0, a // 2), (0, 1, b // 2), (1, 0, a - 1 - a // 2), (0, 1, b - 1 - b // 2), (-1, 0, a - 1), (0, -1, b - 1)])


def line_out_and_back(x0: int, y0: int, n: int):
    """a one-pixel-wide horizontal line of n points traced out and back: 2 n - 2 points"""
    return [(x0 + i, y0) for i in range(n)] + [(x0 + i, y0) for i in range(n - 2, 0, -1)]


def blob(L: int, seed: int, cx: int = 200, cy: int = 150, rx: float = 120.0, ry: float = 90.0):
    """a jittered lattice ellipse of exactly L points (convex up to the jitter)"""
    rng = np.random.default_rng(1000 * seed + L)
    pts = []
    for i in range(L):
        t = 2 * math.pi * i / max(L, 1)
        j = 1.0 + rng.uniform(-0.04, 0.04)
        pts.append((int(round(cx + rx * j * math.cos(t))), int(round(cy + ry * j * math.sin(t)))))
    return pts


def notched_rect(L: int, x0: int = 2, y0: int = 2):
    """a closed lattice curve of exactly L points: a large rectangle, two notches in its top side, one corner cut where L is odd"""
    par = L % 2
    le = L + par
    b = max(6, le // 8)
    d = max(2, b // 3)
    a = (le - 2 * b + 4 - 4 * d) // 2
    q = max(1, a // 8)
    s1, s2 = a // 4, a // 4
    s3 = a - 1 - s1 - s2 - 2 * q
    assert s3 >= 2 and a >= 8
    top = [(1, 0, s1), (0, 1, d), (1, 0, q), (0, -1, d), (1, 0, s2), (0, 1, d), (1, 0, q), (0, -1, d)]
    if par:
        rest = [(1, 0, s3 - 1), (1, 1, 1), (0, 1, b - 2)]
    else:
        rest = [(1, 0, s3), (0, 1, b - 1)]
    c = walk((x0, y0), top + rest + [(-1, 0, a - 1), (0, -1, b - 1)])
    assert len(c) == L, (len(c), L)
    return c


def square(x0: int, y0: int):
    return rect_outline(x0, y0, 4, 4)   # 12 points, a candidate of 4


# ---------------------------------------------------------------------------------------------------------------- named cases
def _case(name, images, h, w, max_jobs=None, max_pts=None, maxc=None, cap=None, guard=64, guard_pts=None):
    tots = [sum(len(c) for c in cs) for _, cs in images]
    cap = max(64, max(tots)) if cap is None else cap
    maxc = max(1, max(len(cs) for _, cs in images)) if maxc is None else maxc
    return {"name": name, "images": images, "h": h, "w": w, "cap": cap, "maxc": maxc,
            "max_jobs": sum(len(cs) for _, cs in images) + 8 if max_jobs is None else max_jobs,
            "max_pts": sum(tots) + 8 if max_pts is None else max_pts, "guard": guard}


LENGTHS = (0, 1, 2, 3, 4, 5, 31, 32, 33, 34, 63, 64, 65, 66, 96, 97, 98, 128, 129, 130)
RECTS = ((70, 5), (5, 70), (130, 66), (200, 150))
LONG_LENGTHS = (2047, 2048, 2049, 2080, 4097, 32767, 32768)
STRIDE_NCS = (31, 32, 33, 64, 65, 700, 4096)
BATCH_NS = (2, 5, 257, 300)


def length_cases():
    """one image of contours of every length in LENGTHS on a 300 x 400 map (x up to 325 is clamped by H), and the same rotated"""
    base = [blob(L, 1) for L in LENGTHS]
    rot = [rotate(c, len(c) // 3 + 1) for c in base]
    return [_case("lengths", [(0, base)], 300, 400), _case("lengths, rotated", [(0, rot)], 300, 400)]


def rect_starts(a: int, b: int):
    """the a x b rectangle outline starting at each of its four corners and at a mid-side point"""
    r = rect_outline(3, 3, a, b)
    corners = (0, a - 1, a + b - 2, 2 * a + b - 3)
    return [rotate(r, k) for k in corners] + [rotate(r, a // 2)]


def tie_cases():
    out = []
    for a, b in RECTS:
        out.append(_case(f"rectangle {a} x {b}, five starts", [(0, rect_starts(a, b))], 256, 256))
    out.append(_case("line of 150 points out and back", [(0, [line_out_and_back(4, 9, 150), rotate(line_out_and_back(4, 9, 150), 75)])], 256, 256))
    out.append(_case("L-shapes", [(0, [ell_outline(3, 3, 140, 70), rotate(ell_outline(3, 3, 140, 70), 69), ell_outline(3, 3, 70, 140)])], 256, 256))
    return out


def long_cases():
    out = [_case(f"L = {L}", [(0, [notched_rect(L)])], 16384, 16384) for L in LONG_LENGTHS]
    out.append(_case("L = 32769 between two healthy images",
                     [(0, [notched_rect(2080), square(5, 5)]), (0, [square(9, 9), notched_rect(K_KEEP_CAP + 1), square(20, 5)]), (0, [notched_rect(2049, 7, 9)])],
                     16384, 16384))
    return out


REPEAT_LENGTHS = (60, 32, 33, 34, 64, 65, 66, 97)   # L - 2 = 30, 31, 0 (mod 32): the mask of the search for the last kept point


def repeat_contour(L: int = 60):
    """revisits P[0] at index L - 2 and ends on a spur: the last kept point below L - 1 repeats P[0] and is dropped"""
    c = blob(L, 3)
    c[-2] = c[0]
    c[-1] = (c[0][0] + 30, c[0][1] - 40)
    return c


def degenerate_cases():
    closed = blob(40, 4)
    closed[-1] = closed[0]                       # the first range has coinciding ends: every distance NaN
    inner = blob(41, 5)
    inner[20] = inner[0]                         # P[0] again in the middle: sub-ranges with coinciding ends where it is kept
    tri = walk((10, 10), [(1, 0, 40), (-1, 1, 20), (-1, -1, 20)])            # 3 kept points: no candidate
    quad = rect_outline(10, 60, 30, 20)                                     # its neighbour with 4
    cs = [[(7, 7)] * 4, [(9, 300)] * 70, closed, inner, repeat_contour(), tri, quad, rotate(tri, 40), rotate(quad, 29)]
    cs += [repeat_contour(L) for L in REPEAT_LENGTHS[1:]]
    return [_case("degenerate", [(0, cs)], 400, 400)]


def stride_contours(nc: int):
    """nc small squares; every third contour is no candidate, alternately 3 points long and a line that collapses"""
    cs = []
    for c in range(nc):
        x, y = 2 + 6 * (c % 100), 2 + 6 * (c // 100)
        if c % 3 == 2:
            cs.append([(x, y), (x + 2, y), (x + 1, y + 2)] if (c // 3) % 2 == 0 else line_out_and_back(x, y, 4))
        else:
            cs.append(square(x, y))
    return cs


def stride_cases():
    out = []
    for nc in STRIDE_NCS:
        for maxc in sorted({nc, 4096}):
            out.append(_case(f"{nc} contours, maxc {maxc}", [(0, stride_contours(nc))], 640, 640, maxc=maxc))
    return out


def _tiny(b: int):
    """one to three tiny contours for image b, at least one of them a candidate"""
    k = 1 + b % 3
    cs = [rect_outline(3 + b % 7, 2 + b % 5, 4 + (b + j) % 3, 4 + (b // 3 + j) % 4) for j in range(k)]
    if b % 4 == 1:
        cs.insert(0, line_out_and_back(1, 1, 5))
    return cs


def status_patterns(n: int):
    pats = {"all 0": [0] * n, "given up first": [1] + [0] * (n - 1), "given up last": [0] * (n - 1) + [2], "every other": [(b % 2) * 3 for b in range(n)]}
    if n > 257:
        for k in (255, 256, 257):
            pats[f"given up at {k}"] = [1 if b == k else 0 for b in range(n)]
    elif n == 257:
        pats["given up at 255"] = [1 if b == 255 else 0 for b in range(n)]
        pats["given up at 256"] = [1 if b == 256 else 0 for b in range(n)]
    return pats


def batch_cases():
    """(status-pattern batches, batches with empty and all-collapsing images)"""
    pat, empt = [], []
    for n in BATCH_NS:
        for pname, st in status_patterns(n).items():
            pat.append(_case(f"{n} images, {pname}", [(st[b], _tiny(b)) for b in range(n)], 64, 48))
        for where, pos in (("first", 0), ("middle", n // 2), ("last", n - 1)):
            for kind, cs in (("no contours", []), ("all collapse", [line_out_and_back(2, 2, 6), [(1, 1), (2, 2)]])):
                imgs = [(0, _tiny(b)) for b in range(n)]
                imgs[pos] = (0, cs)
                empt.append(_case(f"{n} images, {kind} {where}", imgs, 64, 48))
    imgs = [(0, _tiny(b)) for b in range(300)]
    for b in (0, 100, 255, 256, 299):
        imgs[b] = (0, [])
    for b in (1, 101, 257, 298):
        imgs[b] = (1, _tiny(b))
    empt.append(_case("300 images, empty and given-up ones in front of, between and behind live ones", imgs, 64, 48))
    return pat, empt


def capacity_cases():
    """a batch of J jobs and P points against lists of every size around them; guards of 64 jobs and 4096 points"""
    imgs = [(0, _tiny(b)) for b in range(7)]
    imgs[3] = (2, _tiny(3))
    e = expected_chain(imgs, 64, 48, 1 << 20, 1 << 20)
    J, P = e["totals"][0], e["totals"][1]
    out = []
    for mj, mp in ((J, P), (J + 3, P + 3), (J - 1, P), (J, P - 1), (0, P), (J, 0), (J - 1, P - 1), (J + 3, P - 1), (J - 1, P + 3)):
        out.append(dict(_case(f"{J} jobs, {P} points into lists of {mj}, {mp}", imgs, 64, 48, max_jobs=mj, max_pts=mp), guard=4096))
    return out


def pinned_case():
    """PINNED as one batch: four contours per image"""
    cs = [expand(p) for p in PINNED]
    imgs = [(0, cs[i:i + 4]) for i in range(0, len(cs), 4)]
    assert imgs
    return [_case("pinned", imgs, 512, 512)]


def named_groups():
    """{group: [case]}: every named group with scratch_fill 0x00 and 0xA5, the status-pattern batches with 0xFF too.  A case's "key" names
    what its expected values depend on (the fills share them)."""
    pat, empt = batch_cases()
    base = {"lengths": length_cases(), "ties": tie_cases(), "long": long_cases(), "degenerate": degenerate_cases(), "striding": stride_cases(),
            "batches": pat, "batches_empty": empt, "capacities": capacity_cases(), "pinned": pinned_case()}
    out = {}
    for g, cases in base.items():
        fills = (0x00, 0xA5, 0xFF) if g == "batches" else (0x00, 0xA5)
        out[g] = [dict(c, scratch_fill=f, key=(g, k)) for k, c in enumerate(cases) for f in fills]
    return out


GROUPS = ("lengths", "ties", "long", "degenerate", "striding", "batches", "batches_empty", "capacities", "pinned")


def all_contours():
    """every contour of every named case, once"""
    seen, out = set(), []
    for cases in named_groups().values():
        for c in cases:
            if c["scratch_fill"] != 0:
                continue
            for _, cs in c["images"]:
                for q in cs:
                    t = tuple(q)
                    if t not in seen:
                        seen.add(t)
                        out.append(q)
    return out


# ---------------------------------------------------------------------------------------------------------------- rule-sensitive contours
def compress(c):
    """a contour as (start, runs of equal steps): the form PINNED is committed in"""
    runs = []
    for p, q in zip(c, c[1:]):
        d = (q[0] - p[0], q[1] - p[1])
        if runs and runs[-1][:2] == d:
            runs[-1] = (d[0], d[1], runs[-1][2] + 1)
        else:
            runs.append((d[0], d[1], 1))
    return (tuple(c[0]), tuple(runs))


def expand(entry):
    start, runs = entry
    pts = [tuple(start)]
    for dx, dy, n in runs:
        for _ in range(n):
            pts.append((pts[-1][0] + dx, pts[-1][1] + dy))
    return pts


def _random_contour(rng):
    kind = int(rng.integers(0, 6))
    if kind == 0:      # few points on a small lattice: ties, coinciding ends
        span = int(rng.choice([4, 8, 16]))
        return [(int(rng.integers(0, span)), int(rng.integers(0, span))) for _ in range(int(rng.integers(5, 14)))]
    if kind == 1:      # a jittered ellipse whose ends need not be neighbours: the closing segment is a good part of the perimeter
        L = int(rng.integers(6, 40))
        c = blob(L + int(rng.integers(0, 12)), int(rng.integers(0, 1 << 20)), 100, 100, float(rng.integers(10, 90)), float(rng.integers(10, 90)))
        return c[:L]
    if kind == 2:      # ... that revisits P[0] just before its end
        c = blob(int(rng.integers(8, 40)), int(rng.integers(0, 1 << 20)), 100, 100, float(rng.integers(10, 90)), float(rng.integers(10, 90)))
        c[-2] = c[0]
        c[-1] = (c[0][0] + int(rng.integers(-40, 41)), max(0, c[0][1] + int(rng.integers(-40, 41))))
        return [(max(0, x), y) for x, y in c]
    a, b = int(rng.integers(66, 180)), int(rng.integers(3, 180))
    if kind == 3:      # rectangles with a side above 64, often above 128 points, from any start
        r = rect_outline(1, 1, a, b) if rng.integers(0, 2) else rect_outline(1, 1, b, a)
    elif kind == 4:    # L-shapes
        r = ell_outline(1, 1, a, max(b, 6)) if rng.integers(0, 2) else ell_outline(1, 1, max(b, 6), a)
    else:              # a line out and back with a bump
        r = line_out_and_back(1, 5, a)
        r[int(rng.integers(1, a - 1))] = (int(rng.integers(1, a)), int(rng.integers(0, 12)))
    return rotate(r, int(rng.integers(0, len(r))))


def search_rule_sensitive(seed: int = 11, per_rule: int = 10, seconds: float = 240.0):
    """Random lattice contours, kept while some observable mutant that still has fewer than per_rule contours changes their candidate.
    Returns (contours, {mutant: count}, contours tried, largest kept count seen)."""
    rng = np.random.default_rng(seed)
    live = [mu for mu in MUTANTS if mu not in EQUIVALENT_MUTANTS]
    hits = {mu: 0 for mu in live}
    kept, tried, most, t0 = [], 0, 0, time.time()
    while min(hits.values()) < per_rule and time.time() - t0 < seconds:
        c = _random_contour(rng)
        tried += 1
        st = []
        candidate_rules(c, stats=st)
        most = max(most, st[-1][1])
        ch = [mu for mu in mutants_changing(c) if mu in hits]
        if any(hits[mu] < per_rule for mu in ch):
            kept.append(c)
            for mu in ch:
                hits[mu] += 1
    return kept, hits, tried, most


# 42 contours kept of 256 tried; largest kept count 14; candidates changed per mutant: {('tie', 'last'): 10, ('tie', 'stride'): 10, ('tie', 'lane'): 23, ('dist', 'segment'): 17, ('close', 'no_closing_segment'): 12, ('close', 'keep_repeat'): 13}
PINNED = (
    ((1, 78), ((0, -1, 77), (1, 0, 59), (0, 1, 46), (1, 0, 58), (0, 1, 46), (-1, 0, 117), (0, -1, 14))),
    ((79, 5), ((1, 0, 49), (-1, 0, 127), (1, 0, 25), (99, -4, 1), (-97, 4, 1), (1, 0, 50))),
    ((159, 16), ((0, 1, 72), (-1, 0, 158), (0, -1, 87), (1, 0, 158), (0, 1, 14))),
    ((134, 100), ((0, 4, 1), (-3, 3, 1), (0, 4, 1), (-4, 3, 2), (-6, 2, 1), (-5, 2, 1), (-6, 1, 1), (-6, -1, 1), (-6, 0, 2), (-5, -2, 1), (-4, -3, 1), (-5, -2, 1), (-4, -3, 1), (-1, -4, 1), (-1, -3, 1), (-1, -4, 1), (0, -4, 2), (3, -3, 1), (4, -3, 2), (5, -2, 2), (6, 0, 1), (6, -1, 1), (6, 0, 1), (6, 1, 1), (5, 2, 1), (4, 3, 1), (5, 2, 1), (3, 3, 1), (5, 11, 1), (-40, 40, 1))),
    ((131, 100), ((-3, 15, 1), (-6, 14, 1), (-8, 9, 1), (-11, 3, 1), (-11, -1, 1), (-10, -8, 1), (-7, -10, 1), (-3, -15, 1), (-1, -15, 1), (3, -15, 1), (8, -11, 1), (10, -7, 1), (11, -2, 1))),
    ((93, 5), ((1, 0, 6), (-45, -1, 1), (47, 1, 1), (1, 0, 6), (-1, 0, 106), (1, 0, 91))),
    ((1, 70), ((0, -1, 69), (1, 0, 50), (0, 1, 89), (1, 0, 50), (0, 1, 89), (-1, 0, 100), (0, -1, 108))),
    ((69, 58), ((1, 0, 3), (0, 1, 57), (-1, 0, 71), (0, -1, 114), (1, 0, 36), (0, 1, 57), (1, 0, 31))),
    ((31, 89), ((0, 1, 1), (-1, 0, 30), (0, -1, 89), (1, 0, 30), (0, 1, 87))),
    ((74, 11), ((0, 1, 32), (-1, 0, 73), (0, -1, 42), (1, 0, 73), (0, 1, 9))),
    ((115, 21), ((0, 1, 73), (-1, 0, 114), (0, -1, 93), (1, 0, 114), (0, 1, 19))),
    ((139, 100), ((-2, 4, 1), (-3, 3, 1), (-3, 4, 1), (-8, 2, 1), (-7, 2, 2), (-9, 0, 1), (-8, -1, 1), (-9, -1, 1), (-8, -1, 1), (-4, -4, 1), (-6, -2, 1), (-3, -4, 1), (-1, -4, 1), (1, -4, 1), (3, -4, 1), (5, -3, 2), (9, -1, 1), (8, -1, 2), (8, 1, 1), (9, 0, 1), (6, 3, 1), (7, 2, 1), (9, 11, 1), (-30, -22, 1))),
    ((181, 100), ((-1, 8, 1), (2, 10, 1), (-11, 6, 1), (-3, 9, 1), (-9, 6, 1), (-10, 5, 1), (-11, 5, 1), (-12, 5, 1), (-13, -1, 1), (-13, 1, 1), (-13, 0, 1), (-13, -2, 1), (-12, -2, 1), (-12, -4, 1), (-10, -6, 1), (-6, -8, 1), (-5, -8, 1), (-9, -7, 1), (-4, -8, 1), (3, -9, 1), (1, -8, 1), (-1, -9, 1), (5, -9, 1), (9, -6, 1), (7, -8, 1), (12, -4, 1), (11, -5, 1), (11, -3, 1), (13, -2, 1), (13, -1, 2), (13, 2, 1), (13, 4, 1), (10, 5, 1), (8, 7, 1))),
    ((157, 166), ((0, 1, 8), (-1, 0, 156), (0, -1, 173), (1, 0, 78), (0, 1, 87), (1, 0, 78), (0, 1, 77))),
    ((1, 66), ((0, -1, 65), (1, 0, 27), (0, 1, 54), (1, 0, 26), (0, 1, 53), (-1, 0, 53), (0, -1, 41))),
    ((98, 125), ((-1, 0, 97), (0, -1, 124), (1, 0, 112), (0, 1, 124), (-1, 0, 14))),
    ((51, 77), ((1, 0, 43), (0, 1, 76), (-1, 0, 93), (0, -1, 152), (1, 0, 47), (0, 1, 76), (1, 0, 2))),
    ((161, 100), ((-4, 5, 1), (1, 6, 1), (-6, 4, 1), (-2, 6, 1), (-6, 4, 1), (-8, 3, 1), (-7, 4, 1), (-9, 1, 2), (-9, 0, 1), (-9, 2, 1), (-9, -1, 1), (-8, -3, 1), (-7, -3, 1), (-7, -4, 1), (-6, -3, 1), (-6, -4, 1), (-3, -5, 2), (-1, -5, 1), (-3, -6, 1), (3, -5, 1), (4, -5, 1), (3, -4, 1), (6, -5, 1), (5, -4, 1), (8, -3, 1), (7, -2, 1), (8, -3, 1), (9, 0, 1), (9, -1, 1), (10, -1, 1), (8, 2, 1), (8, 4, 1), (8, 2, 1), (6, 4, 2), (5, 4, 1))),
    ((164, 100), ((-8, 33, 1), (-15, 30, 1), (-27, 12, 1), (-29, 6, 1), (-26, -18, 1), (-15, -30, 1), (-11, -33, 1), (6, -36, 1), (20, -27, 1), (27, -14, 1), (29, -2, 1), (49, 79, 1), (-28, 15, 1))),
    ((64, 1), ((1, 0, 12), (0, 1, 63), (1, 0, 74), (0, 1, 63), (-1, 0, 149), (0, -1, 126), (1, 0, 62))),
    ((149, 100), ((-2, 8, 1), (0, 9, 1), (-3, 8, 1), (-6, 7, 1), (-6, 6, 1), (-7, 5, 1), (-8, 4, 1), (-8, 2, 1), (-9, 2, 1), (-8, -4, 1), (-9, 0, 1), (-7, -6, 1), (-8, -3, 1), (-7, -5, 1), (-3, -9, 1), (-3, -7, 1), (-3, -9, 1), (0, -8, 1), (1, -8, 1), (1, -9, 1), (3, -8, 1), (6, -6, 1), (7, -5, 1), (5, -7, 1), (8, -3, 1), (9, 0, 1), (8, -4, 1), (8, 3, 1))),
    ((118, 100), ((-1, 9, 1), (1, 9, 1), (-2, 8, 1), (-3, 5, 1), (-1, 7, 1), (-3, 7, 1), (-3, 1, 1), (-3, 4, 1), (-3, -1, 1), (-3, 1, 1), (-3, -2, 1), (-3, -6, 1), (-3, -3, 1), (-1, -8, 1), (-3, -5, 1), (-1, -9, 1), (-1, -8, 1), (-1, -9, 1), (1, -9, 1), (1, -8, 1), (2, -8, 1), (1, -8, 1), (3, -4, 1), (2, -6, 1), (3, -2, 1), (3, -4, 1), (3, 0, 1), (3, -2, 1), (3, 5, 1), (3, 2, 1), (2, 7, 1), (3, 5, 1), (1, 8, 1), (3, 24, 1), (30, 27, 1))),
    ((171, 100), ((-5, 10, 1), (-1, 10, 1), (-7, 8, 1), (-7, 9, 1), (-7, 8, 1), (-9, 6, 1), (-11, 5, 1), (-12, 0, 1), (-12, 4, 1), (-12, -1, 1), (-11, -6, 1), (-10, -4, 1), (-13, -2, 1), (-7, -9, 1), (-7, -8, 1), (-3, -10, 1), (-4, -10, 2), (5, -10, 1), (-1, -11, 1), (5, -10, 1), (8, -8, 1), (11, -5, 1), (8, -8, 1), (11, -3, 1), (12, -4, 1), (12, 2, 1), (12, -3, 1), (11, 6, 1), (13, 1, 1), (7, 10, 1), (9, 6, 1), (9, 7, 1), (10, 30, 1), (-40, -4, 1))),
    ((179, 100), ((-4, 23, 1), (-10, 20, 1), (-17, 16, 1), (-19, 13, 1), (-23, 2, 1), (-23, 0, 1), (-21, -11, 1), (-18, -12, 1), (-15, -18, 1), (-7, -21, 1), (-1, -24, 1), (6, -22, 1), (18, -16, 1), (15, -17, 1), (23, -6, 1), (23, -2, 1), (22, 6, 1), (21, 9, 1), (30, 60, 1), (-29, 21, 1))),
    ((67, 87), ((-1, 0, 66), (0, -1, 86), (1, 0, 75), (0, 1, 86), (-1, 0, 8))),
    ((143, 100), ((-6, 6, 1), (-15, 5, 1), (-22, 2, 1), (-22, -2, 1), (-15, -5, 1), (-8, -6, 1), (8, -6, 1), (15, -5, 1), (22, -2, 1), (43, 13, 1), (18, 40, 1))),
    ((143, 100), ((-2, 14, 1), (-1, 14, 1), (-3, 13, 1), (-4, 12, 1), (-5, 12, 1), (-5, 9, 1), (-7, 7, 1), (-7, -1, 1), (-7, 4, 1), (-7, -2, 1), (-7, -3, 1), (-7, -4, 1), (-7, -5, 1), (-4, -12, 1), (-5, -10, 1), (-3, -14, 1), (-3, -13, 1), (0, -14, 1), (-2, -14, 1), (1, -15, 1), (4, -13, 1), (3, -13, 1), (4, -11, 1), (6, -7, 1), (5, -12, 1), (7, -5, 1), (7, -3, 1), (8, 0, 1), (7, 6, 1), (7, 1, 1), (7, 5, 1), (5, 9, 1), (4, 14, 1), (4, 11, 1), (7, 40, 1), (20, 15, 1))),
    ((134, 100), ((-9, 41, 1), (-25, 17, 1), (-24, -20, 1), (-11, -38, 1), (10, -40, 1), (59, 40, 1), (30, -33, 1))),
    ((6, 4), ((1, -1, 1), (-4, 3, 1), (-3, -5, 1), (7, 0, 1), (-1, 4, 1), (1, -3, 1))),
    ((117, 100), ((-1, 23, 1), (-3, 22, 1), (-5, 12, 1), (-5, 11, 1), (-6, -2, 1), (-5, -9, 1), (-5, -13, 1), (-2, -22, 1), (-1, -22, 1), (0, -23, 1), (3, -20, 1))),
    ((165, 100), ((-2, 15, 1), (-10, 14, 1), (-13, 12, 1), (-19, 8, 1), (-21, 3, 1), (-20, -5, 1), (-21, -5, 1), (-12, -13, 2), (0, -16, 2), (10, -14, 1), (16, -10, 1), (18, -9, 1), (21, -1, 1), (20, 3, 1))),
    ((7, 7), ((-6, -6, 1), (2, 1, 1), (-2, -1, 1), (6, 4, 1), (-4, -1, 1), (-1, 0, 1), (-1, -4, 1), (3, 4, 1), (-1, -1, 1), (-2, 3, 1))),
    ((134, 100), ((-2, 12, 1), (-2, 11, 2), (-7, 7, 1), (-5, 7, 1), (-7, 5, 2), (-7, -3, 1), (-8, -1, 1), (-7, -6, 1), (-5, -8, 1), (-5, -10, 1), (-3, -11, 1), (0, -13, 1), (-1, -12, 1), (2, -12, 1), (2, -11, 1), (5, -10, 1), (6, -8, 1), (6, -6, 1), (7, -3, 1), (8, -1, 1), (7, 3, 1), (7, 5, 2), (5, 9, 1), (6, 35, 1), (17, -40, 1))),
    ((1, 6), ((0, -1, 5), (1, 0, 3), (0, 1, 40), (1, 0, 2), (0, 1, 39), (-1, 0, 5), (0, -1, 73))),
    ((138, 100), ((0, 6, 1), (-3, 6, 1), (-3, 5, 1), (-5, 5, 1), (-7, 4, 1), (-8, 2, 2), (-8, -1, 1), (-8, -3, 1), (-7, -1, 1), (-7, -4, 1), (-6, -4, 1), (-5, -5, 1), (-1, -6, 2), (0, -6, 1), (5, -5, 1), (2, -6, 1), (6, -5, 1), (7, -3, 1), (7, -2, 1), (8, -2, 1), (8, 1, 2), (7, 2, 1), (7, 3, 1), (6, 5, 1), (4, 5, 1))),
    ((131, 100), ((-1, 16, 1), (-2, 15, 1), (-4, 15, 1), (-5, 10, 1), (-7, 8, 1), (-6, 6, 1), (-8, 0, 1), (-7, -7, 1), (-7, -1, 1), (-5, -13, 1), (-5, -11, 1), (-2, -15, 1), (-3, -15, 1), (-1, -16, 1), (3, -16, 1), (2, -15, 1), (6, -10, 1))),
    ((1, 1), ((1, 1, 1), (-2, -1, 1), (1, 1, 1), (0, 1, 1), (0, -2, 1), (0, 1, 1), (0, -2, 1), (0, 1, 1), (0, -1, 1), (2, 1, 1), (-1, 0, 1), (0, 1, 1))),
    ((132, 100), ((-4, 30, 1), (-9, 24, 1), (-15, 11, 1), (-15, -6, 1), (-12, -18, 1), (-8, -26, 1), (0, -30, 1), (6, -29, 1), (14, -14, 1), (15, -4, 1), (28, 62, 1), (35, -12, 1))),
    ((188, 100), ((-2, 19, 1), (-13, 16, 1), (-6, 18, 1), (-16, 12, 1), (-17, 11, 1), (-19, 3, 1), (-20, 4, 1), (-20, -5, 1), (-18, -7, 1), (-17, -11, 1), (-12, -15, 1), (-9, -17, 1), (-1, -19, 1), (0, -18, 1), (4, -18, 1), (5, -19, 1), (13, -14, 1), (18, -10, 1), (18, -6, 1), (19, -6, 1), (19, 4, 1), (21, 2, 1), (16, 11, 1), (12, 15, 1), (25, 50, 1), (-31, -24, 1))),
    ((176, 100), ((-2, 10, 1), (-3, 10, 1), (-11, 9, 1), (-10, 9, 1), (-16, 5, 1), (-17, 2, 1), (-17, 3, 1), (-18, -1, 1), (-16, -4, 1), (-16, -5, 1), (-11, -9, 1), (-10, -8, 1), (-7, -10, 1), (-2, -11, 1), (5, -10, 1), (4, -11, 1), (8, -9, 1), (15, -6, 1))),
    ((120, 100), ((1, 12, 1), (-2, 10, 1), (-1, 11, 1), (-2, 9, 1), (-3, 7, 1), (-4, 7, 1), (-3, 4, 1), (-4, 2, 2), (-4, -5, 1), (-3, -3, 1), (-4, -7, 1), (-3, -6, 1), (-2, -9, 1), (-1, -12, 1), (-2, -11, 1), (-1, -11, 1), (1, -11, 1), (1, -12, 1), (2, -11, 1), (2, -9, 1), (4, -6, 1), (3, -7, 1), (3, -5, 1), (4, -1, 1), (4, -2, 1), (4, 7, 1), (4, 1, 1), (3, 7, 1), (3, 6, 1), (2, 11, 1), (2, 32, 1), (-12, -31, 1))),
    ((3, 0), ((-3, 2, 1), (2, 0, 1), (1, -2, 1), (-1, 2, 1), (0, -2, 1), (-1, 3, 1), (2, -2, 1), (-1, 1, 1), (0, 0, 1))),
)


if __name__ == "__main__":
    t0 = time.time()
    cs, hits, tried, most = search_rule_sensitive()
    print(f"# {len(cs)} contours kept of {tried} tried in {time.time() - t0:.0f} s; largest kept count {most}; candidates changed per mutant: {hits}", file=sys.stderr)
    print("PINNED = (")
    for c in cs:
        print(f"    {compress(c)},")
    print(")")
