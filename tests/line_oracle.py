"""Numpy f64 restatement of the line-grouping rule of ocr_group_lines (include/ocr_amd.h; kernels csrc/lines.hip).

Every operation is a separately rounded IEEE f64 operation in the order the header states it, so the device result can be compared
bit for bit.  The pair test is vectorised over j for every word i (4 096 words take about a second); the chains are walked word by
word.  No GPU, no library.
"""
import numpy as np

DEFAULTS = {"line_tol": 0.5, "height_ratio": 2.0, "min_cos": 0.866, "max_gap": 3.0}
MAX_WORDS = 4096


def params(**fields):
    p = dict(DEFAULTS)
    for k, v in fields.items():
        if k not in p:
            raise TypeError(f"unknown line parameter {k!r}")
        p[k] = float(v)
    return p


def features(quads):
    """quads P x 8 (TL, TR, BR, BL) -> dict of C, u, v, lu, lv, isolated, per word."""
    q = np.ascontiguousarray(quads, dtype=np.float64).reshape(-1, 8)
    with np.errstate(all="ignore"):
        ux, uy = q[:, 2] - q[:, 0], q[:, 3] - q[:, 1]
        vx, vy = q[:, 6] - q[:, 0], q[:, 7] - q[:, 1]
        lu = np.sqrt(ux * ux + uy * uy)
        lv = np.sqrt(vx * vx + vy * vy)
        cx, cy = (q[:, 0] + q[:, 4]) * 0.5, (q[:, 1] + q[:, 5]) * 0.5
        f = {"cx": cx, "cy": cy, "ux": ux / lu, "uy": uy / lu, "vx": vx / lv, "vy": vy / lv, "lu": lu, "lv": lv}
    f["iso"] = (lu == 0) | (lv == 0)
    return f


def _pair(f, i, p):
    """word i against every j: (candidate mask, a, g / hmax), the test evaluated in i's frame"""
    with np.errstate(all="ignore"):
        dx, dy = f["cx"] - f["cx"][i], f["cy"] - f["cy"][i]
        a = dx * f["ux"][i] + dy * f["uy"][i]
        b = dx * f["vx"][i] + dy * f["vy"][i]
        lvi = f["lv"][i]
        hmin = np.where(lvi < f["lv"], lvi, f["lv"])
        hmax = np.where(lvi < f["lv"], f["lv"], lvi)
        g = a - (f["lu"][i] + f["lu"]) * 0.5
        ok = (a > 0) & (np.abs(b) <= p["line_tol"] * hmin) & (hmax <= p["height_ratio"] * hmin)
        ok &= (f["ux"][i] * f["ux"] + f["uy"][i] * f["uy"]) >= p["min_cos"]
        ok &= g <= p["max_gap"] * hmax
        ok &= ~f["iso"]
        ok[i] = False
        if f["iso"][i]:
            ok[:] = False
        return ok, a, g / hmax


def links(quads, p):
    """one image: right[i], left[j], the gap of every mutual link by its right word, and how many of the two minima were tied"""
    f = features(quads)
    n = len(f["lu"])
    right = np.full(n, -1, np.int64)
    left = np.full(n, -1, np.int64)
    left_a = np.full(n, np.inf)
    left_gap = np.zeros(n)
    left_tied = np.zeros(n, bool)
    ties = 0
    for i in range(n):
        ok, a, gap = _pair(f, i, p)
        if not ok.any():
            continue
        idx = np.flatnonzero(ok)
        j = int(idx[np.argmin(a[idx])])        # the first of equal minima: the smaller j
        right[i] = j
        ties += int((a[idx] == a[j]).sum() > 1)
        better = ok & ((a < left_a) | (left < 0))   # i ascends: a strict improvement only, so the smaller i keeps a tie
        left_tied |= ok & ~better & (a == left_a)
        left_tied &= ~better
        left[better] = i
        left_a[better] = a[better]
        left_gap[better] = gap[better]
    ties += int(left_tied.sum())
    return f, right, left, left_gap, ties


def group_image(quads, p):
    """one image -> (lines as lists of local word indices in reading order, flags per word, gap per word (by word), ties)"""
    f, right, left, left_gap, ties = links(quads, p)
    n = len(right)
    flags = np.where(f["iso"], 1, 0).astype(np.int32)
    nxt = np.full(n, -1, np.int64)
    prv = np.full(n, -1, np.int64)
    for i in range(n):
        j = right[i]
        if j >= 0 and left[j] == i:
            nxt[i], prv[j] = j, i
    # cycles: whatever a walk from the heads does not reach; cut on the link into the smallest index of each
    seen = np.zeros(n, bool)
    for h in range(n):
        if prv[h] < 0:
            k = h
            while k >= 0:
                seen[k] = True
                k = nxt[k]
    for m in range(n):
        if not seen[m]:
            flags[m] |= 2
            nxt[prv[m]] = -1
            prv[m] = -1
            k = m
            while k >= 0:
                seen[k] = True
                k = nxt[k]
    heads = sorted((h for h in range(n) if prv[h] < 0), key=lambda h: (float(f["cy"][h]), float(f["cx"][h]), h))
    lines = []
    for h in heads:
        line, k = [], h
        while k >= 0:
            line.append(int(k))
            k = nxt[k]
        lines.append(line)
    gap = np.where(prv >= 0, left_gap, 0.0)
    return lines, flags, gap, ties


def group(quads, word_img_offsets, p=None):
    """The ocr_lines_t of a batch: dict of img_offsets, line_offsets, order, word_flags, gaps (numpy, the ABI's types) and `ties`."""
    p = params(**(p or {}))
    q = np.ascontiguousarray(quads, dtype=np.float64).reshape(-1, 8)
    off = np.asarray(word_img_offsets, np.int64)
    img_offsets, line_offsets, order, gaps, flags, ties = [0], [0], [], [], [], 0
    for b in range(len(off) - 1):
        w0, w1 = int(off[b]), int(off[b + 1])
        assert w1 - w0 <= MAX_WORDS
        lines, fl, gp, t = group_image(q[w0:w1], p)
        ties += t
        flags.extend(fl.tolist())
        for line in lines:
            order.extend(w0 + k for k in line)
            gaps.extend(float(gp[k]) for k in line)
            line_offsets.append(len(order))
        img_offsets.append(len(line_offsets) - 1)
    return {"img_offsets": np.array(img_offsets, np.int32), "line_offsets": np.array(line_offsets, np.int32),
            "order": np.array(order, np.int32), "word_flags": np.array(flags, np.int32), "gaps": np.array(gaps, np.float64), "ties": ties}


def lines_of(res, b):
    """the lines of image b as lists of batch-global word indices"""
    return [res["order"][res["line_offsets"][l]:res["line_offsets"][l + 1]].tolist()
            for l in range(int(res["img_offsets"][b]), int(res["img_offsets"][b + 1]))]


# ---- case builders shared by the CPU and the GPU tests
def quad(cx, cy, w, h, angle=0.0):
    """an upright w x h word centred on (cx, cy), turned by `angle` about its centre -> TL, TR, BR, BL"""
    c, s = np.cos(angle), np.sin(angle)
    pts = [(-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2)]
    return [v for x, y in pts for v in (cx + x * c - y * s, cy + x * s + y * c)]


def page(rows, cols, angle, seed, pitch_x=70.0, pitch_y=40.0, origin=(300.0, 300.0)):
    """rows x cols jittered words of a page turned by `angle` about `origin`, in shuffled order -> (quads, row of every word, column)"""
    rng = np.random.default_rng(seed)
    c, s = np.cos(angle), np.sin(angle)
    words = []
    for r in range(rows):
        for k in range(cols):
            x = (k - (cols - 1) / 2) * pitch_x + rng.uniform(-4, 4)
            y = (r - (rows - 1) / 2) * pitch_y + rng.uniform(-2, 2)
            words.append((quad(origin[0] + x * c - y * s, origin[1] + x * s + y * c, rng.uniform(40, 56), rng.uniform(16, 20),
                               angle + rng.uniform(-0.03, 0.03)), r, k))
    perm = rng.permutation(len(words))
    return (np.array([words[i][0] for i in perm]), np.array([words[i][1] for i in perm]), np.array([words[i][2] for i in perm]))


def ring(n=24, radius=150.0, centre=(300.0, 300.0), w=30.0, h=14.0):
    """n words along a circle, clockwise on the screen (y down), word 0 at the top: every word's right neighbour is the next one"""
    out = []
    for k in range(n):
        t = 2 * np.pi * k / n
        out.append(quad(centre[0] + radius * np.sin(t), centre[1] - radius * np.cos(t), w, h, t))
    return np.array(out)


def fuzz(n, seed, grid=False, span=None):
    """n random words: mostly near-horizontal, a few steep, heights 8..32; grid=True puts every coordinate on integers (axis-aligned,
    few distinct sizes) so that equal projections occur"""
    rng = np.random.default_rng(seed)
    span = span or max(200.0, 40.0 * np.sqrt(n))
    if grid:
        cx = rng.integers(0, int(span) // 8, n) * 8.0
        cy = rng.integers(0, int(span) // 16, n) * 16.0
        w = rng.choice([16.0, 24.0, 32.0], n)
        h = rng.choice([8.0, 12.0], n)
        return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy - h / 2, cx + w / 2, cy + h / 2, cx - w / 2, cy + h / 2], axis=1)
    out = []
    for _ in range(n):
        ang = rng.uniform(-0.2, 0.2) if rng.random() < 0.85 else rng.uniform(-np.pi, np.pi)
        out.append(quad(rng.uniform(0, span), rng.uniform(0, span), rng.uniform(10, 80), rng.uniform(8, 32), ang))
    return np.array(out)
