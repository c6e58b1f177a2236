"""Numpy f64 restatement of the column rule of ocr_group_columns (include/ocr_amd.h; kernels csrc/columns.hip).

Every operation is a separately rounded IEEE f64 operation in the order the header states it, so the device result can be compared
bit for bit.  Stage A is tests/line_oracle.py with row_gap as max_gap; the pair tests of stages B, D and E are vectorised per
element, the chains are walked.  min and max are selects (`b < a ? b : a`, `b > a ? b : a`), scans replace on a strict improvement.
No GPU, no library.
"""
import numpy as np

from tests import line_oracle as LO

DEFAULTS = {"row_gap": 16.0, "min_gutter": 1.5, "gutter_reach": 2.5, "min_rows": 3, "min_overlap": 0.25, "block_reach": 2.5,
            "max_levels": 64}
INT_FIELDS = ("min_rows", "max_levels")


def params(**fields):
    """line fields and column fields in one dict -> (line params, column params)"""
    lp = {k: fields.pop(k) for k in list(fields) if k in LO.DEFAULTS}
    p = dict(DEFAULTS)
    for k, v in fields.items():
        if k not in p:
            raise TypeError(f"unknown column parameter {k!r}")
        p[k] = int(v) if k in INT_FIELDS else float(v)
    return LO.params(**lp), p


def _mn(a, b):
    return np.where(b < a, b, a)


def _mx(a, b):
    return np.where(b > a, b, a)


def _mutual(live, cand):
    """cand(p) -> (mask over q, a over q), the test in p's frame.  -> nxt, prv (mutual nearest links), ties met by the two minima"""
    n = len(live)
    nxt_c = np.full(n, -1, np.int64)
    prv_c = np.full(n, -1, np.int64)
    prv_a = np.full(n, np.inf)
    prv_tied = np.zeros(n, bool)
    ties = 0
    for p in np.flatnonzero(live):
        ok, a = cand(int(p))
        ok = ok & live
        ok[p] = False
        if not ok.any():
            continue
        idx = np.flatnonzero(ok)
        q = int(idx[np.argmin(a[idx])])
        nxt_c[p] = q
        ties += int((a[idx] == a[q]).sum() > 1)
        better = ok & ((a < prv_a) | (prv_c < 0))
        prv_tied |= ok & ~better & (a == prv_a)
        prv_tied &= ~better
        prv_c[better] = p
        prv_a[better] = a[better]
    ties += int(prv_tied.sum())
    nxt = np.full(n, -1, np.int64)
    prv = np.full(n, -1, np.int64)
    for p in range(n):
        q = nxt_c[p]
        if q >= 0 and prv_c[q] == p:
            nxt[p], prv[q] = q, p
    return nxt, prv, ties


def _walk(nxt, k):
    out = []
    while k >= 0:
        out.append(int(k))
        k = nxt[k]
    return out


def _cycles(nxt, prv):
    """the smallest index of every cycle"""
    n = len(nxt)
    seen = np.zeros(n, bool)
    for h in range(n):
        if prv[h] < 0:
            for k in _walk(nxt, h):
                seen[k] = True
    out = []
    for m in range(n):
        if not seen[m]:
            out.append(m)
            k = m
            while not seen[k]:
                seen[k] = True
                k = nxt[k]
    return out


def group_image(quads, lp, p):
    """one image -> dict(blocks: list of blocks, each a list of lines, each a list of local word indices; flags, gap by word,
    line_flags by head word, levels and quads by block in output order, ties per stage)"""
    q = np.ascontiguousarray(quads, dtype=np.float64).reshape(-1, 8)
    n = len(q)
    rows, flags, _, ties_a = LO.group_image(q, dict(lp, max_gap=p["row_gap"]))
    flags = flags.copy()
    f = LO.features(q)
    cx, cy, ux, uy, vx, vy, lu, lv, iso = (f[k] for k in ("cx", "cy", "ux", "uy", "vx", "vy", "lu", "lv", "iso"))
    with np.errstate(all="ignore"):
        half = lu * 0.5
        Lx, Ly = cx - ux * half, cy - uy * half
        Rx, Ry = cx + ux * half, cy + uy * half
    prv = np.full(n, -1, np.int64)
    for row in rows:
        for a, b in zip(row[:-1], row[1:]):
            prv[b] = a
    # ---- stage B: gap elements by their right word
    elem = prv >= 0
    G = np.zeros((n, 2))
    eu, ev = np.zeros((n, 2)), np.zeros((n, 2))
    ew, eh, gap, gg = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for j in np.flatnonzero(elem):
        i = prv[j]
        dx, dy = cx[j] - cx[i], cy[j] - cy[i]
        a = dx * ux[i] + dy * uy[i]
        g = a - (lu[i] + lu[j]) * 0.5
        hmax = lv[j] if lv[i] < lv[j] else lv[i]
        gg[j], eh[j], ew[j], gap[j] = g, hmax, g * 0.5, g / hmax
        G[j] = (Rx[i] + Lx[j]) * 0.5, (Ry[i] + Ly[j]) * 0.5
        eu[j], ev[j] = (ux[i], uy[i]), (vx[i], vy[i])
    wide = elem & (gg > lp["max_gap"] * eh)
    elig = elem & (gg >= p["min_gutter"] * eh)

    def below_gap(e):
        dx, dy = G[:, 0] - G[e, 0], G[:, 1] - G[e, 1]
        a = dx * ev[e, 0] + dy * ev[e, 1]
        b = dx * eu[e, 0] + dy * eu[e, 1]
        ok = (a > 0) & (np.abs(b) < ew[e] + ew) & (a <= p["gutter_reach"] * _mx(eh[e], eh))
        ok &= (eu[e, 0] * eu[:, 0] + eu[e, 1] * eu[:, 1]) >= lp["min_cos"]
        return ok, a
    gn, gp, ties_b = _mutual(elig, below_gap)
    for m in _cycles(gn, gp):           # the size of a cycle is its length: open it anywhere to count
        gn[gp[m]] = -1
        gp[m] = -1
    size = np.zeros(n, np.int64)
    for h in np.flatnonzero(elig & (gp < 0)):
        chain = _walk(gn, h)
        size[chain] = len(chain)
    gutter = elig & (size >= p["min_rows"])
    flags[gutter] |= 4
    cut = wide | gutter
    # ---- stage C: lines by their head word
    lines = {}
    for row in rows:
        cur = [row[0]]
        for k in row[1:]:
            if cut[k]:
                lines[cur[0]] = cur
                cur = [k]
            else:
                cur.append(k)
        lines[cur[0]] = cur
    gap_by_word = gap.copy()
    live = np.zeros(n, bool)
    S, E, M = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2))
    ln, lh = np.zeros(n), np.zeros(n)
    for h, ws in lines.items():
        gap_by_word[h] = 0.0
        live[h] = not iso[h]
        t = ws[-1]
        S[h], E[h] = (Lx[h], Ly[h]), (Rx[t], Ry[t])
        M[h] = (S[h] + E[h]) * 0.5
        ln[h] = (E[h, 0] - S[h, 0]) * ux[h] + (E[h, 1] - S[h, 1]) * uy[h]
        m = lv[ws[0]]
        for k in ws[1:]:
            m = lv[k] if lv[k] > m else m
        lh[h] = m

    # ---- stage D: blocks
    def below_line(s):
        with np.errstate(all="ignore"):
            x0 = (S[:, 0] - S[s, 0]) * ux[s] + (S[:, 1] - S[s, 1]) * uy[s]
            x1 = (E[:, 0] - S[s, 0]) * ux[s] + (E[:, 1] - S[s, 1]) * uy[s]
            lo, hi = _mn(x0, x1), _mx(x0, x1)
            ov = _mn(hi, ln[s]) - _mx(lo, 0.0)
            a = (M[:, 0] - M[s, 0]) * vx[s] + (M[:, 1] - M[s, 1]) * vy[s]
            hmax, hmin = _mx(lh[s], lh), _mn(lh[s], lh)
            ok = (a > 0) & (ov > 0) & (ov >= p["min_overlap"] * _mn(ln[s], hi - lo)) & (a <= p["block_reach"] * hmax)
            ok &= (hmax <= lp["height_ratio"] * hmin) & ((ux[s] * ux + uy[s] * uy) >= lp["min_cos"])
        return ok, a
    bn, bp, ties_d = _mutual(live, below_line)
    line_flags = np.zeros(n, np.int32)
    for m in _cycles(bn, bp):
        line_flags[m] = 1
        bn[bp[m]] = -1
        bp[m] = -1
    heads = [h for h in sorted(lines) if bp[h] < 0]
    # ---- stage E: block boxes and their order
    B = len(heads)
    quad = np.zeros((B, 8))
    fr = np.zeros((B, 4))       # u, v
    WH = np.zeros((B, 2))
    chains = []
    for b, h in enumerate(heads):
        chain = _walk(bn, h)
        chains.append(chain)
        if iso[h]:
            xs, ys = q[h, 0::2], q[h, 1::2]
            x0 = x1 = xs[0]
            y0 = y1 = ys[0]
            for k in range(1, 4):
                x0, x1 = (xs[k] if xs[k] < x0 else x0), (xs[k] if xs[k] > x1 else x1)
                y0, y1 = (ys[k] if ys[k] < y0 else y0), (ys[k] if ys[k] > y1 else y1)
            quad[b] = x0, y0, x1, y0, x1, y1, x0, y1
            fr[b] = 1.0, 0.0, 0.0, 1.0
            WH[b] = x1 - x0, y1 - y0
            continue
        O, u, v = S[h], (ux[h], uy[h]), (vx[h], vy[h])
        first = True
        for t in chain:
            xs = [(S[t, 0] - O[0]) * u[0] + (S[t, 1] - O[1]) * u[1], (E[t, 0] - O[0]) * u[0] + (E[t, 1] - O[1]) * u[1]]
            mid = (M[t, 0] - O[0]) * v[0] + (M[t, 1] - O[1]) * v[1]
            ya, yb = mid - lh[t] * 0.5, mid + lh[t] * 0.5
            if first:
                X0 = X1 = xs[0]
                Y0, Y1 = ya, yb
                first = False
            for x in xs:
                X0, X1 = (x if x < X0 else X0), (x if x > X1 else X1)
            Y0, Y1 = (ya if ya < Y0 else Y0), (yb if yb > Y1 else Y1)
        for c, (X, Y) in enumerate(((X0, Y0), (X1, Y0), (X1, Y1), (X0, Y1))):
            quad[b, 2 * c] = (O[0] + u[0] * X) + v[0] * Y
            quad[b, 2 * c + 1] = (O[1] + u[1] * X) + v[1] * Y
        fr[b] = u[0], u[1], v[0], v[1]
        WH[b] = X1 - X0, Y1 - Y0
    pred = np.zeros((B, B), bool)      # pred[x, y]: x precedes y
    for x in range(B):
        ax0 = ax1 = ay0 = ay1 = None
        for c in range(4):
            dx, dy = quad[:, 2 * c] - quad[x, 0], quad[:, 2 * c + 1] - quad[x, 1]
            px = dx * fr[x, 0] + dy * fr[x, 1]
            py = dx * fr[x, 2] + dy * fr[x, 3]
            if c == 0:
                ax0, ax1, ay0, ay1 = px, px, py, py
            else:
                ax0, ax1, ay0, ay1 = _mn(ax0, px), _mx(ax1, px), _mn(ay0, py), _mx(ay1, py)
        if B:
            W, H = WH[x]
            left = (ax0 >= W) & ((_mn(ay1, H) - _mx(ay0, 0.0)) > 0)
            above = (ay0 >= H) & ((_mn(ax1, W) - _mx(ax0, 0.0)) > 0)
            pred[x] = left | above
            pred[x, x] = False
    level = np.zeros(B, np.int64)
    cap = p["max_levels"] - 1
    for _ in range(cap):
        new = np.minimum(cap, np.where(pred, (level + 1)[:, None], 0).max(axis=0)) if B else level   # (0 where nothing precedes)
        if np.array_equal(new, level):
            break
        level = new
    order = sorted(range(B), key=lambda b: (int(level[b]), float(quad[b, 1]), float(quad[b, 0]), heads[b]))
    return {"blocks": [[lines[t] for t in chains[b]] for b in order], "flags": flags, "gap": gap_by_word,
            "line_flags": [[int(line_flags[t]) for t in chains[b]] for b in order], "levels": [int(level[b]) for b in order],
            "quads": [quad[b] for b in order], "ties": (ties_a, ties_b, ties_d)}


def group(quads, word_img_offsets, prm=None):
    """The ocr_columns_t of a batch: dict of its arrays (numpy, the ABI's types) and `ties` (stage A, B, D)."""
    lp, p = params(**(prm or {}))
    q = np.ascontiguousarray(quads, dtype=np.float64).reshape(-1, 8)
    off = np.asarray(word_img_offsets, np.int64)
    img, blk, lin, order, gaps, flags, lflags, levels, quads_out = [0], [0], [0], [], [], [], [], [], []
    ties = np.zeros(3, np.int64)
    for b in range(len(off) - 1):
        w0, w1 = int(off[b]), int(off[b + 1])
        assert w1 - w0 <= LO.MAX_WORDS
        r = group_image(q[w0:w1], lp, p)
        ties += r["ties"]
        flags.extend(r["flags"].tolist())
        for block, lf in zip(r["blocks"], r["line_flags"]):
            for line in block:
                order.extend(w0 + k for k in line)
                gaps.extend(float(r["gap"][k]) for k in line)
                lin.append(len(order))
            lflags.extend(lf)
            blk.append(len(lin) - 1)
        levels.extend(r["levels"])
        quads_out.extend(r["quads"])
        img.append(len(blk) - 1)
    return {"img_offsets": np.array(img, np.int32), "block_offsets": np.array(blk, np.int32), "line_offsets": np.array(lin, np.int32),
            "order": np.array(order, np.int32), "word_flags": np.array(flags, np.int32), "gaps": np.array(gaps, np.float64),
            "line_flags": np.array(lflags, np.int32), "block_levels": np.array(levels, np.int32),
            "block_quads": np.array(quads_out, np.float64).reshape(-1), "ties": tuple(int(t) for t in ties)}


ARRAYS = ("img_offsets", "block_offsets", "line_offsets", "order", "word_flags", "gaps", "line_flags", "block_levels", "block_quads")


def blocks_of(res, b):
    """the blocks of image b: lists of lines, lists of batch-global word indices"""
    out = []
    for k in range(int(res["img_offsets"][b]), int(res["img_offsets"][b + 1])):
        out.append([res["order"][res["line_offsets"][l]:res["line_offsets"][l + 1]].tolist()
                    for l in range(int(res["block_offsets"][k]), int(res["block_offsets"][k + 1]))])
    return out


# ---- case builders shared by the CPU and the GPU tests
def columns_page(gutter, angle, rows, extras, seed, n_cols=2, origin=(600.0, 500.0)):
    """A page of `n_cols` columns with rows[c] rows each, 5 words a row, heights 16..18, row pitch 30, ragged right edges, the last
    row of each column half length; the gutters are `gutter` times 18 px wide.  extras: 0 bare, 1 a full-width heading, 2 heading and
    footer, each set off by two row pitches (beyond block_reach: a heading at one pitch joins whichever column starts nearer).  The
    page is turned by `angle` about `origin` and its words are shuffled.
    -> (quads, label of every word), label = (part, row, k) with part 0 heading, 1 + c column c, 99 footer; the page reads in
    ascending label order."""
    rng = np.random.default_rng(seed)
    pitch, space, col_w = 30.0, 8.0, 5 * 44.0 + 4 * 8.0      # (the widest row of five words fills the column)
    gw = gutter * 18.0
    width = n_cols * col_w + (n_cols - 1) * gw
    words = []

    def row_of(x0, x1, y, part, r, short=False):
        """words of width 30..44, 8 apart, from x0: five in a column row, three in a short one, as many as fit in a full-width one"""
        x, k = x0, 0
        count = (3 if short else 5) if part not in (0, 99) else 10 ** 6
        while k < count:
            w = rng.uniform(30.0, 44.0)
            if x + w > x1:
                break
            words.append((x + w / 2, y + rng.uniform(-1.0, 1.0), w, rng.uniform(16.0, 18.0), (part, r, k)))
            x += w + space
            k += 1
    top = 0.0
    if extras >= 1:
        row_of(0.0, width, top, 0, 0)
        top += 2 * pitch
    for c in range(n_cols):
        x0 = c * (col_w + gw)
        for r in range(rows[c]):
            row_of(x0, x0 + col_w, top + r * pitch, 1 + c, r, short=(r == rows[c] - 1))
    if extras >= 2:
        row_of(0.0, width, top + (max(rows) + 1) * pitch, 99, 0)
    c, s = np.cos(angle), np.sin(angle)
    quads, labels = [], []
    for x, y, w, h, lab in words:
        x, y = x - width / 2, y - max(rows) * pitch / 2
        quads.append(LO.quad(origin[0] + x * c - y * s, origin[1] + x * s + y * c, w, h, angle + rng.uniform(-0.01, 0.01)))
        labels.append(lab)
    perm = rng.permutation(len(quads))
    return np.array([quads[i] for i in perm]), [labels[i] for i in perm]


def two_sections(seed=1):
    """two two-column sections with a full-width heading between them, the heading two pitches from either -> (quads, labels); label
    parts ascend in reading order: L1, R1, heading, L2, R2"""
    q1, l1 = columns_page(3, 0.0, (5, 5), 0, seed)
    # section 1's last row is 45 below its origin, section 2's heading 60 above its own: 45 + 60 + 60 puts them two pitches apart
    q2, l2 = columns_page(3, 0.0, (4, 4), 1, seed + 1, origin=(600.0, 500.0 + 165.0))
    labels = [(p, r, k) for p, r, k in l1] + [((3 if p == 0 else p + 3), r, k) for p, r, k in l2]
    return np.concatenate([q1, q2]), labels


def grid_fuzz(n, seed):
    """LO.fuzz(grid=True) on a wider lattice: integer coordinates, few sizes, so gaps stack exactly and projections tie"""
    rng = np.random.default_rng(seed)
    cols, rows = max(4, int(np.sqrt(n) * 1.5)), max(4, int(np.sqrt(n) * 1.5))
    cx = rng.integers(0, cols, n) * 48.0
    cy = rng.integers(0, rows, n) * 24.0
    w = rng.choice([16.0, 24.0, 32.0], n)
    h = rng.choice([8.0, 12.0], n)
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy - h / 2, cx + w / 2, cy + h / 2, cx - w / 2, cy + h / 2], axis=1)
