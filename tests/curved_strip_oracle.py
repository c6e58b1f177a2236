"""ORACLE (test infrastructure) for the BUILD-DEFINED curved strip rule: detected word (polygon, possibly an arc) -> centreline through
the polygon's own ring -> upright strip of strip_height rows whose columns follow the centreline's normals, all strips of a batch side
by side in one atlas.

The reference never built this step; this file restates the rule of include/ocr_amd.h (ocr_plan_curved_strips,
ocr_extract_curved_strips) and ocr-rs_amd/csrc/word_strips.cpp / curved_strips.hip must equal it bit for bit.  Geometry in Python
floats (IEEE f64, every operation separately rounded); hypot is libm's as oracle/postproc_oracle.py restates it.  Per polygon:
  1. the rectangle of tests/strip_oracle.py (steps 1-4): TL, U, V, |U|, |V|; eu = U / |U|, ev = V / |V|; a degenerate word -> step 9;
  2. ring: every vertex in order, P = (x * adj_x, y * adj_y), a = (P - TL) . eu, b = (P - TL) . ev (x term + y term);
  3. scan lines s = 0..31 at a_s = (|U| * (s + 0.5)) / 32: edge A -> B (the ring closed) crosses when (a_A <= a_s) != (a_B <= a_s), at
     b = b_A + ((a_s - a_A) * (b_B - b_A)) / (a_B - a_A); top_s = min b, bot_s = max b (no crossing: both 0), m_s = (top_s + bot_s) * 0.5,
     t_s = bot_s - top_s; more than two crossings on a line: folded;
  4. tm = element 16 of the sorted t_s; line s is valid when t_s * 100 >= valid_pct * tm; lo, hi = first and last valid line;
     tm <= 0 or hi - lo < 1 -> step 9;
  5. Q = (0, m_lo - s0 * a_lo), (a_s, m_s) for s = lo..hi, (|U|, m_hi + s1 * (|U| - a_hi)) with s0 = (m_(lo+1) - m_lo) / (a_(lo+1) - a_lo),
     s1 = (m_hi - m_(hi-1)) / (a_hi - a_(hi-1)); len_i = hypot(da, db), L = their sum in order; |db| * 10 > |da| * 7 on a segment: steep;
  6. per s in lo..hi: d = Q_next - Q_prev, c = d_a / hypot(d_a, d_b), hh_s = (t_s * c) * 0.5; h = element cnt // 2 of the sorted hh_s,
     at least 0.5;
  7. Ws = floor((Hs * L) / (2 * h) + 0.5) clamped to [1, max_width] (above: squeezed); tscale = f32(32.0 / Ws);
  8. knots r = 0..32: l = (L * r) / 32, start_0 = 0, start_(i+1) = start_i + len_i, i = the largest segment with start_i <= l,
     P = Q_i + ((l - start_i) * (Q_(i+1) - Q_i)) / len_i per coordinate, P_32 = the last point of Q; T = (P_min(r+1,32) - P_max(r-1,0)) /
     hypot of it; k = (2 * h) / Hs, N = ((-T_b) * k, T_a * k); p = (TL + P_a * eu) + P_b * ev, n = N_a * eu + N_b * ev, each rounded once
     to f32;
  9. straight fallback: P_r = (TL + U * (r / 32.0)) + V * 0.5, n = V / Hs, h = |V| / 2, L = |U|, Ws = floor((Hs * |U|) / |V| + 0.5).
Sampling, f32: t = (c + 0.5) * tscale, r = min(int(t), 31), f = t - r, knot values px, py, nx, ny = k_r + f * (k_(r+1) - k_r),
o = (i + 0.5) - 0.5 * Hs, sx = (px + o * nx) - 0.5, sy likewise; clamp, taps and blend of tests/strip_oracle.py.
"""
from __future__ import annotations

import math

import numpy as np

from oracle.postproc_oracle import hypot_libm as hypot
from tests import strip_oracle as S

F = np.float32
DEFAULTS = dict(strip_height=32, max_width=1024, valid_pct=80)
SCANLINES, KNOTS = 32, 33
SQUEEZED, DEGENERATE, FOLDED, STEEP, STRAIGHT = 1, 2, 4, 8, 16


def params_with(params=None) -> dict:
    p = dict(DEFAULTS)
    if params:
        p.update(params)
    return p


def plan_word(poly, ax: float, ay: float, hs: int, max_width: int, valid_pct: int):
    """One polygon -> (knots 33 x 4 f32 (px, py, nx, ny), tscale f32, h, L, Ws, flags)."""
    C, _, _, sflags = S.plan_word(poly, ax, ay, hs, max_width)
    tlx, tly = C[0]
    ux, uy = C[1][0] - C[0][0], C[1][1] - C[0][1]
    vx, vy = C[3][0] - C[0][0], C[3][1] - C[0][1]
    lu, lv = math.sqrt(ux * ux + uy * uy), math.sqrt(vx * vx + vy * vy)
    fhs = float(hs)

    def finish(kn, h, length, wd, flags):
        if wd > max_width:
            ws = max_width
            flags |= SQUEEZED
        else:
            ws = max(int(wd), 1)
        return np.array(kn, np.float64).astype(np.float32), F(32.0 / ws), h, length, ws, flags

    def straight(flags):
        kn = []
        for r in range(KNOTS):
            f = r / 32.0
            kn.append(((tlx + ux * f) + vx * 0.5, (tly + uy * f) + vy * 0.5, vx / fhs, vy / fhs))
        return finish(kn, lv / 2, lu, math.floor((fhs * lu) / lv + 0.5), flags | STRAIGHT)

    if sflags & S.DEGENERATE:
        return straight(DEGENERATE)
    eux, euy, evx, evy = ux / lu, uy / lu, vx / lv, vy / lv
    ra, rb = [], []
    for x, y in poly:
        dx, dy = float(x) * ax - tlx, float(y) * ay - tly
        ra.append(dx * eux + dy * euy)
        rb.append(dx * evx + dy * evy)
    nv = len(ra)
    flags = 0
    a_s, m_s, t_s = [], [], []
    for s in range(SCANLINES):
        a = (lu * (s + 0.5)) / 32
        top = bot = 0.0
        cnt = 0
        for i in range(nv):
            j = (i + 1) % nv
            if (ra[i] <= a) != (ra[j] <= a):
                b = rb[i] + ((a - ra[i]) * (rb[j] - rb[i])) / (ra[j] - ra[i])
                if cnt == 0 or b < top:
                    top = b
                if cnt == 0 or b > bot:
                    bot = b
                cnt += 1
        if cnt > 2:
            flags |= FOLDED
        a_s.append(a)
        m_s.append((top + bot) * 0.5)
        t_s.append(bot - top)
    tm = sorted(t_s)[16]
    if not tm > 0:
        return straight(flags)
    valid = [t * 100 >= valid_pct * tm for t in t_s]
    lo = valid.index(True)
    hi = SCANLINES - 1 - valid[::-1].index(True)
    if hi - lo < 1:
        return straight(flags)
    s0 = (m_s[lo + 1] - m_s[lo]) / (a_s[lo + 1] - a_s[lo])
    s1 = (m_s[hi] - m_s[hi - 1]) / (a_s[hi] - a_s[hi - 1])
    Q = [(0.0, m_s[lo] - s0 * a_s[lo])] + [(a_s[s], m_s[s]) for s in range(lo, hi + 1)] + [(lu, m_s[hi] + s1 * (lu - a_s[hi]))]
    lens, start = [], [0.0]
    for i in range(len(Q) - 1):
        da, db = Q[i + 1][0] - Q[i][0], Q[i + 1][1] - Q[i][1]
        if abs(db) * 10 > abs(da) * 7:
            flags |= STEEP
        lens.append(hypot(da, db))
        start.append(start[-1] + lens[-1])
    length = start[-1]
    hh = []
    for s in range(lo, hi + 1):
        i = s - lo + 1
        da, db = Q[i + 1][0] - Q[i - 1][0], Q[i + 1][1] - Q[i - 1][1]
        c = da / hypot(da, db)
        hh.append((t_s[s] * c) * 0.5)
    h = sorted(hh)[len(hh) // 2]
    if h < 0.5:
        h = 0.5
    wd = math.floor((fhs * length) / (2 * h) + 0.5)
    P = []
    for r in range(KNOTS - 1):
        l = (length * r) / 32
        i = 0
        while i + 1 < len(lens) and start[i + 1] <= l:
            i += 1
        d = l - start[i]
        P.append((Q[i][0] + (d * (Q[i + 1][0] - Q[i][0])) / lens[i], Q[i][1] + (d * (Q[i + 1][1] - Q[i][1])) / lens[i]))
    P.append(Q[-1])
    k = (2 * h) / fhs
    kn = []
    for r in range(KNOTS):
        p1, p0 = P[min(r + 1, 32)], P[max(r - 1, 0)]
        da, db = p1[0] - p0[0], p1[1] - p0[1]
        hy = hypot(da, db)
        ta, tb = da / hy, db / hy
        na, nb = (-tb) * k, ta * k
        pa, pb = P[r]
        kn.append(((tlx + pa * eux) + pb * evx, (tly + pa * euy) + pb * evy, na * eux + nb * evx, na * euy + nb * evy))
    return finish(kn, h, length, wd, flags)


def plan(polys, adj, scores=None, params=None) -> dict:
    """polys: per image the polygons in original-image pixels; adj: N x 2.  Returns the arrays of ocr_curved_strips_t."""
    p = params_with(params)
    hs, mw, vp = p["strip_height"], p["max_width"], p["valid_pct"]
    info, knots, ts, hh, ll, cols = [], [], [], [], [], [0]
    for b, plist in enumerate(polys):
        ax, ay = float(adj[b][0]), float(adj[b][1])
        if not (math.isfinite(ax) and ax > 0 and math.isfinite(ay) and ay > 0):
            raise ValueError(f"adjust values ({ax}, {ay})")
        for poly in plist:
            kn, tscale, h, length, ws, flags = plan_word(poly, ax, ay, hs, mw, vp)
            info.append((b, flags))
            knots.append(kn)
            ts.append(tscale)
            hh.append(h)
            ll.append(length)
            cols.append(cols[-1] + ws)
            if cols[-1] * hs > S.MAX_ATLAS:
                raise ValueError("atlas of more than 2^31 elements")
    nw = len(info)
    sc = [s for ss in scores for s in ss] if scores is not None else [0.0] * nw
    return dict(img_offsets=np.cumsum([0] + [len(pl) for pl in polys]).astype(np.int32), col_offsets=np.asarray(cols, np.int32),
                word_info=np.asarray(info, np.int32).reshape(-1, 2), knots=np.asarray(knots, np.float32).reshape(-1, KNOTS, 4),
                tscale=np.asarray(ts, np.float32), half_heights=np.asarray(hh, np.float64), lengths=np.asarray(ll, np.float64),
                scores=np.asarray(sc, np.float64), height=hs, total_width=int(cols[-1]))


def extract(frames: np.ndarray, strips: dict) -> np.ndarray:
    """frames: N x 1 x H x W f32 (raw 0..255) -> the atlas, height x total_width f32."""
    n, _, h, w = frames.shape
    hs, tw = strips["height"], strips["total_width"]
    if tw == 0:
        return np.zeros((hs, 0), np.float32)
    cols = strips["col_offsets"]
    word = np.repeat(np.arange(len(cols) - 1), np.diff(cols))
    fr = strips["word_info"][word, 0].astype(np.int64)[None, :]
    t = ((np.arange(tw) - cols[word]).astype(np.float32) + F(0.5)) * strips["tscale"][word]
    r = np.minimum(t.astype(np.int64), 31)
    f = t - r.astype(np.float32)
    k0, k1 = strips["knots"][word, r], strips["knots"][word, r + 1]          # tw x 4
    kv = k0 + f[:, None] * (k1 - k0)
    px, py, nx, ny = (kv[:, k][None, :] for k in range(4))
    o = ((np.arange(hs).astype(np.float32) + F(0.5)) - F(0.5) * F(hs))[:, None]
    sx = (px + o * nx) - F(0.5)
    sy = (py + o * ny) - F(0.5)
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
    with np.errstate(invalid="ignore"):
        top = a + fx * (b - a)
        bot = c + fx * (d - c)
        return (top + fy * (bot - top)).astype(np.float32)


def strip_polygons(strips: dict):
    """ocr_curved_strip_polygons: the rule of ocr_word_strip_polygons."""
    return S.strip_polygons(strips)


def glyph_quads(strips: dict, word: int, boxes: np.ndarray) -> np.ndarray:
    """Glyph boxes (x0, y0, x1, y1 half-open atlas pixels) of word `word` -> k x 4 x 2 f64 frame coordinates of the corners (x0, y0),
    (x1, y0), (x1, y1), (x0, y1): the sampling map in f64 from the f32 knots, at t = (x - c0) * (32 / Ws), r = min(int(t), 31),
    f = t - r, knot values k_r + f * (k_(r+1) - k_r), and (px + o * nx, py + o * ny) at o = y - Hs / 2."""
    kn = strips["knots"][word].astype(np.float64)
    hs = float(strips["height"])
    c0 = int(strips["col_offsets"][word])
    ws = float(strips["col_offsets"][word + 1] - c0)
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    xs = np.stack([b[:, 0], b[:, 2], b[:, 2], b[:, 0]], axis=1).astype(np.float64)
    ys = np.stack([b[:, 1], b[:, 1], b[:, 3], b[:, 3]], axis=1).astype(np.float64)
    t = (xs - float(c0)) * (32.0 / ws)
    r = np.clip(t.astype(np.int64), 0, 31)
    f = (t - r.astype(np.float64))[..., None]
    kv = kn[r] + f * (kn[r + 1] - kn[r])
    o = ys - hs / 2
    return np.stack([kv[..., 0] + o * kv[..., 2], kv[..., 1] + o * kv[..., 3]], axis=2)
