"""The word strip oracle (tests/strip_oracle.py) held to facts that do not come from itself - containment and minimality of the
rectangle, exact rectangles at known angles, a direct resample of axis-aligned boxes, font-drawn words rotated with PIL - and the
library's host geometry (ocr_plan_word_strips, no GPU) held to the oracle bit for bit.  CPU only; the sampling kernel is held to the
oracle in tests/test_gpu_strips.py."""
import math

import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from tests import glyph_oracle as G
from tests import strip_oracle as S


@pytest.fixture(scope="module", autouse=True)
def _built():
    import os
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()


def _axes(quad):
    """TL, unit U, unit V, |U|, |V| of a quad row (TL, TR, BR, BL)."""
    q = np.asarray(quad, np.float64).reshape(4, 2)
    U, V = q[1] - q[0], q[3] - q[0]
    lu, lv = np.linalg.norm(U), np.linalg.norm(V)
    return q[0], U / lu, V / lv, lu, lv


def _random_polygon(rng, concave):
    k = int(rng.integers(3, 12))
    cx, cy = rng.uniform(300, 700, size=2)
    ang = np.sort(rng.uniform(0, 2 * np.pi, size=k))
    r = rng.uniform(5, 80, size=k) if concave else np.full(k, rng.uniform(5, 80))
    sx, sy = rng.uniform(0.3, 3.0, size=2)
    pts = [(int(round(cx + sx * ri * np.cos(a))), int(round(cy + sy * ri * np.sin(a)))) for ri, a in zip(r, ang)]
    return pts


def _same_plan(got, want):
    assert got.img_offsets.tolist() == want["img_offsets"].tolist()
    assert got.col_offsets.tolist() == want["col_offsets"].tolist()
    assert got.height == want["height"] and got.total_width == want["total_width"]
    assert np.array_equal(got.word_info, want["word_info"])
    assert np.array_equal(got.quads.view(np.uint64), want["quads"].view(np.uint64))
    assert np.array_equal(got.maps.view(np.uint32), want["maps"].view(np.uint32))
    assert np.array_equal(got.scores.view(np.uint64), want["scores"].view(np.uint64))


def _check_c(polys, adj, params=None, h=800, w=800):
    scores = [[0.25 + 0.5 * k for k in range(len(p))] for p in polys]
    want = S.plan(polys, adj, scores, params)
    got = capi.plan_word_strips(polys, adj, h, w, params, scores)
    _same_plan(got, want)
    return want


@pytest.mark.parametrize("concave", [False, True])
def test_rectangle_contains_the_polygon_and_is_minimal(concave):
    rng = np.random.default_rng(7 + concave)
    polys, minimal = [], 0
    for _ in range(150):
        pts = _random_polygon(rng, concave)
        if len(set(pts)) < 3 or len(S.convex_hull(pts)) < 3:
            continue
        polys.append(pts)
        ax, ay = (1.0, 1.0) if len(polys) % 2 else tuple(rng.uniform(0.5, 2.0, size=2))
        C, _, _, flags = S.plan_word(pts, ax, ay, 32, 8192)
        assert flags == 0
        tl, eu, ev, lu, lv = _axes(C)
        P = np.array([(x * ax, y * ay) for x, y in pts])
        s, t = (P - tl) @ eu, (P - tl) @ ev
        tol = 1e-9 * max(1.0, lu, lv)
        assert s.min() >= -tol and s.max() <= lu + tol and t.min() >= -tol and t.max() <= lv + tol
        assert abs(float(eu @ ev)) < 1e-9                          # a rectangle
        th = np.arange(3600) * (np.pi / 3600)                       # bounding rectangles at 3 600 angles over 180 degrees
        d1 = np.stack([np.cos(th), np.sin(th)], 1)
        d2 = np.stack([-np.sin(th), np.cos(th)], 1)
        a1, a2 = P @ d1.T, P @ d2.T
        areas = (a1.max(0) - a1.min(0)) * (a2.max(0) - a2.min(0))
        if min(lu, lv) > 1.0:                                       # (a side under one pixel is widened: larger by design)
            assert lu * lv <= areas.min() * (1 + 1e-9) + 1e-9
            minimal += 1
    assert len(polys) > 100 and minimal > 90
    _check_c([polys], [[1.0, 1.0]])
    _check_c([polys[:40], polys[40:]], [[0.75, 1.25], [1.5, 0.5]])


def test_axis_aligned_rectangle_is_an_axis_aligned_map_and_a_direct_resample():
    rng = np.random.default_rng(3)
    frame = rng.uniform(0, 255, size=(60, 200)).astype(np.float32)
    x0, y0, x1, y1 = 17, 9, 150, 41
    st = S.plan([[[(x0, y0), (x1, y0), (x1, y1), (x0, y1)]]], [[1.0, 1.0]])
    ox, oy, ux, uy, vx, vy = st["maps"][0].tolist()
    ws = st["total_width"]
    assert (ox, oy, uy, vx) == (x0, y0, 0.0, 0.0) and ux > 0 and vy > 0 and st["word_info"][0].tolist() == [0, 0]
    assert ws == math.floor(32 * (x1 - x0) / (y1 - y0) + 0.5)
    atlas = S.extract(frame[None, None], st)
    # the same strip as a plain f64 bilinear resize of the box [x0, x1] x [y0, y1] (pixel centres, edge clamp)
    fx = np.clip(x0 + (np.arange(ws) + 0.5) * (x1 - x0) / ws - 0.5, 0, 199)
    fy = np.clip(y0 + (np.arange(32) + 0.5) * (y1 - y0) / 32 - 0.5, 0, 59)
    ix, iy = np.floor(fx).astype(int), np.floor(fy).astype(int)
    ax_, ay_ = (fx - ix)[None, :], (fy - iy)[:, None]
    f = frame.astype(np.float64)
    ix1, iy1 = np.minimum(ix + 1, 199), np.minimum(iy + 1, 59)
    top = f[iy][:, ix] * (1 - ax_) + f[iy][:, ix1] * ax_
    bot = f[iy1][:, ix] * (1 - ax_) + f[iy1][:, ix1] * ax_
    direct = top * (1 - ay_) + bot * ay_
    assert np.abs(atlas - direct).max() < 1e-3


@pytest.mark.parametrize("deg", list(range(-44, 45, 4)))
def test_rotated_rectangles_give_back_their_corners(deg):
    # an exact integer rectangle at about `deg` degrees (y down: negative angles rise to the right): sides k (p, q) and l (-q, p)
    p, q = 100, int(round(100 * math.tan(math.radians(deg))))
    k, l = 3, 1
    tl = (300, 300)
    corners = [tl, (tl[0] + k * p, tl[1] + k * q), (tl[0] + k * p - l * q, tl[1] + k * q + l * p), (tl[0] - l * q, tl[1] + l * p)]
    for order in (corners, corners[::-1], corners[2:] + corners[:2]):
        C, mp, ws, flags = S.plan_word(order, 1.0, 1.0, 32, 1024)
        assert flags == 0
        assert np.abs(np.asarray(C) - np.asarray(corners, np.float64)).max() < 1e-9
        assert mp[2] > 0
        lu, lv = k * math.hypot(p, q), l * math.hypot(p, q)
        assert ws == math.floor(32 * lu / lv + 0.5) == 96
    _check_c([[corners, corners[::-1]]], [[1.0, 1.0]])
    _check_c([[corners]], [[0.5, 0.5]], dict(strip_height=8, max_width=5))


def test_45_degree_tie_points_up_and_steep_words_turn():
    # long side along (1, -1): both directions have x = 10; the one pointing up wins, the strip runs along the long side
    C, _, ws, _ = S.plan_word([(0, 10), (10, 0), (15, 5), (5, 15)], 1.0, 1.0, 32, 1024)
    assert [tuple(c) for c in C] == [(0.0, 10.0), (10.0, 0.0), (15.0, 5.0), (5.0, 15.0)] and ws == 64
    # long side along (1, 1): the up direction still wins, so this word comes out turned
    C, _, ws, _ = S.plan_word([(0, 5), (5, 0), (15, 10), (10, 15)], 1.0, 1.0, 32, 1024)
    assert [tuple(c) for c in C] == [(0.0, 5.0), (5.0, 0.0), (15.0, 10.0), (10.0, 15.0)] and ws == 16
    # a vertical word (90 degrees) reads along +x: turned by 90 degrees
    C, mp, ws, _ = S.plan_word([(10, 0), (20, 0), (20, 100), (10, 100)], 1.0, 1.0, 32, 1024)
    assert [tuple(c) for c in C] == [(10.0, 0.0), (20.0, 0.0), (20.0, 100.0), (10.0, 100.0)] and ws == 3 and mp[3] == 0
    # upside down (the polygon listed from its bottom right) is not detected: the same strip as upright
    up = S.plan_word([(0, 0), (40, 0), (40, 10), (0, 10)], 1.0, 1.0, 32, 1024)
    down = S.plan_word([(40, 10), (0, 10), (0, 0), (40, 0)], 1.0, 1.0, 32, 1024)
    assert up[0] == down[0]
    _check_c([[[(0, 10), (10, 0), (15, 5), (5, 15)], [(0, 5), (5, 0), (15, 10), (10, 15)], [(10, 0), (20, 0), (20, 100), (10, 100)]]],
             [[1.0, 1.0]])


def test_degenerate_polygons_are_widened_and_flagged():
    C, mp, ws, flags = S.plan_word([(7, 9)], 1.0, 1.0, 32, 1024)            # one point: a 1 x 1 square about it
    assert flags == S.DEGENERATE and ws == 32 and [tuple(c) for c in C] == [(6.5, 8.5), (7.5, 8.5), (7.5, 9.5), (6.5, 9.5)]
    assert S.plan_word([(7, 9)] * 5, 1.0, 1.0, 32, 1024)[0] == C          # repeated copies of one point
    C, mp, ws, flags = S.plan_word([(0, 5), (20, 5)], 1.0, 1.0, 32, 1024)   # two points: the segment, one pixel thick
    assert flags == S.DEGENERATE and ws == 640 and [tuple(c) for c in C] == [(0.0, 4.5), (20.0, 4.5), (20.0, 5.5), (0.0, 5.5)]
    assert S.plan_word([(20, 5), (10, 5), (0, 5), (5, 5)], 1.0, 1.0, 32, 1024)[0] == C   # collinear
    C, _, ws, flags = S.plan_word([(0, 0), (30, 10), (60, 20)], 1.0, 1.0, 32, 1024)   # collinear, slanted: 63 x 1, squeezed
    assert flags == S.DEGENERATE | S.SQUEEZED and ws == 1024
    tl, eu, ev, lu, lv = _axes(C)
    assert abs(lv - 1.0) < 1e-12 and abs(lu - math.hypot(60, 20)) < 1e-12 and abs(eu[0] * 20 - eu[1] * 60) < 1e-12
    # repeated vertices of a real polygon change nothing
    quad = [(3, 3), (40, 5), (39, 20), (2, 18)]
    a, b = S.plan_word(quad + quad[:2], 1.0, 1.0, 32, 1024), S.plan_word(quad, 1.0, 1.0, 32, 1024)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:] and a[3] == 0
    _check_c([[[(7, 9)], [(7, 9)] * 5, [(0, 5), (20, 5)], [(20, 5), (10, 5), (0, 5), (5, 5)], [(0, 0), (30, 10), (60, 20)], quad + quad[:2],
               [(0, 0), (0, 1)], [(5, 5), (6, 6)]]], [[1.0, 1.0]])
    _check_c([[[(7, 9)], [(0, 5), (20, 5)]]], [[0.3, 2.7]])


def test_coordinate_limit_and_squeezing():
    lim = (1 << 24) - 1
    S.plan_word([(lim, lim), (lim - 5, lim)], 1.0, 1.0, 32, 1024)
    _check_c([[[(lim, lim), (lim - 50, lim - 3), (0, 0)]]], [[1.0, 1.0]])
    for bad in ([(1 << 24, 0)], [(0, 1 << 24)]):
        with pytest.raises(ValueError):
            S.plan_word(bad, 1.0, 1.0, 32, 1024)
        with pytest.raises(capi.OcrError) as e:
            capi.plan_word_strips([[bad]], [[1.0, 1.0]], 100, 100)
        assert e.value.code == 1 and "2^24" in str(e.value)
    C, mp, ws, flags = S.plan_word([(0, 0), (5000, 0), (5000, 10), (0, 10)], 1.0, 1.0, 32, 1024)
    assert flags == S.SQUEEZED and ws == 1024 and mp[2] == np.float32(5000 / 1024)
    st = _check_c([[[(0, 0), (5000, 0), (5000, 10), (0, 10)], [(0, 0), (8, 0), (8, 10)], [(1, 1)]]], [[1.0, 1.0]], dict(max_width=20))
    assert st["word_info"][:, 1].tolist() == [1, 1, 2 | 1] and st["col_offsets"].tolist() == [0, 20, 40, 60]


def test_batch_layout_empty_lists_and_scores():
    polys = [[[(0, 0), (40, 0), (40, 10), (0, 10)]], [], [[(5, 5), (9, 5), (9, 20)], [(1, 1), (3, 2)]]]
    st = _check_c(polys, [[1.0, 1.0], [2.0, 2.0], [0.5, 1.5]])
    assert st["img_offsets"].tolist() == [0, 1, 1, 3] and st["word_info"][:, 0].tolist() == [0, 2, 2]
    empty = _check_c([[], []], [[1.0, 1.0]] * 2)
    assert empty["total_width"] == 0 and empty["col_offsets"].tolist() == [0] and S.extract(np.zeros((2, 1, 4, 4), np.float32), empty).shape == (32, 0)
    assert capi.plan_word_strips([[], []], [[1.0, 1.0]] * 2, 10, 10).polygons() == ([[]], [[]])
    got = capi.plan_word_strips(polys, [[1.0, 1.0], [2.0, 2.0], [0.5, 1.5]], 64, 64, scores=[[0.9], [], [0.1, 0.2]])
    rect, sc = got.polygons()
    assert rect == S.strip_polygons(S.plan(polys, [[1.0, 1.0], [2.0, 2.0], [0.5, 1.5]])) and sc == [[0.9, 0.1, 0.2]]


def test_plan_rejects_invalid_arguments():
    import ctypes as C
    L = capi.lib()
    polys = [[[(0, 0), (40, 0), (40, 10), (0, 10)]]]
    st, keep = capi.python_to_polygons(polys, [[0.0]])
    adj = np.ones((1, 2))
    out = C.POINTER(capi.Strips)()

    def plan(*, p=C.byref(st), a=adj.ctypes.data_as(C.POINTER(C.c_double)), n=1, h=20, w=30, prm=None, o=C.byref(out)):
        return L.ocr_plan_word_strips(p, a, n, h, w, prm, o)
    for kw in (dict(p=None), dict(a=None), dict(o=None), dict(n=2), dict(n=0), dict(h=0), dict(w=-1)):
        assert plan(**kw) == 1, kw
        assert L.ocr_last_error()
    for bp in (dict(strip_height=7), dict(strip_height=129), dict(max_width=0), dict(max_width=8193), dict(reserved=(1, 0)),
               dict(reserved=(0, -1))):
        assert plan(prm=C.byref(capi.strip_params(**bp))) == 1, bp
    for bad_adj in ([[0.0, 1.0]], [[1.0, -1.0]], [[np.nan, 1.0]], [[1.0, np.inf]]):
        with pytest.raises(capi.OcrError):
            capi.plan_word_strips(polys, bad_adj, 20, 30)
    with pytest.raises(capi.OcrError):
        capi.plan_word_strips([[[]]], [[1.0, 1.0]], 20, 30)                   # a polygon without vertices
    with pytest.raises(capi.OcrError) as e:                                   # 32 rows x 2^26 columns = 2^31 elements + 1 word
        capi.plan_word_strips([[[(0, 0), (8191 * 4, 0), (8191 * 4, 4), (0, 4)]] * 8193], [[1.0, 1.0]], 20, 30,
                              dict(max_width=8192, strip_height=32))
    assert e.value.code == 1 and "2^31" in str(e.value)
    assert plan() == 0
    L.ocr_word_strips_free(out)
    assert capi.plan_word_strips(polys, adj, 20, 30, dict(strip_height=8, max_width=1)).total_width == 1


def test_reference_pages_ground_truth_polygons(golden_dir):
    from tests.test_gpu_glyphs import load_pages
    _, polys, adj, words = load_pages(golden_dir)
    for params in (None, dict(strip_height=48), dict(strip_height=8, max_width=16)):
        st = _check_c(polys, adj, params)
        assert len(st["word_info"]) == sum(len(w_) for w_ in words) and not (st["word_info"][:, 1] & S.DEGENERATE).any()


def rotated_word(word, angle, dark=True):
    """`word` drawn with draw_word on a 320 x 240 frame, rotated by PIL by `angle` degrees (counter-clockwise on screen) about the frame's
    centre, bilinear -> (H x W f32 frame, the rotated word box as a rounded integer quadrilateral, the upright frame, its word box)."""
    from PIL import Image
    from tests.test_glyph_oracle import draw_word
    img, bbs, _ = draw_word(word, dark, x=40, y=95, size=(320, 240))
    box = (35, 90, bbs[-1][2] + 5, 133)
    cx, cy = 160.0, 120.0
    im = Image.fromarray(img.astype(np.uint8)).rotate(angle, resample=Image.BILINEAR, center=(cx, cy), fillcolor=255 if dark else 0)
    t = math.radians(angle)

    def f(x, y):
        return (int(round(cx + (x - cx) * math.cos(t) + (y - cy) * math.sin(t))), int(round(cy - (x - cx) * math.sin(t) + (y - cy) * math.cos(t))))
    quad = [f(box[0], box[1]), f(box[2], box[1]), f(box[2], box[3]), f(box[0], box[3])]
    return np.asarray(im, np.float32), quad, img, box


def _rectified_count(frame, quad):
    st = S.plan([[quad]], [[1.0, 1.0]])
    atlas = S.extract(frame[None, None], st)
    return int(G.segment(atlas[None, None], S.strip_polygons(st), [[1.0, 1.0]])["word_offsets"][-1])


def test_rotation_matches_pil():
    """rotated_word's quadrilateral is where PIL put the word: the word's ink lies inside it."""
    frame, quad, _, _ = rotated_word("HOUSE", 20)
    ys, xs = np.nonzero(frame < 64)
    C, _, _, _ = S.plan_word(quad, 1.0, 1.0, 32, 1024)
    tl, eu, ev, lu, lv = _axes(C)
    P = np.stack([xs + 0.5, ys + 0.5], 1)
    s, t = (P - tl) @ eu, (P - tl) @ ev
    assert s.min() > 0 and s.max() < lu and t.min() > 0 and t.max() < lv


@pytest.mark.parametrize("dark", [True, False])
def test_rotated_words_read_like_upright_words(dark):
    from tests.test_glyph_oracle import PIL_WORDS
    differs = []
    for word in PIL_WORDS:
        _, _, upright, box = rotated_word(word, 0, dark)
        n_up = int(G.segment(upright[None, None], [[[box[:2], (box[2] - 1, box[3] - 1)]]], [[1.0, 1.0]])["word_offsets"][-1])
        assert n_up == len(word)
        for angle in (-20, -10, 10, 20):
            frame, quad, _, _ = rotated_word(word, angle, dark)
            assert _rectified_count(frame, quad) == n_up, (word, angle)
            n_axis = int(G.segment(frame[None, None], [[quad]], [[1.0, 1.0]])["word_offsets"][-1])
            differs.append(n_axis != n_up)
            _check_c([[quad]], [[1.0, 1.0]])
    assert any(differs)      # the axis-aligned box of a rotated word does not always read the same


@pytest.mark.parametrize("angle", [-44, -40, -35, -30, -25, 25, 30, 35, 40, 44])
def test_rotated_words_beyond_20_degrees(angle):
    """Measured: every PIL word, both polarities, still splits into one glyph per character up to 44 degrees either way."""
    from tests.test_glyph_oracle import PIL_WORDS
    for word in PIL_WORDS:
        for dark in (True, False):
            frame, quad, _, _ = rotated_word(word, angle, dark)
            assert _rectified_count(frame, quad) == len(word), (word, angle, dark)


def test_words_steeper_than_45_degrees_come_out_turned():
    frame, quad, _, _ = rotated_word("Istanbul", 46)
    st = S.plan([[quad]], [[1.0, 1.0]])
    assert st["total_width"] < st["height"]          # the strip runs across the word
    assert _rectified_count(frame, quad) < len("Istanbul")
