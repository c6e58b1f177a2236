"""The curved strip planner (ocr_plan_curved_strips, host code, no GPU) held to tests/curved_strip_oracle.py array for array - the f32
and f64 arrays by bit pattern - and the oracle held to facts that do not come from itself: the half thickness of annular sectors, the
midline of a rectangle, the flags of degenerate, folded and steep shapes.  The sampling kernel is held to the oracle in
tests/test_gpu_curved_strips.py."""
import ctypes as C
import math

import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from tests import curved_strip_oracle as CS
from tests import strip_oracle as S


@pytest.fixture(scope="module", autouse=True)
def _built():
    import os
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()


def sector(cx, cy, radius, half, turn_deg, smile=False, rot_deg=0.0, n=12):
    """An annular sector as a ring of 2 n integer points: n on the outer arc, n on the inner arc back.  The arc's centre is (cx, cy);
    a frown bulges up (y down), a smile bulges down; the ring is turned by rot_deg about the middle of its centreline."""
    th = math.radians(turn_deg)
    phis = [-th / 2 + th * i / (n - 1) for i in range(n)]
    sg = 1.0 if smile else -1.0
    pts = [(cx + (radius + half) * math.sin(p), cy + sg * (radius + half) * math.cos(p)) for p in phis] + \
          [(cx + (radius - half) * math.sin(p), cy + sg * (radius - half) * math.cos(p)) for p in reversed(phis)]
    t = math.radians(rot_deg)
    c, s = math.cos(t), math.sin(t)
    mx, my = cx, cy + sg * radius
    return [(int(round(mx + (x - mx) * c - (y - my) * s)), int(round(my + (x - mx) * s + (y - my) * c))) for x, y in pts]


def same_plan(got, want):
    assert got.img_offsets.tolist() == want["img_offsets"].tolist()
    assert got.col_offsets.tolist() == want["col_offsets"].tolist()
    assert got.height == want["height"] and got.total_width == want["total_width"]
    assert np.array_equal(got.word_info, want["word_info"])
    assert np.array_equal(got.knots.view(np.uint32), want["knots"].view(np.uint32))
    assert np.array_equal(got.tscale.view(np.uint32), want["tscale"].view(np.uint32))
    assert np.array_equal(got.half_heights.view(np.uint64), want["half_heights"].view(np.uint64))
    assert np.array_equal(got.lengths.view(np.uint64), want["lengths"].view(np.uint64))
    assert np.array_equal(got.scores.view(np.uint64), want["scores"].view(np.uint64))


def _check_c(polys, adj, params=None, h=800, w=800):
    scores = [[0.25 + 0.5 * k for k in range(len(p))] for p in polys]
    want = CS.plan(polys, adj, scores, params)
    got = capi.plan_curved_strips(polys, adj, h, w, params, scores)
    same_plan(got, want)
    return want


TURNS = (20, 40, 60)


@pytest.mark.parametrize("rot", [0, 30, 100])
def test_sectors_equal_the_oracle(rot):
    polys = [sector(600, 600, 170, 12, turn, smile, rot) for turn in TURNS for smile in (False, True)]
    st = _check_c([polys], [[1.0, 1.0]])
    assert not (st["word_info"][:, 1] & (CS.DEGENERATE | CS.STRAIGHT | CS.SQUEEZED)).any()
    _check_c([polys[:2], polys[2:]], [[0.75, 1.25], [1.5, 0.5]])
    _check_c([polys], [[1.0, 1.0]], dict(strip_height=8, valid_pct=100))
    _check_c([polys], [[0.37, 0.41]], dict(strip_height=128, max_width=8192, valid_pct=1))


@pytest.mark.parametrize("rot", [0, 30])
@pytest.mark.parametrize("smile", [False, True])
@pytest.mark.parametrize("turn", TURNS)
def test_sector_half_height_is_the_half_thickness(turn, smile, rot):
    """Sectors of half thickness 12: h lies in [11.5, 12.5] (the prototype gave 11.9 - 12.1), the length is the centreline's arc plus the
    end caps' overhang, and no flag is set.  (At 100 degrees the rectangle's reading direction turns by 90 degrees, rule 3 of the
    straight strips, and the strip runs across the word: h is then no thickness.)"""
    kn, tscale, h, length, ws, flags = CS.plan_word(sector(600, 600, 170, 12, turn, smile, rot), 1.0, 1.0, 32, 1024, 80)
    assert 11.5 <= h <= 12.5 and flags == 0
    arc = 170 * math.radians(turn)
    assert arc <= length <= arc + 2 * 12 * math.tan(math.radians(turn) / 2) + 3
    assert ws == math.floor(32 * length / (2 * h) + 0.5) and tscale == np.float32(32.0 / ws)
    # the normals have length 2 h / Hs and stand on the tangent
    n = kn[:, 2:].astype(np.float64)
    assert np.abs(np.hypot(n[:, 0], n[:, 1]) - 2 * h / 32).max() < 1e-5
    tang = kn[2:, :2].astype(np.float64) - kn[:-2, :2]
    assert np.abs((tang * n[1:-1]).sum(1)).max() < 1e-3
    # the knots lie on the circle of radius 170 about the sector's centre, away from the extended ends
    c = np.array([600.0, 600.0])
    mid = np.array([600.0, 600.0 + (170 if smile else -170)])
    t = math.radians(rot)
    centre = mid + np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]]) @ (c - mid)
    r = np.hypot(*(kn[4:-4, :2].astype(np.float64) - centre).T)
    assert np.abs(r - 170).max() < 1.0


def test_rectangle_has_no_flags_and_knots_on_the_midline():
    rect = [(17, 9), (150, 9), (150, 41), (17, 41)]
    kn, tscale, h, length, ws, flags = CS.plan_word(rect, 1.0, 1.0, 32, 1024, 80)
    assert flags == 0 and h == 16.0 and length == 133.0 and ws == 133
    assert kn[:, 1].tolist() == [25.0] * 33 and kn[:, 0].tolist() == [17 + 133 * r / 32 for r in range(33)]
    assert kn[:, 2].tolist() == [0.0] * 33 and kn[:, 3].tolist() == [1.0] * 33
    # rotated: the same up to rounding
    p, q = 100, 36
    corners = [(300, 300), (300 + 3 * p, 300 + 3 * q), (300 + 3 * p - q, 300 + 3 * q + p), (300 - q, 300 + p)]
    kn, _, h, length, ws, flags = CS.plan_word(corners, 1.0, 1.0, 32, 1024, 80)
    lv = math.hypot(p, q)
    assert flags == 0 and abs(h - lv / 2) < 1e-9 and abs(length - 3 * lv) < 1e-9
    mid0 = np.array([300 - q / 2, 300 + p / 2])
    want = mid0[None, :] + np.arange(33)[:, None] / 32 * np.array([3 * p, 3 * q])[None, :]
    assert np.abs(kn[:, :2] - want).max() < 1e-3
    st = _check_c([[rect, corners, corners[::-1]]], [[1.0, 1.0]])
    assert st["word_info"][:, 1].tolist() == [0, 0, 0]
    _check_c([[rect, corners]], [[0.5, 2.0]], dict(strip_height=48))


def test_degenerate_polygons_take_the_straight_fallback():
    polys = [[(7, 9)], [(7, 9)] * 5, [(0, 5), (20, 5)], [(20, 5), (10, 5), (0, 5), (5, 5)], [(0, 0), (30, 10), (60, 20)]]
    st = _check_c([polys], [[1.0, 1.0]])
    assert st["word_info"][:, 1].tolist() == [18, 18, 18, 18, 18 | 1]
    sst = S.plan([polys], [[1.0, 1.0]])
    assert st["col_offsets"].tolist() == sst["col_offsets"].tolist()          # Ws as in the straight rule
    assert st["half_heights"][:4].tolist() == [0.5] * 4 and abs(st["half_heights"][4] - 0.5) < 1e-12      # h = |V| / 2 of the widened side
    assert st["lengths"][:3].tolist() == [1.0, 1.0, 20.0]
    kn = st["knots"][2]                                                       # the segment (0, 5) - (20, 5), one pixel thick
    assert kn[:, 0].tolist() == [20 * r / 32 for r in range(33)] and kn[:, 1].tolist() == [5.0] * 33
    assert kn[:, 2].tolist() == [0.0] * 33 and kn[:, 3].tolist() == [1 / 32] * 33
    _check_c([polys], [[0.3, 2.7]])


def u_shape():
    """A 'U': two prongs of 15 x 60 and a bar of 100 x 20 below them."""
    return [(100, 100), (115, 100), (115, 140), (185, 140), (185, 100), (200, 100), (200, 160), (100, 160)]


def test_folded_and_steep_shapes_are_flagged():
    # upright, the scan lines run along the prongs and cross the ring twice; lying on its side, they cross prong, gap and prong
    side = [(y, x) for x, y in u_shape()]
    st = _check_c([[u_shape(), side, side[::-1]]], [[1.0, 1.0]])
    assert (st["word_info"][:, 1] & CS.FOLDED).tolist() == [0, CS.FOLDED, CS.FOLDED]
    assert not (st["word_info"][:, 1] & CS.STRAIGHT).any()
    wide = sector(600, 600, 170, 12, 120)
    st = _check_c([[wide, sector(600, 600, 170, 12, 120, True, 30)]], [[1.0, 1.0]])
    assert (st["word_info"][:, 1] & CS.STEEP).tolist() == [CS.STEEP] * 2
    for turn in TURNS:
        assert CS.plan_word(sector(600, 600, 170, 12, turn), 1.0, 1.0, 32, 1024, 80)[5] == 0


def test_squeezed_word_and_batch_layout():
    polys = [sector(600, 600, 170, 12, 40), [(0, 0), (8, 0), (8, 10)], [(1, 1)]]
    st = _check_c([polys], [[1.0, 1.0]], dict(max_width=16))
    assert st["word_info"][:, 1].tolist() == [CS.SQUEEZED, CS.SQUEEZED, CS.DEGENERATE | CS.STRAIGHT | CS.SQUEEZED]
    assert CS.plan([polys], [[1.0, 1.0]])["word_info"][:, 1].tolist() == [0, 0, CS.DEGENERATE | CS.STRAIGHT]
    assert st["col_offsets"].tolist()[:2] == [0, 16] and st["tscale"][0] == np.float32(2.0)
    batch = [[sector(300, 300, 170, 12, 20)], [], [sector(300, 300, 170, 12, 60, True), [(1, 1), (3, 2)]]]
    adj = [[1.0, 1.0], [2.0, 2.0], [0.5, 1.5]]
    st = _check_c(batch, adj)
    assert st["img_offsets"].tolist() == [0, 1, 1, 3] and st["word_info"][:, 0].tolist() == [0, 2, 2]
    empty = _check_c([[], []], [[1.0, 1.0]] * 2)
    assert empty["total_width"] == 0 and empty["col_offsets"].tolist() == [0]
    assert CS.extract(np.zeros((2, 1, 4, 4), np.float32), empty).shape == (32, 0)
    assert capi.plan_curved_strips([[], []], [[1.0, 1.0]] * 2, 10, 10).polygons() == ([[]], [[]])
    got = capi.plan_curved_strips(batch, adj, 64, 64, scores=[[0.9], [], [0.1, 0.2]])
    rect, sc = got.polygons()
    assert rect == CS.strip_polygons(CS.plan(batch, adj)) and sc == [[0.9, 0.1, 0.2]]


def test_random_polygons_equal_the_oracle():
    from tests.test_strip_oracle import _random_polygon
    rng = np.random.default_rng(11)
    polys = [_random_polygon(rng, concave) for concave in (False, True) for _ in range(60)]
    st = _check_c([polys[:50], polys[50:]], [[1.0, 1.0], [0.8, 1.3]])
    assert (st["word_info"][:, 1] & CS.STRAIGHT).sum() < len(polys) // 2


def test_plan_rejects_invalid_arguments():
    L = capi.lib()
    polys = [[sector(100, 250, 170, 12, 20)]]
    st, keep = capi.python_to_polygons(polys, [[0.0]])
    adj = np.ones((1, 2))
    out = C.POINTER(capi.CurvedStripsBlock)()

    def plan(*, p=C.byref(st), a=adj.ctypes.data_as(C.POINTER(C.c_double)), n=1, h=256, w=256, prm=None, o=C.byref(out)):
        return L.ocr_plan_curved_strips(p, a, n, h, w, prm, o)
    for kw in (dict(p=None), dict(a=None), dict(o=None), dict(n=2), dict(n=0), dict(h=0), dict(w=-1)):
        assert plan(**kw) == 1, kw
        assert L.ocr_last_error()
    for bp in (dict(strip_height=7), dict(strip_height=129), dict(max_width=0), dict(max_width=8193), dict(valid_pct=0),
               dict(valid_pct=101), dict(reserved=1), dict(reserved=-1)):
        assert plan(prm=C.byref(capi.curve_params(**bp))) == 1, bp
    for bad_adj in ([[0.0, 1.0]], [[1.0, -1.0]], [[np.nan, 1.0]], [[1.0, np.inf]]):
        with pytest.raises(capi.OcrError):
            capi.plan_curved_strips(polys, bad_adj, 256, 256)
    with pytest.raises(capi.OcrError):
        capi.plan_curved_strips([[[]]], [[1.0, 1.0]], 20, 30)                 # a polygon without vertices
    with pytest.raises(capi.OcrError) as e:
        capi.plan_curved_strips([[[(1 << 24, 0)]]], [[1.0, 1.0]], 20, 30)
    assert e.value.code == 1 and "2^24" in str(e.value)
    with pytest.raises(capi.OcrError) as e:                                   # 32 rows x 2^26 columns = 2^31 elements + 1 word
        capi.plan_curved_strips([[[(0, 0), (8191 * 4, 0), (8191 * 4, 4), (0, 4)]] * 8193], [[1.0, 1.0]], 20, 30,
                                dict(max_width=8192, strip_height=32))
    assert e.value.code == 1 and "2^31" in str(e.value)
    # a block whose offsets do not fit
    bad = capi.Polygons(1, 1, st.n_vertices, st.img_offsets, (C.c_int32 * 2)(0, st.n_vertices + 1), st.xy, st.scores)
    assert plan(p=C.byref(bad)) == 1
    bad = capi.Polygons(1, 1, st.n_vertices, (C.c_int32 * 2)(0, 2), st.poly_offsets, st.xy, st.scores)
    assert plan(p=C.byref(bad)) == 1
    assert plan() == 0
    L.ocr_curved_strips_free(out)
    assert capi.plan_curved_strips(polys, adj, 256, 256, dict(strip_height=8, max_width=1)).total_width == 1
    # the straight planner is unchanged by all of it
    from tests.test_strip_oracle import _check_c as straight_check
    straight_check(polys, adj)


def test_glyph_quads_of_the_whole_strip_are_the_words_end_points():
    polys = [[sector(128, 215, 170, 12, 20), sector(128, 40, 170, 12, 40, True)]]
    st = CS.plan(polys, [[1.0, 1.0]])
    for word in range(2):
        c0, c1 = int(st["col_offsets"][word]), int(st["col_offsets"][word + 1])
        q = CS.glyph_quads(st, word, np.array([[c0, 0, c1, 32]]))[0]
        kn = st["knots"][word].astype(np.float64)
        want = [kn[0, :2] - 16 * kn[0, 2:], kn[32, :2] - 16 * kn[32, 2:], kn[32, :2] + 16 * kn[32, 2:], kn[0, :2] + 16 * kn[0, 2:]]
        assert np.array_equal(q, np.array(want))
        # the middle column at the middle row is the middle knot
        mid = CS.glyph_quads(st, word, np.array([[c0, 16, c0, 16]]))[0][0]
        assert np.array_equal(mid, kn[0, :2])
