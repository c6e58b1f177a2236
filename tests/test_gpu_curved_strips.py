"""Curved strips on the MI355X (ocr_extract_curved_strips, csrc/curved_strips.hip): the atlas equals tests/curved_strip_oracle.py bit
for bit from host and from device memory (one word, strips narrower and wider than a workgroup's 256 columns, 64 words over two
frames, normals that leave the frame, strip heights 8 and 128), into an atlas filled with NaN beforehand; eleven radial bars in a 20
degree sector come out as eleven upright glyphs where the straight strip merges them; read_words_rectified(curved=True) equals the
calls composed by hand and curved=None is the straight path; every OCR_ERR_INVALID case leaves the handle usable."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import curved_strip_oracle as CS
from tests import glyph_oracle as G
from tests import strip_oracle as S
from tests.test_curved_strip_oracle import sector

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    yield d
    d.close()


def _bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _atlas(det, frames, strips, device):
    """ocr_extract_curved_strips into an atlas that holds NaN everywhere beforehand."""
    from ocr_rs_amd import capi
    frames = np.ascontiguousarray(frames, np.float32)
    n, _, h, w = frames.shape
    if device:
        import torch
        x = torch.from_numpy(frames).cuda()
        out = torch.full((strips.height, strips.total_width), float("nan"), device="cuda")
        torch.cuda.synchronize()
        det.extract_curved_strips_device(x.data_ptr(), n, h, w, strips, out.data_ptr())
        return out.cpu().numpy()
    out = np.full((strips.height, strips.total_width), np.nan, np.float32)
    blk = strips.block()
    capi.check(capi.lib().ocr_extract_curved_strips(det._h, frames.ctypes.data, n, h, w, capi.MEM_HOST, C.byref(blk),
                                                    out.ctypes.data if out.size else None))
    return out


def _check(det, frames, polys, adj, params=None, devices=(False, True)):
    """plan + atlas through the C ABI against the oracle; returns (oracle strips, oracle atlas, CurvedStrips)."""
    from tests.test_curved_strip_oracle import same_plan
    n, _, h, w = frames.shape
    want = CS.plan(polys, adj, None, params)
    got = det.plan_curved_strips(polys, adj, h, w, params)
    same_plan(got, want)
    atlas = CS.extract(frames, want)
    assert not np.isnan(atlas).any()
    for device in devices:
        _bits(_atlas(det, frames, got, device), atlas)
    return want, atlas, got


def _noise(n, h, w, seed):
    return np.random.default_rng(seed).uniform(0, 255, size=(n, 1, h, w)).astype(np.float32)


def test_one_word_narrower_than_a_workgroup(det):
    want, _, _ = _check(det, _noise(1, 256, 256, 1), [[sector(128, 215, 170, 12, 20)]], [[1.0, 1.0]])
    assert 0 < want["total_width"] < 256 and want["word_info"][0].tolist() == [0, 0]


def test_one_word_wider_than_a_workgroup(det):
    want, _, _ = _check(det, _noise(1, 256, 256, 2), [[sector(128, 230, 170, 12, 80)]], [[1.0, 1.0]])
    assert want["total_width"] > 256 and want["word_info"][0].tolist() == [0, 0]


def _many_words(seed):
    rng = np.random.default_rng(seed)
    polys = []
    for _ in range(2):
        plist = []
        for _ in range(32):
            radius, half = rng.uniform(40, 120), rng.uniform(4, 9)
            turn = rng.uniform(15, 70)
            span = radius * math.sin(math.radians(turn) / 2) + 20
            cx, cy = rng.uniform(span, 256 - span), rng.uniform(60, 196)
            smile = bool(rng.integers(2))
            plist.append(sector(cx, cy + (-radius if smile else radius), radius, half, turn, smile, rng.uniform(-30, 30)))
        polys.append([[(max(x, 0), max(y, 0)) for x, y in p] for p in plist])
    return polys


def test_64_words_over_two_frames(det):
    polys = _many_words(5)
    want, _, _ = _check(det, _noise(2, 256, 256, 3), polys, [[1.0, 1.0], [1.0, 1.0]])
    assert len(want["word_info"]) == 64 and want["total_width"] % 256 != 0 and want["total_width"] > 2048
    assert want["word_info"][:, 0].tolist() == [0] * 32 + [1] * 32 and not (want["word_info"][:, 1] & CS.STRAIGHT).any()
    _check(det, _noise(2, 200, 230, 4), polys, [[0.9, 0.78], [0.85, 0.7]], dict(strip_height=24, max_width=100, valid_pct=60))


def test_normals_that_leave_the_frame_are_clamped(det):
    # arcs over the top left corner, the right edge and wholly outside a 64 x 96 frame
    polys = [[sector(10, 100, 100, 12, 40), sector(96, 200, 170, 12, 30), sector(400, 500, 170, 12, 20), [(0, 0)], [(95, 63)]]]
    polys = [[[(max(x, 0), max(y, 0)) for x, y in p] for p in polys[0]]]
    frames = _noise(1, 64, 96, 6)
    want, atlas, _ = _check(det, frames, polys, [[1.0, 1.0]])
    kn = want["knots"][0]
    ends = np.concatenate([kn[:, :2] - 16 * kn[:, 2:], kn[:, :2] + 16 * kn[:, 2:]])
    assert ends[:, 1].min() < 0 and want["knots"][1][:, 0].max() > 96            # the normals do reach outside
    c2 = want["col_offsets"][2:4]
    assert (atlas[:, c2[0]:c2[1]] == frames[0, 0, 63, 95]).all()                  # wholly outside: the corner pixel


@pytest.mark.parametrize("hs", [8, 128])
def test_strip_heights_8_and_128(det, hs):
    polys = [[sector(128, 215, 170, 12, 20), sector(128, 40, 170, 12, 40, True), [(5, 5), (60, 9), (58, 30), (3, 25)]]]
    want, _, _ = _check(det, _noise(1, 256, 256, 7), polys, [[1.0, 1.0]], dict(strip_height=hs, max_width=8192))
    assert want["height"] == hs


def test_empty_polygon_list(det):
    frames = np.zeros((2, 1, 16, 16), np.float32)
    want, atlas, got = _check(det, frames, [[], []], [[1.0, 1.0]] * 2)
    assert got.total_width == 0 and got.img_offsets.tolist() == [0, 0, 0] and atlas.shape == (32, 0)


BAR_STEP_DEG = 1.7


def bars_frame(h=256, w=256, cx=128.0, cy=215.0, radius=170.0, half=12.0, bar=3.2, n_bars=11, ss=4):
    """Eleven dark radial bars, 3.2 px wide at the centreline and BAR_STEP_DEG apart, across a sector of radius 170 and half thickness
    12 (the bars stop a pixel inside it), on white; 4 x 4 supersampled."""
    ys, xs = np.mgrid[0:h * ss, 0:w * ss]
    x, y = (xs + 0.5) / ss - cx, (ys + 0.5) / ss - cy
    r, phi = np.hypot(x, y), np.arctan2(x, -y)
    ink = np.zeros(r.shape, bool)
    for k in range(n_bars):
        pk = math.radians((k - (n_bars - 1) / 2) * BAR_STEP_DEG)
        ink |= (np.abs(radius * (phi - pk)) < bar / 2) & (np.abs(r - radius) < half - 1.0)
    cov = ink.reshape(h, ss, w, ss).mean((1, 3))
    return (255.0 * (1 - cov)).astype(np.float32)[None, None]


def test_radial_bars_come_out_as_eleven_upright_glyphs(det):
    """The functional fixture: through the curved atlas ocr_segment_glyphs finds the eleven bars, none wider than twice the middle one;
    through the straight strip of the same polygon the slanted end bars share columns and it finds fewer (five: both oracles agree)."""
    frames = bars_frame()
    polys = [[sector(128, 215, 170, 12, 20)]]
    adj = [[1.0, 1.0]]
    want, atlas, got = _check(det, frames, polys, adj)
    rects, _ = got.polygons()
    assert rects == CS.strip_polygons(want)
    gs = det.segment_glyphs(atlas[None, None], rects, adj)
    seg = G.segment(atlas[None, None], rects, adj)
    assert gs.word_offsets.tolist() == seg["word_offsets"].tolist() and np.array_equal(gs.boxes, seg["boxes"])
    widths = (gs.boxes[:, 2] - gs.boxes[:, 0]).tolist()
    print("\ncurved glyph widths", widths)
    assert len(widths) == 11 and max(widths) <= 2 * widths[5]
    straight = det.plan_word_strips(polys, adj, 256, 256)
    satlas = det.extract_word_strips(frames, straight)
    _bits(satlas, S.extract(frames, S.plan(polys, adj)))
    srects, _ = straight.polygons()
    sgs = det.segment_glyphs(satlas[None, None], srects, adj)
    print("straight glyph widths", (sgs.boxes[:, 2] - sgs.boxes[:, 0]).tolist())
    assert sgs.n_glyphs < 11
    assert sgs.n_glyphs == int(G.segment(satlas[None, None], srects, adj)["word_offsets"][-1])


def test_glyph_quads_of_the_whole_strip_are_the_words_end_points(det):
    from ocr_rs_amd import reading
    polys = [[sector(128, 215, 170, 12, 20), sector(128, 40, 170, 12, 40, True)]]
    got = det.plan_curved_strips(polys, [[1.0, 1.0]], 256, 256, dict(strip_height=48))
    co = got.col_offsets
    boxes = np.array([[co[0], 0, co[1], 48], [co[1], 0, co[2], 48]])
    q = reading.curved_glyph_quads(got, np.array([0, 1]), boxes)
    kn = got.knots.astype(np.float64)
    for k in range(2):
        p0, n0, p1, n1 = kn[k, 0, :2], kn[k, 0, 2:], kn[k, 32, :2], kn[k, 32, 2:]
        assert np.array_equal(q[k], np.array([p0 - 24.0 * n0, p1 - 24.0 * n1, p1 + 24.0 * n1, p0 + 24.0 * n0]))
    want = CS.plan(polys, [[1.0, 1.0]], None, dict(strip_height=48))
    inner = np.array([[3, 4, 9, 40], [co[1] + 7, 1, co[1] + 30, 47]])
    qi = reading.curved_glyph_quads(got, np.array([0, 1]), inner)
    assert np.array_equal(qi, np.concatenate([CS.glyph_quads(want, k, inner[k:k + 1]) for k in range(2)]))


def test_read_words_rectified_curved(det):
    import torch

    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    from ocr_rs_amd.char_recognition import VALUES
    rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    try:
        frames = np.concatenate([bars_frame(), bars_frame(cy=225.0)])
        polys = [[sector(128, 215, 170, 12, 20)], [sector(128, 225, 170, 12, 20), [(20, 20), (90, 30), (88, 44), (18, 34)]]]
        adj = [[1.0, 1.0]] * 2

        def by_hand(O, plan_params):
            want = O.plan(polys, adj, None, plan_params)
            atlas = O.extract(frames, want)[None, None]
            rects = O.strip_polygons(want)
            seg = G.segment(atlas, rects, [[1.0, 1.0]])
            labels, probs = rec.classify_host(G.glyph_crops(atlas, seg))
            pages = []
            for b in range(2):
                page = []
                for word in range(int(want["img_offsets"][b]), int(want["img_offsets"][b + 1])):
                    g0, g1 = int(seg["word_offsets"][word]), int(seg["word_offsets"][word + 1])
                    page.append(("".join(VALUES[int(c)] for c in labels[g0:g1]), probs[g0:g1], O.glyph_quads(want, word, seg["boxes"][g0:g1])))
                pages.append(page)
            return pages

        def same(got, want):
            assert [len(p) for p in got] == [len(p) for p in want]
            for pg, pw in zip(got, want):
                for (t, p, q), (tw, pw_, qw) in zip(pg, pw):
                    assert t == tw and np.array_equal(p, pw_) and np.array_equal(q, qw)
        for curved, cp in ((True, None), ({}, None), (dict(valid_pct=60, strip_height=48), dict(valid_pct=60, strip_height=48))):
            got = reading.read_words_rectified(det, rec, frames, polys, adj, curved=curved)
            same(got, by_hand(CS, cp))
            assert len(got[0][0][0]) == 11
        same(reading.read_words_rectified(det, rec, torch.from_numpy(frames).cuda(), polys, adj, curved=True), by_hand(CS, None))
        same(reading.read_words_rectified(det, rec, frames, polys, adj, dict(strip_height=48), curved=True), by_hand(CS, dict(strip_height=48)))
        # curved=None and False: the straight path, bit for bit what it gave before
        for curved in (None, False):
            same(reading.read_words_rectified(det, rec, frames, polys, adj, curved=curved), by_hand(S, None))
        same(reading.read_words_rectified(det, rec, frames, polys, adj), by_hand(S, None))
        assert reading.read_words_rectified(det, rec, np.zeros((2, 1, 8, 8), np.float32), [[], []], adj, curved=True) == [[], []]
    finally:
        rec.close()


def test_invalid_arguments_leave_the_handle_usable(det):
    from ocr_rs_amd import capi
    L = capi.lib()
    frames = _noise(1, 64, 96, 8)
    polys = [[sector(48, 200, 170, 12, 20)]]
    adj = [[1.0, 1.0]]
    st = det.plan_curved_strips(polys, adj, 64, 96)
    blk = st.block()
    atlas = np.empty((st.height, st.total_width), np.float32)
    straight = det.plan_word_strips(polys, adj, 64, 96)

    def ext(*, d=det._h, f=frames.ctypes.data, n=1, h=64, w=96, mk=capi.MEM_HOST, s=C.byref(blk), a=atlas.ctypes.data):
        return L.ocr_extract_curved_strips(d, f, n, h, w, mk, s, a)

    def ok():
        _bits(_atlas(det, frames, st, False), CS.extract(frames, CS.plan(polys, adj)))
        _bits(det.extract_word_strips(frames, straight), S.extract(frames, S.plan(polys, adj)))

    ok()
    for kw in (dict(d=None), dict(f=None), dict(s=None), dict(a=None), dict(mk=2), dict(mk=-1), dict(n=2), dict(n=0), dict(h=0), dict(w=-3)):
        assert ext(**kw) == 1, kw
        assert L.ocr_last_error()
        ok()

    def bad(**change):
        v = dict(img_offsets=st.img_offsets, col_offsets=st.col_offsets, word_info=st.word_info, knots=st.knots, tscale=st.tscale,
                 half_heights=st.half_heights, lengths=st.lengths, scores=st.scores, height=st.height)
        v.update(change)
        return capi.CurvedStrips(**v)
    for b in (bad(word_info=np.array([[1, 0]])), bad(word_info=np.array([[-1, 0]])), bad(col_offsets=np.array([0, 0])),
              bad(col_offsets=np.array([1, st.total_width])), bad(height=7), bad(height=129), bad(img_offsets=np.array([0, 1, 1])),
              bad(tscale=np.array([-1.0])), bad(tscale=np.array([np.nan])), bad(tscale=np.array([0.0])), bad(tscale=np.array([np.inf]))):
        with pytest.raises(capi.OcrError) as e:
            det.extract_curved_strips(frames, b)
        assert e.value.code == 1
        ok()
    # an atlas of more than 2^31 elements: refused before anything is read
    huge = capi.CurvedStripsBlock(1, 1, 128, (1 << 24) + 1, blk.img_offsets, blk.col_offsets, blk.word_info, blk.knots, blk.tscale,
                                  blk.half_heights, blk.lengths, blk.scores)
    assert ext(s=C.byref(huge)) == 1 and "2^31" in L.ocr_last_error().decode()
    ok()
    out = C.POINTER(capi.Polygons)()
    assert L.ocr_curved_strip_polygons(None, C.byref(out)) == 1 and L.ocr_curved_strip_polygons(C.byref(blk), None) == 1
    assert L.ocr_curved_strip_polygons(C.byref(huge), C.byref(out)) == 1
    prm = capi.curve_params(valid_pct=0)
    pst, keep = capi.python_to_polygons(polys, [[0.0]])
    a = np.ones((1, 2))
    o2 = C.POINTER(capi.CurvedStripsBlock)()
    assert L.ocr_plan_curved_strips(C.byref(pst), a.ctypes.data_as(C.POINTER(C.c_double)), 1, 64, 96, C.byref(prm), C.byref(o2)) == 1
    ok()
