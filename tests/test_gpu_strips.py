"""Word strips on the MI355X (ocr_extract_word_strips, csrc/strips.hip): the atlas equals tests/strip_oracle.py bit for bit on the
reference pages with their ground-truth polygons, rotated font-drawn words, polygons that leave the frame, a 32-page batch, squeezed
words and an empty list; the atlas composes with ocr_segment_glyphs / ocr_extract_glyph_crops unchanged; read_words_rectified equals
the recogniser on the oracle crops; every OCR_ERR_INVALID case leaves the handle usable."""
import ctypes as C

import numpy as np
import pytest

from tests import glyph_oracle as G
from tests import strip_oracle as S

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
    if not device:
        return det.extract_word_strips(frames, strips)
    import torch
    x = torch.from_numpy(np.ascontiguousarray(frames, np.float32)).cuda()
    n, _, h, w = frames.shape
    out = torch.full((strips.height, strips.total_width), float("nan"), device="cuda")
    torch.cuda.synchronize()
    det.extract_word_strips_device(x.data_ptr(), n, h, w, strips, out.data_ptr())
    return out.cpu().numpy()


def _check(det, frames, polys, adj, params=None, device=False):
    """plan + atlas through the C ABI against the oracle; returns (oracle strips, oracle atlas, WordStrips)."""
    n, _, h, w = frames.shape
    want = S.plan(polys, adj, None, params)
    got = det.plan_word_strips(polys, adj, h, w, params)
    assert got.col_offsets.tolist() == want["col_offsets"].tolist() and np.array_equal(got.maps.view(np.uint32), want["maps"].view(np.uint32))
    assert np.array_equal(got.word_info, want["word_info"]) and np.array_equal(got.quads.view(np.uint64), want["quads"].view(np.uint64))
    atlas = S.extract(frames, want)
    _bits(_atlas(det, frames, got, device), atlas)
    return want, atlas, got


def _pages(golden_dir):
    from tests.test_gpu_glyphs import load_pages
    return load_pages(golden_dir)


@pytest.mark.parametrize("device", [False, True])
def test_reference_pages_equal_the_oracle(det, golden_dir, device):
    frames, polys, adj, _ = _pages(golden_dir)
    want, _, _ = _check(det, frames, polys, adj, device=device)
    assert want["total_width"] > 0
    _check(det, frames, polys, adj, dict(strip_height=128, max_width=8192), device=device)
    _check(det, frames, polys, adj, dict(strip_height=8, max_width=40), device=device)


def _rotated_batch(dark):
    from tests.test_glyph_oracle import PIL_WORDS
    from tests.test_strip_oracle import rotated_word
    frames, polys = [], []
    for word in PIL_WORDS:
        for angle in (-20, -10, 10, 20):
            f, quad, _, _ = rotated_word(word, angle, dark)
            frames.append(f)
            polys.append([quad])
    return np.stack(frames)[:, None], polys


@pytest.mark.parametrize("dark", [True, False])
def test_rotated_font_words_equal_the_oracle(det, dark):
    frames, polys = _rotated_batch(dark)
    for device in (False, True):
        _check(det, frames, polys, [[1.0, 1.0]] * len(polys), device=device)


def test_polygons_leaving_the_frame_and_scaled_frames(det):
    rng = np.random.default_rng(9)
    h, w = 41, 67
    frames = rng.uniform(-30, 290, size=(3, 1, h, w)).astype(np.float32)
    frames[1, 0, ::4, ::3] = np.nan
    frames[2, 0, 1::5, ::2] = np.inf
    polys = [[[(0, 0)], [(w - 1, h - 1)], [(50, 30), (120, 60), (100, 90), (40, 55)], [(w + 500, h + 900), (w + 700, h + 950), (w + 600, h + 990)]],
             [[(0, 0), (w - 1, h - 1)], [(3, 3), (3, 30)], [(10, 2), (60, 20), (55, 35), (5, 17)]],
             [[((1 << 24) - 1, 5)], [(20, 20), (21, 21), (22, 22)], [(30, 5), (66, 40), (60, 40), (25, 10)]]]
    adj = [[1.0, 1.0], [0.6, 1.7], [1e-6, 2.0]]
    for device in (False, True):
        _check(det, frames, polys, adj, device=device)
        _check(det, frames, polys, adj, dict(strip_height=17, max_width=3), device=device)


def _rotated_pages(n, h, w, seed):
    """The synthetic block-word pages of test_gpu_glyphs, plus per page some rotated quadrilaterals."""
    from tests.test_gpu_glyphs import _synthetic_pages
    frames, polys = _synthetic_pages(n, h, w, 100, seed)
    rng = np.random.default_rng(seed)
    for plist in polys:
        for _ in range(10):
            cx, cy = rng.uniform(40, w - 40), rng.uniform(40, h - 40)
            t = rng.uniform(-np.pi / 3, np.pi / 3)
            a, b = rng.uniform(10, 120), rng.uniform(4, 30)
            pts = [(cx + sx * a * np.cos(t) - sy * b * np.sin(t), cy + sx * a * np.sin(t) + sy * b * np.cos(t))
                   for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
            plist.append([(int(round(max(x, 0))), int(round(max(y, 0)))) for x, y in pts])
    return frames, polys


@pytest.mark.parametrize("device", [True, False])
def test_batch_of_32_pages(det, device):
    frames, polys = _rotated_pages(32, 640, 640, seed=21 if device else 22)
    want, _, _ = _check(det, frames, polys, [[1.0, 1.0]] * 32, device=device)
    assert len(want["word_info"]) > 3000 and want["total_width"] > 100_000


def test_squeezed_word(det):
    frames = np.random.default_rng(4).uniform(0, 255, size=(1, 1, 64, 3000)).astype(np.float32)
    polys = [[[(0, 10), (2999, 12), (2999, 30), (0, 28)], [(5, 5), (40, 5), (40, 20), (5, 20)]]]
    for device in (False, True):
        want, _, _ = _check(det, frames, polys, [[1.0, 1.0]], dict(max_width=100), device=device)
        assert want["word_info"][:, 1].tolist() == [S.SQUEEZED, 0] and want["col_offsets"][1] == 100


def test_empty_polygon_list(det):
    frames = np.zeros((2, 1, 16, 16), np.float32)
    for device in (False, True):
        want, atlas, got = _check(det, frames, [[], []], [[1.0, 1.0]] * 2, device=device)
        assert got.total_width == 0 and got.img_offsets.tolist() == [0, 0, 0] and atlas.shape == (32, 0)


def test_atlas_composes_with_glyph_segmentation(det, golden_dir):
    frames, polys, adj, _ = _pages(golden_dir)
    rframes, rpolys = _rotated_batch(True)
    for fr, pl, ad in ((frames, polys, adj), (rframes, rpolys, [[1.0, 1.0]] * len(rpolys))):
        want, atlas, got = _check(det, fr, pl, ad)
        rects, rscores = got.polygons()
        assert rects == S.strip_polygons(want) and len(rscores[0]) == got.n_words
        a = atlas[None, None]
        for params in (None, dict(polarity=1, glyph_box=28)):
            seg = G.segment(a, rects, [[1.0, 1.0]], params)
            assert [G.word_boxes(rects, [[1.0, 1.0]], got.height, got.total_width)[k][1:] for k in range(got.n_words)] == \
                   [(int(got.col_offsets[k]), 0, int(got.col_offsets[k + 1]), got.height) for k in range(got.n_words)]
            gs = det.segment_glyphs(a, rects, [[1.0, 1.0]], params)
            assert gs.word_offsets.tolist() == seg["word_offsets"].tolist() and np.array_equal(gs.boxes, seg["boxes"])
            assert np.array_equal(gs.word_info, seg["word_info"])
            _bits(det.extract_glyph_crops(a, gs, params), G.glyph_crops(a, seg, params))


def test_read_words_rectified(det, golden_dir):
    import torch

    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    try:
        frames, polys, adj, words = _pages(golden_dir)
        for sp in (None, dict(strip_height=48)):
            got = reading.read_words_rectified(det, rec, frames, polys, adj, sp)
            want = S.plan(polys, adj, None, sp)
            atlas = S.extract(frames, want)[None, None]
            rects = S.strip_polygons(want)
            seg = G.segment(atlas, rects, [[1.0, 1.0]])
            labels, probs = rec.classify_host(G.glyph_crops(atlas, seg))
            from ocr_rs_amd.char_recognition import VALUES
            k = 0
            for b, page in enumerate(got):
                assert len(page) == len(polys[b])
                for wi, (text, pr, quads) in enumerate(page):
                    word = int(want["img_offsets"][b]) + wi
                    g0, g1 = int(seg["word_offsets"][word]), int(seg["word_offsets"][word + 1])
                    assert text == "".join(VALUES[int(c)] for c in labels[g0:g1]) and np.array_equal(pr, probs[g0:g1])
                    assert np.array_equal(quads, S.glyph_quads(want, word, seg["boxes"][g0:g1]))
                    k += g1 - g0
            assert k == len(labels) > 0
            again = reading.read_words_rectified(det, rec, torch.from_numpy(frames).cuda(), polys, adj, sp)
            assert [[(t, p.tolist(), q.tolist()) for t, p, q in pg] for pg in again] == [[(t, p.tolist(), q.tolist()) for t, p, q in pg] for pg in got]
        # glyph count == transcription length, rectified against the axis-aligned boxes (measured, not asserted)
        axis = reading.read_words(det, rec, frames, polys, adj)
        rect = reading.read_words_rectified(det, rec, frames, polys, adj)
        pairs = [(words[b][i], len(axis[b][i][0]), len(rect[b][i][0])) for b in range(len(words)) for i in range(len(words[b])) if words[b][i] != "###"]
        print(f"\nglyph count == transcription length on the reference pages: axis-aligned {sum(a == len(w_) for w_, a, _ in pairs)} / {len(pairs)}, "
              f"rectified {sum(r == len(w_) for w_, _, r in pairs)} / {len(pairs)}")
        print("   (word, axis-aligned glyphs, rectified glyphs):", pairs)
        assert reading.read_words_rectified(det, rec, np.zeros((2, 1, 8, 8), np.float32), [[], []], [[1.0, 1.0]] * 2) == [[], []]
    finally:
        rec.close()


def test_invalid_arguments_leave_the_handle_usable(det):
    from ocr_rs_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(2)
    frames = rng.uniform(0, 255, size=(1, 1, 20, 30)).astype(np.float32)
    polys = [[[(2, 2), (25, 5), (24, 17), (1, 14)]]]
    st = det.plan_word_strips(polys, [[1.0, 1.0]], 20, 30)
    blk = st.block()
    atlas = np.empty((st.height, st.total_width), np.float32)

    def ext(*, d=det._h, f=frames.ctypes.data, n=1, h=20, w=30, mk=capi.MEM_HOST, s=C.byref(blk), a=atlas.ctypes.data):
        return L.ocr_extract_word_strips(d, f, n, h, w, mk, s, a)

    def ok():
        _bits(det.extract_word_strips(frames, st), S.extract(frames, S.plan(polys, [[1.0, 1.0]])))

    for kw in (dict(d=None), dict(f=None), dict(s=None), dict(a=None), dict(mk=2), dict(mk=-1), dict(n=2), dict(n=0), dict(h=0), dict(w=-3)):
        assert ext(**kw) == 1, kw
        assert L.ocr_last_error()
        ok()

    def bad(**change):
        v = dict(img_offsets=st.img_offsets, col_offsets=st.col_offsets, word_info=st.word_info, quads=st.quads, maps=st.maps,
                 scores=st.scores, height=st.height)
        v.update(change)
        return capi.WordStrips(**v)
    for b in (bad(word_info=np.array([[1, 0]])), bad(word_info=np.array([[-1, 0]])), bad(col_offsets=np.array([0, 0])),
              bad(col_offsets=np.array([1, st.total_width])), bad(height=7), bad(height=129), bad(img_offsets=np.array([0, 1, 1]))):
        with pytest.raises(capi.OcrError) as e:
            det.extract_word_strips(frames, b)
        assert e.value.code == 1
        ok()
    # an atlas of more than 2^31 elements: refused before anything is read
    huge = capi.Strips(1, 1, 128, (1 << 24) + 1, blk.img_offsets, blk.col_offsets, blk.word_info, blk.quads, blk.maps, blk.scores)
    assert ext(s=C.byref(huge)) == 1 and "2^31" in L.ocr_last_error().decode()
    ok()
    out = C.POINTER(capi.Polygons)()
    assert L.ocr_word_strip_polygons(None, C.byref(out)) == 1 and L.ocr_word_strip_polygons(C.byref(blk), None) == 1
    assert L.ocr_word_strip_polygons(C.byref(huge), C.byref(out)) == 1
    ok()
