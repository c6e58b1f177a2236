"""Connected-component glyph segmentation on the MI355X (ocr_segment_glyphs_cc, csrc/glyph_cc.hip): every array of the ocr_glyphs_t
equals tests/glyph_cc_oracle.py bit for bit, from host and from device memory, on the reference pages (axis-aligned and as an atlas),
font words, kerned and dotted constructions, a 32-page batch, serpentines, combs, rings, both fallbacks, the limits themselves, frame
edges and every parameter's ends; the crops, read_words(cc=...) and read_words_rectified(cc=...) compose; every OCR_ERR_INVALID case
leaves the handle usable and the column call is unchanged afterwards."""
import ctypes as C

import numpy as np
import pytest

from tests import glyph_cc_oracle as CC
from tests import glyph_oracle as G
from tests import strip_oracle as S
from tests.test_glyph_cc_oracle import BG, INK, PAGE_WORDS, dotted_i, kerned_pair, lattice_word, noise_word

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    yield d
    d.close()


def _assert_equal_seg(got, want):
    assert got.img_offsets.tolist() == want["img_offsets"].tolist()
    assert got.word_offsets.tolist() == want["word_offsets"].tolist()
    assert np.array_equal(got.word_info, want["word_info"])
    assert np.array_equal(got.word_levels.view(np.uint32), want["word_levels"].view(np.uint32))
    assert np.array_equal(got.boxes, want["boxes"])


def _assert_bits(a, b):
    assert a.shape == b.shape
    assert np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _run(det, frames, polys, adj, params=None, cc=None, device=False):
    """(GlyphSet, crops) through the C ABI, host or device memory."""
    from ocr_rs_amd import capi
    prm = capi.segment_params(**(params or {}))
    ccp = capi.cc_params(**(cc or {}))
    if not device:
        g = det.segment_glyphs(frames, polys, adj, prm, cc=ccp)
        return g, det.extract_glyph_crops(frames, g, prm)
    import torch
    x = torch.from_numpy(np.ascontiguousarray(frames, np.float32)).cuda()
    n, _, h, w = frames.shape
    torch.cuda.synchronize()
    g = det.segment_glyphs_device(x.data_ptr(), n, h, w, polys, adj, prm, cc=ccp)
    crops = torch.full((g.n_glyphs, 784), float("nan"), device="cuda")
    if g.n_glyphs:
        det.extract_glyph_crops_device(x.data_ptr(), n, h, w, g, crops.data_ptr(), prm)
    return g, crops.cpu().numpy()


def _check(det, frames, polys, adj, params=None, cc=None, device=False, stats=None):
    frames = np.ascontiguousarray(frames, np.float32)
    want = CC.segment_cc(frames, polys, adj, params, cc, stats)
    got, crops = _run(det, frames, polys, adj, params, cc, device)
    _assert_equal_seg(got, want)
    _assert_bits(crops, G.glyph_crops(frames, want, params))
    return want


def _both(det, frames, polys, adj, params=None, cc=None, stats=None):
    _check(det, frames, polys, adj, params, cc, device=True)
    return _check(det, frames, polys, adj, params, cc, device=False, stats=stats)


def _whole(img):
    """One frame, one word: the whole frame."""
    h, w = img.shape
    return img[None, None], [[[(0, 0), (w - 1, h - 1)]]], [[1.0, 1.0]]


def _pages(golden_dir):
    from tests.test_gpu_glyphs import load_pages
    return load_pages(golden_dir)


def _atlas(frames, polys, adj, strip_params=None):
    plan = S.plan(polys, adj, None, strip_params)
    return S.extract(frames, plan)[None, None], S.strip_polygons(plan), plan


@pytest.mark.parametrize("device", [False, True])
def test_reference_pages_axis_aligned_and_as_an_atlas(det, golden_dir, device):
    frames, polys, adj, words = _pages(golden_dir)
    want = _check(det, frames, polys, adj, device=device)
    assert want["word_offsets"][-1] > 0 and not want["word_info"][:, 3].any()
    _check(det, frames, polys, adj, dict(polarity=2, ink_high=0, glyph_box=28, min_glyph_pixels=0), dict(min_height_pct=0), device=device)
    _check(det, frames, polys, adj, dict(polarity=1, max_glyphs=2, glyph_box=1), dict(merge_overlap_pct=0), device=device)
    atlas, rects, _ = _atlas(frames, polys, adj)
    want = _check(det, atlas, rects, [[1.0, 1.0]], device=device)
    flat = [w for page in words for w in page]
    assert flat == PAGE_WORDS
    hits = sum(len(w) == c for w, c in zip(flat, np.diff(want["word_offsets"])) if w != "###")
    assert hits > 2                                            # the column rule's count on these strips


@pytest.mark.parametrize("dark", [True, False])
def test_font_words_and_rotated_font_words(det, dark):
    from tests.test_glyph_oracle import PIL_WORDS, draw_word
    from tests.test_gpu_strips import _rotated_batch
    rows = [draw_word(wd, dark, size=(160, 48)) for wd in PIL_WORDS]
    frame = np.concatenate([r[0] for r in rows], axis=0)                # one frame, one word per 48-pixel band
    polys = [[[(5, 48 * k + 5), (r[1][-1][2] + 5, 48 * k + 5), (r[1][-1][2] + 5, 48 * k + 42), (5, 48 * k + 42)] for k, r in enumerate(rows)]]
    want = _both(det, frame[None, None], polys, [[1.0, 1.0]])
    assert np.diff(want["word_offsets"]).tolist() == [len(wd) for wd in PIL_WORDS]
    assert want["word_info"][:, 2].tolist() == [1 if dark else 2] * len(PIL_WORDS)
    rframes, rpolys = _rotated_batch(dark)
    adj = [[1.0, 1.0]] * len(rpolys)
    _both(det, rframes, rpolys, adj)                                    # the rotated words by their axis-aligned boxes
    atlas, rects, _ = _atlas(rframes, rpolys, adj)
    _both(det, atlas, rects, [[1.0, 1.0]])                              # ... and upright, as an atlas


def test_kerned_pair_and_dotted_i(det):
    from ocr_rs_amd import capi
    img, boxes = kerned_pair()
    fr, polys, adj = _whole(img)
    want = _both(det, fr, polys, adj)
    assert want["boxes"].tolist() == [list(b) for b in boxes]
    assert det.segment_glyphs(fr, polys, adj).n_glyphs == 1             # the column rule fuses them
    assert det.segment_glyphs(fr, polys, adj, cc=capi.cc_params()).n_glyphs == det.segment_glyphs(fr, polys, adj, cc={}).n_glyphs == 2
    fr, polys, adj = _whole(dotted_i())
    assert _both(det, fr, polys, adj)["boxes"].tolist() == [[10, 5, 13, 25], [17, 4, 19, 25]]
    assert _both(det, fr, polys, adj, cc=dict(merge_overlap_pct=0))["boxes"].tolist() == [[10, 10, 13, 25], [17, 4, 19, 25]]
    assert len(_both(det, fr, polys, adj, cc=dict(merge_overlap_pct=0, min_height_pct=0))["boxes"]) == 3


@pytest.mark.parametrize("device", [True, False])
def test_batch_of_32_pages(det, device):
    from tests.test_gpu_glyphs import _synthetic_pages
    frames, polys = _synthetic_pages(32, 640, 640, 100, seed=31 if device else 32)
    want = _check(det, frames, polys, [[1.0, 1.0]] * 32, device=device)
    assert len(want["word_info"]) > 3000 and want["word_offsets"][-1] > 5000


def serpentine_rows(h=48, w=1024):
    """One component: full-width lines on rows 1, 4, 7, ... joined at alternating ends."""
    img = np.full((h, w), BG, np.float32)
    rows = list(range(1, h - 1, 3))
    for k, y in enumerate(rows):
        img[y, :] = INK
        if k + 1 < len(rows):
            img[y:y + 3, w - 1 if k % 2 == 0 else 0] = INK
    return img


def serpentine_columns(h=48, w=1024):
    """One component of about 8000 runs: 170 vertical lines six columns apart, joined at alternating ends - the long union chain."""
    img = np.full((h, w), BG, np.float32)
    xs = [1 + 6 * k for k in range(170)]
    for k, x in enumerate(xs):
        img[1:h - 1, x] = INK
        if k + 1 < len(xs):
            img[h - 1 if k % 2 == 0 else 0, x:xs[k + 1] + 1] = INK
    return img


def test_serpentines_stay_one_component(det):
    for img in (serpentine_rows(), serpentine_columns(), serpentine_columns()[::-1].copy(), serpentine_columns()[:, ::-1].copy()):
        fr, polys, adj = _whole(img)
        st = []
        want = _both(det, fr, polys, adj, stats=st)
        assert st[0]["components"] == 1 and st[0]["runs"] <= CC.MAX_RUNS and want["word_info"][0, 3] == 0
        assert len(want["boxes"]) == 1 and want["boxes"][0, 2] - want["boxes"][0, 0] >= 1015
    assert st[0]["runs"] > 7900
    # a serpentine inside a larger frame, the box off the 64-column grid
    frame = np.full((60, 1100), BG, np.float32)
    frame[7:55, 37:1061] = serpentine_columns()
    _both(det, frame[None, None], [[[(37, 7), (1060, 54)]]], [[1.0, 1.0]])


def comb(h=40, w=200, up=False):
    """Teeth two columns apart hanging from one bar (or, up = True, standing on it: separate until the last row)."""
    img = np.full((h, w), BG, np.float32)
    img[2:h - 2, 2:w - 2:2] = INK
    img[h - 3 if up else 2, 2:w - 2] = INK
    return img


def rings(n=9, gap=2):
    """Nested square rings, one pixel thick, `gap` - 1 background pixels apart: n components around one centre."""
    s = 2 * gap * n + 3
    img = np.full((s, s), BG, np.float32)
    for k in range(n):
        a, b = 1 + gap * k, s - 2 - gap * k
        img[a, a:b + 1] = img[b, a:b + 1] = INK
        img[a:b + 1, a] = img[a:b + 1, b] = INK
    return img


def test_combs_and_nested_rings(det):
    for img in (comb(), comb(up=True), comb(up=True)[:, ::-1].copy()):
        fr, polys, adj = _whole(img)
        st = []
        want = _both(det, fr, polys, adj, stats=st)
        assert st[0]["components"] == 1 and want["boxes"].tolist() == [[2, 2, 198, 38]]
    fr, polys, adj = _whole(rings())
    st = []
    assert len(_both(det, fr, polys, adj, stats=st)["boxes"]) == 1 and st[0]["components"] == 9      # every ring merges into the outermost
    want = _both(det, fr, polys, adj, cc=dict(merge_overlap_pct=0, min_height_pct=0))
    assert len(want["boxes"]) == 9 and np.all(np.diff(want["boxes"][:, 0]) > 0)
    _both(det, fr, polys, adj, dict(polarity=2))                                                        # the background between the rings
    # two rings side by side with a third inside the first, plus specks
    img = np.full((40, 90), BG, np.float32)
    img[2:38, 2:40] = rings(9)[:36, :38]
    img[5:30, 50:80] = rings(7)[:25, :30]
    img[33, 60], img[35, 70:73] = INK, INK
    for cc in (None, dict(merge_overlap_pct=1), dict(merge_overlap_pct=100, min_height_pct=1)):
        _both(det, *_whole(img), dict(min_glyph_pixels=0), cc)


def test_both_fallbacks_and_the_limits_themselves(det):
    for img, params in ((noise_word(), None), (lattice_word(), None), (lattice_word(), dict(max_glyphs=256, min_glyph_pixels=0))):
        fr, polys, adj = _whole(img)
        want = _both(det, fr, polys, adj, params)
        col = G.segment(fr, polys, adj, params)
        assert want["word_info"][0, 3] == (col["word_info"][0, 3] | 2) and np.array_equal(want["boxes"], col["boxes"])
    # flagged and unflagged words in one call, on two frames
    frames = np.full((2, 1, 64, 700), BG, np.float32)
    frames[0, 0, :, :600] = noise_word()
    frames[0, 0, 5:40, 620:640] = INK
    frames[1, 0, :50, :100] = lattice_word()
    frames[1, 0, 10:30, 200:210] = INK
    polys = [[[(615, 0), (650, 50)], [(0, 0), (599, 63)], [(0, 0), (699, 63)]], [[(0, 0), (99, 49)], [(190, 5), (220, 40)], [(0, 0), (100, 50)]]]
    want = _both(det, frames, polys, [[1.0, 1.0]] * 2)
    col = G.segment(frames, polys, [[1.0, 1.0]] * 2)["word_info"][:, 3]
    assert want["word_info"][:, 3].tolist() == [0, col[1] | 2, col[2] | 2, col[3] | 2, 0, col[5] | 2]
    # 1024 components and 8192 runs are within the limits, one more is not
    lat = np.full((64, 66), BG, np.float32)
    lat[::2, 0:64:2] = INK
    assert _both(det, *_whole(lat))["word_info"][0, 3] == 0
    lat[1, 65] = INK
    st = []
    assert _both(det, *_whole(lat), stats=st)["word_info"][0, 3] & 2 and st[0]["components"] == 1025
    bars = np.full((65, 256), BG, np.float32)
    bars[:64, ::2] = INK                                       # 128 vertical lines: 64 x 128 = 8192 runs
    st = []
    assert _both(det, *_whole(bars), stats=st)["word_info"][0, 3] == 1 and st[0]["runs"] == 8192 and st[0]["components"] == 128
    bars[64, 0] = INK
    st = []
    assert _both(det, *_whole(bars), stats=st)["word_info"][0, 3] & 2 and st[0]["runs"] == 8193


def test_frame_edges_one_pixel_boxes_noise_and_tall_boxes(det):
    rng = np.random.default_rng(5)
    h, w = 37, 53
    frames = rng.uniform(-20, 280, size=(3, 1, h, w)).astype(np.float32)
    frames[1, 0, ::3, ::2] = np.nan
    frames[1, 0, 1::5, 1::3] = np.inf
    frames[2, 0] = np.where(rng.random((h, w)) < 0.3, 30.0, 220.0).astype(np.float32)
    polys = [[[(0, 0)], [(w - 1, h - 1)], [(0, 0), (w + 40, h + 40)], [(w - 1, 0), (w - 1, h - 1)], [(0, h - 1), (w - 1, h - 1)], [(7, 9), (8, 9)]],
             [[(0, 0), (w - 1, h - 1)], [(3, 3), (20, 30)], [(10, 2)]],
             [[(0, 0), (w - 1, h - 1)], [(w - 5, h - 5), (w + 3, h + 3)], [(0, 10), (4, 20)]]]
    _both(det, frames, polys, [[1.0, 1.0]] * 3)
    _both(det, frames, polys, [[1.0, 1.0]] * 3, dict(min_glyph_pixels=0, max_glyphs=256), dict(min_height_pct=0))
    _both(det, frames, polys, [[0.7, 1.3], [1.0, 1.0], [2.5, 0.4]], dict(polarity=2), dict(merge_overlap_pct=0))
    # more rows than the kernel's row chunk; ink in the last column of a box 128 columns wide
    tall = np.where(rng.random((2500, 5)) < 0.3, 30.0, 220.0).astype(np.float32)
    _both(det, *_whole(tall), dict(min_glyph_pixels=0, max_glyphs=256), dict(min_height_pct=0))
    wide = np.where(rng.random((9, 128)) < 0.6, 30.0, 220.0).astype(np.float32)
    wide[:, 127], wide[::2, 63:65] = 30.0, 30.0
    _both(det, *_whole(wide), dict(min_glyph_pixels=0, max_glyphs=256, polarity=1), dict(min_height_pct=0, merge_overlap_pct=0))


def test_empty_polygon_list(det):
    frames = np.zeros((2, 1, 16, 16), np.float32)
    for device in (False, True):
        g, crops = _run(det, frames, [[], []], [[1.0, 1.0]] * 2, device=device)
        assert g.img_offsets.tolist() == [0, 0, 0] and g.word_offsets.tolist() == [0] and g.n_glyphs == 0 and crops.shape == (0, 784)


def _many_blocks():
    img = np.full((24, 2600), BG, np.float32)
    x, k = 3, 0
    while x < 2590:
        gw = 1 + (k * 7) % 9
        img[2 + k % 5: 20 - k % 3, x:x + gw] = INK
        x += gw + 1 + k % 3
        k += 1
    return img


def test_max_glyphs_and_the_percentages_at_their_ends(det):
    fr, polys, adj = _whole(_many_blocks())
    polys[0] += [[(100, 0), (300, 23)], [(1000, 0), (1100, 23)]]
    for mg in (1, 256):
        want = _both(det, fr, polys, adj, dict(max_glyphs=mg))
        assert want["word_info"][0, 3] == 1 and want["word_offsets"][1] == mg
    img = np.full((40, 90), BG, np.float32)
    img[2:38, 2:40] = rings(9)[:36, :38]
    img[5:30, 50:80] = rings(7)[:25, :30]
    img[4:6, 84:88], img[20:30, 83:89] = INK, INK
    counts = {}
    for mo in (0, 1, 100):
        for mh in (0, 1, 100):
            for src in (_whole(img), _whole(dotted_i())):
                want = _both(det, *src, None, dict(merge_overlap_pct=mo, min_height_pct=mh))
                counts[(mo, mh, src[0].shape[-1])] = len(want["boxes"])
    assert counts[(0, 0, 24)] == 3 and counts[(1, 0, 24)] == 2 and counts[(100, 0, 24)] == 2 and counts[(100, 100, 24)] == 0


def test_read_words_with_components(det, golden_dir):
    import torch

    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    from ocr_rs_amd.char_recognition import VALUES
    rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    try:
        frames, polys, adj, words = _pages(golden_dir)
        flat = [w for page in words for w in page]
        # axis-aligned boxes
        got = reading.read_words(det, rec, frames, polys, adj, cc={})
        seg = CC.segment_cc(frames, polys, adj)
        labels, probs = rec.classify_host(G.glyph_crops(frames, seg))
        k = 0
        for b, page in enumerate(got):
            assert len(page) == len(polys[b])
            for text, pr, boxes in page:
                n = len(text)
                assert text == "".join(VALUES[int(c)] for c in labels[k:k + n]) and np.array_equal(pr, probs[k:k + n])
                assert np.array_equal(boxes, seg["boxes"][k:k + n])
                k += n
        assert k == len(labels) > 0
        again = reading.read_words(det, rec, torch.from_numpy(frames).cuda(), polys, adj, cc=capi.cc_params())
        assert [[(t, p.tolist(), bx.tolist()) for t, p, bx in pg] for pg in again] == [[(t, p.tolist(), bx.tolist()) for t, p, bx in pg] for pg in got]
        axis_counts = [len(t) for pg in got for t, _, _ in pg]
        # strips
        got = reading.read_words_rectified(det, rec, frames, polys, adj, cc={})
        atlas, rects, plan = _atlas(frames, polys, adj)
        seg = CC.segment_cc(atlas, rects, [[1.0, 1.0]])
        labels, probs = rec.classify_host(G.glyph_crops(atlas, seg))
        for b, page in enumerate(got):
            assert len(page) == len(polys[b])
            for wi, (text, pr, quads) in enumerate(page):
                word = int(plan["img_offsets"][b]) + wi
                g0, g1 = int(seg["word_offsets"][word]), int(seg["word_offsets"][word + 1])
                assert text == "".join(VALUES[int(c)] for c in labels[g0:g1]) and np.array_equal(pr, probs[g0:g1])
                assert np.array_equal(quads, S.glyph_quads(plan, word, seg["boxes"][g0:g1]))
        strip_counts = [len(t) for pg in got for t, _, _ in pg]
        col_axis = [len(t) for pg in reading.read_words(det, rec, frames, polys, adj) for t, _, _ in pg]
        col_strip = [len(t) for pg in reading.read_words_rectified(det, rec, frames, polys, adj) for t, _, _ in pg]

        def hits(c):
            return sum(len(w) == n for w, n in zip(flat, c) if w != "###")
        print("\nglyphs per word on the reference pages (word, columns / components on axis-aligned boxes, columns / components on strips):")
        for row in zip(flat, col_axis, axis_counts, col_strip, strip_counts):
            print("  ", row)
        print(f"count == transcription length: axis-aligned {hits(col_axis)} -> {hits(axis_counts)}, strips {hits(col_strip)} -> {hits(strip_counts)} of 12")
        assert hits(axis_counts) > 2 and hits(strip_counts) > 2
    finally:
        rec.close()


def test_invalid_arguments_leave_the_handle_usable_and_the_column_call_unchanged(det):
    from ocr_rs_amd import capi
    L = capi.lib()
    img, _ = kerned_pair()
    frames, polys, adj = _whole(img)
    frames = np.ascontiguousarray(frames)
    st, keep = capi.python_to_polygons(polys, [[0.0]])
    adj = np.ones((1, 2))
    adj_p = adj.ctypes.data_as(C.POINTER(C.c_double))
    out = C.POINTER(capi.Glyphs)()
    h, w = img.shape

    def seg(*, d=det._h, f=frames.ctypes.data, n=1, h=h, w=w, mk=capi.MEM_HOST, p=C.byref(st), a=adj_p, prm=None, cc=None, o=C.byref(out)):
        return L.ocr_segment_glyphs_cc(d, f, n, h, w, mk, p, a, prm, cc, o)

    def ok():
        _check(det, frames, polys, adj)
        assert seg() == 0 and out.contents.n_glyphs == 2        # null params and cc: the defaults
        L.ocr_glyphs_free(out)

    def cc_raw(mo=50, mh=25, r0=0, r1=0):
        return C.byref(capi.CcParams(mo, mh, (C.c_int32 * 2)(r0, r1)))

    ok()
    for kw in (dict(d=None), dict(f=None), dict(p=None), dict(a=None), dict(o=None), dict(mk=2), dict(mk=-1), dict(n=2), dict(n=0),
               dict(h=0), dict(w=-3)):
        assert seg(**kw) == 1, kw
        assert L.ocr_last_error()
        ok()
    for bad in (cc_raw(mo=-1), cc_raw(mo=101), cc_raw(mh=-1), cc_raw(mh=101), cc_raw(r0=1), cc_raw(r1=-7)):
        assert seg(cc=bad) == 1
        assert b"cc" in L.ocr_last_error()
        ok()
    for bp in (dict(polarity=3), dict(min_col_ink=0), dict(min_glyph_pixels=-1), dict(max_glyphs=0), dict(max_glyphs=257), dict(glyph_box=29),
               dict(ink_high=2)):
        assert seg(prm=C.byref(capi.segment_params(**bp))) == 1, bp
        ok()
    with pytest.raises(TypeError):
        capi.cc_params(reserved=1)
    big = np.zeros((1, 1, 2100, 2100), np.float32)
    with pytest.raises(capi.OcrError) as e:
        det.segment_glyphs(big, [[[(0, 0), (2099, 2099)]]], adj, cc={})
    assert e.value.code == 1 and "2^22" in str(e.value)
    ok()
    # the column call on the same handle, after all of the above and after a fallback, still equals its own oracle
    fr2, polys2, adj2 = _whole(noise_word())
    assert det.segment_glyphs(fr2, polys2, adj2, cc={}).word_info[0, 3] & 2
    for fr, pl, ad in ((frames, polys, adj), (fr2, polys2, adj2)):
        want = G.segment(fr, pl, ad)
        g = det.segment_glyphs(fr, pl, ad)
        _assert_equal_seg(g, want)
        _assert_bits(det.extract_glyph_crops(fr, g), G.glyph_crops(fr, want))
