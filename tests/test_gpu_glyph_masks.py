"""Label planes and masked glyph crops on the MI355X (ocr_segment_glyphs_cc_labelled, ocr_glyph_labels_read,
ocr_extract_glyph_crops_masked; csrc/glyph_cc.hip segment_cc_labelled_kernel, csrc/glyphs.hip glyph_crop_masked_kernel): the glyph
block, every plane and every crop equal tests/glyph_mask_oracle.py bit for bit, from host and from device memory; the labelled call's
glyph block equals ocr_segment_glyphs_cc's array for array; the page readers compose; every OCR_ERR_INVALID case leaves the handle
usable and the unmasked calls unchanged."""
import ctypes as C

import numpy as np
import pytest

from tests import glyph_cc_oracle as CC
from tests import glyph_mask_oracle as M
from tests import glyph_oracle as G
from tests.test_glyph_cc_oracle import BG, INK, dotted_i, kerned_pair, lattice_word, noise_word
from tests.test_glyph_mask_oracle import bits, slashes, whole
from tests.test_gpu_glyphs_cc import _assert_equal_seg, _atlas, _many_blocks, _pages, comb, rings, serpentine_columns, serpentine_rows

pytestmark = pytest.mark.gpu

ONE = [[1.0, 1.0]]


@pytest.fixture(scope="module")
def det():
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    yield d
    d.close()


def _same_blocks(a, b):
    for f in ("img_offsets", "word_offsets", "word_info", "boxes"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(a.word_levels.view(np.uint32), b.word_levels.view(np.uint32))


def _run(det, frames, polys, adj, params, cc, halos, device):
    """(GlyphSet, word_boxes, plane_offsets, planes, {halo: crops}) through the C ABI, host or device memory."""
    from ocr_rs_amd import capi
    prm = capi.segment_params(**(params or {}))
    ccp = capi.cc_params(**(cc or {}))
    n, _, h, w = frames.shape
    if device:
        import torch
        x = torch.from_numpy(frames).cuda()
        torch.cuda.synchronize()
        g, lab = det.segment_glyphs_cc_labelled_device(x.data_ptr(), n, h, w, polys, adj, prm, ccp)
        _same_blocks(g, det.segment_glyphs_device(x.data_ptr(), n, h, w, polys, adj, prm, cc=ccp))
    else:
        g, lab = det.segment_glyphs_cc_labelled(frames, polys, adj, prm, ccp)
        _same_blocks(g, det.segment_glyphs(frames, polys, adj, prm, cc=ccp))
    with lab:
        crops = {}
        for halo in halos:
            if device:
                c = torch.full((g.n_glyphs, 784), float("nan"), device="cuda")
                det.extract_glyph_crops_masked_device(x.data_ptr(), n, h, w, g, lab, c.data_ptr(), prm, dict(halo=halo))
                crops[halo] = c.cpu().numpy()
            else:
                crops[halo] = det.extract_glyph_crops_masked(frames, g, lab, prm, capi.mask_params(halo=halo))
        assert lab.device == det.device
        return g, lab.word_boxes, lab.plane_offsets, lab.read(), crops


def _check(det, frames, polys, adj, params=None, cc=None, device=False, halos=(0, 1)):
    frames = np.ascontiguousarray(frames, np.float32)
    want = CC.segment_cc(frames, polys, adj, params, cc)
    planes = M.label_planes(frames, polys, adj, params, cc)
    g, boxes, offs, got_planes, crops = _run(det, frames, polys, adj, params, cc, halos, device)
    _assert_equal_seg(g, want)
    assert np.array_equal(boxes, planes["word_boxes"]) and offs.tolist() == planes["plane_offsets"].tolist()
    assert got_planes.dtype == np.uint16 and np.array_equal(got_planes, planes["planes"])
    for halo in halos:
        assert np.array_equal(bits(crops[halo]), bits(M.masked_glyph_crops(frames, want, planes, params, dict(halo=halo)))), halo
    return want, planes, crops


def _both(det, frames, polys, adj, params=None, cc=None, halos=(0, 1)):
    _check(det, frames, polys, adj, params, cc, True, halos)
    return _check(det, frames, polys, adj, params, cc, False, halos)


@pytest.mark.parametrize("glyph_box", [1, 20, 28])
@pytest.mark.parametrize("ink_high", [0, 1])
def test_kerned_and_dotted_fixtures(det, glyph_box, ink_high):
    prm = dict(glyph_box=glyph_box, ink_high=ink_high)
    img, _ = kerned_pair()
    fr, polys, adj = whole(img)
    want, planes, crops = _both(det, fr, polys, adj, prm)
    assert set(np.unique(planes["planes"]).tolist()) == {0, 1, 2}
    plain = det.extract_glyph_crops(fr, det.segment_glyphs(fr, polys, adj, prm, cc={}), prm)
    assert np.array_equal(bits(plain), bits(G.glyph_crops(fr, want, prm)))
    if glyph_box > 1:
        assert not np.array_equal(bits(plain[0]), bits(crops[1][0]))          # the neighbour's ink is in the unmasked crop, not in the masked
    assert np.array_equal(bits(plain[1]), bits(crops[1][1]))
    _both(det, *whole(slashes()[0]), prm)
    for cc in (None, dict(merge_overlap_pct=0), dict(merge_overlap_pct=0, min_height_pct=0)):
        _both(det, *whole(dotted_i()), prm, cc)


@pytest.mark.parametrize("device", [False, True])
def test_reference_pages_axis_aligned_and_as_an_atlas(det, golden_dir, device):
    frames, polys, adj, _ = _pages(golden_dir)
    want, planes, crops = _check(det, frames, polys, adj, device=device)
    assert want["word_offsets"][-1] > 0 and planes["planes"].any()
    _check(det, frames, polys, adj, dict(polarity=2, ink_high=0, glyph_box=28, min_glyph_pixels=0), dict(min_height_pct=0), device=device)
    _check(det, frames, polys, adj, dict(polarity=1, max_glyphs=2, glyph_box=1), dict(merge_overlap_pct=0), device=device, halos=(1,))
    atlas, rects, _ = _atlas(frames, polys, adj)
    _check(det, atlas, rects, ONE, device=device)


@pytest.mark.parametrize("dark", [True, False])
def test_font_words_and_rotated_font_words(det, dark):
    from tests.test_glyph_oracle import PIL_WORDS, draw_word
    from tests.test_gpu_strips import _rotated_batch
    rows = [draw_word(wd, dark, size=(160, 48)) for wd in PIL_WORDS]
    frame = np.concatenate([r[0] for r in rows], axis=0)
    polys = [[[(5, 48 * k + 5), (r[1][-1][2] + 5, 48 * k + 5), (r[1][-1][2] + 5, 48 * k + 42), (5, 48 * k + 42)] for k, r in enumerate(rows)]]
    _both(det, frame[None, None], polys, ONE)
    rframes, rpolys = _rotated_batch(dark)
    adj = ONE * len(rpolys)
    _check(det, rframes, rpolys, adj, device=True)
    atlas, rects, _ = _atlas(rframes, rpolys, adj)
    _check(det, atlas, rects, ONE, device=False)


def test_halo_on_a_three_level_frame_with_hand_widened_boxes(det):
    """Grey pixels (not ink, nonzero level) in the gap between two bars; glyph 0's box widened by hand over the gap, so the crop call sees
    a block that no segmentation made: halo 1 clears the grey pixel that only the neighbour touches, halo 0 keeps it."""
    from ocr_rs_amd import capi
    img = np.full((12, 16), BG, np.float32)
    img[2:10, 3:5], img[2:10, 8:10] = INK, INK
    img[4, 7], img[6, 5], img[8, 6] = 150.0, 150.0, 150.0
    fr, polys, adj = whole(img)
    fr = np.ascontiguousarray(fr)
    want = CC.segment_cc(fr, polys, adj)
    planes = M.label_planes(fr, polys, adj)
    wide = dict(want, boxes=np.asarray([[3, 2, 8, 10], [8, 2, 10, 10]], np.int32))
    g, lab = det.segment_glyphs_cc_labelled(fr, polys, adj)
    with lab:
        gw = capi.GlyphSet(g.img_offsets, g.word_offsets, g.word_info, g.word_levels, wide["boxes"])
        for prm in (dict(glyph_box=8), None, dict(glyph_box=28, ink_high=0)):
            got = {halo: det.extract_glyph_crops_masked(fr, gw, lab, prm, dict(halo=halo)) for halo in (0, 1)}
            for halo in (0, 1):
                assert np.array_equal(bits(got[halo]), bits(M.masked_glyph_crops(fr, wide, planes, prm, dict(halo=halo))))
            assert np.array_equal(bits(got[0]), bits(det.extract_glyph_crops(fr, gw, prm))) and not np.array_equal(bits(got[0]), bits(got[1]))
        assert np.array_equal(bits(det.extract_glyph_crops_masked(fr, gw, lab)), bits(M.masked_glyph_crops(fr, wide, planes)))


def test_many_runs_per_component_and_wide_rows(det):
    for img in (serpentine_rows(), serpentine_columns(), comb(), comb(up=True), rings()):
        want, planes, _ = _both(det, *whole(img), halos=(1,))
        assert set(np.unique(planes["planes"]).tolist()) == {0, 1} and len(want["boxes"]) == 1
    want, planes, _ = _both(det, *whole(rings()), None, dict(merge_overlap_pct=0, min_height_pct=0))
    assert set(np.unique(planes["planes"]).tolist()) == set(range(10))
    frame = np.full((60, 1100), BG, np.float32)                   # a serpentine off the 64-column grid, its plane at an odd width
    frame[7:55, 37:1060] = serpentine_columns()[:, :1023]
    _both(det, frame[None, None], [[[(37, 7), (1059, 54)]]], ONE, halos=(1,))


def test_the_limits_themselves_and_both_fallbacks(det):
    lat = np.full((64, 66), BG, np.float32)
    lat[::2, 0:64:2] = INK                                        # 1024 components: labelled (all too small: no glyph)
    want, planes, _ = _both(det, *whole(lat))
    assert want["word_info"][0, 3] == 0 and set(np.unique(planes["planes"]).tolist()) == {0, M.NO_GLYPH}
    want, planes, _ = _both(det, *whole(lat), dict(min_glyph_pixels=0, max_glyphs=256), dict(min_height_pct=0, merge_overlap_pct=0))
    assert planes["planes"].max() == M.NO_GLYPH and set(range(257)) <= set(np.unique(planes["planes"]).tolist())
    lat[1, 65] = INK                                              # 1025: a zero plane and flag 2
    want, planes, _ = _both(det, *whole(lat))
    assert want["word_info"][0, 3] & 2 and not planes["planes"].any()
    bars = np.full((65, 256), BG, np.float32)
    bars[:64, ::2] = INK                                          # 8192 runs
    want, planes, _ = _both(det, *whole(bars))
    assert want["word_info"][0, 3] == 1 and np.array_equal(M.plane_of(planes, 0) != 0, bars == INK)
    bars[64, 0] = INK                                             # 8193
    want, planes, _ = _both(det, *whole(bars))
    assert want["word_info"][0, 3] & 2 and not planes["planes"].any()
    for img, params in ((noise_word(), None), (lattice_word(), dict(max_glyphs=256, min_glyph_pixels=0))):
        want, planes, crops = _both(det, *whole(img), params)
        assert want["word_info"][0, 3] & 2 and not planes["planes"].any()
        assert np.array_equal(bits(crops[1]), bits(G.glyph_crops(img[None, None], want, params)))
    # flagged and unflagged words in one call, on two frames: the fallback pass over the flagged ones keeps working
    frames = np.full((2, 1, 64, 700), BG, np.float32)
    frames[0, 0, :, :600] = noise_word()
    frames[0, 0, 5:40, 620:640] = INK
    frames[1, 0, :50, :100] = lattice_word()
    frames[1, 0, 10:30, 200:210] = INK
    polys = [[[(615, 0), (650, 50)], [(0, 0), (599, 63)], [(0, 0), (699, 63)]], [[(0, 0), (99, 49)], [(190, 5), (220, 40)], [(0, 0), (100, 50)]]]
    want, planes, _ = _both(det, frames, polys, ONE * 2)
    assert [bool(M.plane_of(planes, k).any()) for k in range(6)] == [True, False, False, False, True, False]


def test_edges_one_pixel_boxes_odd_offsets_and_tall_boxes(det):
    rng = np.random.default_rng(5)
    h, w = 37, 53
    frames = rng.uniform(-20, 280, size=(3, 1, h, w)).astype(np.float32)
    frames[1, 0, ::3, ::2] = np.nan
    frames[1, 0, 1::5, 1::3] = np.inf
    frames[2, 0] = np.where(rng.random((h, w)) < 0.3, 30.0, 220.0).astype(np.float32)
    # one-pixel boxes, boxes on all four edges, and words of odd width and height: planes start at odd element offsets
    polys = [[[(0, 0)], [(w - 1, h - 1)], [(0, 0), (w + 40, h + 40)], [(w - 1, 0), (w - 1, h - 1)], [(0, h - 1), (w - 1, h - 1)], [(7, 9), (8, 9)]],
             [[(0, 0), (w - 1, h - 1)], [(3, 3), (19, 29)], [(10, 2)], [(0, 5), (6, 9)], [(20, 0), (30, 2)]],
             [[(0, 0), (w - 1, h - 1)], [(w - 5, h - 5), (w + 3, h + 3)], [(0, 10), (4, 20)], [(11, 11), (13, 13)]]]
    want, planes, _ = _both(det, frames, polys, ONE * 3)
    assert (planes["plane_offsets"] % 2).any()
    _both(det, frames, polys, ONE * 3, dict(min_glyph_pixels=0, max_glyphs=256), dict(min_height_pct=0))
    _both(det, frames, polys, [[0.7, 1.3], [1.0, 1.0], [2.5, 0.4]], dict(polarity=2), dict(merge_overlap_pct=0))
    tall = np.where(rng.random((2500, 5)) < 0.3, 30.0, 220.0).astype(np.float32)                # more rows than the kernel's row chunk
    _both(det, *whole(tall), dict(min_glyph_pixels=0, max_glyphs=256), dict(min_height_pct=0), halos=(1,))
    wide = np.where(rng.random((9, 128)) < 0.6, 30.0, 220.0).astype(np.float32)
    wide[:, 127], wide[::2, 63:65] = 30.0, 30.0
    _both(det, *whole(wide), dict(min_glyph_pixels=0, max_glyphs=256, polarity=1), dict(min_height_pct=0, merge_overlap_pct=0))


def test_max_glyphs_and_the_percentages_at_their_ends(det):
    fr, polys, adj = whole(_many_blocks())
    polys[0] += [[(100, 0), (300, 23)], [(1000, 0), (1100, 23)]]
    for mg in (1, 256):
        want, planes, _ = _both(det, fr, polys, adj, dict(max_glyphs=mg), halos=(1,))
        p0 = M.plane_of(planes, 0)
        assert want["word_info"][0, 3] == 1 and set(np.unique(p0).tolist()) == set(range(mg + 1)) | {M.NO_GLYPH}
    img = np.full((40, 90), BG, np.float32)
    img[2:38, 2:40] = rings(9)[:36, :38]
    img[5:30, 50:80] = rings(7)[:25, :30]
    img[4:6, 84:88], img[20:30, 83:89] = INK, INK
    for mo in (0, 100):
        for mh in (0, 100):
            for src in (whole(img), whole(dotted_i())):
                _both(det, *src, None, dict(merge_overlap_pct=mo, min_height_pct=mh))


def test_empty_polygon_list(det):
    from ocr_rs_amd import capi
    frames = np.zeros((2, 1, 16, 16), np.float32)
    for device in (False, True):
        g, boxes, offs, planes, crops = _run(det, frames, [[], []], ONE * 2, None, None, (0, 1), device)
        assert g.word_offsets.tolist() == [0] and g.n_glyphs == 0 and boxes.shape == (0, 4) and offs.tolist() == [0] and len(planes) == 0
        assert crops[0].shape == crops[1].shape == (0, 784)
    g, lab = det.segment_glyphs_cc_labelled(frames, [[], []], ONE * 2)
    assert lab.block.contents.n_words == 0 and not lab.block.contents.planes
    lab.free()
    lab.free()                                                    # freeing twice is harmless
    with pytest.raises(capi.OcrError):
        lab.read()


def test_no_stale_labels_between_calls(det):
    img, _ = kerned_pair()
    fr, polys, adj = whole(img)
    _, _, _, planes, _ = _run(det, fr, polys, adj, None, None, (1,), False)
    assert planes.any()
    flat = np.full_like(fr, 93.0)
    g, _, _, planes, _ = _run(det, flat, polys, adj, None, None, (1,), False)
    assert g.word_info[0, 1] == -1 and len(planes) == img.size and not planes.any()


def test_batch_of_32_pages_on_the_device(det):
    from tests.test_gpu_glyphs import _synthetic_pages
    frames, polys = _synthetic_pages(32, 320, 320, 25, seed=33)
    want, planes, _ = _check(det, frames, polys, ONE * 32, device=True)
    assert len(want["word_info"]) > 600 and want["word_offsets"][-1] > 1000 and planes["planes"].any()


def test_read_words_masked(det, golden_dir):
    import torch

    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    from ocr_rs_amd.char_recognition import VALUES
    from tests import strip_oracle as S
    rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    try:
        frames, polys, adj, _ = _pages(golden_dir)

        def as_lists(pages):
            return [[(t, p.tolist(), bx.tolist()) for t, p, bx in pg] for pg in pages]
        got = reading.read_words(det, rec, frames, polys, adj, cc={}, mask=True)
        seg = CC.segment_cc(frames, polys, adj)
        labels, probs = rec.classify_host(M.masked_glyph_crops(frames, seg, M.label_planes(frames, polys, adj)))
        k = 0
        for b, page in enumerate(got):
            assert len(page) == len(polys[b])
            for text, pr, boxes in page:
                n = len(text)
                assert text == "".join(VALUES[int(c)] for c in labels[k:k + n]) and np.array_equal(pr, probs[k:k + n])
                assert np.array_equal(boxes, seg["boxes"][k:k + n])
                k += n
        assert k == len(labels) > 0
        x = torch.from_numpy(frames).cuda()
        assert as_lists(reading.read_words(det, rec, x, polys, adj, cc=capi.cc_params(), mask={})) == as_lists(got)
        assert as_lists(reading.read_words(det, rec, x, polys, adj, cc={}, mask=capi.mask_params())) == as_lists(got)
        halo0 = reading.read_words(det, rec, frames, polys, adj, cc={}, mask={"halo": 0})
        lab0, pr0 = rec.classify_host(M.masked_glyph_crops(frames, seg, M.label_planes(frames, polys, adj), None, dict(halo=0)))
        assert np.array_equal(np.concatenate([p for pg in halo0 for _, p, _ in pg]), pr0)
        # mask=None and mask=False are the unmasked path
        plain = as_lists(reading.read_words(det, rec, frames, polys, adj, cc={}))
        l2, p2 = rec.classify_host(G.glyph_crops(frames, seg))
        assert [p for pg in plain for _, pr, _ in pg for p in pr] == p2.tolist()
        assert as_lists(reading.read_words(det, rec, frames, polys, adj, cc={}, mask=None)) == plain
        assert as_lists(reading.read_words(det, rec, frames, polys, adj, cc={}, mask=False)) == plain
        assert as_lists(reading.read_words(det, rec, frames, polys, adj, mask=None)) == as_lists(reading.read_words(det, rec, frames, polys, adj))
        # strips
        got = reading.read_words_rectified(det, rec, frames, polys, adj, cc={}, mask=True)
        atlas, rects, plan = _atlas(frames, polys, adj)
        seg = CC.segment_cc(atlas, rects, ONE)
        labels, probs = rec.classify_host(M.masked_glyph_crops(atlas, seg, M.label_planes(atlas, rects, ONE)))
        for b, page in enumerate(got):
            assert len(page) == len(polys[b])
            for wi, (text, pr, quads) in enumerate(page):
                word = int(plan["img_offsets"][b]) + wi
                g0, g1 = int(seg["word_offsets"][word]), int(seg["word_offsets"][word + 1])
                assert text == "".join(VALUES[int(c)] for c in labels[g0:g1]) and np.array_equal(pr, probs[g0:g1])
                assert np.array_equal(quads, S.glyph_quads(plan, word, seg["boxes"][g0:g1]))
        rplain = reading.read_words_rectified(det, rec, frames, polys, adj, cc={})
        rnone = reading.read_words_rectified(det, rec, frames, polys, adj, cc={}, mask=None)
        assert [[(t, p.tolist(), q.tolist()) for t, p, q in pg] for pg in rplain] == [[(t, p.tolist(), q.tolist()) for t, p, q in pg] for pg in rnone]
        for fn in (reading.read_words, reading.read_words_rectified):
            for mk in (True, {}, {"halo": 0}):
                with pytest.raises(capi.OcrError) as e:
                    fn(det, rec, frames, polys, adj, mask=mk)
                assert e.value.code == 1
    finally:
        rec.close()


def test_invalid_arguments_leave_the_handle_usable_and_the_unmasked_calls_unchanged(det):
    from ocr_rs_amd import capi
    L = capi.lib()
    img, _ = kerned_pair()
    frames, polys, adj = whole(img)
    frames = np.ascontiguousarray(frames)
    h, w = img.shape
    g, lab = det.segment_glyphs_cc_labelled(frames, polys, adj)
    blk = g.block()
    crops = np.zeros((g.n_glyphs, 784), np.float32)
    want_seg = CC.segment_cc(frames, polys, adj)
    want = M.masked_glyph_crops(frames, want_seg, M.label_planes(frames, polys, adj))

    def call(*, d=det._h, f=frames.ctypes.data, n=1, h=h, w=w, mk=capi.MEM_HOST, gl=None, lb=None, prm=None, mask=None, c=crops.ctypes.data):
        return L.ocr_extract_glyph_crops_masked(d, f, n, h, w, mk, C.byref(blk) if gl is None else gl, lab.block if lb is None else lb, prm, mask, c)

    def ok():
        crops[:] = np.nan
        assert call() == 0 and np.array_equal(bits(crops), bits(want))         # null params and mask: the defaults
        col = det.segment_glyphs(frames, polys, adj, cc={})
        _assert_equal_seg(col, want_seg)
        assert np.array_equal(bits(det.extract_glyph_crops(frames, col)), bits(G.glyph_crops(frames, want_seg)))

    def labels_like(**kw):
        b = lab.block.contents
        f = dict(n_words=b.n_words, device=b.device, word_boxes=b.word_boxes, plane_offsets=b.plane_offsets, planes=b.planes)
        f.update(kw)
        return C.pointer(capi.GlyphLabelsBlock(**f))

    def glyphs_like(src):
        return C.byref(src.block()), src

    ok()
    null_lab = C.POINTER(capi.GlyphLabelsBlock)()
    small = np.asarray([[8, 3, 17, 21]], np.int32)                # a word box that glyph 0 (7, 2, 18, 22) is not inside
    small_off = np.asarray([0, 9 * 18], np.int64)
    bad_off = np.asarray([0, 7], np.int64)
    many = capi.GlyphSet([0, 1], [0, 65535], g.word_info, g.word_levels, np.tile(g.boxes[:1], (65535, 1)))
    two_words = capi.GlyphSet([0, 2], [0, 1, 2], np.tile(g.word_info, (2, 1)), np.tile(g.word_levels, (2, 1)), g.boxes)
    many_crops = np.zeros((65535, 784), np.float32)
    cases = [dict(d=None), dict(f=None), dict(c=None), dict(lb=null_lab), dict(mk=2), dict(n=2), dict(h=0), dict(w=-3),
             dict(lb=labels_like(n_words=2)), dict(gl=glyphs_like(two_words)[0]), dict(lb=labels_like(device=det.device + 1)),
             dict(lb=labels_like(word_boxes=small.ctypes.data_as(C.POINTER(C.c_int32)), plane_offsets=small_off.ctypes.data_as(C.POINTER(C.c_int64)))),
             dict(lb=labels_like(plane_offsets=bad_off.ctypes.data_as(C.POINTER(C.c_int64)))),
             dict(lb=labels_like(planes=None)),
             dict(gl=glyphs_like(many)[0], c=many_crops.ctypes.data),
             dict(mask=C.byref(capi.MaskParams(2, (C.c_int32 * 3)(0, 0, 0)))), dict(mask=C.byref(capi.MaskParams(-1, (C.c_int32 * 3)(0, 0, 0)))),
             dict(mask=C.byref(capi.MaskParams(1, (C.c_int32 * 3)(1, 0, 0)))), dict(mask=C.byref(capi.MaskParams(1, (C.c_int32 * 3)(0, 0, -4)))),
             dict(prm=C.byref(capi.segment_params(glyph_box=29))), dict(prm=C.byref(capi.segment_params(ink_high=2)))]
    for kw in cases:
        assert call(**kw) == 1, kw
        assert L.ocr_last_error()
        ok()
    # the labelled segmentation and the read call
    st, keep = capi.python_to_polygons(polys, [[0.0]])
    adj_p = np.ones((1, 2)).ctypes.data_as(C.POINTER(C.c_double))
    out, lout = C.POINTER(capi.Glyphs)(), C.POINTER(capi.GlyphLabelsBlock)()

    def seg(*, d=det._h, f=frames.ctypes.data, n=1, mk=capi.MEM_HOST, p=C.byref(st), a=adj_p, cc=None, o=C.byref(out), lo=C.byref(lout)):
        return L.ocr_segment_glyphs_cc_labelled(d, f, n, h, w, mk, p, a, None, cc, o, lo)
    for kw in (dict(d=None), dict(f=None), dict(p=None), dict(a=None), dict(o=None), dict(lo=None), dict(mk=3), dict(n=2),
               dict(cc=C.byref(capi.CcParams(101, 25, (C.c_int32 * 2)(0, 0))))):
        assert seg(**kw) == 1, kw
        assert L.ocr_last_error() and not lout
        ok()
    assert seg() == 0 and out.contents.n_glyphs == 2 and lout.contents.n_words == 1
    host = np.zeros(img.size, np.uint16)
    assert L.ocr_glyph_labels_read(det._h, lout, host.ctypes.data) == 0 and np.array_equal(host, M.label_planes(frames, polys, adj)["planes"])
    assert L.ocr_glyph_labels_read(None, lout, host.ctypes.data) == 1 and L.ocr_glyph_labels_read(det._h, None, host.ctypes.data) == 1
    assert L.ocr_glyph_labels_read(det._h, lout, None) == 1 and L.ocr_glyph_labels_read(det._h, labels_like(device=det.device + 1), host.ctypes.data) == 1
    L.ocr_glyphs_free(out)
    L.ocr_glyph_labels_free(lout)
    L.ocr_glyph_labels_free(None)
    big = np.zeros((1, 1, 2100, 2100), np.float32)
    with pytest.raises(capi.OcrError) as e:
        det.segment_glyphs_cc_labelled(big, [[[(0, 0), (2099, 2099)]]], adj)
    assert e.value.code == 1 and "2^22" in str(e.value)
    ok()
    # 512 words of 2^22 pixels each: 2^31 plane elements, one too many - refused before anything is allocated
    big = np.zeros((1, 1, 2048, 2048), np.float32)
    with pytest.raises(capi.OcrError) as e:
        det.segment_glyphs_cc_labelled(big, [[[(0, 0), (2047, 2047)]] * 512], adj)
    assert e.value.code == 1 and "2^31" in str(e.value)
    ok()
    lab.free()
