"""The label-plane and masked-crop oracle (tests/glyph_mask_oracle.py) held to facts that do not come from itself: strokes whose
pixels are known by construction, the unmasked crop of a frame with the neighbour painted out, the filters and limits of the
component rule, the two fallbacks, a hand-made three-level frame for the halo, scipy's labelling on random masks.  CPU only; the
kernels are held to this oracle bit for bit in tests/test_gpu_glyph_masks.py."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import glyph_cc_oracle as CC
from tests import glyph_mask_oracle as M
from tests import glyph_oracle as G
from tests.test_glyph_cc_oracle import BG, INK, dotted_i, kerned_pair, lattice_word, noise_word
from tests.test_glyph_oracle import _blocks_frame


def whole(img):
    """One frame, one word: the whole frame."""
    h, w = img.shape
    return img[None, None], [[[(0, 0), (w - 1, h - 1)]]], [[1.0, 1.0]]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def slashes():
    """The '//' frame of test_kerned_pair_is_one_glyph_by_columns_and_two_by_components -> (frame, the pixels of each stroke)."""
    img = np.full((30, 40), BG, np.float32)
    a = [(y, 20 - y // 2) for y in range(4, 26)]
    b = [(y, 26 - y // 2) for y in range(4, 26)]
    for y, x in a + b:
        img[y, x] = INK
    return img, (a, b)


def kerned_strokes():
    """kerned_pair() -> (frame, the pixels of '/' and of '\\')."""
    img, _ = kerned_pair()
    a = [(y, 16 - (y - 2) // 2 + d) for y in range(2, 22) for d in (0, 1)]
    b = [(y, 17 + (y - 8) // 2 + d) for y in range(8, 28) for d in (0, 1)]
    ink = np.zeros(img.shape, bool)
    for y, x in a + b:
        ink[y, x] = True
    assert np.array_equal(ink, img == INK)
    return img, (a, b)


def everything(img, params=None, cc=None, mask=None):
    """(seg, planes, unmasked crops, masked crops) of a whole-frame word."""
    fr, polys, adj = whole(img)
    seg = CC.segment_cc(fr, polys, adj, params, cc)
    planes = M.label_planes(fr, polys, adj, params, cc)
    return seg, planes, G.glyph_crops(fr, seg, params), M.masked_glyph_crops(fr, seg, planes, params, mask)


@pytest.mark.parametrize("strokes", [kerned_strokes, slashes])
def test_kerned_strokes_are_labelled_and_cropped_apart(strokes):
    img, (a, b) = strokes()
    seg, planes, plain, masked = everything(img)
    assert len(seg["boxes"]) == 2
    plane = M.plane_of(planes, 0)
    want = np.zeros(img.shape, np.uint16)
    for y, x in a:
        want[y, x] = 1
    for y, x in b:
        want[y, x] = 2
    assert np.array_equal(plane, want)                           # labels 1 and 2 are exactly the two strokes
    for g, other in ((0, b), (1, a)):
        alone = img.copy()
        for y, x in other:
            alone[y, x] = BG                                     # the other stroke painted out: same boxes, levels given by seg
        crop_alone = G.glyph_crops(alone[None, None], seg)[g]
        assert np.array_equal(bits(masked[g]), bits(crop_alone))
        differs = not np.array_equal(bits(plain[g]), bits(crop_alone))
        in_box = any(seg["boxes"][g][0] <= x < seg["boxes"][g][2] and seg["boxes"][g][1] <= y < seg["boxes"][g][3] for y, x in other)
        assert differs == in_box                                 # the unmasked crop carries the neighbour exactly when its ink is in the box
        assert np.array_equal(bits(masked[g]), bits(plain[g])) == (not in_box)
    assert not np.array_equal(bits(masked), bits(plain))         # the feature does something on this frame
    for halo in (0, 1):
        assert np.array_equal(bits(M.masked_glyph_crops(img[None, None], seg, planes, None, dict(halo=halo))), bits(masked))   # two-level frame


def test_kerned_pair_figures_of_the_unmasked_crop():
    img, _ = kerned_strokes()
    seg, planes, plain, masked = everything(img)
    d = np.abs(plain - masked)
    assert int((d[0] != 0).sum()) == 4 and float(d[0].max()) == 0.5 and not d[1].any()


def test_dotted_i_at_three_settings():
    img = dotted_i()
    dot, stem, ell = (slice(5, 8), slice(10, 13)), (slice(10, 25), slice(10, 13)), (slice(4, 25), slice(17, 19))
    for cc, want in ((None, (1, 1, 2)), (dict(merge_overlap_pct=0), (M.NO_GLYPH, 1, 2)), (dict(merge_overlap_pct=0, min_height_pct=0), (1, 2, 3))):
        seg, planes, plain, masked = everything(img, None, cc)
        plane = M.plane_of(planes, 0)
        assert np.array_equal(plane != 0, img == INK)
        for part, lab in zip((dot, stem, ell), want):
            assert (plane[part] == lab).all(), (cc, lab)
        assert len(seg["boxes"]) == len(set(want) - {M.NO_GLYPH})
        assert np.array_equal(bits(plain), bits(masked))         # nothing foreign in or next to any box


def test_small_components_and_truncated_groups_are_no_glyph():
    blocks = [(12, 8, 17, 20), (19, 10, 22, 19), (25, 8, 33, 21), (36, 14, 37, 16), (40, 9, 46, 20)]
    img = _blocks_frame(30, 60, blocks)
    plane = M.word_plane(img, 10, 5, 50, 25)                     # the 1 x 2 speck has 2 ink pixels < min_glyph_pixels = 4
    assert [int(plane[y0 - 5, x0 - 10]) for x0, y0, _, _ in blocks] == [1, 2, 3, M.NO_GLYPH, 4]
    plane = M.word_plane(img, 10, 5, 50, 25, dict(min_glyph_pixels=2))          # kept by size, dropped by height: still no glyph
    assert [int(plane[y0 - 5, x0 - 10]) for x0, y0, _, _ in blocks] == [1, 2, 3, M.NO_GLYPH, 4]
    plane = M.word_plane(img, 10, 5, 50, 25, dict(min_glyph_pixels=2), dict(min_height_pct=0))
    assert [int(plane[y0 - 5, x0 - 10]) for x0, y0, _, _ in blocks] == [1, 2, 3, 4, 5]
    blocks = [(2 + 4 * k, 2, 4 + 4 * k, 8) for k in range(10)]
    img = _blocks_frame(10, 44, blocks)
    img[2:3, 42] = INK                                           # a dropped speck behind everything
    plane = M.word_plane(img, 0, 0, 44, 10, dict(max_glyphs=4))
    assert [int(plane[2, x0]) for x0, _, _, _ in blocks] == [1, 2, 3, 4] + [M.NO_GLYPH] * 6 and plane[2, 42] == M.NO_GLYPH
    assert np.array_equal(plane != 0, img == INK)
    seg, planes, plain, masked = everything(img, dict(max_glyphs=4))
    assert seg["word_info"][0, 3] == CC.FLAG_TRUNCATED and np.array_equal(bits(plain), bits(masked))


def test_both_fallbacks_and_flat_words_are_not_masked():
    for img, params in ((noise_word(), None), (lattice_word(), None), (lattice_word(), dict(max_glyphs=256, min_glyph_pixels=0)),
                        (np.full((12, 20), 93.0, np.float32), None)):
        seg, planes, plain, masked = everything(img, params)
        assert not planes["planes"].any() and len(planes["planes"]) == img.size
        assert np.array_equal(bits(plain), bits(masked))
        assert seg["word_info"][0, 3] & CC.FLAG_FALLBACK or seg["word_info"][0, 1] == -1


def test_separated_blocks_are_unchanged_by_the_mask():
    blocks = [(12, 8, 17, 20), (19, 10, 22, 19), (25, 8, 33, 21), (40, 9, 46, 20)]
    img = _blocks_frame(30, 60, blocks)
    fr = img[None, None]
    polys, adj = [[[(10, 5), (49, 24)]]], [[1.0, 1.0]]
    seg = CC.segment_cc(fr, polys, adj)
    planes = M.label_planes(fr, polys, adj)
    assert planes["word_boxes"].tolist() == [[10, 5, 50, 25]] and planes["plane_offsets"].tolist() == [0, 800]
    for prm in (None, dict(glyph_box=28, ink_high=0), dict(glyph_box=1)):
        for halo in (0, 1):
            assert np.array_equal(bits(M.masked_glyph_crops(fr, seg, planes, prm, dict(halo=halo))), bits(G.glyph_crops(fr, seg, prm)))


def test_halo_clears_a_grey_rim_of_foreign_ink_only():
    """Three levels: two solid bars (ink) 3 columns apart, grey pixels (between the Otsu threshold and the background, so not ink, but a
    nonzero level) in the gap.  Glyph 0's box is widened by hand to hold the gap."""
    img = np.full((12, 16), BG, np.float32)
    img[2:10, 3:5] = INK                                         # glyph 0
    img[2:10, 8:10] = INK                                        # glyph 1
    GREY = 150.0
    img[4, 7] = GREY                                             # touches glyph 1 only
    img[6, 5] = GREY                                             # touches glyph 0 only
    img[8, 6] = GREY                                             # touches neither
    fr, polys, adj = whole(img)
    seg = CC.segment_cc(fr, polys, adj)
    planes = M.label_planes(fr, polys, adj)
    plane = M.plane_of(planes, 0)
    assert seg["boxes"].tolist() == [[3, 2, 5, 10], [8, 2, 10, 10]]
    assert plane[4, 7] == plane[6, 5] == plane[8, 6] == 0 and plane[4, 8] == 2 and plane[6, 4] == 1
    wide = dict(seg, boxes=np.asarray([[3, 2, 8, 10], [8, 2, 10, 10]], np.int32))     # glyph 0's box over the gap, 5 x 8
    prm = dict(glyph_box=8)                                      # s = 1: sample (i, j) sits on pixel (cx - 14 + j, cy - 14 + i) exactly

    plain = G.glyph_crops(fr, wide, prm)
    on = M.masked_glyph_crops(fr, wide, planes, prm, dict(halo=1))
    off = M.masked_glyph_crops(fr, wide, planes, prm, dict(halo=0))
    assert np.array_equal(bits(off), bits(plain))                # no foreign ink inside the widened box: halo 0 changes nothing
    # the same frame with the pixel that only glyph 1 touches painted out is what halo 1 gives
    gone = img.copy()
    gone[4, 7] = BG
    assert np.array_equal(bits(on[0]), bits(G.glyph_crops(gone[None, None], wide, prm)[0]))
    assert not np.array_equal(bits(on[0]), bits(plain[0]))
    # a grey pixel next to both own and foreign ink is kept
    img3 = np.full((12, 16), BG, np.float32)
    img3[2:10, 3:5] = INK
    img3[2:10, 6:8] = INK
    img3[5, 5] = GREY
    fr3, polys3, adj3 = whole(img3)
    seg3 = CC.segment_cc(fr3, polys3, adj3)
    assert seg3["boxes"].tolist() == [[3, 2, 5, 10], [6, 2, 8, 10]]
    wide3 = dict(seg3, boxes=np.asarray([[3, 2, 6, 10], [6, 2, 8, 10]], np.int32))
    planes3 = M.label_planes(fr3, polys3, adj3)
    assert np.array_equal(bits(M.masked_glyph_crops(fr3, wide3, planes3, prm)), bits(G.glyph_crops(fr3, wide3, prm)))
    lvl = G.glyph_crops(fr3, wide3, prm)[0]
    assert ((lvl > 0) & (lvl < 1)).any()                         # ... and the grey level is in the crop


@pytest.mark.parametrize("density", [0.05, 0.3, 0.5, 0.7, 0.95])
def test_planes_on_random_masks(density):
    try:
        from scipy import ndimage as ndi
    except ImportError:                                          # only the "one component, one label" assertion needs scipy
        ndi = None
    rng = np.random.default_rng(int(density * 100) + 1)
    for shape in ((1, 1), (1, 70), (33, 1), (17, 64), (40, 129)):
        mask = rng.random(shape) < density
        img = np.where(mask, INK, BG).astype(np.float32)
        for params, cc in ((dict(polarity=1), None), (dict(polarity=1, min_glyph_pixels=0, max_glyphs=3), dict(min_height_pct=0, merge_overlap_pct=0))):
            plane = M.word_plane(img, 0, 0, shape[1], shape[0], params, cc)
            t = CC.word_ink(img, 0, 0, shape[1], shape[0], params)[0]
            if t < 0:
                assert not plane.any()
                continue
            st = {}
            flags = CC.segment_word_cc(img, 0, 0, shape[1], shape[0], params, cc, st)[2]
            if flags & CC.FLAG_FALLBACK:
                assert not plane.any()
                continue
            assert np.array_equal(plane != 0, mask)              # the nonzero set is the ink set
            if ndi is not None:
                comp, n = ndi.label(mask, structure=np.ones((3, 3), int))
                for k in range(1, n + 1):
                    assert len(np.unique(plane[comp == k])) == 1  # the pixels of one component share one label
            runs = CC.runs_of(mask)                              # ... and by the oracle's own components, which need no scipy
            of_root = {}
            for (y, a0, a1), r in zip(runs.tolist(), CC.label_runs(runs).tolist()):
                assert len(np.unique(plane[y, a0:a1])) == 1 and of_root.setdefault(r, int(plane[y, a0])) == int(plane[y, a0])
            used = set(np.unique(plane).tolist()) - {0, M.NO_GLYPH}
            n_glyphs = len(CC.segment_word_cc(img, 0, 0, shape[1], shape[0], params, cc)[5])
            assert used == set(range(1, n_glyphs + 1))


def test_batch_layout_offsets_and_empty_lists():
    img = _blocks_frame(20, 30, [(5, 5, 9, 15), (12, 5, 20, 15)])
    frames = np.stack([img, np.full_like(img, 7.0), img])[:, None]
    rect = [(2, 2), (24, 2), (24, 17), (2, 17)]
    polys = [[rect], [], [rect, [(0, 0), (2, 0), (2, 2), (0, 2)]]]
    planes = M.label_planes(frames, polys, [[1.0, 1.0]] * 3)
    assert planes["word_boxes"].tolist() == [[2, 2, 25, 18], [2, 2, 25, 18], [0, 0, 3, 3]]
    assert planes["plane_offsets"].tolist() == [0, 368, 736, 745] and planes["planes"].dtype == np.uint16 and len(planes["planes"]) == 745
    assert np.array_equal(M.plane_of(planes, 0), M.plane_of(planes, 1)) and not M.plane_of(planes, 2).any()
    seg = CC.segment_cc(frames, polys, [[1.0, 1.0]] * 3)
    assert np.array_equal(bits(M.masked_glyph_crops(frames, seg, planes)), bits(G.glyph_crops(frames, seg)))
    empty = M.label_planes(frames[:1], [[]], [[1.0, 1.0]])
    assert empty["plane_offsets"].tolist() == [0] and empty["word_boxes"].shape == (0, 4) and len(empty["planes"]) == 0
    assert M.masked_glyph_crops(frames[:1], CC.segment_cc(frames[:1], [[]], [[1.0, 1.0]]), empty).shape == (0, 784)


def test_mask_defaults_and_struct_sizes():
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    assert M.MASK_DEFAULTS == dict(halo=1) and M.mask_params_with(dict(halo=0)) == dict(halo=0) and M.NO_GLYPH == 0xFFFF
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    p = capi.MaskParams(7, (C.c_int32 * 3)(1, 2, 3))
    capi.lib().ocr_mask_default_params(C.byref(p))
    assert (p.halo, list(p.reserved)) == (1, [0, 0, 0])
    assert capi.mask_params(halo=0).halo == 0 and capi.mask_params().halo == 1
    with pytest.raises(TypeError):
        capi.mask_params(reserved=1)
    with pytest.raises(TypeError):
        capi._as_mask_params(False)                              # the unmasked call is another method, not a value of mask
    assert capi._as_mask_params(None) is None and capi._as_mask_params(True) is None and capi._as_mask_params({}).halo == 1
    assert C.sizeof(capi.MaskParams) == 16
    assert C.sizeof(capi.GlyphLabelsBlock) == 8 + 3 * C.sizeof(C.c_void_p)
    assert [f[0] for f in capi.GlyphLabelsBlock._fields_] == ["n_words", "device", "word_boxes", "plane_offsets", "planes"]
    assert capi.GlyphLabelsBlock.word_boxes.offset == 8 and capi.GlyphLabelsBlock.planes.offset == 8 + 2 * C.sizeof(C.c_void_p)
