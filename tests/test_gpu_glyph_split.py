"""ocr_split_glyphs on the MI355X (csrc/glyph_split.hip) against tests/glyph_split_oracle.py, array for array: the drawn cases, a
seeded fuzz over column and component input blocks at max_pieces 1..4, a block in which nothing is wide, both memory kinds and every
OCR_ERR_INVALID case with the handle used again."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import glyph_split_oracle as SO

pytestmark = pytest.mark.gpu

INVALID = 1      # OCR_ERR_INVALID (include/ocr_amd.h)


@pytest.fixture(scope="module")
def det():
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    yield d
    d.close()


def _set(blk):
    from ocr_rs_amd import capi
    return capi.GlyphSet(blk["img_offsets"], blk["word_offsets"], blk["word_info"], blk["word_levels"], blk["boxes"])


def _as_dict(gs):
    return dict(img_offsets=gs.img_offsets, word_offsets=gs.word_offsets, word_info=gs.word_info, word_levels=gs.word_levels, boxes=gs.boxes)


def _same(got, pmap, want):
    assert np.array_equal(got.boxes, want["boxes"]) and np.array_equal(got.word_offsets, want["word_offsets"])
    assert np.array_equal(got.word_info, want["word_info"]) and np.array_equal(got.img_offsets, want["img_offsets"])
    assert np.array_equal(got.word_levels.view(np.uint32), want["word_levels"].view(np.uint32))
    assert np.array_equal(pmap, want["map"])


CASES = {c[0]: c for c in SO.drawn_cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_drawn_case(det, name):
    _, frames, blk, prm, want_boxes, bits = CASES[name]
    got, pmap = det.split_glyphs(frames, _set(blk), prm)
    _same(got, pmap, SO.split(frames, blk, prm))
    assert got.boxes.tolist() == want_boxes and got.word_info[:, 3].tolist() == bits


def test_the_bridge_from_the_component_rule(det):
    _, frames, blk, _, want_boxes, _ = CASES["bridge"]
    cc = det.segment_glyphs(frames, [[[(0, 0), (39, 23)]]], np.ones((1, 2)), cc={})
    assert cc.boxes.tolist() == [[4, 6, 22, 18]]
    got, pmap = det.split_glyphs(frames, cc)
    assert got.boxes.tolist() == want_boxes and got.boxes[0, 2] == 13 and pmap.tolist() == [[0, 0], [0, 1]]


@functools.lru_cache(maxsize=None)
def _fuzz():
    return SO.fuzz_case()


@pytest.mark.parametrize("rule", ["column", "cc"])
def test_seeded_fuzz(det, rule):
    import torch
    frames, polys, adj = _fuzz()
    blk = det.segment_glyphs(frames, polys, adj, dict(polarity=1), cc={} if rule == "cc" else None)
    assert blk.n_words == 64
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    seen = set()
    for mp in (1, 2, 3, 4):
        prm = dict(max_pieces=mp)
        want = SO.split(frames, _as_dict(blk), prm)
        seen |= set(want["asked"].tolist())
        got, pmap = det.split_glyphs(frames, blk, prm)
        _same(got, pmap, want)
        dev, dmap = det.split_glyphs_device(d.data_ptr(), 2, 96, 160, blk, prm)            # both memory kinds
        _same(dev, dmap, want)
        if mp == 1:   # nothing may be cut: the block comes back array for array
            _same(got, pmap, dict(_as_dict(blk), map=np.stack([np.arange(blk.n_glyphs), np.zeros(blk.n_glyphs)], axis=1).astype(np.int32)))
    assert seen == {1, 2, 3, 4}
    want = SO.split(frames, _as_dict(blk), dict(max_pieces=4, max_word_pieces=2, aspect_pct=50, min_piece_w=4))
    assert np.any(want["word_info"][:, 3] & 4) and not np.all(want["word_info"][:, 3] & 4)
    _same(*det.split_glyphs(frames, blk, dict(max_pieces=4, max_word_pieces=2, aspect_pct=50, min_piece_w=4)), want)


def test_nothing_wide_comes_back_array_for_array(det):
    frames = np.full((1, 1, 32, 64), 210.0, np.float32)
    boxes = [[(4 + 10 * i, 6, 10 + 10 * i, 20) for i in range(5)]]
    for x0, y0, x1, y1 in boxes[0]:
        frames[0, 0, y0:y1, x0:x1] = 30.0
    blk = SO.block([0], SO.T_HAND, 1, boxes)
    got, pmap = det.split_glyphs(frames, _set(blk))
    _same(got, pmap, dict(blk, map=np.array([[i, 0] for i in range(5)], np.int32)))
    empty, emap = det.split_glyphs(frames, _set(SO.block([0], SO.T_HAND, 1, [[]])))
    assert empty.n_glyphs == 0 and empty.n_words == 1 and emap.shape == (0, 2)


def _invalid(fn, *needles):
    from ocr_rs_amd import capi
    with pytest.raises(capi.OcrError) as e:
        fn()
    assert e.value.code == INVALID, e.value
    for n in needles:
        assert n in str(e.value), e.value


def test_invalid_arguments(det):
    from ocr_rs_amd import capi
    L = capi.lib()
    _, frames, blk, _, want_boxes, _ = CASES["bridge"]
    gs = _set(blk)
    good = lambda: det.split_glyphs(frames, gs)[0].boxes.tolist() == want_boxes
    b = gs.block()
    out, pm = C.POINTER(capi.Glyphs)(), C.POINTER(capi.PieceMapBlock)()
    raw = lambda *a: capi.check(L.ocr_split_glyphs(*a))
    ok = (det._h, frames.ctypes.data, 1, 24, 40, capi.MEM_HOST, C.byref(b), None, C.byref(out), C.byref(pm))
    for k in (0, 1, 6, 8, 9):      # det, frames, glyphs, pieces, map
        args = list(ok)
        args[k] = None
        _invalid(lambda: raw(*args), "null")
        assert good()
    _invalid(lambda: raw(*ok[:5], 7, *ok[6:]), "mem_kind")
    _invalid(lambda: raw(*ok[:2], 2, *ok[3:]), "images")                              # n_images != n
    for bad in ((-1, 6, 22, 18), (4, 6, 41, 18), (4, 6, 22, 25), (4, -2, 22, 18), (22, 6, 4, 18), (4, 6, 4, 18)):
        _invalid(lambda: det.split_glyphs(frames, _set(SO.block([0], SO.T_HAND, 1, [[bad]]))), "outside")
        assert good()
    for field, vals in (("aspect_pct", (24, 401, -1)), ("max_pieces", (0, 5)), ("min_piece_w", (2, 65, 0)), ("max_word_pieces", (0, 257))):
        for v in vals:
            _invalid(lambda: det.split_glyphs(frames, gs, {field: v}), "params")
    _invalid(lambda: det.split_glyphs(frames, gs, dict(reserved=(0, 0, 1, 0))), "params")
    assert good()
    for info in ((1, 120, 1, 0), (-1, 120, 1, 0), (0, -1, 1, 0), (0, 255, 1, 0), (0, 120, 0, 0), (0, 120, 3, 0)):
        bad = dict(blk, word_info=np.array([info], np.int32))
        _invalid(lambda: det.split_glyphs(frames, _set(bad)), "word 0")
    bad = _set(blk)
    bad.word_offsets = np.array([1, 1], np.int32)
    _invalid(lambda: det.split_glyphs(frames, bad), "span")
    assert good()
    L.ocr_piece_map_free(None)
    with pytest.raises(TypeError):
        capi.split_params(width=3)
