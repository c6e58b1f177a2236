"""ocr_split_glyphs on the MI355X (csrc/glyph_split.hip) against tests/glyph_split_oracle.py, array for array: the drawn cases, a
seeded fuzz over column and component input blocks at max_pieces 1..4, a block in which nothing is wide, both memory kinds and every
OCR_ERR_INVALID case with the handle used again.  Past one wave's 64 columns (tests/test_glyph_split_oracle.py shows which wrong
kernels these tell from the right one): the wide drawn cases in both polarities, the wide fuzz (48 x 1201 frames, glyphs up to 1201
columns) over SO.WIDE_PARAMS in both polarities and memory kinds with its reach counters re-asserted, 1 to 257 glyphs around the
workgroup's four, a probe glyph moved through a batch and across frames, and a frame that starts 2^31 bytes into a device block."""
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


WIDE = {c[0]: c for c in SO.wide_drawn_cases()}


@pytest.mark.parametrize("name", sorted(WIDE))
def test_wide_drawn_case(det, name):
    import torch
    _, frames, blk, prm, want_boxes, bits = WIDE[name]
    want = SO.split(frames, blk, prm)
    got, pmap = det.split_glyphs(frames, _set(blk), prm)
    _same(got, pmap, want)
    assert got.boxes.tolist() == want_boxes and got.word_info[:, 3].tolist() == bits
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    n, _, h, w = frames.shape
    dev, dmap = det.split_glyphs_device(d.data_ptr(), n, h, w, _set(blk), prm)
    _same(dev, dmap, want)
    assert dev.boxes.tolist() == want_boxes


@functools.lru_cache(maxsize=None)
def _wide(pol):
    return SO.wide_fuzz_case(polarity=pol)


@pytest.mark.parametrize("pol", [1, 2])
def test_wide_fuzz(det, pol):
    """Windows and pieces of several steps of 64, both polarities, every parameter set of SO.WIDE_PARAMS, both memory kinds; the
    counters say that the oracle's result holds what the case is for."""
    import torch
    frames, blk = _wide(pol)
    gs = _set(blk)
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    total = None
    for prm in SO.WIDE_PARAMS:
        want = SO.split(frames, blk, prm)
        r = SO.reach(frames, blk, prm)
        total = r if total is None else SO.add_reach(total, r)
        if prm == dict(max_pieces=2):
            assert r["cut_ge128"] >= 1
        if "max_word_pieces" in prm:
            bit4 = want["word_info"][:, 3] & 4
            assert bit4.any() and not bit4.all() and (bit4[np.diff(blk["word_offsets"]) > 1] == 0).any()
        _same(*det.split_glyphs(frames, gs, prm), want)
        _same(*det.split_glyphs_device(d.data_ptr(), 2, SO.WIDE_H, SO.WIDE_W, gs, prm), want)
    assert all(total[k] >= 1 for k in SO.REACH_KEYS), total
    assert set(total["asked"]) == {1, 2, 3, 4}


def _scatter(rng, n_glyphs, n_frames, pol, widths=(200, 3, 70, 3, 400, 5, 130, 3, 1000)):
    """n_glyphs boxes over the wide frames, glyph i of width widths[i % 9] (nine is prime to the workgroup's four, so a glyph that asks
    for one piece meets every position of a workgroup), words of 1, 2, 3, 1, ... glyphs, the words spread over the frames in order"""
    boxes = []
    for i in range(n_glyphs):
        w, h = widths[i % len(widths)], int(rng.integers(3, 7))
        x, y = int(rng.integers(0, SO.WIDE_W - w + 1)), int(rng.integers(0, SO.WIDE_H - h + 1))
        boxes.append((x, y, x + w, y + h))
    words, i = [], 0
    while i < n_glyphs:
        k = len(words) % 3 + 1
        words.append(boxes[i:i + k])
        i += k
    return _on_frames([len(words) * f // n_frames for f in range(n_frames)] + [len(words)], pol, words, n_frames)


def _on_frames(first_word, pol, words, n_frames):
    """SO.block with the frame of each word from first_word (n_frames + 1 word offsets), img_offsets covering every frame"""
    frame_of_word = [f for f in range(n_frames) for _ in range(first_word[f + 1] - first_word[f])]
    return dict(SO.block(frame_of_word, SO.T_HAND, pol, words), img_offsets=np.asarray(first_word, np.int32))


@pytest.mark.parametrize("n_glyphs", [1, 3, 4, 5, 8, 9, 257])
def test_glyph_counts_around_a_workgroup(det, n_glyphs):
    """kSplitGlyphs = 4 glyphs a workgroup: the last workgroup holds 1, 3, 4, 1, 4, 1 and 1 glyphs, and waves that copy their box sit
    beside waves that cut."""
    for pol in (1, 2):
        frames, _ = _wide(pol)
        blk = _scatter(np.random.default_rng([n_glyphs, pol]), n_glyphs, 2, pol)
        prm = dict(max_pieces=4, max_word_pieces=12)
        want = SO.split(frames, blk, prm)
        assert len(want["asked"]) == n_glyphs and want["asked"][0] > 1
        if n_glyphs >= 3:
            assert set((want["asked"][:4] > 1).tolist()) == {False, True}
        _same(*det.split_glyphs(frames, _set(blk), prm), want)


def test_a_glyph_does_not_depend_on_its_neighbours(det):
    """One probe glyph (three cuts, windows of 150 columns) as glyph 0, 3 and last of a batch of nine, on frames 0 and 2 of three
    (frame 2 a copy of frame 0, frame 1 another image): its pieces are the same six times, and the whole block is the oracle's."""
    two, _ = _wide(1)
    frames = np.ascontiguousarray(two[[0, 1, 0]])
    probe, prm = (1, 7, 1201, 12), dict(max_pieces=4)
    alone = SO.split(frames, SO.block([0], SO.T_HAND, 1, [[probe]]), prm)["boxes"]
    assert len(alone) == 4
    fill = _scatter(np.random.default_rng(9), 8, 1, 1, widths=(3, 300, 64, 3, 700, 65, 3, 129))
    fill = [fill["boxes"][a:e].tolist() for a, e in zip(fill["word_offsets"][:-1], fill["word_offsets"][1:])]
    assert [len(w) for w in fill] == [1, 2, 3, 1, 1]
    for fr in (0, 2):
        for n_before in (0, 2, 5):          # words in front of the probe: it is glyph 0, 3 and 8
            words = fill[:n_before] + [[probe]] + fill[n_before:]
            # the words before the probe lie on the frames up to its own, those after it on the frames from its own on
            first = [0, n_before + 1, n_before + 1 + (5 - n_before) // 2, 6] if fr == 0 else [0, n_before // 2, n_before, 6]
            blk = _on_frames(first, 1, words, 3)
            pos = sum(len(w) for w in fill[:n_before])
            assert pos == {0: 0, 2: 3, 5: 8}[n_before] and blk["word_info"][n_before, 0] == fr and blk["boxes"][pos].tolist() == list(probe)
            got, pmap = det.split_glyphs(frames, _set(blk), prm)
            _same(got, pmap, SO.split(frames, blk, prm))
            assert np.array_equal(got.boxes[pmap[:, 0] == pos], alone), (fr, n_before)


def test_frame_past_2_31_bytes(det):
    """257 frames of 1024 x 2049 f32 on the device: frame 256 starts 2^31 + 2^20 bytes into the block and is the only one drawn and
    the only one with words; the oracle sees that frame alone, as frame 0."""
    import torch
    n, h, w = 257, 1024, 2049
    rng = np.random.default_rng(31)
    ink = rng.random((h, w)) < 0.1
    one = np.where(ink, rng.integers(0, 121, (h, w)), rng.integers(121, 256, (h, w))).astype(np.float32)[None, None]
    words = [[(0, 0, w, 6)], [(5, 500, 705, 512), (706, 503, 709, 509)], [(1000, h - 5, w, h)]]
    blk0 = SO.block([0, 0, 0], SO.T_HAND, 1, words)
    prm = dict(max_pieces=4)
    want = SO.split(one, blk0, prm)
    r = SO.reach(one, blk0, prm)
    assert want["asked"].tolist() == [4, 4, 1, 4] and r["win_gt128"] >= 3 and r["piece_gt128"] >= 9
    blk = _on_frames([0] * n + [3], 1, words, n)
    want["word_info"][:, 0] = n - 1
    want["img_offsets"] = blk["img_offsets"]
    block = torch.empty((n, 1, h, w), dtype=torch.float32, device="cuda")
    assert (n - 1) * h * w * 4 >= 1 << 31
    block[n - 1] = torch.from_numpy(one[0]).cuda()
    torch.cuda.synchronize()
    _same(*det.split_glyphs_device(block.data_ptr(), n, h, w, _set(blk), prm), want)


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
