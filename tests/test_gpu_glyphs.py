"""Glyph segmentation on the MI355X (ocr_segment_glyphs / ocr_extract_glyph_crops, csrc/glyphs.hip): word info, levels, glyph boxes
and crop bits equal tests/glyph_oracle.py exactly, on the reference's four pages, font-drawn words, frame edges, noise, truncation and a
32-page batch; every OCR_ERR_INVALID case leaves the handle usable; read_words composes segment -> crops -> classify."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from tests import glyph_oracle as G

pytestmark = pytest.mark.gpu

PAGES = ["img55", "img224", "img494", "img545"]


@pytest.fixture(scope="module")
def det():
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    yield d
    d.close()


def _seg_params(params):
    from ocr_rs_amd import capi
    return capi.segment_params(**(params or {}))


def _assert_equal_seg(got, want):
    assert got.img_offsets.tolist() == want["img_offsets"].tolist()
    assert got.word_offsets.tolist() == want["word_offsets"].tolist()
    assert np.array_equal(got.word_info, want["word_info"])
    assert np.array_equal(got.word_levels.view(np.uint32), want["word_levels"].view(np.uint32))
    assert np.array_equal(got.boxes, want["boxes"])


def _assert_bits(a, b):
    assert a.shape == b.shape
    assert np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _run(det, frames, polys, adj, params=None, device=False):
    """(GlyphSet, crops) through the C ABI, host or device memory."""
    if not device:
        g = det.segment_glyphs(frames, polys, adj, _seg_params(params))
        return g, det.extract_glyph_crops(frames, g, _seg_params(params))
    import torch
    x = torch.from_numpy(np.ascontiguousarray(frames, np.float32)).cuda()
    n, _, h, w = frames.shape
    torch.cuda.synchronize()
    g = det.segment_glyphs_device(x.data_ptr(), n, h, w, polys, adj, _seg_params(params))
    crops = torch.full((g.n_glyphs, 784), float("nan"), device="cuda")
    if g.n_glyphs:
        det.extract_glyph_crops_device(x.data_ptr(), n, h, w, g, crops.data_ptr(), _seg_params(params))
    return g, crops.cpu().numpy()


def _check(det, frames, polys, adj, params=None, device=False):
    want = G.segment(frames, polys, adj, params)
    got, crops = _run(det, frames, polys, adj, params, device)
    _assert_equal_seg(got, want)
    _assert_bits(crops, G.glyph_crops(frames, want, params))
    return want


def load_pages(golden_dir):
    """The four reference pages: 800 x 800 preprocessed frames, gt word polygons (original pixels), adjust values, transcriptions."""
    from PIL import Image
    from oracle import preprocess_oracle as P
    frames, polys, adj, words = [], [], [], []
    for name in PAGES:
        (gt,) = glob.glob(os.path.join(golden_dir, "text_det", "gts", "*", f"{name}.jpg.txt"))
        rows = [l.strip().split(",") for l in open(gt, encoding="utf-8-sig") if l.strip()]
        polys.append([[(int(r[i]), int(r[i + 1])) for i in range(0, len(r) - 1, 2)] for r in rows])
        words.append([r[-1] for r in rows])
        rgba = np.asarray(Image.open(os.path.join(golden_dir, "text_det", f"{name}.jpg")).convert("RGBA"))
        _, ax, ay = P.preprocess_image(rgba, 800, 800)
        adj.append((ax, ay))
        frames.append(np.asarray(Image.open(os.path.join(golden_dir, f"preprocessed_{name}.png")).convert("L"), np.float32))
    return np.stack(frames)[:, None], polys, np.asarray(adj, np.float64), words


@pytest.mark.parametrize("device", [False, True])
def test_reference_pages_equal_the_oracle(det, golden_dir, device):
    frames, polys, adj, _ = load_pages(golden_dir)
    want = _check(det, frames, polys, adj, device=device)
    assert want["word_offsets"][-1] > 0
    _check(det, frames, polys, adj, dict(polarity=2, ink_high=0, glyph_box=28, min_glyph_pixels=0), device=device)
    _check(det, frames, polys, adj, dict(polarity=1, min_col_ink=3, max_glyphs=2, glyph_box=1), device=device)


@pytest.mark.parametrize("dark", [True, False])
def test_font_words_equal_the_oracle(det, dark):
    from tests.test_glyph_oracle import PIL_WORDS, draw_word
    rows = [draw_word(wd, dark, size=(160, 48)) for wd in PIL_WORDS]
    frame = np.concatenate([r[0] for r in rows], axis=0)                # one frame, one word per 48-pixel band
    polys = [[[(5, 48 * k + 5), (r[1][-1][2] + 5, 48 * k + 5), (r[1][-1][2] + 5, 48 * k + 42), (5, 48 * k + 42)] for k, r in enumerate(rows)]]
    want = _check(det, frame[None, None], polys, [[1.0, 1.0]])
    assert np.diff(want["word_offsets"]).tolist() == [len(wd) for wd in PIL_WORDS]
    assert want["word_info"][:, 2].tolist() == [1 if dark else 2] * len(PIL_WORDS)
    _check(det, frame[None, None], polys, [[1.0, 1.0]], dict(ink_high=0), device=True)


def test_frame_edges_one_pixel_boxes_and_noise(det):
    rng = np.random.default_rng(5)
    h, w = 37, 53
    frames = rng.uniform(-20, 280, size=(3, 1, h, w)).astype(np.float32)
    frames[1, 0, ::3, ::2] = np.nan
    frames[1, 0, 1::5, 1::3] = np.inf
    frames[2, 0] = np.where(rng.random((h, w)) < 0.3, 30.0, 220.0).astype(np.float32)
    polys = [[[(0, 0)], [(w - 1, h - 1)], [(0, 0), (w + 40, h + 40)], [(w - 1, 0), (w - 1, h - 1)], [(0, h - 1), (w - 1, h - 1)], [(7, 9), (8, 9)]],
             [[(0, 0), (w - 1, h - 1)], [(3, 3), (20, 30)], [(10, 2)]],
             [[(0, 0), (w - 1, h - 1)], [(w - 5, h - 5), (w + 3, h + 3)], [(0, 10), (4, 20)]]]
    for device in (False, True):
        _check(det, frames, polys, [[1.0, 1.0]] * 3, device=device)
        _check(det, frames, polys, [[1.0, 1.0]] * 3, dict(min_glyph_pixels=0, max_glyphs=256), device=device)
    _check(det, frames, polys, [[0.7, 1.3], [1.0, 1.0], [2.5, 0.4]], dict(polarity=2))


def test_empty_polygon_list(det):
    frames = np.zeros((2, 1, 16, 16), np.float32)
    for device in (False, True):
        g, crops = _run(det, frames, [[], []], [[1.0, 1.0]] * 2, device=device)
        assert g.img_offsets.tolist() == [0, 0, 0] and g.word_offsets.tolist() == [0] and g.n_glyphs == 0 and crops.shape == (0, 784)


def test_truncation_and_spans_across_profile_chunks(det):
    h, w = 24, 2600                  # wider than the kernel's 1024-column profile chunk: spans cross chunk and 64-column boundaries
    img = np.full((h, w), 210.0, np.float32)
    x, k = 3, 0
    while x < w - 10:
        gw = 1 + (k * 7) % 9
        img[2 + k % 5: 20 - k % 3, x:x + gw] = 35.0
        x += gw + 1 + k % 3
        k += 1
    for c in (1023, 1024, 2047, 2048, 1087, 1088):
        img[5:15, c - 2:c + 3] = 35.0
    frames = img[None, None]
    polys = [[[(0, 0), (w - 1, h - 1)], [(100, 0), (300, h - 1)], [(1000, 0), (1100, h - 1)]]]
    for params in (None, dict(max_glyphs=3), dict(max_glyphs=256), dict(max_glyphs=256, min_glyph_pixels=30), dict(min_col_ink=12)):
        want = _check(det, frames, polys, [[1.0, 1.0]], params)
        if params == dict(max_glyphs=3):
            assert want["word_info"][:, 3].tolist() == [1, 1, 1] and np.diff(want["word_offsets"]).tolist() == [3, 3, 3]
        if params == dict(max_glyphs=256):
            assert want["word_info"][0, 3] == 1 and want["word_offsets"][1] == 256


def _synthetic_pages(n, h, w, words_per_page, seed):
    """n pages of ~words_per_page block words (random levels, polarity, glyph widths and gaps, noise) -> frames, polygons."""
    rng = np.random.default_rng(seed)
    frames = rng.normal(0, 6, size=(n, 1, h, w)).astype(np.float32)
    polys = []
    for b in range(n):
        frames[b, 0] += np.float32(rng.uniform(60, 200))
        plist = []
        for _ in range(words_per_page + int(rng.integers(-10, 11))):
            gh = int(rng.integers(6, 40))
            x0, y0 = int(rng.integers(0, w - 20)), int(rng.integers(0, h - gh - 4))
            bg, ink = (rng.uniform(150, 250), rng.uniform(0, 100)) if rng.random() < 0.7 else (rng.uniform(0, 100), rng.uniform(150, 250))
            x = x0 + 2
            frames[b, 0, y0:y0 + gh + 4, x0:min(w, x0 + 2 + 12 * 12)] = np.float32(bg)
            for _ in range(int(rng.integers(1, 12))):
                gw = int(rng.integers(1, 10))
                if x + gw >= w:
                    break
                top = y0 + 2 + int(rng.integers(0, 3))
                frames[b, 0, top:y0 + 2 + gh - int(rng.integers(0, 3)), x:x + gw] = np.float32(ink)
                x += gw + int(rng.integers(0, 4))
            x1 = min(w - 1, x + 2)
            if rng.random() < 0.2:   # a slanted quadrilateral: its axis-aligned box is the word box
                plist.append([(x0, y0 + 3), (x1, y0), (x1 - 2, y0 + gh + 3), (x0 + 1, y0 + gh + 2)])
            else:
                plist.append([(x0, y0), (x1, y0), (x1, y0 + gh + 3), (x0, y0 + gh + 3)])
        polys.append(plist)
    return frames, polys


@pytest.mark.parametrize("device", [True, False])
def test_batch_of_32_pages(det, device):
    frames, polys = _synthetic_pages(32, 640, 640, 100, seed=11 if device else 12)
    want = _check(det, frames, polys, [[1.0, 1.0]] * 32, device=device)
    assert len(want["word_info"]) > 3000 and want["word_offsets"][-1] > 5000


def test_invalid_arguments_leave_the_handle_usable(det):
    from ocr_rs_amd import capi
    L = capi.lib()
    frames = np.full((1, 1, 20, 30), 200.0, np.float32)
    frames[0, 0, 5:15, 5:9] = 30.0
    polys = [[[(2, 2), (25, 17)]]]
    st, keep = capi.python_to_polygons(polys, [[0.0]])
    adj = np.ones((1, 2))
    adj_p = adj.ctypes.data_as(C.POINTER(C.c_double))
    out = C.POINTER(capi.Glyphs)()
    fp = frames.ctypes.data

    def seg(*, d=det._h, f=fp, n=1, h=20, w=30, mk=capi.MEM_HOST, p=C.byref(st), a=adj_p, prm=None, o=C.byref(out)):
        return L.ocr_segment_glyphs(d, f, n, h, w, mk, p, a, prm, o)

    def ok():
        want = G.segment(frames, polys, adj)
        g = det.segment_glyphs(frames, polys, adj)
        _assert_equal_seg(g, want)
        _assert_bits(det.extract_glyph_crops(frames, g), G.glyph_crops(frames, want))
        return g

    cases = [dict(d=None), dict(f=None), dict(p=None), dict(a=None), dict(o=None), dict(mk=2), dict(mk=-1), dict(n=2), dict(n=0),
             dict(h=0), dict(w=-3)]
    bad_params = [dict(polarity=3), dict(polarity=-1), dict(min_col_ink=0), dict(min_glyph_pixels=-1), dict(max_glyphs=0),
                  dict(max_glyphs=257), dict(glyph_box=0), dict(glyph_box=29), dict(ink_high=2), dict(ink_high=-1)]
    for kw in cases:
        assert seg(**kw) == 1, kw
        assert L.ocr_last_error()
        ok()
    for bp in bad_params:
        assert seg(prm=C.byref(capi.segment_params(**bp))) == 1, bp
        ok()
    big = np.zeros((1, 1, 2100, 2100), np.float32)         # a 2100 x 2100 word box: 4 410 000 pixels > 2^22
    with pytest.raises(capi.OcrError) as e:
        det.segment_glyphs(big, [[[(0, 0), (2099, 2099)]]], adj)
    assert e.value.code == 1 and "2^22" in str(e.value)
    g = ok()
    # the crop call: null crops, a glyph block of another batch size, boxes outside the frames, a bad frame index, bad params
    blk = g.block()
    crops = np.empty((g.n_glyphs, 784), np.float32)

    def crop(*, d=det._h, f=fp, n=1, h=20, w=30, mk=capi.MEM_HOST, b=C.byref(blk), prm=None, c=crops.ctypes.data):
        return L.ocr_extract_glyph_crops(d, f, n, h, w, mk, b, prm, c)
    assert g.n_glyphs == 1
    for kw in (dict(d=None), dict(f=None), dict(b=None), dict(c=None), dict(mk=5), dict(n=2), dict(w=8), dict(h=14),
               dict(prm=C.byref(capi.segment_params(glyph_box=30)))):
        assert crop(**kw) == 1, kw
        ok()
    for bad_box in ([-1, 5, 9, 15], [5, 5, 31, 15], [5, 5, 5, 15], [5, 15, 9, 5]):
        g2 = capi.GlyphSet(g.img_offsets, g.word_offsets, g.word_info, g.word_levels, np.asarray([bad_box], np.int32))
        with pytest.raises(capi.OcrError):
            det.extract_glyph_crops(frames, g2)
        ok()
    info = g.word_info.copy()
    info[0, 0] = 1
    with pytest.raises(capi.OcrError):
        det.extract_glyph_crops(frames, capi.GlyphSet(g.img_offsets, g.word_offsets, info, g.word_levels, g.boxes))
    ok()


def test_read_words_equals_classify_on_the_oracle_crops_and_the_torch_reference(det, golden_dir):
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    from ocr_rs_amd.char_recognition import VALUES
    from oracle import torch_ref as T
    from tests.test_glyph_oracle import PIL_WORDS, draw_word
    rec_w = W.make_rec_weights(0)
    rec = capi.Recognizer(W.pack_blob(rec_w), 0)
    try:
        frames, polys, adj, words = load_pages(golden_dir)
        # plus a page of font-drawn words, so that every glyph path is exercised on more than the four pages
        band = np.concatenate([draw_word(wd, size=(800, 48))[0] for wd in PIL_WORDS] + [np.full((800 - 48 * 4, 800), 255.0, np.float32)])
        frames = np.concatenate([frames, band[None, None]])
        polys = polys + [[[(5, 48 * k + 5), (200, 48 * k + 5), (200, 48 * k + 42), (5, 48 * k + 42)] for k in range(len(PIL_WORDS))]]
        adj = np.concatenate([adj, [[1.0, 1.0]]])
        got = reading.read_words(det, rec, frames, polys, adj)
        seg = G.segment(frames, polys, adj)
        crops = G.glyph_crops(frames, seg)
        labels, probs = rec.classify_host(crops)
        ref_logits = T.rec_forward(rec_w, crops)
        ref_labels, _ = T.rec_classify(ref_logits)
        top2 = np.sort(ref_logits.astype(np.float64), axis=1)[:, -2:]
        margin = top2[:, 1] - top2[:, 0]
        k = 0
        for b, page in enumerate(got):
            assert len(page) == len(polys[b])
            for wi, (text, pr, boxes) in enumerate(page):
                n = len(text)
                assert text == "".join(VALUES[int(c)] for c in labels[k:k + n])
                assert np.array_equal(pr, probs[k:k + n])
                assert np.array_equal(boxes, seg["boxes"][k:k + n])
                for j in range(k, k + n):
                    if margin[j] > 1e-4:
                        assert labels[j] == ref_labels[j], (b, wi, j)
                k += n
        assert k == len(crops) > 0
        hits = sum(len(got[b][i][0]) == len(words[b][i]) for b in range(len(PAGES)) for i in range(len(words[b])) if words[b][i] != "###")
        total = sum(1 for b in range(len(PAGES)) for w_ in words[b] if w_ != "###")
        print(f"\nglyph count == transcription length on the reference pages: {hits} / {total} words "
              f"(synthetic recogniser weights: the strings themselves are not meaningful)")
        for b in range(len(PAGES)):
            print("  ", PAGES[b], [(words[b][i], len(got[b][i][0])) for i in range(len(words[b]))])
        # the same through a device-resident frame tensor
        import torch
        again = reading.read_words(det, rec, torch.from_numpy(frames).cuda(), polys, adj)
        assert [[(t, p.tolist(), bx.tolist()) for t, p, bx in pg] for pg in again] == [[(t, p.tolist(), bx.tolist()) for t, p, bx in pg] for pg in got]
    finally:
        rec.close()
