"""ocr_preprocess_batch / ocr_preprocess_batch_async: a batch of decoded pages of differing sizes to detector frames in one launch.
Every frame is bit for bit oracle/preprocess_oracle.py's and ocr_preprocess_image's for that image alone; the shapes are the smallest
at which each mechanism of the kernel and of the staging can go wrong (tile edges, padding-only tiles, a span of several LDS chunks,
clamped sizes, strides, chunked staging, the plan buffers' event guard, a pending pipelined batch)."""
import ctypes as C
import os

import numpy as np
import pytest
from PIL import Image

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from ocr_rs_amd import text_detection as td
from ocr_rs_amd import weights as W
from tests import preprocess_batch_oracle as PB

pytestmark = pytest.mark.gpu

# (w, h): up-scaling; one pixel; identity at 64 x 32; both use_width branches at odd sizes; ordinary down-scaling with a ragged last
# tile; ratio 187 along x (the span of a tile is several LDS chunks, nh clamps to 1); the same along y (nw clamps to 1)
SIZES = [(3, 5), (1, 1), (64, 32), (97, 211), (211, 97), (1600, 1200), (12000, 6), (6, 12000)]
TARGETS = {(64, 32): 8, (640, 640): 6}    # target -> how many of SIZES (at 640 x 640 padding-only tiles exist)


@pytest.fixture(scope="module")
def det():
    d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    yield d
    d.close()


_IMAGES = []


def images(k=len(SIZES)):
    if not _IMAGES:
        rng = np.random.RandomState(20)
        _IMAGES.extend(rng.randint(0, 256, (h, w, 4)).astype(np.uint8) for w, h in SIZES)
    return _IMAGES[:k]


_WANT = {}


def want(target):
    """(oracle frames, oracle adjust) of the mixed batch at `target`, computed once and never written to"""
    if target not in _WANT:
        g, a = PB.preprocess_batch(images(TARGETS[target]), *target)
        g.setflags(write=False)
        a.setflags(write=False)
        _WANT[target] = (g, a)
    return _WANT[target]


def raw_batch(det, descs, n, src_kind, tw, th, gray, f32, dst_kind, adj):
    """the C call itself -> (code, message)"""
    p = lambda a: None if a is None else (a if isinstance(a, int) else capi._ptr(a))
    code = capi.lib().ocr_preprocess_batch(det._h if det is not None else None, descs, n, src_kind, tw, th, p(gray), p(f32), dst_kind,
                                           adj.ctypes.data_as(C.POINTER(C.c_double)) if adj is not None else None)
    return code, capi.lib().ocr_last_error().decode()


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8,f32", [(True, False), (False, True), (True, True)], ids=["u8", "f32", "both"])
@pytest.mark.parametrize("target", sorted(TARGETS))
def test_mixed_batch_equals_the_oracle_and_the_single_image_call(det, target, u8, f32):
    imgs = images(TARGETS[target])
    ogray, oadj = want(target)
    gray, fr, adj = det.preprocess_batch(imgs, target[0], target[1], want_u8=u8, want_f32=f32)
    assert (adj == oadj).all()
    assert (gray is None) == (not u8) and (fr is None) == (not f32)
    if u8:
        assert gray.shape == ogray.shape and np.array_equal(gray, ogray)
    if f32:
        assert fr.shape == (len(imgs), 1, target[1], target[0])
        assert np.array_equal(fr[:, 0].view(np.uint32), ogray.astype(np.float32).view(np.uint32))   # f32 == u8.astype(f32)
    if u8 and f32:
        assert np.array_equal(fr[:, 0], gray.astype(np.float32))
        for i, im in enumerate(imgs):      # ... and the single-image call
            g1, f1, ax, ay = det.preprocess_image(im, target[0], target[1], want_f32=True)
            assert (ax, ay) == (adj[i, 0], adj[i, 1]), i
            assert np.array_equal(g1, gray[i]) and np.array_equal(f1[0, 0], fr[i, 0]), i


# 2 ------------------------------------------------------------------------------------------------------------------------------
def test_reference_pages_in_one_batch_equal_four_single_calls(det, golden_dir):
    pages = [np.array(Image.open(os.path.join(golden_dir, "text_det", n + ".jpg")).convert("RGBA")) for n in ("img224", "img55", "img494", "img545")]
    net = td.resnet18(W.pack_blob(W.make_det_weights(0)), 0)
    try:
        gray, adj = td.preprocess_images(net, pages, (800, 800))
    finally:
        net.close()
    assert gray.shape == (4, 800, 800) and adj.shape == (4, 2)
    for i, p in enumerate(pages):
        g1, ax, ay = det.preprocess_image(p, 800, 800)
        assert np.array_equal(gray[i], g1), i
        assert (adj[i, 0], adj[i, 1]) == (ax, ay), i


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_row_stride_is_passed_through_from_host_and_device_memory(det):
    import torch
    big = np.random.RandomState(3).randint(0, 256, (60, 80, 4)).astype(np.uint8)
    view = big[11:11 + 41, 7:7 + 53]            # 4 * 7 bytes into the row, 53 x 41 pixels, the parent's stride
    descs, kind, _ = capi.Detector._image_descs([view])
    assert (descs[0].w, descs[0].h, descs[0].stride_bytes, descs[0].rgba) == (53, 41, 320, big.ctypes.data + 11 * 320 + 28) and kind == capi.MEM_HOST
    wantg, _, wanta = det.preprocess_batch([np.ascontiguousarray(view)], 64, 32)
    assert np.array_equal(wantg, PB.preprocess_batch([view], 64, 32)[0])
    g, _, a = det.preprocess_batch([view], 64, 32)
    assert np.array_equal(g, wantg) and (a == wanta).all()
    big_d = torch.from_numpy(big).cuda()
    torch.cuda.synchronize()
    view_d = big_d[11:11 + 41, 7:7 + 53]
    descs, kind, _ = capi.Detector._image_descs([view_d])
    assert (descs[0].stride_bytes, descs[0].rgba) == (320, big_d.data_ptr() + 11 * 320 + 28) and kind == capi.MEM_DEVICE
    g, _, a = det.preprocess_batch([view_d], 64, 32)
    assert np.array_equal(g, wantg) and (a == wanta).all()
    # strides and pointers the ABI refuses
    out, adj = np.empty((1, 32, 64), np.uint8), np.zeros((1, 2))
    for stride, kind, ptr in ((4 * 53 - 4, capi.MEM_HOST, view.ctypes.data), (4 * 53 + 2, capi.MEM_HOST, view.ctypes.data),
                              (320, capi.MEM_DEVICE, view_d.data_ptr() + 2)):
        d = (capi.ImageDesc * 1)(capi.ImageDesc(ptr, 53, 41, stride))
        code, msg = raw_batch(det, d, 1, kind, 64, 32, out, None, capi.MEM_HOST, adj)
        assert code == 1 and "image 0" in msg, (stride, kind, code, msg)
    g, _, _ = det.preprocess_batch([view], 64, 32)
    assert np.array_equal(g, wantg)


# 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_dev,dst_dev", [(False, False), (False, True), (True, False), (True, True)], ids=["h2h", "h2d", "d2h", "d2d"])
def test_memory_kinds_give_identical_frames(det, src_dev, dst_dev):
    import torch
    imgs = images()
    ogray, oadj = want((64, 32))
    src = [torch.from_numpy(im).cuda() for im in imgs] if src_dev else imgs
    torch.cuda.synchronize()
    gray, fr, adj = det.preprocess_batch(src, 64, 32, want_u8=True, want_f32=True, device_out=dst_dev)
    if dst_dev:
        assert gray.is_cuda and fr.is_cuda
        gray, fr = gray.cpu().numpy(), fr.cpu().numpy()
    assert np.array_equal(gray, ogray) and np.array_equal(fr[:, 0], ogray.astype(np.float32)) and (adj == oadj).all()


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_reversing_the_batch_reverses_the_frames_and_nothing_else(det):
    ogray, oadj = want((64, 32))
    gray, _, adj = det.preprocess_batch(images()[::-1], 64, 32)
    assert np.array_equal(gray, ogray[::-1]) and (adj == oadj[::-1]).all()


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_chunked_staging(det):
    rng = np.random.RandomState(6)
    imgs = [rng.randint(0, 256, (300, 300, 4)).astype(np.uint8) for _ in range(7)]     # 360 000 bytes each: two to a chunk of 1 MiB
    wantg, wantf, wanta = det.preprocess_batch(imgs, 64, 64, want_f32=True)
    assert np.array_equal(wantg, PB.preprocess_batch(imgs, 64, 64)[0])
    small = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0, options="pre_stage_mb=1")
    try:
        g, f, a = small.preprocess_batch(imgs, 64, 64, want_f32=True)
        assert np.array_equal(g, wantg) and np.array_equal(f, wantf) and (a == wanta).all()
        one = rng.randint(0, 256, (600, 600, 4)).astype(np.uint8)                        # 1.44 MB: more than the budget
        g, _, a = small.preprocess_batch([imgs[0], one, imgs[1]], 64, 64)
        g2, _, a2 = det.preprocess_batch([imgs[0], one, imgs[1]], 64, 64)
        assert np.array_equal(g, g2) and (a == a2).all() and np.array_equal(g[1], PB.preprocess_batch([one], 64, 64)[0][0])
    finally:
        small.close()
    for bad in ("pre_stage_mb=0", "pre_stage_mb=5000"):
        with pytest.raises(capi.OcrError) as e:
            capi.Detector(W.pack_blob(W.make_det_weights(0)), 0, options=bad)
        assert e.value.code == 1 and "pre_stage_mb" in str(e.value)


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_async_frames_feed_the_forward_without_a_synchronise(det):
    import torch
    rng = np.random.RandomState(7)
    sizes = [(90, 70), (64, 64), (33, 200), (301, 150)]
    imgs = [torch.from_numpy(rng.randint(0, 256, (h, w, 4)).astype(np.uint8)).cuda() for w, h in sizes]
    more = [torch.from_numpy(rng.randint(0, 256, (h, w, 4)).astype(np.uint8)).cuda() for w, h in sizes[::-1]]
    _, frames, adj = det.preprocess_batch(imgs, 64, 64, want_u8=False, want_f32=True, device_out=True)
    _, frames2, adj2 = det.preprocess_batch(more, 64, 64, want_u8=False, want_f32=True, device_out=True)
    want_prob = torch.empty_like(frames)
    torch.cuda.synchronize()
    capi.check(capi.lib().ocr_det_forward(det._h, frames.data_ptr(), 4, 64, 64, want_prob.data_ptr(), capi.MEM_DEVICE))
    buf, prob = torch.empty_like(frames), torch.empty_like(frames)
    torch.cuda.synchronize()
    a = det.preprocess_batch_async(imgs, 64, 64, f32=buf)
    det.forward_device(buf.data_ptr(), 4, 64, 64, prob.data_ptr())
    det.synchronize()
    assert (a == adj).all()
    assert torch.equal(buf, frames) and torch.equal(prob, want_prob)
    assert bool(torch.isfinite(prob).all())
    # two calls back to back, different batches into different buffers, one synchronise: the plan buffers' event guard
    b1, b2 = torch.empty_like(frames), torch.empty_like(frames)
    g2 = torch.empty((4, 64, 64), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    a1 = det.preprocess_batch_async(imgs, 64, 64, f32=b1)
    a2 = det.preprocess_batch_async(more, 64, 64, gray=g2, f32=b2)
    det.synchronize()
    assert (a1 == adj).all() and (a2 == adj2).all()
    assert torch.equal(b1, frames) and torch.equal(b2, frames2) and torch.equal(g2.float(), frames2[:, 0])


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_beside_a_pending_pipelined_batch():
    import torch
    S = 128
    d = capi.Detector(W.pack_blob(W.make_det_weights_text()), 0)
    params = capi.default_params(skip_degenerate=True)
    x = torch.from_numpy(W.synth_text_pages(880, 2, S, S, dense=True)[0]).cuda()     # (dense: the grid that puts words on a 128 x 128 page)
    prob, prob_ref = torch.empty_like(x), torch.empty_like(x)
    torch.cuda.synchronize()
    imgs = images(5)[2:]
    try:
        assert d.detect_pipelined(x.data_ptr(), 2, S, S, prob_ref.data_ptr(), np.ones((2, 2)), params) is None
        ref = d.detect_pipelined(0, 0, 0, 0, 0)
        assert d.detect_pipelined(x.data_ptr(), 2, S, S, prob.data_ptr(), np.ones((2, 2)), params) is None
        gray, _, adj = d.preprocess_batch(imgs, 64, 32)
        got = d.detect_pipelined(0, 0, 0, 0, 0)
    finally:
        d.close()
    print("polygons of the pending batch:", [len(p) for p in ref[0]])
    assert got == ref and len(ref[0]) == 2 and sum(len(p) for p in ref[0]) > 0
    assert torch.equal(prob, prob_ref)
    ogray, oadj = want((64, 32))
    assert np.array_equal(gray, ogray[2:5]) and (adj == oadj[2:5]).all()


# 9 ------------------------------------------------------------------------------------------------------------------------------
def test_arguments(det):
    import torch
    imgs = images(3)
    ogray, oadj = want((64, 32))
    good, _, _ = capi.Detector._image_descs(imgs)
    out, outf, adj = np.empty((3, 32, 64), np.uint8), np.empty((3, 1, 32, 64), np.float32), np.zeros((3, 2))
    H, D = capi.MEM_HOST, capi.MEM_DEVICE

    def descs(i, **kw):
        d = (capi.ImageDesc * 3)(*[capi.ImageDesc(g.rgba, g.w, g.h, g.stride_bytes) for g in good])
        for k, v in kw.items():
            setattr(d[i], k, v)
        return d

    dev = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    cases = [  # (what, args of raw_batch, index the message must name or None)
        ("null det", (None, good, 3, H, 64, 32, out, None, H, adj), None),
        ("null images", (det, None, 3, H, 64, 32, out, None, H, adj), None),
        ("null adj", (det, good, 3, H, 64, 32, out, None, H, None), None),
        ("both outputs null", (det, good, 3, H, 64, 32, None, None, H, adj), None),
        ("n < 0", (det, good, -1, H, 64, 32, out, None, H, adj), None),
        ("null pixels", (det, descs(1, rgba=None), 3, H, 64, 32, out, None, H, adj), 1),
        ("w = 0", (det, descs(2, w=0), 3, H, 64, 32, out, None, H, adj), 2),
        ("w = 16385", (det, descs(0, w=16385), 3, H, 64, 32, out, None, H, adj), 0),
        ("h = 0", (det, descs(1, h=0), 3, H, 64, 32, out, None, H, adj), 1),
        ("h = 16385", (det, descs(1, h=16385), 3, H, 64, 32, out, None, H, adj), 1),
        ("stride below 4 w", (det, descs(2, stride_bytes=4 * 64 - 4), 3, H, 64, 32, out, None, H, adj), 2),
        ("stride not a multiple of 4", (det, descs(2, stride_bytes=4 * 64 + 6), 3, H, 64, 32, out, None, H, adj), 2),
        ("negative stride", (det, descs(0, stride_bytes=-12), 3, H, 64, 32, out, None, H, adj), 0),
        ("target w = 0", (det, good, 3, H, 0, 32, out, None, H, adj), None),
        ("target h = 0", (det, good, 3, H, 64, 0, out, None, H, adj), None),
        ("src kind", (det, good, 3, 2, 64, 32, out, None, H, adj), None),
        ("dst kind", (det, good, 3, H, 64, 32, out, None, -1, adj), None),
        ("misaligned device source", (det, descs(1, rgba=dev.data_ptr() + 2, w=2, h=2, stride_bytes=0), 3, D, 64, 32, out, None, H, adj), 1),
    ]
    for what, args, idx in cases:
        code, msg = raw_batch(*args)
        assert code == 1 and msg, (what, code, msg)
        if idx is not None:
            assert f"image {idx}" in msg, (what, msg)
        g, f, a = det.preprocess_batch(imgs, 64, 32, want_f32=True)      # the handle stays usable
        assert np.array_equal(g, ogray[:3]) and np.array_equal(f[:, 0], ogray[:3].astype(np.float32)) and (a == oadj[:3]).all(), what
    # the async form refuses the same
    code = capi.lib().ocr_preprocess_batch_async(det._h, descs(1, w=0), 3, 64, 32, None, dev.data_ptr(), adj.ctypes.data_as(C.POINTER(C.c_double)))
    assert code == 1 and "image 1" in capi.lib().ocr_last_error().decode()
    code = capi.lib().ocr_preprocess_batch_async(det._h, good, 3, 64, 32, None, None, adj.ctypes.data_as(C.POINTER(C.c_double)))
    assert code == 1
    # n = 0: OCR_OK, outputs untouched
    out[:], outf[:], adj[:] = 77, 5.0, -1.0
    assert raw_batch(det, good, 0, H, 64, 32, out, outf, H, adj) == (0, "")
    assert (out == 77).all() and (outf == 5.0).all() and (adj == -1.0).all()
    g, f, a = det.preprocess_batch([], 64, 32, want_f32=True)
    assert g.shape == (0, 32, 64) and f.shape == (0, 1, 32, 64) and a.shape == (0, 2)
