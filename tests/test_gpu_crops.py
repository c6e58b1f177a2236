"""ocr_extract_crops (crops.hip crop_kernel + api.hip crop_boxes) through its own entry point, held to oracle/crop_oracle.py BIT FOR BIT
(uint32 views: -0.0 is not +0.0) on the hand-written cases of tests/crop_cases.py - which tests/test_crop_cases.py shows to reach the
frame borders, the one-pixel widening, polygons off the frame, non-integer boxes, tiny / wide / tall frames, empty images in a batch and
the grid sizes 1, 255, 256, 257, 1025.  Both memory forms, with guard rows around the crops; the device form reads its frames from
inside a block of NaN, so a tap in front of or behind the frame block shows as a NaN crop.  Then a caller-set stream, permuted polygons,
empty blocks, every refused call (nothing written, the handle still works), non-finite adjust values, and a frame block past 2^31 bytes.
No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from ocr_rs_amd import weights as W
from oracle import crop_oracle as CR
from tests import crop_cases as CC

pytestmark = pytest.mark.gpu
NAMES = CC.case_names()
SENT = 0xDEADBEEF            # the bit pattern of every float the call must not write
SENT_I32 = SENT - (1 << 32)


@pytest.fixture(scope="module")
def det():
    d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    yield d
    d.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _block(polys):
    return capi.python_to_polygons(polys, [[0.0] * len(p) for p in polys])


def _adj_p(adj):
    return adj.ctypes.data_as(C.POINTER(C.c_double))


def _host(det, fr, polys, adj):
    """the host form into rows 1..P of a (P + 2) x 784 buffer of SENT; returns the whole buffer as uint32"""
    n, _, h, w = fr.shape
    st, keep = _block(polys)
    buf = np.full((st.n_polygons + 2, 784), SENT, np.uint32)
    capi.check(capi.lib().ocr_extract_crops(det._h, fr.ctypes.data, n, h, w, capi.MEM_HOST, C.byref(st), _adj_p(adj), buf[1:].ctypes.data))
    return buf


def _device(det, fr, polys, adj):
    """the device form: frames inside a block of NaN, crops into rows 1..P of a (P + 2) x 784 buffer of SENT"""
    import torch
    n, _, h, w = fr.shape
    st, keep = _block(polys)
    guard = 2 * w + 64
    block = torch.full((fr.size + 2 * guard,), float("nan"), dtype=torch.float32, device="cuda")
    block[guard:guard + fr.size] = torch.from_numpy(fr.reshape(-1)).cuda()
    buf = torch.full((st.n_polygons + 2, 784), SENT_I32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    capi.check(capi.lib().ocr_extract_crops(det._h, block.data_ptr() + 4 * guard, n, h, w, capi.MEM_DEVICE, C.byref(st), _adj_p(adj),
                                            buf.data_ptr() + 4 * 784))
    assert torch.isnan(block[:guard]).all() and torch.isnan(block[guard + fr.size:]).all()
    return buf.cpu().numpy().view(np.uint32)


def _assert_rows(buf, want, tag):
    assert (buf[0] == SENT).all() and (buf[-1] == SENT).all(), (tag, "guard rows")
    assert buf.shape[0] == want.shape[0] + 2 and np.array_equal(buf[1:-1], _bits(want)), tag


@pytest.mark.parametrize("name", NAMES)
def test_host_form_equals_the_oracle(det, name):
    _, fr, polys, adj = CC.case(name)
    _assert_rows(_host(det, fr, polys, adj), CC.oracle_crops(name), name)


@pytest.mark.parametrize("name", NAMES)
def test_device_form_writes_rows_1_to_p_only(det, name):
    _, fr, polys, adj = CC.case(name)
    dev = _device(det, fr, polys, adj)
    _assert_rows(dev, CC.oracle_crops(name), name)
    assert np.array_equal(dev, _host(det, fr, polys, adj)), name


def test_constant_frames_and_ramps(det):
    got = _host(det, *CC.case("constant and ramp/constant 137")[1:])[1:-1]
    assert (got == _bits(np.float32(137.0) / np.float32(255.0))).all()
    x = _host(det, *CC.case("constant and ramp/v = x")[1:])[1:-1].view(np.float32).reshape(-1, 28, 28)
    y = _host(det, *CC.case("constant and ramp/v = y")[1:])[1:-1].view(np.float32).reshape(-1, 28, 28)
    assert (np.diff(x, axis=2) >= 0).all() and (x == x[:, :1, :]).all()
    assert (np.diff(y, axis=1) >= 0).all() and (y == y[:, :, :1]).all()


def test_caller_set_stream(det):
    import torch
    name = "borders/37x53"
    _, fr, polys, adj = CC.case(name)
    stream = torch.cuda.Stream()
    det.set_stream(stream.cuda_stream)
    try:
        _assert_rows(_host(det, fr, polys, adj), CC.oracle_crops(name), "host form on a caller-set stream")
        _assert_rows(_device(det, fr, polys, adj), CC.oracle_crops(name), "device form on a caller-set stream")
    finally:
        det.set_stream(None)
    _assert_rows(_host(det, fr, polys, adj), CC.oracle_crops(name), "back on the handle's own stream")


def test_permuted_polygons_permute_the_crops(det):
    _, fr, polys, adj = CC.case("batch/4 x 24x32")
    k = len(polys[1])
    base = _host(det, fr, polys, adj)[1:-1]
    perm = [2, 0, 3, 1]
    got = _host(det, fr, [[], [polys[1][i] for i in perm], [], polys[3]], adj)[1:-1]
    assert np.array_equal(got[:k], base[:k][perm]) and np.array_equal(got[k:], base[k:])
    # each image alone, as a batch of one: no image's crops depend on another's
    for img, rows in ((1, slice(0, k)), (3, slice(k, 2 * k))):
        alone = _host(det, np.ascontiguousarray(fr[img:img + 1]), [polys[img]], np.ascontiguousarray(adj[img:img + 1]))[1:-1]
        assert np.array_equal(alone, base[rows]), img


def test_empty_blocks_write_nothing(det):
    import torch
    L = capi.lib()
    fr = CC.case("batch/4 x 24x32")[1]
    adj = np.ones((4, 2))
    dfr = torch.from_numpy(fr).cuda()
    dbuf = torch.full((2, 784), SENT_I32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for n, polys in ((4, [[], [], [], []]), (0, [])):
        st, keep = _block(polys)
        assert st.n_polygons == 0 and st.n_images == n
        buf = np.full((2, 784), SENT, np.uint32)
        assert L.ocr_extract_crops(det._h, fr.ctypes.data, n, 24, 32, capi.MEM_HOST, C.byref(st), _adj_p(adj), buf.ctypes.data) == 0
        assert L.ocr_extract_crops(det._h, fr.ctypes.data, n, 24, 32, capi.MEM_HOST, C.byref(st), _adj_p(adj), None) == 0
        assert L.ocr_extract_crops(det._h, dfr.data_ptr(), n, 24, 32, capi.MEM_DEVICE, C.byref(st), _adj_p(adj), dbuf.data_ptr()) == 0
        assert (buf == SENT).all() and (dbuf.cpu().numpy().view(np.uint32) == SENT).all()


def test_refused_calls_write_nothing_and_leave_the_handle_usable(det):
    L = capi.lib()
    name = "borders/37x53"
    _, fr, polys, adj = CC.case(name)
    st, keep = _block(polys)
    two, keep2 = _block([polys[0], []])                       # a block of two images
    neg = capi.Polygons(-1, st.n_polygons, st.n_vertices, st.img_offsets, st.poly_offsets, st.xy, st.scores)
    buf = np.full((st.n_polygons, 784), SENT, np.uint32)

    def call(*, d=det._h, f=fr.ctypes.data, n=1, h=37, w=53, mk=capi.MEM_HOST, p=C.byref(st), a=_adj_p(adj), c=buf.ctypes.data):
        return L.ocr_extract_crops(d, f, n, h, w, mk, p, a, c)

    refused = [dict(d=None), dict(f=None), dict(p=None), dict(a=None), dict(c=None),                     # each null pointer
               dict(mk=7), dict(mk=2), dict(mk=-1),
               dict(n=2), dict(n=0), dict(p=C.byref(two)),                                               # polys->n_images != n
               dict(n=-1), dict(n=-1, p=C.byref(neg)),                                                   # n < 0, whatever the block says
               dict(h=0), dict(h=-5), dict(w=0), dict(w=-1), dict(h=0, w=0),
               dict(h=(1 << 24) + 1), dict(w=(1 << 24) + 1)]                                             # beyond what an f32 position can address
    for kw in refused:
        assert call(**kw) == 1, kw                                                                       # OCR_ERR_INVALID
        assert L.ocr_last_error(), kw
        assert (buf == SENT).all(), kw
        _assert_rows(_host(det, fr, polys, adj), CC.oracle_crops(name), ("after", kw))
    assert call() == 0 and np.array_equal(buf, _bits(CC.oracle_crops(name)))


def test_non_finite_adjust_values_stay_inside_the_frame(det):
    for name, fr, polys, adj, boxes in CC.nonfinite_cases():
        want = CR.extract_crops(fr, polys, adj)
        assert np.isfinite(want).all()
        _assert_rows(_host(det, fr, polys, adj), want, name)
        _assert_rows(_device(det, fr, polys, adj), want, name)      # (a tap off the frame block would have read a NaN)


def test_frame_block_past_2_31_bytes(det):
    """129 frames of 2048 x 2048 f32: frame 128 starts 2^31 bytes into the block.  The same polygons on frames 0 and 128 (the others
    hold none and are never read); the oracle sees those two frames as a batch of two."""
    import torch
    n, h, w = 129, 2048, 2048
    two = np.random.default_rng(60).integers(0, 256, size=(2, 1, h, w)).astype(np.float32)
    pl = [CC.rect(2000, 2010, 2047, 2047), CC.rect(0, 0, 30, 9), CC.rect(1000, 3, 1003, 2040), CC.point(2047, 2047)]
    want = CR.extract_crops(two, [pl, pl], np.ones((2, 2)))
    assert not np.array_equal(want[:4], want[4:])
    block = torch.empty((n, 1, h, w), dtype=torch.float32, device="cuda")
    assert block.numel() * 4 > 1 << 31 and 128 * h * w * 4 == 1 << 31
    block[0] = torch.from_numpy(two[0]).cuda()
    block[128] = torch.from_numpy(two[1]).cuda()
    st, keep = _block([pl] + [[]] * 127 + [pl])
    buf = torch.full((10, 784), SENT_I32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    capi.check(capi.lib().ocr_extract_crops(det._h, block.data_ptr(), n, h, w, capi.MEM_DEVICE, C.byref(st), _adj_p(np.ones((n, 2))),
                                            buf.data_ptr() + 4 * 784))
    _assert_rows(buf.cpu().numpy().view(np.uint32), want, "frame 128")
