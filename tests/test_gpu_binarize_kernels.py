"""Kernel-level tests of the two-kernel head's second half and of the binarisers (stem_tail.hip's convt2_sigmoid_kernel,
binarize_kernel, binarize_pack_kernel - the bit packer feeds the host contour tracer) through the ocr_test_convt2_sigmoid /
ocr_test_binarize / ocr_test_binarize_pack hooks: one call of the shipped launcher each, the source between two leads (zeros, quiet NaN
or +inf), the outputs with guard rows / bytes / words behind them.

B1  binarize_pack: every image packed on its own, bit i & 31 of word i >> 5, padded with zero bits to whole 64-bit words, at px % 64 = 0,
    1, 63 and across the 1024-block cap; thresh itself is 0, its successor 1, NaN 0, +inf 1; a +inf lead or a neighbour's first pixels
    must not reach an image's last word.
B2  binarize: the same values at the block edges and across the 4096-block cap.
B3  convt2_sigmoid: integer logits from one-hot inputs, distinct across the four taps - placement and the sigmoid within 4 ulps, the bitmap
    equal to prob > thresh, up to a grid-stride sweep past the 8192-block cap."""
import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from ocr_rs_amd import weights as W

pytestmark = pytest.mark.gpu

THRESH = np.float32(0.6)


@pytest.fixture(scope="module")
def det():
    d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    yield d
    d.close()


def _planted(shape, seed):
    """random probabilities with, at random places of every row, thresh itself (-> 0), the next float above (-> 1) and below (-> 0), NaN
    (-> 0), +inf (-> 1), -inf, -0.0 and 0.0; a row's first 64 values are above thresh wherever they were not planted, so that a read
    past the end of the row in front would show"""
    rng = np.random.default_rng(seed)
    p = rng.random(shape, dtype=np.float32).reshape(shape[0] if len(shape) > 1 else 1, -1)
    p[:, :64] = np.float32(0.9)
    special = np.array([THRESH, np.nextafter(THRESH, np.float32(1)), np.nextafter(THRESH, np.float32(0)), np.nan, np.inf, -np.inf, -0.0, 0.0], np.float32)
    want = np.array([0, 1, 0, 0, 1, 0, 0, 0], np.uint8)
    px = p.shape[1]
    for row in p:
        at = rng.integers(0, px, max(8, px // 16))
        row[at] = special[np.arange(at.size) % 8]
        row[px - 1] = special[1 + 3 * (px % 2)]       # the last pixel is a 1: the tail's own bit is not the padding's value
    with np.errstate(invalid="ignore"):
        bits = (p > THRESH).astype(np.uint8)
    assert np.array_equal((special > THRESH).astype(np.uint8), want)
    return p.reshape(shape), bits.reshape(shape)


# px % 64 = 1, 63, 0, 1; a whole block of 256 and one pixel either side; one sweep of the 1024-block cap (262 144 pixels) + a 65-pixel tail
@pytest.mark.parametrize("n_images", [1, 3])
@pytest.mark.parametrize("px", [1, 63, 64, 65, 255, 256, 257, 262209])
def test_binarize_pack_packs_every_image_on_its_own(det, px, n_images):
    prob, bits = _planted((n_images, px), seed=px + n_images)
    w64 = (px + 63) // 64
    want = np.zeros((n_images, w64 * 8), np.uint8)
    for i in range(n_images):
        b = np.packbits(bits[i], bitorder="little")
        want[i, :b.size] = b
    want = want.view(np.uint32)
    assert all(int(want[i, (px - 1) >> 5]) >> ((px - 1) & 31) == 1 for i in range(n_images))      # the last pixel's bit is set, none above it
    for poison in (0, 1, 2):
        words, guard = det.debug_binarize_pack(prob, THRESH, poison=poison)
        assert np.array_equal(guard, np.full_like(guard, 0xA5A5A5A5)), ("words behind the bit images were written", poison)
        assert np.array_equal(words, want), (poison, np.argwhere(words != want)[:4])


# one pixel; a block but one; a block and one; one sweep of the 4096-block cap (4096 x 256 pixels) + one pixel
@pytest.mark.parametrize("n", [1, 255, 257, 1048577])
def test_binarize_compares_every_pixel_once(det, n):
    prob, bits = _planted((n,), seed=n)
    for poison in (0, 1, 2):
        got, guard = det.debug_binarize(prob, THRESH, poison=poison)
        assert np.array_equal(guard, np.full_like(guard, 9)), ("bytes behind the bitmap were written", poison)
        assert np.array_equal(got, bits), (poison, np.argwhere(got != bits)[:4])


def _convt2_case(n, h2, w2):
    """pixel (n, i, j) has the single input 1.0 at channel k (a hash of its position); w4x64[t][k] = (k + 4 t) % 16 - 8: the four taps of a
    pixel are four different integers, in an arrangement that differs between neighbours; + bias 1: logits -7 .. 8, exact in f32"""
    ni, ii, jj = np.meshgrid(np.arange(n), np.arange(h2), np.arange(w2), indexing="ij")
    k = (jj + 5 * ii + 7 * (jj // 64) + 11 * ni) % 64
    x = np.zeros((n, h2, w2, 64), np.float32)
    np.put_along_axis(x, k[..., None], 1.0, axis=3)
    w = ((np.arange(64)[None, :] + 4 * np.arange(4)[:, None]) % 16 - 8).astype(np.float32)
    z = w[:, k].astype(np.float64) + 1.0                          # [t][n][i][j]
    want = np.zeros((n, 2 * h2, 2 * w2))
    for a in range(2):
        for b in range(2):
            want[:, a::2, b::2] = 1.0 / (1.0 + np.exp(-z[2 * a + b]))
    return x, w, 1.0, want


# one row of the smallest legal width; two images; an odd height; 131 584 pixels: past the cap of 8192 blocks of 16 pixels (131 072)
@pytest.mark.parametrize("shape", [(1, 1, 4), (2, 3, 12), (1, 5, 8), (1, 257, 512)], ids=lambda s: "x".join(map(str, s)))
def test_convt2_sigmoid_places_every_tap_and_pixel(det, shape):
    x, w, bias, want = _convt2_case(*shape)
    assert len(set(want[0, :2, :2].ravel())) == 4
    prob, bm, gp, gb = det.debug_convt2_sigmoid(x, w, bias, 0.5)
    assert np.array_equal(gp, np.full_like(gp, -7.0)) and np.array_equal(gb, np.full_like(gb, 9)), "rows behind prob or the bitmap were written"
    # expf is within 1 ulp, then one add and one divide: 4 ulps of p
    ulps = np.abs(prob.astype(np.float64) - want) / np.spacing(want.astype(np.float32)).astype(np.float64)
    assert ulps.max() <= 4, (float(ulps.max()), np.argwhere(ulps > 4)[:4])
    assert np.array_equal(bm, (prob > np.float32(0.5)).astype(np.uint8))
    assert bm.any() and not bm.all()
    for poison in (1, 2):
        p2, b2, gp2, gb2 = det.debug_convt2_sigmoid(x, w, bias, 0.5, poison=poison)
        assert np.array_equal(gp2, gp) and np.array_equal(gb2, gb)
        assert np.array_equal(p2.view(np.uint32), prob.view(np.uint32)) and np.array_equal(b2, bm), poison
    p3, none, gp3, none2 = det.debug_convt2_sigmoid(x, w, bias, 0.5, want_bitmap=False, poison=1)
    assert none is None and none2 is None and np.array_equal(p3.view(np.uint32), prob.view(np.uint32)) and np.array_equal(gp3, gp)


def test_convt2_sigmoid_refuses_a_width_it_cannot_vectorise(det):
    x, w, bias, _ = _convt2_case(1, 2, 6)
    with pytest.raises(capi.OcrError):
        det.debug_convt2_sigmoid(x, w, bias, 0.5)
