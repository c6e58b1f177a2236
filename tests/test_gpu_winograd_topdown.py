"""winograd43_input_up2_kernel (winograd.hip): out4's F(4x4) input transform with the FPN's top-down add made on load, d = up2(low) + x, as
the engine launches it under option top_side - through ocr_test_winograd_topdown, which places x and low between
NaN regions of one allocation each and returns V.

The check is exact equality of V, bit for bit, with the existing input transform (winograd43_input_kernel through launch_winograd_input)
applied to the sum computed on the host, low.repeat(2, 2) + x: one f32 add per element on the same two operands, which is what conv_igemm's
epilogue stored into sum_[2] before.  The existing Winograd hook (ocr_test_winograd_run) returns the conv's output, not V, and takes Cin in
multiples of 32 only, so the existing transform is reached through the same new hook with low = None: it then calls launch_winograd_input.
No tolerance anywhere.  Taps outside the image must come out as 0 + 0 whatever surrounds the tensors (NaN here), and nothing is written
behind V."""
import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from ocr_rs_amd import weights as W

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 4, 4), (2, 6, 10, 8), (2, 10, 14, 256), (3, 40, 40, 256)]   # (N, H, W, C); 6 x 10: ragged tiles both ways; the last: out4 at the bench size


@pytest.fixture(scope="module")
def det():
    d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    yield d
    d.close()


def _check(det, x, low):
    sentinel = np.float32(-7.0)
    host_sum = (np.repeat(np.repeat(low, 2, axis=1), 2, axis=2) + x).astype(np.float32)   # f32 + f32, rounded once
    got, guard = det.debug_winograd_topdown(x, low)
    want, guard0 = det.debug_winograd_topdown(host_sum)
    assert (guard == sentinel).all() and (guard0 == sentinel).all(), "a launch wrote behind V"
    assert not np.isnan(want).any() and not np.isnan(got).any(), "a tap outside the image read its surroundings"
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))   # ... and the signs of the zeros: the same operations on the same bits
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_topdown_transform_equals_the_transform_of_the_host_sum(det, shape):
    n, h, w, c = shape
    rng = np.random.default_rng(h * 1000 + w * 10 + c)
    x = rng.standard_normal((n, h, w, c)).astype(np.float32)
    low = rng.standard_normal((n, h // 2, w // 2, c)).astype(np.float32)
    v = _check(det, x, low)
    assert np.abs(v).max() > 1.0      # (not a transform of nothing)


def test_negative_zero_and_denormals_in_both_operands(det):
    n, h, w, c = 2, 6, 10, 8
    rng = np.random.default_rng(7)
    tiny = np.float32(1e-41)          # denormal
    pool = np.array([-0.0, 0.0, tiny, -tiny, 3 * tiny, np.float32(1.17549435e-38), 1.0, -1.0], np.float32)
    x = pool[rng.integers(0, len(pool), size=(n, h, w, c))]
    low = pool[rng.integers(0, len(pool), size=(n, h // 2, w // 2, c))]
    x[0, 0, 0, :] = -0.0
    low[0, 0, 0, :] = -0.0            # -0 + -0 = -0 in the first patch
    _check(det, x, low)


def test_refused_shapes(det):
    x = np.zeros((1, 5, 4, 4), np.float32)
    with pytest.raises(capi.OcrError):
        det.debug_winograd_topdown(x, np.zeros((1, 2, 2, 4), np.float32))     # H odd: no half-resolution partner
    with pytest.raises(capi.OcrError):
        det.debug_winograd_topdown(np.zeros((1, 4, 4, 6), np.float32), np.zeros((1, 2, 2, 6), np.float32))   # C no multiple of 4
