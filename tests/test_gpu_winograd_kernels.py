"""Kernel-level tests of the Winograd convs of the detector's trunk - winograd43_fused_kernel<4|8|16> (layer1, layer2, the FPN's lateral terms,
bin_conv1.p2, out4 with out4_fused=1) and the three-launch form (winograd43_input_kernel, the 36 batched split-bf16 conv_igemm GEMMs over
cw.wino_x3, winograd43_output_kernel: layer3, layer4, out4, out5) - through ocr_test_winograd_run: ONE launch, or the engine's three, on
caller data.  Cases, references and every assertion live in tests/winograd_oracle.py, where tests/test_winograd_oracle.py runs the same
assertions against a numpy model of the kernels and shows that seven kinds of deliberately wrong model each fail one of them.

Forms: 0 launch_winograd43_fused, 1 three launches with the split-bf16 GEMMs AS THE ENGINE RUNS THEM (launch_winograd_gemm), 2 three launches
with the exact-f32 GEMMs, 3 three launches of F(2x2,3x3) (the non-default winograd43= setting; W1 and W3 only).

W1 equality   integer families (small-integer activations, weights 576 k, power-of-two scales, integer bias and residual): every value of the
              F(4x4) pipeline is an integer below 2^24, so the result must EQUAL the int64 direct conv, element for element, for every
              epilogue of the graph (none, scale + bias, residual, in-place residual) with ReLU on and off
W2 the walk   the fused kernel over 18 pixel blocks with num_cus 1, 2, 3, 4, 8, 9, 40: linear order with up to nine blocks per workgroup and
              the next block's patch in flight, per-XCD runs with a remainder (18 = 8 x 2 + 2), a grid clipped to the block count - equal to
              the reference on integers, and bit-identical to each other on real values
W3 poison     NaN in front of and behind the source inside its allocation: still equal, no NaN, every guard row behind the output untouched
              (the guard rows are asserted for EVERY launch of this file); one ragged case, then H and W one past a block and a tile edge
W4 rms        real-valued families relu(N(0,1)) and 0.1 N(0,1) + 3: rms(kernel - f64) <= sqrt(rms_six x min rms_five) in units of the
              Winograd-domain norm (docs/split_bf16_error.md), the largest element within 10 x the CPU emulation's, forms 1 and 2 apart by no
              more than the same bar"""
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from ocr_rs_amd import weights as W
from tests import winograd_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    yield d
    d.close()


def _ids(v):
    return "x".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


FUSED_SHAPES = [(3, 1, 1), (1, 4, 4), (2, 15, 17), (1, 16, 16), (2, 17, 33), (1, 33, 17), (1, 5, 40)]
FUSED_PAIRS = [(64, 64), (64, 128), (128, 64), (128, 128), (256, 64), (256, 128), (128, 192), (64, 256)]
# T = the F(4x4) tiles = the GEMM rows per component: 1, 6, 18, 54, and 135 - a partial second 128-row tile, none may span two of the 36 problems
THREE_SHAPES = [(1, 1, 1), (3, 3, 5), (1, 9, 21), (3, 9, 21), (3, 17, 33)]
THREE_PAIRS = [(256, 64), (256, 256), (512, 512)]      # both tile shapes of the split-bf16 GEMM


@pytest.mark.parametrize("pair", FUSED_PAIRS, ids=_ids)
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=_ids)
def test_w1_fused_kernel_equals_the_direct_conv(det, shape, pair):
    O.check_w1(det.debug_winograd_run, O.FUSED, shape, *pair)


@pytest.mark.parametrize("form", [O.SPLIT3, O.F32_3, O.F22])
@pytest.mark.parametrize("pair", THREE_PAIRS, ids=_ids)
@pytest.mark.parametrize("shape", THREE_SHAPES, ids=_ids)
def test_w1_three_launch_form_equals_the_direct_conv(det, shape, pair, form):
    O.check_w1(det.debug_winograd_run, form, shape, *pair)


@pytest.mark.parametrize("pair", [(64, 64), (128, 128)], ids=_ids)
def test_w2_fused_kernel_gives_the_same_bits_under_every_grid(det, pair):
    O.check_w2(det.debug_winograd_run, *pair)


def _w3_cases():
    return [(form, shape, pair) for form in (O.FUSED, O.SPLIT3, O.F32_3, O.F22) for shape in O.w3_shapes(form)
            for pair in (((64, 64), (128, 128), (256, 64)) if form == O.FUSED else ((256, 64), (512, 512)))]


@pytest.mark.parametrize("form,shape,pair", _w3_cases(), ids=_ids)
def test_w3_nothing_around_the_source_is_used_and_nothing_behind_the_output_written(det, form, shape, pair):
    O.check_w3(det.debug_winograd_run, form, shape, *pair)


@pytest.mark.parametrize("family", O.W4_FAMILIES)
@pytest.mark.parametrize("forms,cin,cout,shape", O.W4_CASES, ids=_ids)
def test_w4_rms_error_stays_under_the_lost_product_bar(det, forms, cin, cout, shape, family):
    O.check_w4(det.debug_winograd_run, forms, cin, cout, shape, family)


def test_refused_shapes(det):
    """what the launchers refuse comes back as an error, not as a launch"""
    case = O.integer_case((1, 4, 4), 64, 64)
    with pytest.raises(capi.OcrError):
        det.debug_winograd_run(O.FUSED, case.x[..., :32], case.w[:, :, :32])       # the fused kernel takes Cin 64, 128, 256
    with pytest.raises(capi.OcrError):
        det.debug_winograd_run(O.SPLIT3, case.x[..., :48], case.w[:, :, :48])      # the split-bf16 GEMMs take Cin in multiples of 32
    with pytest.raises(capi.OcrError):
        det.debug_winograd_run(4, case.x, case.w)
