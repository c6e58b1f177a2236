"""Kernel-level tests of the trunk convs of the bf16 precision - conv3x3_bf16_c64_kernel (layer1's convs as single launches, the p2 lateral
term), basic_block_bf16_c64_kernel (layer1's blocks as one launch) and conv_igemm with bf16 operands and results (layer2-4 with the tap-sharing
loop, the stride-2 convs, the downsamples, the laterals) - through ocr_test_bf16_trunk_run: ONE launch on caller data, the source between two
lead regions of one allocation, guard rows behind every output.  Cases, references and every assertion live in tests/bf16_conv_oracle.py, where
tests/test_bf16_conv_oracle.py runs the same assertions against a numpy model of the kernels and shows that nine kinds of deliberately wrong
model each fail them.

Forms: 0 launch_conv3x3_bf16_c64 (grid 2 x num_cus), 1 launch_basic_block_bf16_c64 (grid num_cus), 2 launch_conv_igemm with in_bf16 = out_bf16 = 1.

B1 equality   integer families (small signed or non-negative integer activations, small integer weights, scales 1/4, 1/2, 1, integer bias and
              residuals): products of bf16 values are exact in f32 and every partial sum stays below 2^24 quanta, so the only rounding is the
              one f32 -> bf16 conversion of the output (in the block: and of the intermediate) and the result must EQUAL the reference
              int64-exact conv -> fma(acc, scale, bias) -> + residual -> ReLU -> round to nearest even, element for element, for every
              epilogue of the graph (none, scale + bias, + residual) with ReLU on and off.  Every case has outputs beyond 256, exact ties of the
              rounding and a quarter of its outputs behind ReLU
B2 the walk   forms 0 and 1 over 60 blocks with num_cus 1, 2, 3, 8, 16, 29, 64: up to thirty blocks per workgroup with the next patch (and the
              residual) in flight, the block kernel's per-XCD runs, a grid clipped to the block count - equal to the reference on integers with a
              residual and without, and bit-identical to each other on real values
B3 poison     NaN in front of and behind the source inside its allocation: still equal, no NaN, every guard row behind every output untouched
              (the guard rows are asserted for EVERY launch of this file); image 1 of a 3-image batch all NaN: images 0 and 2 as from the
              clean batch, bit for bit
B4 real       relu(N(0,1)) activations, N(0,1) / sqrt(K) weights.  Every element lies within an a-priori bound of the f64 value - the f32
              summation bound plus half a bf16 step; for the block plus what the elements of its bf16 intermediate that sit on a rounding
              boundary may move it.  Every element is the f64 reference rounded once to bf16 or one of its two bf16 neighbours: all of them in
              the cases of forms 0 and 2 whose residual cancels the sum down to 2^-7, those above 2^10 x the bound in the natural cases and the
              block.  The share of elements that differ stays under 2 x the share of a CPU emulation of the same case
              (docs/split_bf16_error.md, "The bf16 trunk against f64")"""
import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from ocr_rs_amd import weights as W
from tests import bf16_conv_oracle as O

pytestmark = pytest.mark.gpu
INVALID = 1      # OCR_ERR_INVALID (include/ocr_amd.h)


@pytest.fixture(scope="module")
def det():
    d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    yield d
    d.close()


def _ids(v):
    return "-".join(_ids(e) for e in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("family", O.FAMILIES)
@pytest.mark.parametrize("shape", O.C64_SHAPES, ids=_ids)
@pytest.mark.parametrize("form", [O.C64, O.BLOCK])
def test_b1_c64_kernels_equal_the_reference(det, form, shape, family):
    O.check_b1(det.debug_bf16_trunk_run, form, O.c64_spec(shape), family)


@pytest.mark.parametrize("family", O.FAMILIES)
@pytest.mark.parametrize("spec", O.IGEMM_SPECS, ids=_ids)
def test_b1_conv_igemm_equals_the_reference(det, spec, family):
    O.check_b1(det.debug_bf16_trunk_run, O.IGEMM, spec, family)


@pytest.mark.parametrize("form", [O.C64, O.BLOCK])
def test_b2_the_walk_gives_the_reference_and_the_same_bits_under_every_grid(det, form):
    O.check_b2(det.debug_bf16_trunk_run, form)


@pytest.mark.parametrize("form,spec", [(form, spec) for form, specs in sorted(O.B3_SPECS.items()) for spec in specs], ids=_ids)
def test_b3_nothing_around_the_source_is_used_and_nothing_behind_the_outputs_written(det, form, spec):
    O.check_b3_poison(det.debug_bf16_trunk_run, form, spec)


@pytest.mark.parametrize("form,spec", [(form, spec) for form, specs in sorted(O.B3_BATCH_SPECS.items()) for spec in specs], ids=_ids)
def test_b3_a_nan_image_leaves_its_neighbours_in_the_batch_alone(det, form, spec):
    O.check_b3_batch(det.debug_bf16_trunk_run, form, spec)


@pytest.mark.parametrize("form,spec", [(form, spec) for form, specs in sorted(O.B4_SPECS.items()) for spec in specs], ids=_ids)
def test_b4_real_values_stay_next_to_the_f64_reference(det, form, spec):
    O.check_b4(det.debug_bf16_trunk_run, form, spec)


@pytest.mark.parametrize("form,spec", [(form, spec) for form, specs in sorted(O.B4_NATURAL_SPECS.items()) for spec in specs], ids=_ids)
def test_b4_natural_magnitudes_under_relu_stay_within_the_bound(det, form, spec):
    O.check_b4_natural(det.debug_bf16_trunk_run, form, spec)


def test_refused_shapes(det):
    """what cannot run comes back as OCR_ERR_INVALID, not as a launch.  The 64 -> 64 launchers take no channel count, so another Cin is the
    hook's own refusal; conv_igemm's Cin and every tensor of 2^31 bytes are refused by the launchers' checks, which the hook calls first"""
    case = O.integer_case(O.C64, O.c64_spec((1, 8, 16)), "signed")
    run = det.debug_bf16_trunk_run
    wide = np.zeros((64, 9, 128), np.float32)
    for form in (O.C64, O.BLOCK):      # the 64 -> 64 kernels: refused by the hook
        with pytest.raises(capi.OcrError) as e:
            run(form, np.zeros((1, 8, 16, 128), np.float32), wide, wgt2=wide if form == O.BLOCK else None, relu=True)
        assert e.value.code == INVALID
    with pytest.raises(capi.OcrError) as e:      # conv_igemm takes bf16 Cin in multiples of 64
        run(O.IGEMM, case.x[..., :32], case.w[:, :, :32])
    assert e.value.code == INVALID
    # tensors of 2^31 bytes and more, by the arguments alone: 4 x 2048 x 2048 x 64 bf16 = 2^31 bytes
    for form in (O.C64, O.BLOCK, O.IGEMM):
        with pytest.raises(capi.OcrError) as e:
            run(form, case.x, case.w, wgt2=case.w if form == O.BLOCK else None, relu=True, claim=(4, 2048, 2048))
        assert e.value.code == INVALID, (form, e.value)
    with pytest.raises(capi.OcrError) as e:
        run(3, case.x, case.w)
    assert e.value.code == INVALID
