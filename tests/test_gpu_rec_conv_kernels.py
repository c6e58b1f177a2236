"""Kernel-level tests of the recogniser's conv stage (rec_net.hip) in all four of its forms - rec_conv_kernel<T> at T = 1, 2 and 4 crops per
workgroup, forced through launch_rec_conv's crops_per_block, and rec_conv_small_x3_kernel - through the ocr_test_rec_features hook: one
launch of the shipped launcher on caller data.  The batch alone picks T in the engine (2 above 768 crops, 4 above 3072), so without the
hook's argument only T = 1 meets small batches; the staging of crop pairs, the crop_local offsets into the shared p1, the row tiles
(wave >> 1) * T + r and the ragged last workgroup exist at T = 2 and 4 only.

Cases, references and assertions are tests/rec_conv_cases.py's (tests/test_rec_conv_cases.py runs them on the CPU against a model of the
kernels and against seven wrong models):
R1  placement by equality on one-hot weights           R4  every f32 form within an a-priori bound of f64; form 1 under the dropped-product bar
R2  dense integers below 2^24 equal the int64 result   R5  EVERY launch here: guard rows untouched, NaN leads change no bit; a NaN crop stays alone
R3  T = 1, 2, 4 give the same bits                     R6  refusals"""
import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from ocr_rs_amd import weights as W
from tests import rec_conv_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    yield lambda form, T, ops, poison=0: rec.debug_rec_features(form, *ops, crops_per_block=T, poison=poison, guard=R.GUARD, sentinel=R.SENTINEL)
    rec.close()


_FORMS = pytest.mark.parametrize("form_t", R.FORMS, ids=R.FORM_IDS)


@pytest.mark.parametrize("form_t,n", [(ft, n) for ft in R.FORMS for n in R.PLACEMENT_BATCHES[ft]],
                         ids=[f"{i}-n{n}" for ft, i in zip(R.FORMS, R.FORM_IDS) for n in R.PLACEMENT_BATCHES[ft]])
def test_rec_conv_places_every_tap_channel_half_and_crop(run, form_t, n):
    R.check_placement(run, *form_t, n)


@_FORMS
@pytest.mark.parametrize("n", R.DENSE_BATCHES)
def test_rec_conv_dense_integers_equal_int64(run, form_t, n):
    R.check_dense_int(run, *form_t, n)


def test_rec_conv_crops_per_workgroup_do_not_change_a_bit(run):
    R.check_forms_agree(run)


@pytest.mark.parametrize("T", [1, 2, 4])
def test_rec_conv_f32_within_the_a_priori_bound_of_f64(run, T):
    R.check_f64_bound(run, T)


@pytest.mark.parametrize("n", [17, 64])
def test_rec_conv_small_loses_none_of_its_six_products(run, n):
    R.check_bar(run, n)


@pytest.mark.parametrize("k", R.NAN_CROPS)
@pytest.mark.parametrize("T", [2, 4])
def test_rec_conv_nan_crop_leaves_the_other_crops_alone(run, T, k):
    R.check_nan_crop(run, 0, T, k)


@pytest.mark.parametrize("k", R.NAN_CROPS)
def test_rec_conv_small_nan_crop_leaves_the_other_crops_alone(run, k):
    R.check_nan_crop(run, 1, 0, k)


def test_rec_conv_default_choice_is_the_unforced_kernel(run):
    """crops_per_block = 0 is what the engine passes: at these batches T = 1, bit for bit"""
    ops, _ = R.real_case(9)
    assert np.array_equal(R.launch(run, 0, 0, ops).view(np.uint32), R.launch(run, 0, 1, ops).view(np.uint32))


def test_rec_conv_refusals(run):
    R.check_refusals(run, capi.OcrError)
