"""Kernel-level tests of conv_igemm's launches with a SRC_PLAIN / SRC_CAT4 source and a STORE_NHWC / STORE_SHUFFLE2 store - the trunk's convs,
the laterals with the top-down sum, bin_conv1 over the concat, the transposed conv's pixel shuffle, the batched GEMM of the Winograd F(2x2)
conv - through ocr_test_igemm_run: ONE launch_conv_igemm on caller data with the descriptor the engine builds, against
tests/igemm_oracle.py (the operation by definition in f64, integer families that determine the result bit for bit, and the checks below as
functions of `run`; tests/test_igemm_oracle.py runs the same checks on a CPU stand-in and shows that each of its named faults fails one).

G1 exact        integer families: small integers on both sides (every form, (ks, stride), tile, epilogue: none | scale + bias + ReLU |
                scale + bias + residual + ReLU | out2 beside out | out2 alone | out2 with a residual); for the split form three families
                with operands of 21 and 11 bits that pin where each of the six products' planes sits.  array_equal; bf16 results: the exact
                value rounded once
G2 f64 parity   N(0,1) activations, the images of a batch scaled 1, 16, 1/16, weights N(0,1) / sqrt(K), every epilogue
                  f32 results  |err| <= 4e-6 (sum |a||b| |scale| + |bias| + |residual| + |up_residual|) per element AND max |err| <= 2e-5 of
                               the tensor's maximum
                  bf16 results the recipe of tests/test_gpu_conv_kernel.py::_check: reference from the rounded operands, one bf16 ulp + 1e-5
                               of the scale, fewer than 1 % of the elements beyond 1e-5 of the scale
G3 who writes   the guard rows behind out and out2 come back untouched - asserted for EVERY launch of this file (igemm_oracle.launch); two
                runs over different prefills give the same bits, behind ReLU no element is the prefill; with out == null the sum alone is
                stored, with the bits it has beside out
G4 poison       NaN in front of and behind the source inside its allocation (CAT4: between the levels too), without an epilogue - a NaN
                that was read is stored - and behind residual + ReLU: finite, the bits of the clean run; the middle image of three NaN: the other two keep their bits; one image alone has the bits it has in the middle of a
                batch whose images are no multiple of the tile's rows
G5 lost product rms(kernel - f64) <= sqrt(rms_six x min rms_five) (docs/split_bf16_error.md), split bf16 and exact f32 alike, K groups of 32
G6 size         a result beyond what an epilogue's 32-bit offsets address is refused by its shape, before anything is allocated: bf16 NHWC
                results take BYTE offsets (m0 + row) Cout 2 + column of every row of the last tile, the rows beyond M included, against the
                range M Cout 2 - both wrap from 2^32 bytes on; the pixel shuffle keeps an int ELEMENT index per row - 2^31 elements.  (f32
                NHWC results without out2 are stored relative to each wave's corner of the output, found by a size_t index, and the general
                form of epilogue B indexes with size_t: they hold at any size the source's own bound allows.  out2's row_aux indexes
                up_residual, a quarter of the output: refused from 2^31 elements on, which needs Cout >= 512 and is not launched here.)

The combinations conv_igemm.hip's check() accepts for these modes, each launched by G1 and G2 (the engine's use in brackets); tiles by the
override, 128 x 128 where Cout is a multiple of 128:

  SRC_PLAIN / STORE_NHWC, ks 1 | 3, stride 1 | 2, residual, out2 (even output grid; out may then be null)
    exact f32       tiles 128 x 128, 128 x 64, 64 x 64   [mfma=f32: trunk, downsample, laterals in2..in5 with the top-down sum, out2..out5]
    split bf16      tiles 128 x 128, 128 x 64            [default f32 engine: the same launches]
    bf16 -> bf16    tiles 128 x 128, 128 x 64, 64 x 64   [bf16 precision: the same launches]
    bf16 -> f32     3x3 s1 only, the three tiles          [bf16 precision: a 3x3 conv whose consumer reads f32 (f32_out)]
  SRC_PLAIN / STORE_NHWC, batched (1x1 s1, no residual, no out2)
    exact f32       the three tiles                       [mfma=f32: the sixteen GEMMs of a Winograd F(2x2) conv]
    split bf16      both tiles                            [default f32 engine: the same]
  SRC_CAT4 / STORE_NHWC (3x3 s1 256 -> 64 on a grid divisible by 8; Cout 64: tiles 128 x 64, 64 x 64)
    exact f32, bf16 -> bf16, bf16 -> f32                  [bin_conv1 with bin_pyr=0; the bf16 precision writes bf16 for the fused head, f32 otherwise]
  SRC_PLAIN / STORE_SHUFFLE2 (1x1 s1, Cout 256, no residual, no out2)
    exact f32       the three tiles                       [bin_conv_tr1 when the head is unfused]
  check() refuses everything else - the split form with CAT4, SHUFFLE2 or bf16 results, SHUFFLE2 with a residual, out2, bf16, stride 2, a 3x3
  kernel or Cout != 256, out2 on an odd grid or without up_residual, f32 -> bf16, bf16 -> f32 of a 1x1 conv, the batched GEMM with a residual,
  in bf16 or 3x3, CAT4 off a grid divisible by 8 - and the hook passes the refusal on: test_refused_combinations.

Measured on the MI355X (printed by the tests): docs/split_bf16_error.md, section "conv_igemm's plain, concat and shuffle forms".
"""
import re

import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from ocr_rs_amd import weights as W
from tests import igemm_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    yield d.debug_igemm_run
    d.close()


def _id(l):
    return l.name().replace(" ", "_") if isinstance(l, O.Launch) else str(l)


ALL = O.all_launches()
N3 = [l for l in ALL if l.grid[0] == 3 and l.batch == 1] + [O.Launch(f, obf, 3, 1, (3, 8, 8), 256, 64, src=O.CAT4, tile=t)
                                                            for f, obf in ((O.F32, False), (O.BF16, True), (O.BF16, False)) for t in (2, 3)]


# ---- G1 ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("l", ALL, ids=_id)
def test_g1_integers_come_out_exact(run, l):
    O.check_g1(run, l)


@pytest.mark.parametrize("family", O.SPLIT_FAMILIES)
@pytest.mark.parametrize("l", O.split_launches(), ids=_id)
def test_g1_split_form_places_every_plane(run, l, family):
    O.check_g1(run, l, family)


# ---- G2 ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("l", ALL, ids=_id)
def test_g2_real_data_matches_f64(run, l):
    O.check_g2(run, l)


# ---- G3 ----------------------------------------------------------------------------------------------------------------------------------------

G3 = [l for l in ALL if l.grid in ((1, 5, 13), (1, 3, 43), (2, 6, 10), (2, 12, 20), (1, 12, 22), (1, 24, 44), (2, 3, 5), (2, 8, 16), (1, 1, 63))]


@pytest.mark.parametrize("l", G3, ids=_id)
def test_g3_every_element_is_written_once_and_nothing_else(run, l):
    O.check_g3(run, l)


# ---- G4 ----------------------------------------------------------------------------------------------------------------------------------------

G4 = [l for l in ALL if l.batch == 1 and (l.src == O.CAT4 or l.grid in ((1, 1, 1), (3, 5, 3), (1, 3, 130), (2, 10, 18), (1, 9, 15)))]


@pytest.mark.parametrize("l", G4, ids=_id)
def test_g4_no_byte_around_the_source_is_used(run, l):
    O.check_g4_poison(run, l)


@pytest.mark.parametrize("l", N3, ids=_id)
def test_g4_a_nan_image_leaves_its_neighbours_alone(run, l):
    O.check_g4_batch(run, l)


# (a CAT4 grid is divisible by 8, an image a multiple of 64 rows: only the 128-row tile can be misaligned, by the 64 rows of an 8 x 8 image)
@pytest.mark.parametrize("l", [l for l in N3 if not (l.src == O.CAT4 and l.tile == 3)], ids=_id)
def test_g4_an_image_alone_has_the_bits_it_has_in_a_batch(run, l):
    O.check_g4_alone(run, l)


# ---- G5 ----------------------------------------------------------------------------------------------------------------------------------------

G5 = [(c, f, t) for c in O.G5_CASES for f, t in ((O.SPLIT, 1), (O.SPLIT, 2), (O.F32, 3), (O.F32, 2)) if t != 1 or c[4] % 128 == 0]


@pytest.mark.parametrize("case,form,tile", G5, ids=str)
def test_g5_no_product_of_the_six_is_lost(run, case, form, tile):
    O.check_g5(run, case, form, tile)


# ---- G6 ----------------------------------------------------------------------------------------------------------------------------------------

def test_g6_an_output_beyond_32_bit_offsets_is_refused_by_its_shape(run):
    """See G6 above.  Each shape's source is below 2^31 bytes, so only the output's size can refuse it; the hook hands it to the launcher
    without operands and before anything is allocated.  A bf16 output between 2^31 and 2^32 bytes is addressable: that shape gets as far as
    the null-operand check."""
    x64, x32 = np.zeros((1, 1, 1, 64), np.float32), np.zeros((1, 1, 1, 32), np.float32)
    w64, w32 = np.zeros((256, 1, 64), np.float32), np.zeros((256, 1, 32), np.float32)
    with pytest.raises(capi.OcrError, match="output of 4299161600 bytes"):      # 8 396 800 pixels x 256 x 2
        run(O.BF16, x64, w64, out_bf16=True, claim=(1, 2048, 4100))
    with pytest.raises(capi.OcrError, match="output of 4294967296 bytes"):      # 2^23 pixels x 256 x 2 = 2^32: the range itself wraps to 0
        run(O.BF16, x64, w64, out_bf16=True, claim=(1, 2048, 4096))
    with pytest.raises(capi.OcrError, match="null operand"):                    # 2^23 - 128 pixels, whole tiles: ends 65 536 bytes below 2^32
        run(O.BF16, x64, w64, out_bf16=True, claim=(1, 2040, 4112))
    with pytest.raises(capi.OcrError, match="output of 8589934592 bytes"):      # 2^23 pixels x 256 x 4: 2^31 elements
        run(O.F32, x32, w32, store_mode=O.SHUFFLE2, claim=(1, 2048, 4096))
    with pytest.raises(capi.OcrError, match="null operand"):                    # 2^31 + 2^20 bytes of bf16
        run(O.BF16, x64, w64, out_bf16=True, claim=(1, 2048, 2049))


# ---- what check() refuses comes back as an error -------------------------------------------------------------------------------------------------

def test_refused_combinations(run):
    for name, message, kw in O.refused_combinations():
        kw = dict(kw)
        with pytest.raises(capi.OcrError, match=re.escape(message)):
            run(kw.pop("form"), kw.pop("x"), kw.pop("wgt"), **kw)
            pytest.fail(f"{name}: launched")
