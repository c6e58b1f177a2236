"""The CPU yardstick of the split-bf16 kernels (tests/split_bf16_emul.py), no GPU: the split is exact, and every input family that
tests/test_gpu_stem_head_kernels.py holds a kernel to separates "one of the six products lost" from "all six" by at least 5 x in
normalised rms error - the condition under which the geometric mean of the two is a bar with sqrt(5) of room on either side."""
import numpy as np
import pytest

from tests import split_bf16_emul as E

SEPARATION = 5.0


@pytest.mark.parametrize("family", ["normal", "wide_exponents", "integer_luma", "luma_plus_fraction"])
def test_split3_is_exact(family):
    rng = np.random.default_rng(0)
    if family == "normal":
        x = rng.standard_normal(1 << 16)
    elif family == "wide_exponents":
        x = rng.standard_normal(1 << 16) * np.exp2(rng.integers(-60, 60, 1 << 16))
    elif family == "integer_luma":
        x = np.arange(256).repeat(4)
    else:
        x = rng.integers(0, 256, 1 << 16) + rng.random(1 << 16)
    x = x.astype(np.float32)
    hi, mid, lo = E.split3(x)
    for p in (hi, mid, lo):
        assert np.array_equal(p, E.bf16_round(p))          # each term IS a bf16 value
    assert np.array_equal((hi.astype(np.float64) + mid + lo), x.astype(np.float64))
    assert np.array_equal(((hi + mid).astype(np.float32) + lo).astype(np.float32), x)
    if family == "integer_luma":
        assert not mid.any() and not lo.any()


def test_emulate_with_all_nine_products_is_the_f64_product_rounded_per_group():
    """Sanity of the emulation itself: on operands that ARE bf16 only hi.hi is non-zero, and one K group is one f64 dot product."""
    rng = np.random.default_rng(1)
    A, B = E.bf16_round(rng.standard_normal((37, 16))), E.bf16_round(rng.standard_normal((16, 5)))
    want = (A.astype(np.float64) @ B.astype(np.float64)).astype(np.float32)
    assert np.array_equal(E.emulate(A, B), want)
    assert np.array_equal(E.emulate(A, B, products=((0, 0),)), want)
    assert not E.emulate(A, B, products=E.PRODUCTS[:5]).any()


def test_f32_chain_is_sequential_fma():
    A = np.array([[2.0 ** 24, 1.0, 1.0]], np.float32)
    B = np.ones((3, 1), np.float32)
    assert E.f32_chain(A, B)[0, 0] == 2.0 ** 24            # 2^24 + 1 rounds back twice; the f64 sum would be 2^24 + 2
    assert E.f32_chain(A[:, ::-1].copy(), B)[0, 0] == 2.0 ** 24 + 2


def _separated(case, want_drops=None):
    six, five, bar, names = E.bar(case)
    print(f"six {six:.3g}  five {five:.3g}  ratio {five / six:.1f}  bar {bar:.3g}  drops {names}")
    if want_drops is not None:
        assert set(names) - {"hi.hi"} == set(want_drops)
    assert five >= SEPARATION * six, (six, five)
    assert six < bar < five


@pytest.mark.parametrize("family", E.STEM_FAMILIES)
def test_stem_families_separate_five_products_from_six(family):
    w, scale, bias = E.stem_weights(1)
    # integer luma has no mid / lo term: only the products of its hi plane exist
    want = None if family == "fraction" else ["hi.lo", "hi.mid"]
    _separated(E.StemCase(E.stem_family(family), w, scale, bias), want)


@pytest.mark.parametrize("shape", [(2, 8, 24), (1, 3, 43)], ids=str)
def test_head_family_separates_and_keeps_its_logits_in_range(shape):
    case = E.HeadCase(*E.head_family(*shape))
    assert case.left_out <= 0.10, case.left_out
    _separated(case)


def test_rec_family_separates_five_products_from_six():
    crops, w1, b1, w2, b2, p1 = E.rec_family(64)
    _separated(E.RecCase(p1, w2, b2))


@pytest.mark.parametrize("case", E.CONV_CASES, ids=str)
def test_conv_families_separate_five_products_from_six(case):
    _separated(E.ConvCase(*E.conv_family(case)))


@pytest.mark.parametrize("case", E.IGEMM_CASES, ids=str)
def test_igemm_families_separate_five_products_from_six_at_the_kernels_k_step(case):
    """the inputs of tests/test_gpu_igemm_kernels.py (G5), K groups of 32 as in conv_igemm's K-step"""
    x, wg, stride = E.igemm_family(case)
    _separated(E.ConvCase(x, wg, stride, kgroup=32))


def test_rec_pooled_onehot_is_conv1_of_its_weights():
    """The host-side pooled map is what conv1 + bias + 2x2 max pool of the returned weights computes (f64 conv: one non-zero term per sum)."""
    crops, w1, b1, w2, b2, p1 = E.rec_family(3)
    x = crops.reshape(3, 28, 28).astype(np.float64)
    c1 = np.zeros((3, 24, 24, 32))
    for t in range(25):
        ky, kx = divmod(t, 5)
        c1 += x[:, ky:ky + 24, kx:kx + 24, None] * w1[:, t].astype(np.float64)
    want = (c1.reshape(3, 12, 2, 12, 2, 32).max(axis=(2, 4)).astype(np.float32) + b1).astype(np.float32)
    assert np.array_equal(p1, want)


def test_head_place_puts_tap_and_phase_where_the_kernel_does():
    v = np.arange(2 * 3 * 5 * 16, dtype=np.float64).reshape(2, 3, 5, 4, 4)
    out = E.head_place(v)
    for n, i, j, a, b, c, d in [(0, 0, 0, 0, 0, 0, 0), (1, 2, 4, 1, 0, 1, 1), (0, 1, 3, 0, 1, 1, 0), (1, 0, 2, 1, 1, 0, 1)]:
        assert out[n, 4 * i + 2 * a + c, 4 * j + 2 * b + d] == v[n, i, j, 2 * a + b, 2 * c + d]
