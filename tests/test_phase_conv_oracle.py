"""The weight builders of the composed FPN (engine.hip: compose_taps, phase_weights, pyr4_weights, through the host-only hooks of the test
library) against the definition of what they stand for, and the oracle that tests/test_gpu_phase_kernels.py holds the kernels to
(tests/phase_conv_oracle.py) against itself.  No GPU.

The bound: a built weight is ONE f32 rounding of a sum of at most nine f64 taps, |w_built - sum| <= 2^-24 |sum| <= 2^-24 sum |tap|, so the
low-res evaluation of the built weights differs from the definition by at most 2^-24 of sum |x||tap| per output element; the tests allow
9 x that (the f64 evaluations on either side differ by summation order, some 1e-13 of the same sum)."""
import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from tests import phase_conv_oracle as O
from tests import split_bf16_emul as E

BOUND = 9 * 2.0 ** -24
GRIDS = [(1, 1), (1, 7), (7, 1), (3, 5)]


def _within(got, ref, mag):
    return bool((np.abs(got - ref) <= BOUND * mag).all())


def _worst(got, ref, mag):
    return float((np.abs(got - ref) / mag).max())


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("cin", [64, 128, 256])
@pytest.mark.parametrize("up", [2, 4, 8])
def test_phase_weights_evaluate_to_the_upsampled_conv(up, cin, grid):
    rng = np.random.default_rng(100 * up + cin + grid[0])
    x = O.activations(rng, 2, grid[0], grid[1], cin)
    t = O.taps(rng, 64, cin)
    wp = capi.phase_weights(t, up)
    ref, mag = O.upsampled_conv_ref(x, t, up), O.upsampled_conv_ref(np.abs(x), np.abs(t), up)
    got = O.phase_eval(x, wp, up)
    assert _within(got, ref, mag), _worst(got, ref, mag)
    # the inactive tap slots of a phase hold zeros: the kernel skips them, whatever they hold
    for a in range(up):
        for b in range(up):
            assert not wp[a * up + b, :, O.taps_of(a, up) * O.taps_of(b, up):].any()


def _pyr_inputs(seed, grid):
    rng = np.random.default_rng(seed)
    levels = [O.activations(rng, 2, grid[0] << i, grid[1] << i, 64) for i in range(4)]
    wg = (rng.standard_normal((64, 9, 256)) / np.sqrt(9 * 256)).astype(np.float32)
    scale = ((0.5 + rng.random(64)) * rng.choice([-1.0, 1.0], 64)).astype(np.float32)
    return levels, wg, scale


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_pyr4_weights_evaluate_to_bin_conv1_of_the_pyramid(grid):
    levels, wg, scale = _pyr_inputs(7 + grid[1], grid)
    wp = capi.pyr4_weights(wg, scale)
    ref = O.pyr4_ref(levels, wg, scale)
    mag = O.pyr4_ref([np.abs(a) for a in levels], np.abs(wg), np.abs(scale))
    got = O.pyr4_eval(levels, wp, 4)
    assert _within(got, ref, mag), _worst(got, ref, mag)
    # three sources: the same without p2's slice of the weights
    wg3 = wg.copy()
    wg3[:, :, 192:] = 0
    got3 = O.pyr4_eval(levels, wp, 3)
    assert _within(got3, O.pyr4_ref(levels, wg3, scale), mag)
    assert not np.array_equal(got3, got)


def test_compose_taps_is_the_f64_product():
    rng = np.random.default_rng(3)
    for cin in (128, 256):
        out = (rng.standard_normal((64, 9, 256)) / 48).astype(np.float32)
        inn = (rng.standard_normal((256, cin)) / np.sqrt(cin)).astype(np.float32)
        got = capi.compose_taps(out, inn)
        want = np.einsum("okc,ci->oki", out.astype(np.longdouble), inn.astype(np.longdouble))
        mag = np.einsum("okc,ci->oki", np.abs(out).astype(np.float64), np.abs(inn).astype(np.float64))
        assert float((np.abs(got - want).astype(np.float64) / mag).max()) <= 1e-14


@pytest.mark.parametrize("cin", [128, 256])
def test_composed_phase_conv_is_the_layerwise_fpn_term(cin):
    """B_k = out_k o up2 o in_{k+1}: phase_eval(x_{k+1}, build(compose(out, in))) against the 1x1 lateral, the upsample and the 3x3 conv
    computed one after the other in f64"""
    rng = np.random.default_rng(cin)
    out = (rng.standard_normal((64, 9, 256)) / 48).astype(np.float32)
    inn = (rng.standard_normal((256, cin)) / np.sqrt(cin)).astype(np.float32)
    x = O.activations(rng, 2, 3, 5, cin)
    t = capi.compose_taps(out, inn)
    lateral = np.einsum("nhwi,ci->nhwc", x.astype(np.float64), inn.astype(np.float64))
    ref = O.upsampled_conv_ref(lateral, out, 2)
    mag = O.upsampled_conv_ref(np.abs(x), np.abs(t), 2)
    got = O.phase_eval(x, capi.phase_weights(t, 2), 2)
    assert _within(got, ref, mag), _worst(got, ref, mag)


# ---- the oracle can fail: one deliberate layout error each, and the comparison above rejects it --------------------------------------

@pytest.mark.parametrize("up", [2, 4, 8])
def test_swapped_taps_of_the_last_phase_are_rejected(up):
    rng = np.random.default_rng(up)
    x, t = O.activations(rng, 2, 3, 5, 64), O.taps(rng, 64, 64)
    ref, mag = O.upsampled_conv_ref(x, t, up), O.upsampled_conv_ref(np.abs(x), np.abs(t), up)
    wp = capi.phase_weights(t, up)
    assert _within(O.phase_eval(x, wp, up), ref, mag)
    bad = wp.copy()
    bad[-1, :, [0, 1]] = wp[-1, :, [1, 0]]
    got = O.phase_eval(x, bad, up)
    assert not _within(got, ref, mag)
    # ... and only the last phase's outputs are off
    off = np.abs(got - ref) > BOUND * mag
    assert off[:, up - 1::up, up - 1::up].any()
    off[:, up - 1::up, up - 1::up] = False
    assert not off.any()


@pytest.mark.parametrize("up", [2, 4, 8])
def test_a_window_of_phase_0_started_at_i_is_rejected(up):
    rng = np.random.default_rng(10 + up)
    x, t = O.activations(rng, 2, 3, 5, 64), O.taps(rng, 64, 64)
    ref, mag = O.upsampled_conv_ref(x, t, up), O.upsampled_conv_ref(np.abs(x), np.abs(t), up)
    wp = capi.phase_weights(t, up)
    got = O.phase_eval(x, wp, up, fault="window0")
    assert not _within(got, ref, mag)
    ok = np.abs(got - ref) <= BOUND * mag
    assert ok[:, 1::up, 1::up].all()          # a phase off the rim reads row i either way


def test_exchanged_p4_and_p3_slot_groups_are_rejected():
    levels, wg, scale = _pyr_inputs(5, (3, 5))
    ref = O.pyr4_ref(levels, wg, scale)
    mag = O.pyr4_ref([np.abs(a) for a in levels], np.abs(wg), np.abs(scale))
    wp = capi.pyr4_weights(wg, scale)
    assert _within(O.pyr4_eval(levels, wp, 4), ref, mag)
    bad = wp.copy()
    bad[:, :, 4:8], bad[:, :, 8:12] = wp[:, :, 8:12], wp[:, :, 4:8]
    assert not _within(O.pyr4_eval(levels, bad, 4), ref, mag)


# ---- the K5 families of tests/test_gpu_phase_kernels.py separate five products from six ------------------------------------------------

SEPARATION = 5.0


def _separated(case):
    six, five, bar, names = E.bar(case)
    print(f"six {six:.3g}  five {five:.3g}  ratio {five / six:.1f}  chain {case.rms(case.chain()):.3g}  bar {bar:.3g}  drops {names}")
    assert five >= SEPARATION * six, (six, five)
    assert six < bar < five


@pytest.mark.parametrize("case", E.PHASE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_phase_families_separate_five_products_from_six(case):
    _separated(E.PhaseCase(*E.phase_family(case, capi.phase_weights)))


@pytest.mark.parametrize("case", E.PYR_CASES, ids=lambda c: "x".join(map(str, c)))
def test_pyr_families_separate_five_products_from_six(case):
    _separated(E.PyrCase(*E.pyr_family(case, capi.pyr4_weights)))


def test_phased_cases_are_the_oracles_evaluation():
    """PhaseCase / PyrCase place their per-phase GEMMs where phase_eval / pyr4_eval do"""
    x, wp, up = E.phase_family(E.PHASE_CASES[0], capi.phase_weights)
    assert np.allclose(E.PhaseCase(x, wp, up).ref, O.phase_eval(x, wp, up), rtol=0, atol=1e-12)
    levels, wq, nsrc = E.pyr_family(E.PYR_CASES[0], capi.pyr4_weights)
    assert np.allclose(E.PyrCase(levels, wq, nsrc).ref, O.pyr4_eval(levels, wq, nsrc), rtol=0, atol=1e-12)
