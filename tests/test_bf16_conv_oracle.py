"""tests/bf16_conv_oracle.py on the CPU: the integer cases meet their conditions (asserted by integer_case: partial sums below 2^24 quanta,
outputs beyond 256, exact ties, a quarter of the outputs behind ReLU), the numpy model of the three kernels passes every assertion of
tests/test_gpu_bf16_trunk_kernels.py, every deliberately wrong model fails at least one of the integer assertions on the committed case lists,
and the real-valued cases are large enough for their bars to mean something."""
import functools

import numpy as np
import pytest

from tests import bf16_conv_oracle as O


def _ids(v):
    return "-".join(_ids(e) for e in v) if isinstance(v, tuple) else str(v)


def test_bf16_roundings():
    a = np.array([1.0, 257.0, 259.0, 258.0, -257.0, 1.00390625, 0.0, 3.0e38], np.float32)
    assert O.bf16_rne(a).tolist()[:7] == [1.0, 256.0, 260.0, 258.0, -256.0, 1.0, 0.0]
    assert O.bf16_trunc(a).tolist()[:5] == [1.0, 256.0, 258.0, 258.0, -256.0]
    assert O.is_tie(a).tolist() == [False, True, True, False, True, True, False, False]
    v = np.array([257.0, 259.0, 1.00390625, 1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 2.0 ** -8 - 2.0 ** -30, -0.3])
    assert O.bf16_from_f64(v).tolist() == [256.0, 260.0, 1.0, 1.0078125, 1.0, float(O.bf16_rne(np.float32(-0.3)).item())]
    assert O.bf16_steps(np.array([1.0, 1.0, -2.0 ** -133, 2.0], np.float32), np.array([1.0078125, 0.99609375, 2.0 ** -133, 1.984375], np.float32)).tolist() == [1, 1, 2, 2]
    up = O.bf16_at_least(np.array([1.001, -1.001, 1.0, 255.5]))
    assert up.tolist() == [1.0078125, -1.0, 1.0, 256.0]


@pytest.mark.parametrize("nblocks", [1, 7, 8, 59, 60, 61, 400])
def test_walks_visit_every_block_once(nblocks):
    for cus in (0,) + O.B2_CUS:
        for walk in (O.c64_walk, O.block_walk):
            seen = sorted(b for wg in walk(nblocks, cus) for b in wg)
            assert seen == list(range(nblocks)), (walk.__name__, nblocks, cus)
    assert max(len(w) for w in O.c64_walk(60, 1)) == 30 and max(len(w) for w in O.block_walk(60, 16)) == 4


@pytest.mark.parametrize("family", O.FAMILIES)
@pytest.mark.parametrize("form", [O.C64, O.BLOCK])
def test_model_passes_b1_on_the_block_shapes(form, family):
    for shape in O.C64_SHAPES:
        O.check_b1(O.standin, form, O.c64_spec(shape), family)


@pytest.mark.parametrize("family", O.FAMILIES)
def test_model_passes_b1_on_the_igemm_launches(family):
    for spec in O.IGEMM_SPECS:
        O.check_b1(O.standin, O.IGEMM, spec, family)


@pytest.mark.parametrize("form", [O.C64, O.BLOCK])
def test_model_passes_b2(form):
    O.check_b2(O.standin, form)


def test_model_passes_b3():
    for form, specs in O.B3_SPECS.items():
        for spec in specs:
            O.check_b3_poison(O.standin, form, spec)
    for form, specs in O.B3_BATCH_SPECS.items():
        for spec in specs:
            O.check_b3_batch(O.standin, form, spec)


# per fault and form the integer assertions that have to catch it: (check, arguments); "any" = at least one of them fails
def _b1(form, spec, family="signed"):
    return (O.check_b1, (form, spec, family))


_C64, _IG = O.c64_spec, O.IGEMM_SPECS
CATCHES = {
    ("top_halo", O.C64): [_b1(O.C64, _C64((3, 1, 1))), _b1(O.C64, _C64((2, 17, 33))), (O.check_b3_batch, (O.C64, O.B3_BATCH_SPECS[O.C64][0]))],
    ("top_halo", O.BLOCK): [_b1(O.BLOCK, _C64((3, 1, 1))), _b1(O.BLOCK, _C64((2, 7, 15))), (O.check_b3_batch, (O.BLOCK, O.B3_BATCH_SPECS[O.BLOCK][0]))],
    ("top_halo", O.IGEMM): [_b1(O.IGEMM, _IG[1]), _b1(O.IGEMM, _IG[6]), (O.check_b3_batch, (O.IGEMM, O.B3_BATCH_SPECS[O.IGEMM][0]))],
    ("halo_right", O.C64): [_b1(O.C64, _C64((1, 9, 17))), _b1(O.C64, _C64((1, 16, 32))), (O.check_b3_poison, (O.C64, O.B3_SPECS[O.C64][1]))],
    ("halo_right", O.BLOCK): [_b1(O.BLOCK, _C64((1, 9, 17))), _b1(O.BLOCK, _C64((1, 16, 32))), (O.check_b3_poison, (O.BLOCK, O.B3_SPECS[O.BLOCK][1]))],
    ("halo_right", O.IGEMM): [_b1(O.IGEMM, _IG[3]), _b1(O.IGEMM, _IG[9]), (O.check_b3_poison, (O.IGEMM, O.B3_SPECS[O.IGEMM][1]))],
    ("mid_outside", O.BLOCK): [_b1(O.BLOCK, _C64(s)) for s in O.C64_SHAPES],
    ("mid_f32", O.BLOCK): [_b1(O.BLOCK, _C64((1, 8, 16))), _b1(O.BLOCK, _C64((2, 17, 33)), "nonneg")],
    ("round_before_residual", O.C64): [_b1(O.C64, _C64((3, 1, 1))), _b1(O.C64, _C64((1, 9, 17)), "nonneg")],
    ("round_before_residual", O.BLOCK): [_b1(O.BLOCK, _C64((3, 1, 1))), _b1(O.BLOCK, _C64((1, 9, 17)), "nonneg")],
    ("round_before_residual", O.IGEMM): [_b1(O.IGEMM, _IG[0]), _b1(O.IGEMM, _IG[12]), _b1(O.IGEMM, _IG[14])],
    ("relu_before_residual", O.C64): [_b1(O.C64, _C64((3, 1, 1))), _b1(O.C64, _C64((1, 5, 40)))],
    ("relu_before_residual", O.BLOCK): [_b1(O.BLOCK, _C64((3, 1, 1))), _b1(O.BLOCK, _C64((1, 5, 40)))],
    ("relu_before_residual", O.IGEMM): [_b1(O.IGEMM, _IG[4]), _b1(O.IGEMM, _IG[13])],
    ("truncate", O.C64): [_b1(O.C64, _C64((3, 1, 1))), _b1(O.C64, _C64((1, 33, 17)), "nonneg")],
    ("truncate", O.BLOCK): [_b1(O.BLOCK, _C64((3, 1, 1))), _b1(O.BLOCK, _C64((1, 33, 17)), "nonneg")],
    ("truncate", O.IGEMM): [_b1(O.IGEMM, s) for s in (_IG[0], _IG[8], _IG[13], _IG[15], _IG[16])],
    ("ragged_row", O.C64): [_b1(O.C64, _C64((1, 9, 17))), _b1(O.C64, _C64((2, 7, 15)))],
    ("ragged_row", O.BLOCK): [_b1(O.BLOCK, _C64((1, 9, 17))), _b1(O.BLOCK, _C64((2, 7, 15)))],
    ("ragged_row", O.IGEMM): [_b1(O.IGEMM, _IG[0]), _b1(O.IGEMM, _IG[7]), _b1(O.IGEMM, _IG[14])],
    ("stale_block", O.C64): [(O.check_b2, (O.C64, (1,))), (O.check_b2, (O.C64, (29,)))],
    ("stale_block", O.BLOCK): [(O.check_b2, (O.BLOCK, (2,))), (O.check_b2, (O.BLOCK, (8,))), (O.check_b2, (O.BLOCK, (16,)))],
}


def test_every_fault_and_form_is_listed():
    assert {f for f, _ in CATCHES} == set(O.FAULTS)
    block_only = {"mid_outside", "mid_f32"}
    assert {k for k in CATCHES} == {(f, form) for f in O.FAULTS for form in (O.C64, O.BLOCK, O.IGEMM)
                                    if (form == O.BLOCK or f not in block_only) and not (f == "stale_block" and form == O.IGEMM)}


@pytest.mark.parametrize("fault,form", sorted(CATCHES), ids=_ids)
def test_wrong_model_fails_every_check_listed_for_it(fault, form):
    """... and with the fault taken out the same checks pass (the test_model_passes_* tests above)"""
    wrong = functools.partial(O.standin, fault=fault)
    for check, args in CATCHES[(fault, form)]:
        with pytest.raises(AssertionError):
            check(wrong, *args)


def test_a_stale_block_needs_a_walk():
    """under the default grid every workgroup has one block: B1 cannot see the fault, which is what B2 is for"""
    O.check_b1(functools.partial(O.standin, fault="stale_block"), O.C64, O.c64_spec((2, 17, 33)), "signed")


def _b4_cases():
    return [(form, spec) for form, specs in sorted(O.B4_SPECS.items()) for spec in specs]


@pytest.mark.parametrize("form,spec", _b4_cases(), ids=_ids)
def test_real_cases_are_large_enough(form, spec):
    """the emulation differs from the reference in at least 100 elements, meets RealCase.assert_close (the a-priori bound in every element, the
    neighbour demand where it is made), and the same emulation with the sum rounded before the residual is added lies 5 x above the bar"""
    flips, emulated = O.real_bar(form, spec)
    case = O.real_case(form, spec)
    twice = O.real_emulation(form, spec, "round_before_residual")
    assert flips >= O.MIN_FLIPS, (flips, emulated)
    assert case.share(twice) >= O.TWICE_FACTOR * O.SHARE_FACTOR * emulated, (case.share(twice), emulated)
    assert case.ref.size <= 3 * 40 * 56 * 64

    def replay(out):
        return lambda *a, **kw: (out, None, np.full(1, O.SENTINEL, np.float32))

    with pytest.raises(AssertionError):
        O.check_b4(replay(twice), form, spec, report=lambda s: None)
    O.check_b4(replay(O.real_emulation(form, spec)), form, spec, report=lambda s: None)


def _replay(out):
    return lambda *a, **kw: (out, None, np.full(1, O.SENTINEL, np.float32))


@pytest.mark.parametrize("form,spec", [(form, spec) for form, specs in sorted(O.B4_NATURAL_SPECS.items()) for spec in specs], ids=_ids)
def test_natural_cases_hold_for_the_emulation_and_notice_a_wrong_model(form, spec):
    case = O.real_case(form, spec, True)
    assert 0.25 < (case.ref == 0).mean() < 0.6      # ReLU is at work
    largest, held, _ = O.check_b4_natural(_replay(O.real_emulation(form, spec, None, True)), form, spec, report=lambda s: None)
    assert held >= 5000 and largest <= 1
    for fault in ("top_halo", "truncate", "ragged_row"):
        with pytest.raises(AssertionError):
            O.check_b4_natural(functools.partial(O.standin, fault=fault), form, spec, report=lambda s: None)


@pytest.mark.parametrize("form", sorted(O.B4_SPECS))
def test_one_wrong_element_fails_b4(form):
    """a single element eight bf16 steps off, in a case whose differing share stays far under its bar: the bound is asserted, not printed"""
    spec = O.B4_SPECS[form][0]
    case, out = O.real_case(form, spec), O.real_emulation(form, spec).copy()
    at = tuple(np.argwhere(case.ref == case.ref.max())[0])
    out[at] = case.ref[at] + 8 * O.bf16_step(case.ref[at])
    assert case.share(out) <= O.SHARE_FACTOR * O.real_bar(form, spec)[1]
    with pytest.raises(AssertionError, match="beyond the bound"):
        O.check_b4(_replay(out), form, spec, report=lambda s: None)


def test_the_blocks_bound_is_what_its_intermediate_allows():
    """the block's emulation - a correct kernel - is further than one step from the reference in some elements (which is why the neighbour demand
    holds above a floor only), yet within the a-priori bound everywhere; a block that leaves its intermediate in f32 or evaluates it outside
    the image is not"""
    spec = O.B4_SPECS[O.BLOCK][0]
    case, emul = O.real_case(O.BLOCK, spec), O.real_emulation(O.BLOCK, spec)
    assert (O.bf16_steps(emul, case.ref) > 1).sum() > 10
    assert 0.05 < (case.slack > 0).mean() < 0.3
    largest, held, furthest = case.assert_close(emul)
    assert largest <= 1 and held > 100 and furthest <= 1
    for fault in ("mid_f32", "mid_outside"):
        with pytest.raises(AssertionError):
            case.assert_close(case.run(O.standin, chain=True, fault=fault))
