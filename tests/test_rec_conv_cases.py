"""The CPU side of the recogniser conv-stage kernel tests (tests/rec_conv_cases.py), no GPU: the check_* functions that
tests/test_gpu_rec_conv_kernels.py runs against the hook pass against a numpy model of the kernels, and a model with any of seven
deliberate faults fails at least one of them - so the GPU tests' demands are both fair and sharp."""
import numpy as np
import pytest

from tests import rec_conv_cases as R


def _run(bug=None):
    return lambda form, T, ops, poison=0: R.model(form, T, ops, poison, bug)


def _all_checks(run, quick=False):
    """every check the GPU file runs, in its order; quick: the cheap half, enough for the wrong models"""
    for (form, T) in R.FORMS:
        for n in R.PLACEMENT_BATCHES[(form, T)]:
            R.check_placement(run, form, T, n)
    for (form, T) in R.FORMS:
        for n in R.DENSE_BATCHES:
            R.check_dense_int(run, form, T, n)
    R.check_forms_agree(run)
    for T in (1, 2, 4):
        R.check_f64_bound(run, T)
    for T in (2, 4):
        for k in R.NAN_CROPS:
            R.check_nan_crop(run, 0, T, k)
    R.check_refusals(run, R.Refused)
    if not quick:
        R.check_bar(run, 17)


def test_the_model_of_the_kernels_passes_every_check():
    _all_checks(_run())


@pytest.mark.parametrize("bug", R.BUGS)
def test_a_wrong_model_fails_a_check(bug):
    with pytest.raises(AssertionError) as e:
        _all_checks(_run(bug), quick=True)
    print(bug, "->", str(e.value)[:200])


@pytest.mark.parametrize("bug,check", [
    ("swap_pair", lambda run: R.check_placement(run, 0, 2, 2)),
    ("swap_pair", lambda run: R.check_dense_int(run, 0, 4, 5)),
    ("store_ragged", lambda run: R.check_placement(run, 0, 2, 1)),
    ("store_ragged", lambda run: R.check_placement(run, 0, 4, 5)),
    ("swap_halves", lambda run: R.check_placement(run, 0, 4, 4)),
    ("drop_tap", lambda run: R.check_placement(run, 0, 2, 3)),
    ("drop_tap", lambda run: R.check_dense_int(run, 1, 0, 5)),
    ("pad_tap", lambda run: R.check_placement(run, 0, 1, 1)),
    ("pad_tap", lambda run: R.check_dense_int(run, 0, 2, 9)),
    ("copy_last", lambda run: R.check_placement(run, 0, 4, 7)),
    ("copy_last", lambda run: R.check_nan_crop(run, 0, 2, 8)),
    ("lead_read", lambda run: R.check_placement(run, 0, 4, 1)),
    ("lead_read", lambda run: R.check_forms_agree(run)),
], ids=lambda v: v if isinstance(v, str) else "")
def test_the_check_meant_for_a_fault_catches_it(bug, check):
    """not merely the first check of the list: each fault is caught where the issue expects it, the dense integers included"""
    check(_run())
    with pytest.raises(AssertionError):
        check(_run(bug))


@pytest.mark.parametrize("n", R.DENSE_BATCHES)
def test_dense_integer_cases_are_exact_in_any_f32_order(n):
    ops, want = R.dense_int_case(n)          # the builder asserts the 2^24 bound and the share of late-decided pool windows
    crops, w1, b1, w2, b2 = ops
    assert crops.min() >= 0 and crops.max() <= 255 and np.abs(w1).max() <= 1 and np.abs(b1).max() <= 3 and np.abs(w2).max() <= 2
    assert all(np.array_equal(v, np.rint(v)) for v in ops)
    # conv2 tap by tap in f32, taps last to first: another order than the model's single f64 sum, the same integers
    got, _ = R.model(0, 1, ops)
    p1 = (R._pool2((R._windows(crops.reshape(n, 28, 28, 1))[..., 0] @ w1.T).astype(np.float32))[0] + b1).astype(np.float32)
    acc = np.zeros((n, 8, 8, 64), np.float32)
    win = R._windows(p1)
    for tap in reversed(range(25)):
        acc = (acc + win[:, :, :, tap] @ w2[:, :, tap].T).astype(np.float32)
    back = (R._pool2(acc)[0] + b2).astype(np.float32).transpose(0, 3, 1, 2).reshape(n, 1024)
    assert np.array_equal(back, want) and np.array_equal(got, want)


def test_the_f64_bound_is_a_bound_and_not_a_loose_one():
    """a sequential f32 chain of the 800 products (E.f32_chain, the kernels' arithmetic) stays inside the a-priori bound, and the bound
    keeps out a conv2 operand rounded to bf16"""
    ops, case = R.real_case(9)
    bound = R.f64_bound(case)
    chain = np.abs(case.chain().astype(np.float64) - case.ref)
    assert (chain <= bound).all()
    rounded = case.epilogue((R.E.bf16_round(case.A).astype(np.float64) @ case.B.astype(np.float64)), np.float64)
    assert (np.abs(rounded - case.ref) > bound).mean() > 0.5
