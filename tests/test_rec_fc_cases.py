"""The CPU side of the recogniser's fc kernel tests (tests/rec_fc_cases.py), no GPU: the conditions under which the demands of
tests/test_gpu_rec_fc_kernels.py are fair - equality on the integer cases, the softmax reference, and an rms bar that keeps out
what it is there to keep out by at least 10 x."""
import numpy as np
import pytest

from oracle import torch_ref as T
from tests import rec_fc_cases as R

# every (n, K, N) the GPU tests run an integer case at
INT_SIZES = ([(n, 1024, 512) for n in (1, 15, 16, 17, 40, 63, 64, 65, 127, 129, 200)] +
             [(n, 512, 62) for n in (1, 15, 16, 17, 31, 32, 33, 40, 63, 64, 65, 130)])
KEEP_OUT = 10.0


@pytest.mark.parametrize("size", INT_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_integer_cases_are_exact_in_any_f32_order(size):
    n, K, N = size
    a, w, b, want = R.fc_int_case(n, K, N, seed=n, relu=N == 512)
    assert R.int_case_bound(a, w, b) < 2 ** 24
    assert a.min() >= 0 and a.max() <= 15 and np.abs(w).max() <= 3 and np.abs(b).max() <= 50
    assert all(np.array_equal(v, np.rint(v)) for v in (a, w, b))
    assert len({r.tobytes() for r in a}) == n                    # every row is distinct
    if N == 512:
        clamped = float((want == 0).mean())
        assert 0.4 <= clamped <= 0.6, clamped
        assert want.min() == 0
    # two very different orders in f32 give the int64 result
    fwd = np.zeros((n, N), np.float32)
    for k0 in range(0, K, 64):
        fwd = (fwd + a[:, k0:k0 + 64] @ w[:, k0:k0 + 64].T).astype(np.float32)
    fwd = fwd + b
    assert np.array_equal(np.maximum(fwd, 0) if N == 512 else fwd, want)


def test_injected_logits_come_out_of_fc2_exactly():
    rng = np.random.default_rng(3)
    L = (rng.standard_normal((5, 62)) * np.exp2(rng.integers(-20, 100, (5, 62)))).astype(np.float32)
    L[4] = -np.finfo(np.float32).max
    hid, w, b = R.inject_logits(L)
    # every product other than L[o] * 1 is +-0: four partial sums over K quarters, a fixed tree, + bias, all in f32
    part = [(hid[:, q:q + 128].astype(np.float64) @ w[:, q:q + 128].T.astype(np.float64)).astype(np.float32) for q in range(0, 512, 128)]
    out = ((part[0] + part[1]) + (part[2] + part[3])) + b
    assert out.dtype == np.float32 and np.array_equal(out, L)
    assert not any(p.any() for p in part[1:])


def test_softmax_reference_agrees_with_the_torch_oracle():
    rng = np.random.default_rng(4)
    L = (rng.standard_normal((4096, 62)) * rng.choice([0.01, 1.0, 10.0, 100.0], (4096, 1))).astype(np.float32)
    top2 = np.sort(L, axis=1)[:, -2:]
    L = L[top2[:, 1] > top2[:, 0]]                               # untied
    assert len(L) > 4000
    lab, p = R.softmax_top1_ref(L)
    tl, tp = T.rec_classify(L)
    assert np.array_equal(lab, tl)
    assert float((np.abs(p - tp) / tp).max()) <= 1e-14


def test_softmax_reference_on_the_edges_the_gpu_tests_use():
    big = np.finfo(np.float32).max
    L = np.stack([np.zeros(62), np.full(62, -1e30), np.full(62, -big), np.where(np.arange(62) == 7, 0.0, -1e5)]).astype(np.float32)
    lab, p = R.softmax_top1_ref(L)
    assert lab.tolist() == [0, 0, 0, 7]
    assert np.allclose(p[:3], 1 / 62, rtol=1e-15, atol=0) and p[3] == 1.0


@pytest.mark.parametrize("name", [c[0] for c in R.REAL_CASES])
def test_rms_bar_keeps_out_bf16_activations_and_a_three_product_split(name):
    case = R.real_case(name)
    bar = case.bar()
    chain_max = float(case.errors(case.chain()).max())
    rounded, three = case.rms(case.bf16_activation()), case.rms(case.three_products())
    print(f"{name}: chain rms {bar / R.RMS_FACTOR:.3g}  bar {bar:.3g}  chain max {chain_max:.3g} (bound {case.max_bound():.3g})  "
          f"bf16 activations {rounded:.3g} ({rounded / bar:.0f} x)  three products {three:.3g} ({three / bar:.0f} x)")
    assert case.keep.mean() > 0.3                                # fc1: about half of the references are positive
    assert chain_max <= case.max_bound()                         # the sequential chain itself meets the a-priori bound
    assert rounded >= KEEP_OUT * bar and three >= KEEP_OUT * bar
