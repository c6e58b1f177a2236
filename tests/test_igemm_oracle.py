"""tests/igemm_oracle.py without a GPU: the f64 evaluation against torch's convs, the integer families (exact, and - for the split form's
three - sensitive to every product they are meant to pin), and the stand-in: without a fault it passes every check that
tests/test_gpu_igemm_kernels.py makes of the kernel, with any of its named faults it fails at least one."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import igemm_oracle as O
from tests import split_bf16_emul as E

f64 = np.float64


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, f64).transpose(0, 3, 1, 2)))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


# ---- the evaluation is the definition ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ks,stride,grid", [(1, 1, (2, 3, 5)), (3, 1, (2, 5, 4)), (3, 1, (1, 1, 1)), (1, 2, (2, 5, 6)), (3, 2, (2, 5, 6)), (3, 2, (1, 6, 7))], ids=str)
def test_conv_is_torch_conv2d(ks, stride, grid):
    rng = np.random.default_rng(ks + stride)
    x, w = rng.standard_normal(grid + (6,)), rng.standard_normal((5, ks * ks, 6))
    want = F.conv2d(_nchw(x), torch.from_numpy(w.reshape(5, ks, ks, 6).transpose(0, 3, 1, 2).copy()), stride=stride, padding=(ks - 1) // 2)
    assert np.abs(O.conv(x, w, stride) - _nhwc(want)).max() < 1e-12


def test_shuffled_1x1_conv_is_torch_conv_transpose2d():
    rng = np.random.default_rng(3)
    x, wt = rng.standard_normal((2, 3, 5, 8)), rng.standard_normal((8, 64, 2, 2))      # conv_transpose2d's weight: [cin][co][a][b]
    w = wt.transpose(2, 3, 1, 0).reshape(256, 1, 8)                                     # row (2 a + b) 64 + co
    bias = rng.standard_normal(64)
    l = O.Launch(O.F32, False, 1, 1, (2, 3, 5), 8, 256, store=O.SHUFFLE2)
    got, _ = O.finish(l, O.accumulate(l, x, w), bias=np.tile(bias, 4), relu=True)
    want = F.relu(F.conv_transpose2d(_nchw(x), torch.from_numpy(wt.copy()), torch.from_numpy(bias), stride=2))
    assert got.shape == (2, 6, 10, 64) and np.abs(got - _nhwc(want)).max() < 1e-12


def test_concat_and_top_down_sum_are_torch_interpolate():
    rng = np.random.default_rng(4)
    levels = [rng.standard_normal((2, 8 >> (3 - i), 16 >> (3 - i), 64)) for i in range(4)]
    want = torch.cat([F.interpolate(_nchw(a), scale_factor=8 >> i, mode="nearest") if i < 3 else _nchw(a) for i, a in enumerate(levels)], dim=1)
    assert np.array_equal(O.concat4(levels), _nhwc(want))
    l = O.Launch(O.F32, False, 1, 1, (2, 4, 6), 8, 64)
    acc, up, res = rng.standard_normal((2, 4, 6, 64)), rng.standard_normal((2, 2, 3, 64)), rng.standard_normal((2, 4, 6, 64))
    sc, bi = rng.standard_normal(64), rng.standard_normal(64)
    out, out2 = O.finish(l, acc, sc, bi, res, up, relu=True)
    v = np.maximum(acc * sc + bi + res, 0)
    assert np.array_equal(out, v) and np.abs(out2 - (v + _nhwc(F.interpolate(_nchw(up), scale_factor=2, mode="nearest")))).max() < 1e-15


def test_batched_gemm_is_b_products():
    rng = np.random.default_rng(5)
    x, w = rng.standard_normal((3, 1, 1, 7, 32)), rng.standard_normal((3, 64, 1, 32))
    l = O.Launch(O.F32, False, 1, 1, (1, 1, 7), 32, 64, batch=3)
    assert np.abs(O.accumulate(l, x, w) - np.einsum("bnhwk,bck->bnhwc", x, w[:, :, 0])).max() < 1e-12


# ---- the integer families ---------------------------------------------------------------------------------------------------------------------

def test_every_integer_case_is_exact():
    """operands() asserts the 2^24 bound and f32 exactness per epilogue; here: every launch of the GPU file builds, and both families meet
    every form and (ks, stride)"""
    seen = set()
    for l in O.all_launches():
        O.operands(l.shape_key(), O.family_of(l))
        seen.add((l.form, l.ks, l.stride, O.family_of(l)))
    assert seen >= {(f, ks, s, fam) for f in (O.F32, O.SPLIT, O.BF16) for ks, s in O.KS_STRIDE for fam in O.INT_FAMILIES}
    for l in O.split_launches():
        for fam in O.SPLIT_FAMILIES:
            O.operands(l.shape_key(), fam)


@pytest.mark.parametrize("family", O.SPLIT_FAMILIES)
@pytest.mark.parametrize("l", O.split_launches()[::2], ids=lambda l: l.name())
def test_split_families_pin_their_products(l, family):
    """six products give the integer result bit for bit (the three dropped ones are zero), and without any product the family pins they do not"""
    o = O.operands(l.shape_key(), family)
    cc = E.ConvCase(o.x, o.w, l.stride, kgroup=32)
    want = o.acc.astype(np.float32)
    assert np.array_equal(cc.emulated(), want)
    for d, name in enumerate(E.PRODUCT_NAMES):
        out = cc.emulated(tuple(p for q, p in enumerate(E.PRODUCTS) if q != d))
        assert np.array_equal(out, want) == (name not in O.PINNED[family]), (family, name)


# ---- the stand-in -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("part", range(4))
def test_the_stand_in_is_exact_on_every_launch_of_g1(part):
    for l in [l for l in O.all_launches() if l.tile in (0, 2)][part::4]:      # the model's only use of the tile is the row it drops under a fault
        O.check_g1(O.standin, l)
    for l in O.split_launches()[::2][part::4]:
        for fam in O.SPLIT_FAMILIES:
            O.check_g1(O.standin, l, fam)


L = O.Launch
SECTION3 = [
    ("g1 3x3 s1 f32", lambda run: O.check_g1(run, L(O.F32, False, 3, 1, (2, 9, 17), 64, 256, tile=3), "signed")),
    ("g1 3x3 s2 split", lambda run: O.check_g1(run, L(O.SPLIT, False, 3, 2, (2, 10, 18), 32, 64, tile=2), "signed")),
    ("g1 1x1 lateral bf16", lambda run: O.check_g1(run, L(O.BF16, True, 1, 1, (2, 6, 10), 64, 64, tile=3), "signed")),
    ("g1 shuffle", lambda run: O.check_g1(run, L(O.F32, False, 1, 1, (2, 3, 5), 64, 256, store=O.SHUFFLE2, tile=3), "signed")),
    ("g1 cat4", lambda run: O.check_g1(run, L(O.F32, False, 3, 1, (2, 8, 16), 256, 64, src=O.CAT4, tile=3), "signed")),
    ("g1 batched", lambda run: O.check_g1(run, L(O.F32, False, 1, 1, (1, 1, 63), 64, 64, batch=3, tile=3), "signed")),
    ("g1 split wide_w", lambda run: O.check_g1(run, O.split_launches()[0], "wide_w")),
    ("g1 split mid", lambda run: O.check_g1(run, O.split_launches()[0], "mid")),
    ("g2 3x3 s1 f32", lambda run: O.check_g2(run, L(O.F32, False, 3, 1, (3, 5, 3), 32, 64, tile=3), report=lambda s: None)),
    ("g2 3x3 s1 bf16", lambda run: O.check_g2(run, L(O.BF16, True, 3, 1, (3, 5, 3), 64, 64, tile=3), report=lambda s: None)),
    ("g3 M = 65", lambda run: O.check_g3(run, L(O.F32, False, 3, 1, (1, 5, 13), 32, 64, tile=3))),
    ("g3 out2", lambda run: O.check_g3(run, L(O.F32, False, 1, 1, (2, 6, 10), 32, 64, tile=3))),
    ("g4 poison", lambda run: O.check_g4_poison(run, L(O.F32, False, 3, 1, (3, 5, 3), 32, 64, tile=3))),
    ("g4 poison cat4", lambda run: O.check_g4_poison(run, L(O.BF16, True, 3, 1, (2, 8, 16), 256, 64, src=O.CAT4, tile=3))),
    ("g4 batch", lambda run: O.check_g4_batch(run, L(O.F32, False, 3, 1, (3, 5, 3), 32, 64, tile=3))),
    ("g4 alone", lambda run: O.check_g4_alone(run, L(O.SPLIT, False, 3, 1, (3, 5, 9), 32, 64, tile=2))),
    ("g5 split", lambda run: O.check_g5(run, O.G5_CASES[0], O.SPLIT, 2, report=lambda s: None)),
    ("g5 batched", lambda run: O.check_g5(run, O.G5_CASES[5], O.F32, 3, report=lambda s: None)),
]


def test_the_stand_in_passes_every_check():
    for name, check in SECTION3:
        check(O.standin)


@pytest.mark.parametrize("fault", O.FAULTS)
def test_every_named_fault_fails_a_check(fault):
    def run(*a, **kw):
        return O.standin(*a, fault=fault, **kw)
    caught = []
    for name, check in SECTION3:
        try:
            check(run)
        except AssertionError:
            caught.append(name)
    print(f"{fault}: caught by {caught}")
    assert caught, fault


def test_the_stand_in_refuses_what_check_refuses():
    for name, _, kw in O.refused_combinations():
        with pytest.raises(O.Refused):
            O.standin(**kw)
