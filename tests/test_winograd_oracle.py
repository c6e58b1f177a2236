"""tests/winograd_oracle.py held to itself, and the host side of the Winograd convs held to it (no GPU):

  * the two f64 statements of the conv agree (definition against the documented matrices, F(4x4) and F(2x2));
  * winograd_weights (engine.hip, through its hook) is G g G^T rounded ONCE: within half an f32 ulp of the f64 value, which a transform
    computed with an f32 G is not; on weights 576 k it is exactly integral;
  * winograd43_fragments (winograd43_fused.hip, through its hook) has the layout its comment states, and three plausible other layouts differ;
  * the integer families keep every value of the pipeline below 2^24 (asserted by the builder) for every Cin in use;
  * the real-valued families keep five split-bf16 products at least 5 x above six, and V rounded to bf16 at least 1000 x above the bar;
  * the numpy stand-in passes every assertion of tests/test_gpu_winograd_kernels.py, and each deliberately wrong stand-in fails at least one.

Largest element (W4's second bar, 10 x the emulation's largest): every STRUCTURAL fault of the stand-in exceeds it by far more than 100 x.
A dropped product does NOT - its largest element stays within a few times the bar (it moves a result by ~1e-7 of the norm, which is what
a maximum over 1e5 elements of a correct kernel looks like too); the rms bar is what notices it, and test_a_dropped_product_is_an_rms_finding
says so with figures."""
import functools

import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from tests import split_bf16_emul as E
from tests import winograd_oracle as O

f32, f64 = np.float32, np.float64
fast = functools.partial(O.standin, gemm=O.gemm_exact)      # integer cases: every order of the sums is exact, so take the quickest


# ---- the two statements ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [4, 2])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 7, 9), (1, 8, 4), (3, 5, 13)])
def test_definition_and_matrices_agree(m, shape):
    rng = np.random.default_rng(sum(shape) + m)
    x = rng.standard_normal(shape + (24,))
    w = rng.standard_normal((16, 9, 24))
    want, got = O.direct_conv(x, w), O.by_matrices(x, w, m)
    mag = O.direct_conv(np.abs(x), np.abs(w))
    assert got.shape == want.shape
    assert (np.abs(got - want) <= 1e-12 * mag).all(), float((np.abs(got - want) / mag).max())


def test_the_f32_steps_are_the_matrices():
    """bt6 / at6 / bt4 / at4 as the kernels write them against B^T and A^T"""
    rng = np.random.default_rng(3)
    for step, mat in ((O.bt6, O.BT[4]), (O.at6, O.AT[4]), (O.bt4, O.BT[2]), (O.at4, O.AT[2])):
        d = rng.integers(-9, 10, (mat.shape[1], 50)).astype(f64)
        assert np.array_equal(np.stack(step(list(d))), mat @ d)


# ---- winograd_weights ---------------------------------------------------------------------------------------------------------------------

def _half_ulp_off(u, exact):
    """elements of f32 u further from the f64 value than half an ulp (+ 1e-12 relative for the f64 evaluation itself)"""
    return np.abs(u.astype(f64) - exact) > 0.5 * np.spacing(np.abs(u)).astype(f64) + 1e-12 * np.abs(exact)


@pytest.mark.parametrize("m", [4, 2])
def test_winograd_weights_are_rounded_once(m):
    rng = np.random.default_rng(40 + m)
    w = (rng.standard_normal((32, 9, 48)) / 20).astype(f32)
    u = capi.winograd_weights(w, m)
    exact = O.weight_transform(w, m)
    assert u.shape == exact.shape and u.dtype == f32
    assert not _half_ulp_off(u, exact).any(), int(_half_ulp_off(u, exact).sum())
    # the same transform with G and every intermediate in f32 is NOT within half an ulp: the check notices a second rounding
    g32 = O.G[m].astype(f32)
    t = np.einsum("ip,kpqc->kiqc", g32, w.reshape(32, 3, 3, 48)).astype(f32)
    u32 = np.einsum("kiqc,jq->ijkc", t, g32).astype(f32).reshape(exact.shape)
    share = float(_half_ulp_off(u32, exact).mean())
    print(f"F({m}x{m}): an f32 transform is beyond half an ulp in {share:.1%} of the elements")
    assert share > (0.05 if m == 4 else 0.01)


@pytest.mark.parametrize("m", [4, 2])
def test_winograd_weights_of_multiples_of_576_are_integers(m):
    rng = np.random.default_rng(41)
    w = (576 * rng.integers(-3, 4, (16, 9, 32))).astype(f32)
    u = capi.winograd_weights(w, m)
    assert np.array_equal(u, np.rint(u)) and np.array_equal(u.astype(f64), O.weight_transform_576(w, m))
    assert np.abs(u).max() > 576


# ---- winograd43_fragments -----------------------------------------------------------------------------------------------------------------

def _fragment_layout(u, lane_cout=lambda wv, l: 16 * wv + (l & 15), cin_of=lambda l, e: 4 * (l >> 4) + e, chunk_major=True):
    """[Cout/64][Cin/16][36][wave][lane][4] written out from the comment above winograd43_fragments"""
    comps, cout, cin = u.shape
    f = np.empty((cout // 64, cin // 16, 36, 4, 64, 4), f32)
    for wv in range(4):
        for l in range(64):
            for e in range(4):
                for kb in range(cout // 64):
                    for c in range(cin // 16):
                        f[kb, c, :, wv, l, e] = u[:, kb * 64 + lane_cout(wv, l), 16 * c + cin_of(l, e)]
    return f if chunk_major else np.ascontiguousarray(f.transpose(0, 2, 1, 3, 4, 5)).reshape(f.shape)


def test_winograd43_fragments_have_the_documented_layout():
    rng = np.random.default_rng(43)
    u = rng.permutation(36 * 128 * 32).astype(f32).reshape(36, 128, 32)      # every value once: a misplaced element cannot hide
    got = capi.winograd43_fragments(u)
    assert np.array_equal(got, _fragment_layout(u))
    wrong = {"lane and wave swapped": np.ascontiguousarray(_fragment_layout(u).transpose(0, 1, 2, 4, 3, 5)).reshape(got.shape),     # [lane][wave] in memory
             "4 e + (l >> 4)": _fragment_layout(u, cin_of=lambda l, e: 4 * e + (l >> 4)),
             "component-major": _fragment_layout(u, chunk_major=False)}
    for name, f in wrong.items():
        assert sorted(f.ravel()) == sorted(got.ravel()), name       # a permutation of the same values ...
        assert not np.array_equal(got, f), name                      # ... and a different one


# ---- integer families --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cin", sorted(O.INT_FAMILIES))
def test_integer_families_stay_below_2_to_24(cin):
    """integer_case asserts the bound and the non-zero share per epilogue; here: for every Cin, at the largest and the smallest shape in use"""
    for shape in ((1, 1, 1), (3, 17, 33)):
        c = O.integer_case(shape, cin, 64)
        assert c.bound * 1.02 < O.LIMIT and np.array_equal(c.x, np.rint(c.x)) and np.array_equal(c.w / 576, np.rint(c.w / 576))
        assert set(np.abs(c.scale)) <= {1.0, 2.0, 4.0}
        print(f"Cin {cin} {shape}: bound {c.bound:.3g} of {O.LIMIT:.3g}")


def test_integer_split_has_no_lo_term():
    c = O.integer_case((2, 15, 17), 256, 64)
    v = O._both_ways(O.patches(c.x, 4), O.bt6)
    for a in (v, O.weight_transform_576(c.w, 4).astype(f32)):
        hi, mid, lo = E.split3(a)
        assert not lo.any() and np.array_equal(hi + mid, a)


@pytest.mark.parametrize("kblocks", [1, 2, 4])
def test_fused_walk_visits_every_block_once(kblocks):
    for cus in O.W2_CUS + (0,):
        walks = O.fused_walk(18, kblocks, cus)
        assert sorted(b for wk in walks for b in wk) == list(range(18 * kblocks)), cus
        assert all(len({b % kblocks for b in wk}) <= 1 for wk in walks), cus     # a workgroup keeps its output-channel block
    assert max(len(wk) for wk in O.fused_walk(18, 1, 1)) == 9 and max(len(wk) for wk in O.fused_walk(18, 1, 40)) == 2


# ---- rms cases ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", O.W4_FAMILIES)
@pytest.mark.parametrize("forms,cin,cout,shape", O.W4_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_families_separate_five_products_from_six(forms, cin, cout, shape, family):
    case = O.wino_case(cin, cout, shape, family)
    six, five, bar, names, chain, big_six, big_chain = O.wino_bar(cin, cout, shape, family)
    vb = case.rms(case.v_bf16())
    ratio = float(np.median(case.norm / case.direct_norm))
    print(f"{cin} -> {cout} {shape} {family}: six {six:.3g}  five {five:.3g} ({five / six:.1f} x, drops {names})  chain {chain:.3g}  bar {bar:.3g}  "
          f"V in bf16 {vb:.3g} ({vb / bar:.0f} x the bar)  largest six {big_six:.3g} chain {big_chain:.3g}  left out {case.left_out:.2f}  "
          f"Winograd norm / direct norm {ratio:.2f}")
    assert case.left_out < 0.6
    assert set(names) >= set(E.PRODUCT_NAMES[:3])
    assert five >= 5 * six
    assert vb >= 1000 * bar
    assert chain <= bar and six <= bar


# ---- the stand-in passes what the GPU file asserts ... ----------------------------------------------------------------------------------------

def test_standin_is_exact_on_the_integer_families_with_its_own_gemms():
    """the model's six products and its f32 chain, not the quick exact product"""
    O.check_w1(O.standin, O.FUSED, (2, 15, 17), 64, 64)
    O.check_w1(O.standin, O.SPLIT3, (3, 3, 5), 256, 64)
    O.check_w1(O.standin, O.F32_3, (3, 3, 5), 256, 64)
    O.check_w1(O.standin, O.F22, (3, 3, 5), 256, 64)


@pytest.mark.parametrize("shape", [(3, 1, 1), (1, 4, 4), (2, 15, 17), (1, 16, 16), (2, 17, 33), (1, 33, 17), (1, 5, 40)])
def test_standin_passes_w1_fused(shape):
    for cin, cout in ((64, 64), (128, 192)) if shape != (2, 15, 17) else ((64, 64), (64, 128), (128, 64), (128, 128), (256, 64), (256, 128), (128, 192), (64, 256)):
        O.check_w1(fast, O.FUSED, shape, cin, cout)


@pytest.mark.parametrize("form", [O.SPLIT3, O.F32_3, O.F22])
def test_standin_passes_w1_three_launch(form):
    for shape in ((1, 1, 1), (3, 3, 5), (1, 9, 21), (3, 9, 21), (3, 17, 33)):
        O.check_w1(fast, form, shape, 256, 64)
    O.check_w1(fast, form, (3, 3, 5), 256, 256)
    O.check_w1(fast, form, (3, 3, 5), 512, 512)


def test_standin_passes_w2_and_w3():
    O.check_w2(fast, 64, 64)
    for form in (O.FUSED, O.SPLIT3, O.F32_3, O.F22):
        for shape in O.w3_shapes(form):
            O.check_w3(fast, form, shape, 64 if form == O.FUSED else 256, 64)


@pytest.mark.parametrize("forms,cin,cout,shape", O.W4_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_standin_passes_w4(forms, cin, cout, shape):
    for family in O.W4_FAMILIES:
        O.check_w4(O.standin, forms, cin, cout, shape, family)


# ---- ... and every wrong stand-in fails one -----------------------------------------------------------------------------------------------

def _faulty(fault, gemm=O.gemm_exact):
    return functools.partial(O.standin, fault=fault, gemm=gemm)


# fault -> the assertion of the GPU file that must notice it
CAUGHT_BY = {
    "halo_right": lambda run: O.check_w1(run, O.FUSED, (1, 4, 4), 64, 64),
    "top_halo": lambda run: O.check_w1(run, O.F32_3, (3, 3, 5), 256, 64),
    "stale_patch": lambda run: O.check_w2(run, 64, 64),
    "ragged_row": lambda run: O.check_w1(run, O.FUSED, (2, 15, 17), 64, 64),
    "inplace_late": lambda run: O.check_w1(run, O.FUSED, (1, 4, 4), 64, 64),
    ("drop", 0): lambda run: O.check_w4(run, (O.SPLIT3, O.F32_3), 512, 512, (1, 8, 8), "relu"),
    ("drop", 1): lambda run: O.check_w4(run, (O.SPLIT3, O.F32_3), 512, 512, (1, 8, 8), "offset"),
    ("drop", 2): lambda run: O.check_w4(run, (O.SPLIT3, O.F32_3), 256, 256, (2, 9, 21), "relu"),
    "kb_block0": lambda run: O.check_w1(run, O.FUSED, (1, 4, 4), 64, 128),
}


@pytest.mark.parametrize("fault", O.FAULTS, ids=str)
def test_every_wrong_standin_fails_an_assertion(fault):
    drop = isinstance(fault, tuple)
    with pytest.raises(AssertionError):
        CAUGHT_BY[fault](_faulty(fault, None if drop else O.gemm_exact))


def test_poison_shows_a_failed_mask_as_nan():
    """the front region is what the three-launch input transform would read for the row above image 0 and the pixel left of its rows"""
    case = O.integer_case((2, 5, 5), 256, 64)
    sc, bi, rs, inplace = case.operands("scale_bias")
    out, _ = O.standin(O.F32_3, case.x, case.w, scale=sc, bias=bi, poison=True, fault="halo_right", gemm=O.gemm_exact)
    assert np.isnan(out).any()
    with pytest.raises(AssertionError):
        O.check_w3(_faulty("halo_right"), O.F32_3, (2, 5, 5), 256, 64)


# structural fault -> (case of W4, form, what the run needs) on which its largest element is compared with W4's second bar
STRUCTURAL = {
    "halo_right": ((64, 64, (2, 20, 24)), O.FUSED, {}),
    "top_halo": ((64, 64, (2, 20, 24)), O.FUSED, {}),
    "stale_patch": ((64, 64, (2, 20, 24)), O.FUSED, {"num_cus": 1}),
    "ragged_row": ((128, 64, (1, 13, 37)), O.FUSED, {}),
    "kb_block0": ((256, 256, (2, 9, 21)), O.F32_3, {}),
}


@pytest.mark.parametrize("family", O.W4_FAMILIES)
@pytest.mark.parametrize("fault", sorted(STRUCTURAL))
def test_structural_faults_exceed_the_largest_element_bar_100_fold(fault, family):
    (cin, cout, shape), form, kw = STRUCTURAL[fault]
    case = O.wino_case(cin, cout, shape, family)
    big_chain = O.wino_bar(cin, cout, shape, family)[6]
    big = case.largest(case.run(_faulty(fault, None), form, **kw))
    print(f"{fault} {family}: largest element {big:.3g}, the bar {O.MAX_FACTOR * big_chain:.3g} ({big / (O.MAX_FACTOR * big_chain):.3g} x)")
    assert big >= 100 * O.MAX_FACTOR * big_chain


def test_a_late_inplace_residual_exceeds_the_largest_element_bar_100_fold():
    case = O.wino_case(64, 64, (2, 20, 24), "relu")
    big_chain = O.wino_bar(64, 64, (2, 20, 24), "relu")[6]
    res = np.random.default_rng(5).standard_normal(case.ref.shape).astype(f32)
    kw = dict(scale=case.scale, bias=case.bias, residual=res, inplace=True)
    ref = O.epilogue(O.direct_conv(case.x, case.w), case.scale, case.bias, res)
    norm = case.norm + np.abs(res)
    good, _ = O.standin(O.FUSED, case.x, case.w, **kw)
    bad, _ = O.standin(O.FUSED, case.x, case.w, fault="inplace_late", **kw)
    assert float((np.abs(good - ref) / norm).max()) <= O.MAX_FACTOR * big_chain
    assert float((np.abs(bad - ref) / norm).max()) >= 100 * O.MAX_FACTOR * big_chain


@pytest.mark.parametrize("d", [0, 1, 2])
def test_a_dropped_product_is_an_rms_finding(d):
    """it stays under 100 x the largest-element bar - that bar cannot see it - and above the rms bar, on every family of the split form"""
    for _, cin, cout, shape in O.W4_CASES[3:]:
        for family in O.W4_FAMILIES:
            case = O.wino_case(cin, cout, shape, family)
            six, five, bar, names, chain, big_six, big_chain = O.wino_bar(cin, cout, shape, family)
            out = case.run(_faulty(("drop", d), None), O.SPLIT3)
            rms, big = case.rms(out), case.largest(out)
            print(f"drop {E.PRODUCT_NAMES[d]} {cin} -> {cout} {family}: rms {rms:.3g} (bar {bar:.3g}, {rms / bar:.1f} x)  largest {big:.3g} ({big / (O.MAX_FACTOR * big_six):.2f} x its bar)")
            assert rms > bar
            assert big < 100 * O.MAX_FACTOR * big_six
