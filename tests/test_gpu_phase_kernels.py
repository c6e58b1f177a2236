"""Kernel-level tests of conv_igemm's STORE_PHASE and SRC_PYR4 forms - the low-resolution convs the detector's composed FPN and bin_conv1
run by default - through ocr_test_phase_conv_run / ocr_test_pyr4_conv_run: ONE launch (or the engine's pair of launches) on caller data,
against tests/phase_conv_oracle.py's f64 evaluation of the SAME built weights (phase_eval / pyr4_eval: what the kernel's operands mean by
the layout the comments state; tests/test_phase_conv_oracle.py holds that evaluation to the definition without a GPU).

Inputs: N(0,1) activations, taps N(0,1) / sqrt(9 cin) merged by the engine's own builders, the images of a batch scaled 1, 16, 1/16.

K1 parity       every form against the oracle, without an epilogue, with bias + ReLU, with a residual (PHASE: in place, PYR4: separate) + bias + ReLU
                  f32 results  |err| <= 4e-6 (sum |a||b| + |bias| + |residual|) per element AND max |err| <= 2e-5 of the tensor's maximum
                  bf16 results the recipe of tests/test_gpu_conv_kernel.py::_check: reference from the rounded operands, one bf16 ulp + 1e-5 of
                               the scale, fewer than 1 % of the elements beyond 1e-5 of the scale
K2 same bits    win = 1 against win = 0, launches = 3 (phase blocks, then corners) against one launch
K3 who writes   pyr_group 1 writes exactly the 60 phases with (y mod 8, x mod 8) not both in {0, 7}, pyr_group 2 exactly the other four,
                the window-indexed form writes every element; guard rows behind the output come back untouched - asserted for EVERY launch
                of this file
K4 poison       NaN around the source(s) inside their allocation: finite results, the bits of the unpoisoned run
K5 lost product rms(kernel - f64) <= sqrt(rms_six x min rms_five) (docs/split_bf16_error.md), split bf16 and exact f32 alike

The combinations conv_igemm.hip's check() accepts, each launched by K1 (the engine's use in brackets):

  STORE_PHASE / SRC_PLAIN, up 2 | 4 | 8
    exact f32            win 0                      [mfma=f32: fpn.upsampled up 2, bin_conv1.upsampled up 2 / 4 / 8 with bin_pyr=0]
    split bf16           win 0                      [default f32 engine with phase_windows=0; up 4 / 8 with bin_pyr=0]
    split bf16           win 1 (up 2, Cout 64)      [default f32 engine: fpn.upsampled 128 -> 64 and 256 -> 64]
    bf16 -> bf16         win 0, win 1 (up 2)        [bf16 precision: fpn.upsampled; up 4 / 8 are never selected]
    bf16 -> f32          win 0, win 1 (up 2)        [never selected by the engine: its bf16 phase convs write bf16]
  SRC_PYR4 (STORE_PHASE, up 8, 64 -> 64)
    exact f32            nsrc 3, nsrc 4, group 0    [mfma=f32: nsrc 3 with p2 as a Winograd conv, nsrc 4 without it]
    split bf16           nsrc 3, group 0            [pyr_grouped=0]
    split bf16           nsrc 3, groups 1 then 2    [default f32 engine]
    bf16 -> bf16         nsrc 3 | 4, group 0        [bf16 precision: nsrc 4 without pyr_p2_direct, nsrc 3 with pyr_grouped=0]
    bf16 -> bf16         nsrc 3, groups 1 then 2    [bf16 precision, default]
    bf16 -> f32          nsrc 3 | 4, group 0; nsrc 3, groups 1 then 2   [never selected: the bf16 engine's pyramid writes bf16]
  (pyr_group 1 or 2 ALONE is what K3 launches.)  check() refuses everything else - f32 operands with bf16 results, win or pyr_group on the
  exact-f32 form, win with up 4 / 8, the split form with four sources - and the hooks pass the refusal on: test_refused_combinations.
"""
import functools

import numpy as np
import pytest
import torch

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from ocr_rs_amd import weights as W
from tests import phase_conv_oracle as O
from tests import split_bf16_emul as E

pytestmark = pytest.mark.gpu

SENTINEL = -7.0     # below every ReLU output, exact in bf16
F32, SPLIT, BF16 = 0, 1, 2
FORM_NAMES = {F32: "f32", SPLIT: "split", BF16: "bf16"}


@pytest.fixture(scope="module")
def det():
    d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    yield d
    d.close()


def _q(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _ids(v):
    """a parameter's id: tuples as 2x3x5, flags as 0 / 1"""
    return "x".join(str(int(e)) if isinstance(e, bool) else str(e) for e in v) if isinstance(v, tuple) else str(v)


def _check_f32(name, got, ref, mag):
    """the per-element bar of test_conv_split_bf16_wide_exponents and the 2e-5 of the scale of test_gpu_conv_kernel._check"""
    err = np.abs(got.astype(np.float64) - ref)
    scale = float(np.abs(ref).max()) + 1e-12
    print(f"{name}: max |err| / sum|a||b| {float((err / mag).max()):.3g}  max |err| / scale {float(err.max()) / scale:.3g}")
    assert np.isfinite(got).all()
    assert (err <= 4e-6 * mag).all(), float((err / mag).max())
    assert float(err.max()) / scale < 2e-5


def _check_bf16(name, got, ref):
    """tests/test_gpu_conv_kernel.py::_check for bf16 results"""
    scale = float(np.abs(ref).max()) + 1e-12
    refq = _q(ref)
    tol = np.abs(refq) * 2.0 ** -7 + 1e-5 * scale
    diff = np.abs(got - refq)
    print(f"{name}: max (diff - tol) {float((diff - tol).max()):.3g}  beyond 1e-5 of the scale {float((diff > 1e-5 * scale).mean()):.4f}")
    assert (diff <= tol).all(), float((diff - tol).max())
    assert float((diff > 1e-5 * scale).mean()) < 0.01


def _untouched(guard):
    assert guard.size and (guard == SENTINEL).all(), "the launch wrote behind its output"


# ---- PHASE ---------------------------------------------------------------------------------------------------------------------------

PHASE_GRIDS = [(1, 1, 1),       # every window crosses every border
               (2, 3, 5),       # ragged
               (3, 1, 7), (2, 7, 1),   # one row, one column
               (2, 12, 20),
               (2, 32, 16),     # M = 1024: 8 row tiles of 128, 16 of 64, the chunked tile order
               (1, 33, 35)]     # M = 1155: a partial last tile, the plain order
PHASE_CHANNELS = [(128, 64, 2), (256, 64, 2),            # the FPN's fpn_b_
                  (64, 64, 2), (64, 64, 4), (64, 64, 8)]  # bin_up_
# form, win, bf16 results
PHASE_FORMS = [(F32, 0, False), (SPLIT, 0, False), (SPLIT, 1, False), (BF16, 0, True), (BF16, 1, True), (BF16, 0, False), (BF16, 1, False)]


def _guard_rows(grid, up):
    return 2 * up * grid[2] + 64     # more than two output rows


@functools.lru_cache(maxsize=2)
def _phase_case(grid, chans):
    """operands and the f64 accumulators of the f32 and of the bf16-rounded operands (computed once, shared, never modified)"""
    cin, cout, up = chans
    rng = np.random.default_rng(1000 * cin + 10 * up + sum(grid))
    x = O.activations(rng, *grid, cin)
    wp = capi.phase_weights(O.taps(rng, cout, cin), up)
    bias = rng.standard_normal(cout).astype(np.float32)
    res = O.activations(rng, grid[0], up * grid[1], up * grid[2], cout)
    case = {"x": x, "w": wp, "bias": bias, "res": res, "up": up}
    for bf in (False, True):
        xx, ww = (_q(x), _q(wp)) if bf else (x, wp)
        case["acc", bf] = O.phase_eval(xx, ww, up)
        case["mag", bf] = O.phase_eval(np.abs(xx), np.abs(ww), up)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


EPILOGUES = ("plain", "bias_relu", "residual_bias_relu")


def _phase_run(det, case, form, win, out_bf16, epi, grid, poison=False):
    bias = None if epi == "plain" else case["bias"]
    res = case["res"] if epi == "residual_bias_relu" else None
    out, guard = det.debug_phase_conv_run(form, case["x"], case["w"], case["up"], win, out_bf16, bias, epi != "plain", res, poison,
                                          _guard_rows(grid, case["up"]), SENTINEL)
    _untouched(guard)
    return out


def _phase_cases(forms, grids=PHASE_GRIDS):
    return [(g, c, f) for g in grids for c in PHASE_CHANNELS for f in forms if not (f[1] and c[2] != 2)]


@pytest.mark.parametrize("grid,chans,form", _phase_cases(PHASE_FORMS), ids=_ids)
def test_k1_phase_conv_matches_the_oracle(det, grid, chans, form):
    fm, win, out_bf16 = form
    case = _phase_case(grid, chans)
    bf = fm == BF16
    for epi in EPILOGUES:
        got = _phase_run(det, case, fm, win, out_bf16, epi, grid)
        bias = None if epi == "plain" else case["bias"]
        res = case["res"] if epi == "residual_bias_relu" else None
        if res is not None and out_bf16:
            res = _q(res)       # the in-place residual is the bf16 output buffer
        ref = O.epilogue(case["acc", bf], bias, res, epi != "plain")
        name = f"phase {grid} {chans} {FORM_NAMES[fm]} win {win} {epi}"
        if out_bf16:
            _check_bf16(name, got, ref)
        else:
            _check_f32(name, got, ref, O.magnitude(case["mag", bf], bias, res))


@pytest.mark.parametrize("grid,chans,form", [c for c in _phase_cases([(SPLIT, 1, False), (BF16, 1, True), (BF16, 1, False)])], ids=_ids)
def test_k2_window_indexed_phase_conv_has_the_bits_of_the_phase_indexed_one(det, grid, chans, form):
    fm, _, out_bf16 = form
    case = _phase_case(grid, chans)
    for epi in ("plain", "residual_bias_relu"):
        a = _phase_run(det, case, fm, 0, out_bf16, epi, grid)
        b = _phase_run(det, case, fm, 1, out_bf16, epi, grid)
        assert np.isfinite(a).all() and float(np.abs(a).max()) > 0.1
        assert np.array_equal(a, b), (epi, float(np.abs(a - b).max()))


@pytest.mark.parametrize("grid,chans,form", _phase_cases([(SPLIT, 1, False), (BF16, 1, True), (SPLIT, 0, False), (F32, 0, False), (BF16, 0, True)]), ids=_ids)
def test_k3_phase_conv_writes_every_element_and_nothing_else(det, grid, chans, form):
    """bias + ReLU, no residual: every result is >= 0, so an element the launch left alone still holds the sentinel"""
    fm, win, out_bf16 = form
    out = _phase_run(det, _phase_case(grid, chans), fm, win, out_bf16, "bias_relu", grid)
    assert (out >= 0).all(), int((out == SENTINEL).sum())


@pytest.mark.parametrize("grid,chans,form", _phase_cases(PHASE_FORMS, [(1, 1, 1), (2, 3, 5), (1, 33, 35)]), ids=_ids)
def test_k4_phase_conv_uses_no_byte_around_its_source(det, grid, chans, form):
    fm, win, out_bf16 = form
    case = _phase_case(grid, chans)
    clean = _phase_run(det, case, fm, win, out_bf16, "residual_bias_relu", grid)
    dirty = _phase_run(det, case, fm, win, out_bf16, "residual_bias_relu", grid, poison=True)
    assert np.isfinite(dirty).all(), int((~np.isfinite(dirty)).sum())
    assert np.array_equal(clean, dirty)


# ---- PYR4 ------------------------------------------------------------------------------------------------------------------------------

PYR_GRIDS = [(1, 1, 1), (2, 3, 5), (3, 1, 4), (2, 5, 1),   # small and ragged
             (3, 7, 11),     # 231 cells, plain order, ragged
             (2, 16, 16),    # 512 cells: chunked order, one chunk
             (2, 16, 32)]    # 1024 cells: two chunks
# form, nsrc, bf16 results, launches
PYR_FORMS = [(F32, 3, False, 0), (F32, 4, False, 0), (SPLIT, 3, False, 0), (SPLIT, 3, False, 3),
             (BF16, 3, True, 0), (BF16, 4, True, 0), (BF16, 3, False, 0), (BF16, 4, False, 0), (BF16, 3, True, 3), (BF16, 3, False, 3)]
PYR_GUARD = 1024


@functools.lru_cache(maxsize=2)
def _pyr_case(grid):
    n, h, w = grid
    rng = np.random.default_rng(77 + 100 * h + w)
    levels = [O.activations(rng, n, h << i, w << i, 64) for i in range(4)]
    wg = (rng.standard_normal((64, 9, 256)) / np.sqrt(9 * 256)).astype(np.float32)
    scale = ((0.5 + rng.random(64)) * rng.choice([-1.0, 1.0], 64)).astype(np.float32)
    wp = capi.pyr4_weights(wg, scale)
    bias = rng.standard_normal(64).astype(np.float32)
    res = O.activations(rng, n, 8 * h, 8 * w, 64)
    case = {"levels": levels, "w": wp, "bias": bias, "res": res}
    for bf in (False, True):
        lv, ww = ([_q(a) for a in levels], _q(wp)) if bf else (levels, wp)
        for nsrc in (3, 4):
            case["acc", bf, nsrc] = O.pyr4_eval(lv, ww, nsrc)
            case["mag", bf, nsrc] = O.pyr4_eval([np.abs(a) for a in lv], np.abs(ww), nsrc)
    for v in list(case.values()) + levels:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _pyr_run(det, case, form, nsrc, out_bf16, launches, epi, poison=False):
    bias = None if epi == "plain" else case["bias"]
    res = case["res"] if epi == "residual_bias_relu" else None
    levels = case["levels"] if nsrc == 4 else case["levels"][:3] + [None]     # three sources: the kernel gets no p2 to read
    out, guard = det.debug_pyr4_conv_run(form, levels, case["w"], nsrc, out_bf16, bias, epi != "plain", res, launches, poison, PYR_GUARD, SENTINEL)
    _untouched(guard)
    return out


@pytest.mark.parametrize("grid,form", [(g, f) for g in PYR_GRIDS for f in PYR_FORMS], ids=_ids)
def test_k1_pyr4_conv_matches_the_oracle(det, grid, form):
    fm, nsrc, out_bf16, launches = form
    case = _pyr_case(grid)
    bf = fm == BF16
    for epi in EPILOGUES:
        got = _pyr_run(det, case, fm, nsrc, out_bf16, launches, epi)
        bias = None if epi == "plain" else case["bias"]
        res = case["res"] if epi == "residual_bias_relu" else None
        if res is not None and out_bf16:
            res = _q(res)       # the residual has the results' element type
        ref = O.epilogue(case["acc", bf, nsrc], bias, res, epi != "plain")
        name = f"pyr4 {grid} {FORM_NAMES[fm]} nsrc {nsrc} launches {launches} {epi}"
        if out_bf16:
            _check_bf16(name, got, ref)
        else:
            _check_f32(name, got, ref, O.magnitude(case["mag", bf, nsrc], bias, res))


PYR_GROUPED = [(SPLIT, False), (BF16, True), (BF16, False)]


@pytest.mark.parametrize("grid,form", [(g, f) for g in PYR_GRIDS for f in PYR_GROUPED], ids=_ids)
def test_k2_phase_blocks_and_corners_have_the_bits_of_the_single_launch(det, grid, form):
    fm, out_bf16 = form
    case = _pyr_case(grid)
    for epi in ("plain", "residual_bias_relu"):
        one = _pyr_run(det, case, fm, 3, out_bf16, 0, epi)
        two = _pyr_run(det, case, fm, 3, out_bf16, 3, epi)
        assert np.isfinite(one).all() and float(np.abs(one).max()) > 0.1
        assert np.array_equal(one, two), (epi, float(np.abs(one - two).max()))


def _corner_mask(shape):
    n, hh, ww, c = shape
    y, x = np.arange(hh) % 8, np.arange(ww) % 8
    m = np.isin(y, (0, 7))[:, None] & np.isin(x, (0, 7))[None, :]
    return np.broadcast_to(m[None, :, :, None], shape)


@pytest.mark.parametrize("grid,form", [(g, f) for g in PYR_GRIDS for f in PYR_GROUPED], ids=_ids)
def test_k3_each_pyramid_launch_writes_exactly_its_phases(det, grid, form):
    """bias + ReLU: every result is >= 0 and the sentinel survives exactly where a launch wrote nothing"""
    fm, out_bf16 = form
    case = _pyr_case(grid)
    whole = _pyr_run(det, case, fm, 3, out_bf16, 0, "bias_relu")
    assert (whole >= 0).all()
    corners = _corner_mask(whole.shape)
    blocks = _pyr_run(det, case, fm, 3, out_bf16, 1, "bias_relu")
    assert (blocks[corners] == SENTINEL).all() and np.array_equal(blocks[~corners], whole[~corners])
    four = _pyr_run(det, case, fm, 3, out_bf16, 2, "bias_relu")
    assert (four[~corners] == SENTINEL).all() and np.array_equal(four[corners], whole[corners])
    assert corners.mean() == 4 / 64


@pytest.mark.parametrize("grid,form", [(g, f) for g in [(1, 1, 1), (2, 3, 5), (3, 7, 11)] for f in PYR_FORMS], ids=_ids)
def test_k4_pyr4_conv_uses_no_byte_of_a_gap_between_its_sources(det, grid, form):
    fm, nsrc, out_bf16, launches = form
    case = _pyr_case(grid)
    clean = _pyr_run(det, case, fm, nsrc, out_bf16, launches, "residual_bias_relu")
    dirty = _pyr_run(det, case, fm, nsrc, out_bf16, launches, "residual_bias_relu", poison=True)
    assert np.isfinite(dirty).all(), int((~np.isfinite(dirty)).sum())
    assert np.array_equal(clean, dirty)


# ---- what check() refuses comes back as an error ------------------------------------------------------------------------------------------

def test_refused_combinations(det):
    case = _phase_case((2, 3, 5), (64, 64, 2))
    case4 = _phase_case((2, 3, 5), (64, 64, 4))
    for fm, win, out_bf16, c in [(F32, 0, True, case), (F32, 1, False, case), (SPLIT, 0, True, case), (SPLIT, 1, False, case4), (BF16, 1, True, case4)]:
        with pytest.raises(capi.OcrError):
            det.debug_phase_conv_run(fm, c["x"], c["w"], c["up"], win, out_bf16)
    pyr = _pyr_case((2, 3, 5))
    for fm, nsrc, out_bf16, launches in [(F32, 3, False, 3), (F32, 3, True, 0), (SPLIT, 4, False, 0), (SPLIT, 3, True, 0), (BF16, 4, True, 3), (BF16, 4, False, 1)]:
        with pytest.raises(capi.OcrError):
            det.debug_pyr4_conv_run(fm, pyr["levels"], pyr["w"], nsrc, out_bf16, launches=launches)


# ---- K5: the dropped-product bar ------------------------------------------------------------------------------------------------------------

_BARS = {}


def _held_to_the_bar(key, name, case, got):
    if key not in _BARS:        # the forms of a case share operands, reference and bar
        _BARS[key] = E.bar(case)
    six, five, bar, _ = _BARS[key]
    rms = case.rms(got)
    print(f"{name}: measured rms {rms:.3g}  emulated six {six:.3g}  five {five:.3g}  bar {bar:.3g}")
    assert rms <= bar, (name, rms, bar)


@functools.lru_cache(None)
def _k5_phase(conv):
    x, wp, up = E.phase_family(conv, capi.phase_weights)
    return x, wp, up, E.PhaseCase(x, wp, up)


@pytest.mark.parametrize("conv,form,win", [(E.PHASE_CASES[0], SPLIT, 0), (E.PHASE_CASES[0], SPLIT, 1), (E.PHASE_CASES[0], F32, 0),
                                           (E.PHASE_CASES[1], SPLIT, 0), (E.PHASE_CASES[1], F32, 0)], ids=_ids)
def test_k5_phase_conv_loses_none_of_its_six_products(det, conv, form, win):
    x, wp, up, case = _k5_phase(conv)
    out, guard = det.debug_phase_conv_run(form, x, wp, up, win, guard=64, sentinel=SENTINEL)
    _untouched(guard)
    _held_to_the_bar(conv, f"PHASE{up} {conv[3]} -> {conv[4]} {conv[:3]} {FORM_NAMES[form]} win {win}", case, out)


@functools.lru_cache(None)
def _k5_pyr(conv):
    levels, wp, nsrc = E.pyr_family(conv, capi.pyr4_weights)
    return levels, wp, nsrc, E.PyrCase(levels, wp, nsrc)


@pytest.mark.parametrize("conv,form,launches", [(E.PYR_CASES[0], SPLIT, 0), (E.PYR_CASES[0], SPLIT, 3), (E.PYR_CASES[0], F32, 0)], ids=_ids)
def test_k5_pyr4_conv_loses_none_of_its_six_products(det, conv, form, launches):
    levels, wp, nsrc, case = _k5_pyr(conv)
    out, guard = det.debug_pyr4_conv_run(form, levels[:3] + [None], wp, nsrc, launches=launches, guard=PYR_GUARD, sentinel=SENTINEL)
    _untouched(guard)
    _held_to_the_bar(conv, f"PYR4 nsrc {nsrc} {conv[:3]} {FORM_NAMES[form]} launches {launches}", case, out)
