"""Kernel-level tests of the recogniser's fc1, fc2, softmax and top-1 (rec_net.hip) through the ocr_test_rec_fc1 / ocr_test_rec_fc2
hooks: one launch of the shipped launcher on caller data.  fc1 form 0 is the large-batch conv_igemm GEMM (launch_rec_fc1), form 1
rec_fc1_ksplit_kernel; fc2 form 0 is rec_fc2_softmax_kernel, form 1 rec_fc2_small_kernel.  Every call carries 8 guard rows behind the
batch, filled with -7, which must come back untouched.

F1  placement, by equality: integer operands whose every partial sum is exact in f32 (tests/rec_fc_cases.py), against int64.
F2  rows do not leak: NaN in the rows a tile reads past the batch changes nothing; a permuted batch gives the permuted result and a
    row alone gives what it gives inside a batch, bit for bit.
F3  softmax and top-1 on injected logits: exact ties (first index wins), the padding columns' mask, one-ulp margins, spreads from 0 to
    1e5 at 1e-12 relative against a long-double reference.  +-inf and NaN logits are left out: the reference yields NaN there and the
    kernels promise nothing.
F4  the f32 chains against f64: the a-priori bound (K + 2) 2^-24 of sum |a||w| + |b| on every element, and a normalised rms of at most
    twice that of a sequential K-long f32 chain emulated on the same operands.  docs/split_bf16_error.md records the measured values
    (run with -s to print them)."""
import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from ocr_rs_amd import weights as W
from tests import rec_fc_cases as R

pytestmark = pytest.mark.gpu

GUARD = 8
FORMS = {0: "large", 1: "small"}
ALL = ("logits", "labels", "probs")
FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def rec():
    r = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    yield r
    r.close()


def _fc1(rec, form, a, w, b, poison=False):
    out = rec.debug_rec_fc1(form, a, w, b, poison=poison, guard=GUARD, sentinel=-7.0)
    n = len(a)
    assert out.shape == (n + GUARD, 512)
    assert np.array_equal(out[n:], np.full((GUARD, 512), -7.0, np.float32)), "fc1 wrote behind the batch"
    return out[:n]


def _fc2(rec, form, hid, w, b, want=ALL):
    n = len(hid)
    outs = rec.debug_rec_fc2(form, hid, w, b, want=want, guard=GUARD, sentinel=-7)
    for name, o in zip(ALL, outs):
        assert (o is None) == (name not in want)
        if o is not None:
            assert len(o) == n + GUARD and (o[n:] == -7).all(), f"fc2 wrote {name} behind the batch"
    return tuple(None if o is None else o[:n] for o in outs)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _same_bits(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), (what, np.argwhere(_bits(got) != _bits(want))[:4])


# ---- F1: placement ---------------------------------------------------------------------------------------------------------------

# n around the 16-row tile of the small kernels, the 32-row MFMA tile and 64-crop workgroup of the large fc2, conv_igemm's 64 / 128 row tiles
FC1_SIZES = [(1, n) for n in (1, 15, 16, 17, 40)] + [(0, n) for n in (1, 63, 64, 65, 127, 129, 200)]
FC2_SIZES = [(1, n) for n in (1, 15, 16, 17, 40)] + [(0, n) for n in (1, 31, 32, 33, 63, 64, 65, 130)]
_ids = lambda fn: f"{FORMS[fn[0]]}-{fn[1]}"


@pytest.mark.parametrize("form_n", FC1_SIZES, ids=_ids)
def test_fc1_places_every_row_column_and_k(rec, form_n):
    form, n = form_n
    a, w, b, want = R.fc_int_case(n, 1024, 512, seed=n, relu=True)
    got = _fc1(rec, form, a, w, b)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


@pytest.mark.parametrize("form_n", FC2_SIZES, ids=_ids)
def test_fc2_places_every_row_column_and_k(rec, form_n):
    form, n = form_n
    a, w, b, want = R.fc_int_case(n, 512, 62, seed=n)
    got, _, _ = _fc2(rec, form, a, w, b, want=("logits",))
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


# ---- F2: rows do not leak ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form_n", [(1, 1), (1, 17), (0, 1), (0, 65)], ids=_ids)
def test_fc1_ignores_nan_in_the_rows_a_tile_reads_past_the_batch(rec, form_n):
    form, n = form_n
    a, w, b, want = R.fc_int_case(n, 1024, 512, seed=n, relu=True)
    got = _fc1(rec, form, a, w, b, poison=True)
    assert np.isfinite(got).all(), np.argwhere(~np.isfinite(got))[:4]
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


_BASE = {}


def _real(rec, kernel, form):
    """the real-valued case of a kernel and form (48 rows small, 130 large) and its GPU result, computed once"""
    key = (kernel, form)
    if key not in _BASE:
        case = R.real_case(f"{kernel} n={48 if form == 1 else 130}")
        run = (lambda a: (_fc1(rec, form, a, case.w, case.b),)) if kernel == "fc1" else (lambda a: _fc2(rec, form, a, case.w, case.b))
        _BASE[key] = (case, run, run(case.a))
    return _BASE[key]


@pytest.mark.parametrize("form", [1, 0], ids=FORMS.get)
@pytest.mark.parametrize("kernel", ["fc1", "fc2"])
def test_a_permuted_batch_gives_the_permuted_result(rec, kernel, form):
    case, run, base = _real(rec, kernel, form)
    perm = np.random.default_rng(5).permutation(len(case.a))
    assert (perm != np.arange(len(perm))).sum() > len(perm) // 2
    for name, got, b in zip(ALL, run(case.a[perm]), base):
        _same_bits(got, b[perm], (kernel, name))


@pytest.mark.parametrize("form", [1, 0], ids=FORMS.get)
@pytest.mark.parametrize("kernel", ["fc1", "fc2"])
def test_a_row_alone_gives_what_it_gives_inside_a_batch(rec, kernel, form):
    case, run, base = _real(rec, kernel, form)
    n = len(case.a)
    for r in ((0, 15, 16, 31, n - 1) if form == 1 else (0, 31, 32, 63, 64, 127, 128, n - 1)):
        for name, got, b in zip(ALL, run(case.a[r:r + 1]), base):
            _same_bits(got, b[r:r + 1], (kernel, name, r))


# ---- F3: softmax and top-1 on injected logits ----------------------------------------------------------------------------------------

REL_BAR = 1e-12       # 62 f64 exponentials of about an ulp, a 62-term sum, one division: a few 1e-14 expected
_WORST = {}


def _in_every_row_class(cases):
    """[m][62] -> [16 m'][62], m' = m or m + 1 odd (the first case repeated): case c sits in rows c + s m', s = 0 .. 15, and as m' is
    odd these fall into all 16 row positions of a 16-row tile"""
    cases = np.asarray(cases, np.float32).reshape(-1, 62)
    if len(cases) % 2 == 0:
        cases = np.concatenate([cases, cases[:1]])
    assert len(cases) % 2 == 1
    return np.tile(cases, (16, 1))


def _softmax_held(rec, form, L, name, bias=None, want_logits=None):
    """run fc2 on injected logits: the logits come back bit for bit, the label is the reference's exactly, p within REL_BAR relative"""
    hid, w, b0 = R.inject_logits(L)
    logits, labels, probs = _fc2(rec, form, hid, w, b0 if bias is None else bias)
    want_logits = np.asarray(L, np.float32) if want_logits is None else want_logits
    _same_bits(logits, want_logits, name)
    ref_label, ref_p = R.softmax_top1_ref(want_logits)
    assert labels.min() >= 0 and labels.max() < 62, (name, labels.min(), labels.max())
    assert np.array_equal(labels, ref_label), (name, [(int(r), int(labels[r]), int(ref_label[r])) for r in np.flatnonzero(labels != ref_label)[:4]])
    rel = np.abs(probs - ref_p) / ref_p
    worst = float(rel.max())
    _WORST[(name, form)] = worst
    print(f"{name} form {form}: {len(L)} rows, largest relative softmax error {worst:.3g} = {worst / REL_BAR:.3g} of the bar; over all cases so far {max(_WORST.values()):.3g}")
    assert worst <= REL_BAR, (name, worst, np.flatnonzero(rel > REL_BAR)[:4])
    assert (probs >= (1 - 1e-12) / 62).all() and (probs <= 1).all()
    return logits, labels, probs


TIE_PAIRS = [(4, 5), (6, 7), (0, 4), (0, 8), (0, 16), (0, 32), (0, 61), (60, 61), (31, 32), (13, 50)]


def _pair_rows(pairs, first, second, floor, later_first=False):
    """one row per pair (i, j): floor(c) everywhere, then column i = first and column j = second - written in that order, or with
    later_first the later column before the earlier one"""
    rows = []
    for i, j in pairs:
        row = np.array([floor(c) for c in range(62)], np.float32)
        for col in ((j, i) if later_first else (i, j)):
            row[col] = first if col == i else second
        rows.append(row)
    return np.stack(rows)


@pytest.mark.parametrize("form", [1, 0], ids=FORMS.get)
def test_exact_ties_go_to_the_first_index(rec, form):
    """two columns share the maximum, everything else is lower: a positive maximum with the earlier column written first, a negative
    one with the later column written first"""
    rows = np.concatenate([_pair_rows(TIE_PAIRS, t, t, lambda c: t - 1 - c / 64, later_first=lf) for t, lf in ((3.5, False), (-2.25, True))])
    assert all((r == r.max()).sum() == 2 for r in rows)
    L = _in_every_row_class(rows)
    _, labels, _ = _softmax_held(rec, form, L, "ties")
    want = np.tile([min(p) for p in TIE_PAIRS] * 2 + [4], 16)
    assert np.array_equal(labels, want), np.flatnonzero(labels != want)[:8]


@pytest.mark.parametrize("form", [1, 0], ids=FORMS.get)
def test_all_equal_and_all_very_negative_logits(rec, form):
    """every real logit below 0: the only case in which the -inf mask of the padding columns 62 and 63 (logit 0 without it) decides"""
    c = np.arange(62)
    rows = [np.full(62, v) for v in (0.0, 5.25, -1e30, -FLT_MAX)]
    rows += [-1e30 * (1 + ((c - 37) % 62) / 64), -FLT_MAX * (0.5 + ((c - 11) % 62) / 128), -3.0 - ((c - 61) % 62) / 8, -1e-30 * (1 + ((c - 50) % 62))]
    L = _in_every_row_class(np.stack(rows))
    _, labels, probs = _softmax_held(rec, form, L, "equal / very negative")
    m = len(L) // 16
    assert labels[:m].tolist() == [0, 0, 0, 0, 37, 11, 61, 50] + [0] * (m - 8)
    for r in (0, 1, 2, 3):
        assert abs(probs[r] * 62 - 1) <= 1e-15, (r, probs[r])
    assert probs[4] == 1.0 and probs[5] == 1.0


@pytest.mark.parametrize("form", [1, 0], ids=FORMS.get)
def test_a_margin_of_one_ulp_decides(rec, form):
    rows = []
    for mag in (1e-3, 1.0, 1e4):
        lo = np.float32(mag)
        hi = np.nextafter(lo, np.float32(np.inf))
        assert hi > lo
        for first, second in ((hi, lo), (lo, hi)):      # the larger one in the earlier column, then in the later one
            rows.append(_pair_rows([(4, 5), (0, 8), (0, 32), (60, 61)], first, second, lambda c: mag * (0.5 - c / 1024)))
    cases = np.concatenate(rows)
    L = _in_every_row_class(cases)
    _, labels, _ = _softmax_held(rec, form, L, "one ulp")
    assert np.array_equal(labels[:len(cases)], np.argmax(cases, axis=1))
    assert len(set(labels[:len(cases)].tolist())) == 7           # 4, 5, 0, 8, 32, 60, 61: both members of every pair win somewhere


@pytest.mark.parametrize("form", [1, 0], ids=FORMS.get)
def test_softmax_over_spreads_from_0_to_1e5(rec, form):
    c = np.arange(62)
    rows = []
    for spread in (0.0, 1e-3, 30.0, 88.0, 700.0, 1e5):
        for top in (0, 37, 61):
            row = 2.5 - spread * (1 + ((c * 29) % 62) / 62)      # the others 1 .. 2 spreads below the maximum, all different
            row[top] = 2.5
            rows.append(row)
    _softmax_held(rec, form, _in_every_row_class(np.stack(rows)), "spreads")


@pytest.mark.parametrize("form", [1, 0], ids=FORMS.get)
def test_the_bias_is_one_f32_addition_and_outputs_are_independent(rec, form):
    rng = np.random.default_rng(9)
    L = (3 * rng.standard_normal((80, 62))).astype(np.float32)
    bias = rng.standard_normal(62).astype(np.float32)
    want = L + bias
    assert want.dtype == np.float32
    full = _softmax_held(rec, form, L, "bias", bias=bias, want_logits=want)
    hid, w, _ = R.inject_logits(L)
    for k, name in enumerate(ALL):      # each output alone: the other two pointers are null
        alone = _fc2(rec, form, hid, w, bias, want=(name,))
        _same_bits(alone[k], full[k], name)


# ---- F4: the f32 chains against f64 -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", [1, 0], ids=FORMS.get)
@pytest.mark.parametrize("kernel", ["fc1", "fc2"])
def test_f32_chain_accuracy_against_f64(rec, kernel, form):
    case, _, base = _real(rec, kernel, form)
    got = base[0]
    if kernel == "fc1":
        assert (got >= 0).all() and np.array_equal(got == 0, ~(got > 0))
        assert not got[case.ref < -case.max_bound() * case.norm].any()      # ReLU: a reference below zero by more than the error bound is clamped
    err = case.errors(got)
    chain, bar, rms = case.rms(case.chain()), case.bar(), case.rms(got)
    print(f"{kernel} n={len(case.a)} form {form}: measured rms {rms:.3g}  emulated chain {chain:.3g}  bar {bar:.3g}  measured / bar {rms / bar:.2f}  "
          f"max {err.max():.3g} (bound {case.max_bound():.3g})")
    assert err.max() <= case.max_bound(), (float(err.max()), case.max_bound())
    assert rms <= bar, (rms, bar)


# ---- the hooks' own argument checks ---------------------------------------------------------------------------------------------------

def test_hooks_refuse_bad_arguments(rec):
    a1, w1, b1, _ = R.fc_int_case(2, 1024, 512, seed=0)
    a2, w2, b2, _ = R.fc_int_case(2, 512, 62, seed=0)
    L = capi.test_lib()
    hid = np.zeros((2 + GUARD, 512), np.float32)
    p = capi._ptr
    for bad in (lambda: rec.debug_rec_fc1(2, a1, w1, b1), lambda: rec.debug_rec_fc1(-1, a1, w1, b1), lambda: rec.debug_rec_fc2(2, a2, w2, b2),
                lambda: capi.check(L.ocr_test_rec_fc1(rec._h, 0, p(a1), 0, p(w1), p(b1), 0, p(hid), GUARD)),
                lambda: capi.check(L.ocr_test_rec_fc1(rec._h, 1, None, 2, p(w1), p(b1), 0, p(hid), GUARD)),
                lambda: capi.check(L.ocr_test_rec_fc1(rec._h, 1, p(a1), 2, p(w1), p(b1), 0, None, GUARD)),
                lambda: capi.check(L.ocr_test_rec_fc2(rec._h, 0, p(a2), -1, p(w2), p(b2), None, None, None, GUARD)),
                lambda: capi.check(L.ocr_test_rec_fc2(rec._h, 0, p(a2), 2, None, p(b2), None, None, None, GUARD)),
                lambda: capi.check(L.ocr_test_rec_fc2(None, 0, p(a2), 2, p(w2), p(b2), None, None, None, GUARD))):
        with pytest.raises(capi.OcrError) as e:
            bad()
        assert e.value.code == 1      # OCR_ERR_INVALID
