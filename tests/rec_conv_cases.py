"""Cases, references and every assertion (numpy, no GPU) of the kernel-level tests of the recogniser's conv stage at 1, 2 and 4 crops per
workgroup and of its small-batch form (rec_net.hip's rec_conv_kernel<T> and rec_conv_small_x3_kernel) - tests/test_gpu_rec_conv_kernels.py
hands the check_* functions the hook, tests/test_rec_conv_cases.py a numpy model of the kernel and deliberately wrong models.

`run(form, T, ops, poison)` is one launch: form 0 = rec_conv_kernel<T> (T = 0: chosen by the batch as shipped), form 1 = the small-batch
kernel (T must be 0); ops = (crops [n][784], w1 [32][25], b1 [32], w2 [64][32][25], b2 [64]); the crops sit between two leads of four crops,
zeros or (poison = 1) quiet NaN.  It returns (feat [n][1024] as co * 16 + p, the rows behind feat): GUARD rows for form 0, the pad rows of
the last 16-crop tile and one further tile for form 1, all of which went to the device as SENTINEL.

  launch                R5, part of EVERY launch of every check: the guard comes back as the sentinel, and the NaN leads change no bit
  check_placement       R1  one-hot conv1 and conv2 over integer crops: feat is a 2x2 max of a shifted pooled map, exactly
  check_dense_int       R2  dense small integers, every partial sum below 2^24: any f32 order (and form 1's three bf16 terms) is exact
  check_forms_agree     R3  T = 1, 2 and 4 are one computation: the same bits
  check_f64_bound       R4  every element of an f32 form within gamma_801 sum |p1||w2| + one rounding of the bias add of f64
  check_bar             R4  form 1 under the dropped-product bar of tests/split_bf16_emul.py
  check_nan_crop        R5  a crop of NaN leaves every other crop's bits alone
  check_refusals        R6  T = 3, T with form 1, an empty batch"""
import functools

import numpy as np

from tests import split_bf16_emul as E

f32, f64 = np.float32, np.float64
GUARD = 8
SENTINEL = -7.0
FORMS = ((0, 1), (0, 2), (0, 4), (1, 0))          # (form, T)
FORM_IDS = ("f32_T1", "f32_T2", "f32_T4", "small_split_bf16")
# T = 2: one crop of a pair; a full pair; a ragged second workgroup; three workgroups.  T = 4: a second pair wholly past the end (1, 2),
# half past it (3, 7), full (4), a ragged second and third workgroup (5, 7, 9).  Form 1: below, at, across one and two 16-crop tiles
PLACEMENT_BATCHES = {(0, 1): (1, 2, 5), (0, 2): (1, 2, 3, 5), (0, 4): (1, 2, 3, 4, 5, 7, 9), (1, 0): (1, 16, 17, 33)}
DENSE_BATCHES = (5, 9)


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def launch(run, form, T, ops, nan_crop=None):
    """one launch with zero leads and one with NaN leads.  Nothing is written behind the result (nor, form 1, into the pad rows of the
    last tile); the leads change no bit; no NaN comes out of finite crops.  With nan_crop = k crop k of ops is NaN and must come out
    holding NaN - every other row still must not."""
    feat, guard = run(form, T, ops, 0)
    feat_p, guard_p = run(form, T, ops, 1)
    n = np.asarray(ops[0]).reshape(-1, 784).shape[0]
    for name, f, g in (("zero leads", feat, guard), ("NaN leads", feat_p, guard_p)):
        assert f.shape == (n, 1024) and g.shape[0] >= (GUARD if form == 0 else 16) and g.shape[1] == 1024, (name, f.shape, g.shape)
        assert np.array_equal(g, np.full_like(g, SENTINEL)), (name, "rows behind the result were written", np.argwhere(g != f32(SENTINEL))[:4])
        clean = np.ones(n, bool)
        if nan_crop is not None:
            clean[nan_crop] = False
            assert np.isnan(f[nan_crop]).any(), (name, "the NaN crop came out finite")
        assert not np.isnan(f[clean]).any(), (name, "NaN in the result", np.argwhere(np.isnan(f))[:4])
    keep = np.ones(n, bool)
    if nan_crop is not None:
        keep[nan_crop] = False
        assert np.array_equal(np.isnan(feat[nan_crop]), np.isnan(feat_p[nan_crop]))
    assert np.array_equal(_bits(feat[keep]), _bits(feat_p[keep])), ("the leads were read", np.argwhere(_bits(feat[keep]) != _bits(feat_p[keep]))[:4])
    return feat


# ---- R1 ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def placement_case(n):
    """Integer crops; conv1 channel c = the crop shifted by tap 3 c mod 25, + b1; conv2 output co = sign * (channel 5 co + 1 mod 32 shifted
    by tap 7 co + 2 mod 25 - every tap occurs) + b2, where the odd co have sign -1 and b2 >= 300: their 2x2 maximum is the window's SMALLEST
    pooled value, and no zero can stand in for it.  Returns ops and the expected feat, exact in any order."""
    rng = np.random.default_rng(n)
    crops = rng.integers(0, 256, (n, 784)).astype(f32)
    b1 = rng.integers(-3, 4, 32).astype(f32)
    p1, w1 = E.rec_pooled_onehot(crops, (3 * np.arange(32)) % 25, np.ones(32, f32), b1)
    co = np.arange(64)
    ci_of, tap_of, sign = (5 * co + 1) % 32, (7 * co + 2) % 25, np.where(co % 2 == 0, 1.0, -1.0)
    assert set(tap_of) == set(range(25)) and set(ci_of) == set(range(32))
    w2 = np.zeros((64, 32, 25), f32)
    w2[co, ci_of, tap_of] = sign
    b2 = np.where(co % 2 == 0, 0.0, 300.0).astype(f32) + (co % 5)
    want = np.zeros((n, 64, 4, 4), f32)
    for c in co:
        ky, kx = divmod(int(tap_of[c]), 5)
        v = sign[c] * p1[:, ky:ky + 8, kx:kx + 8, ci_of[c]]
        want[:, c] = v.reshape(n, 4, 2, 4, 2).max(axis=(2, 4)) + b2[c]
    want = want.reshape(n, 1024)
    assert len({r.tobytes() for r in want}) == n                  # every crop's features are its own
    return (crops, w1, b1, w2, b2), want


def check_placement(run, form, T, n):
    ops, want = placement_case(n)
    got = launch(run, form, T, ops)
    assert np.array_equal(got, want), (form, T, n, np.argwhere(got != want)[:4])


# ---- R2 ------------------------------------------------------------------------------------------------------------------------

def _windows(x):
    """[n][H][W][C] -> [n][H - 4][W - 4][25][C], tap = 5 ky + kx"""
    H, W = x.shape[1] - 4, x.shape[2] - 4
    return np.stack([x[:, ky:ky + H, kx:kx + W] for ky in range(5) for kx in range(5)], axis=3)


def _pool2(a):
    """2x2 max of [n][H][W][C]; also the index of the deciding element of each window (first of the maxima, in the order (dy, dx))"""
    n, H, W, C = a.shape
    w = a.reshape(n, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(n, H // 2, W // 2, C, 4)
    return w.max(axis=4), w.argmax(axis=4)


@functools.lru_cache(None)
def dense_int_case(n):
    """crops 0 .. 255, w1 in {-1, 0, 1}, b1 in -3 .. 3, w2 in -2 .. 2, b2 in -50 .. 50: conv1 stays within 25 x 255 + 3 = 6378, conv2's
    partial sums within 800 x 6378 x 2 = 1.02e7 < 2^24 = 1.68e7, so every f32 summation order gives the int64 result; the three bf16
    terms of an integer below 2^24 are integers that sum to it, and their products with w2 stay under the same bound (asserted on
    sum (|hi| + |mid| + |lo|) |w2|).  Returns ops and the int64 feat."""
    rng = np.random.default_rng(100 + n)
    crops = rng.integers(0, 256, (n, 784))
    w1 = rng.integers(-1, 2, (32, 25))
    b1 = rng.integers(-3, 4, 32)
    w2 = rng.integers(-2, 3, (64, 32, 25))
    b2 = rng.integers(-50, 51, 64)
    c1 = _windows(crops.reshape(n, 28, 28, 1).astype(np.int64))[..., 0] @ w1.T.astype(np.int64)          # [n][24][24][32]
    p1, dec1 = _pool2(c1)
    p1 = p1 + b1
    B = w2.transpose(2, 1, 0).reshape(800, 64).astype(np.int64)
    A = _windows(p1).reshape(n, 8, 8, 800)
    c2 = A @ B
    p2, dec2 = _pool2(c2)
    want = (p2 + b2).transpose(0, 3, 1, 2).reshape(n, 1024)
    pieces = sum(np.abs(t).astype(f64) for t in E.split3(p1.astype(f32)))
    assert np.array_equal(sum(t.astype(f64) for t in E.split3(p1.astype(f32))), p1)
    bound = float((_windows(pieces).reshape(n, 8, 8, 800) @ np.abs(B).astype(f64)).max() + np.abs(b2).max())
    assert bound < 2 ** 24 and np.abs(c1).max() + 3 <= 6378, bound
    assert (dec1 != 0).mean() >= 0.25 and (dec2 != 0).mean() >= 0.25, ((dec1 != 0).mean(), (dec2 != 0).mean())
    assert len({r.tobytes() for r in want}) == n
    return (crops.astype(f32), w1.astype(f32), b1.astype(f32), w2.astype(f32), b2.astype(f32)), want


def check_dense_int(run, form, T, n):
    ops, want = dense_int_case(n)
    got = launch(run, form, T, ops)
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, np.rint(got)), (form, T, n, np.argwhere(got != want)[:4])


# ---- R3, R4 --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def real_case(n):
    """E.rec_family: real crops, one-hot conv1 (so that conv2's operand p1 is known exactly on the host), conv2 ~ N(0,1)/28; with the f64
    reference and sum |p1||w2| of every element (E.RecCase)"""
    crops, w1, b1, w2, b2, p1 = E.rec_family(n)
    return (crops, w1, b1, w2, b2), E.RecCase(p1, w2, b2)


def check_forms_agree(run, n=9):
    """every output's MFMA chain runs tap, g, e in the same order whatever T: the three instantiations give the same bits"""
    ops, _ = real_case(n)
    got = [launch(run, 0, T, ops) for T in (1, 2, 4)]
    for T, g in zip((2, 4), got[1:]):
        assert np.array_equal(_bits(g), _bits(got[0])), (T, np.argwhere(_bits(g) != _bits(got[0]))[:4])


def f64_bound(case):
    """|feat - ref| per element for ANY f32 summation of the 800 products: gamma_801 sum |p1||w2| (the pooled maximum of it - a maximum
    of four moves by no more than its operands do), and one rounding of the bias add, 2^-24 of the largest value the sum can have"""
    u = 2.0 ** -24
    gamma = 801 * u / (1 - 801 * u)
    acc = gamma * case.norm
    return acc + u * (np.abs(case.ref) + acc)


def check_f64_bound(run, T, n=9):
    ops, case = real_case(n)
    got = launch(run, 0, T, ops)
    err, bound = np.abs(got.astype(f64) - case.ref), f64_bound(case)
    print(f"rec conv T={T} n={n}: max error / bound {float((err / bound).max()):.3g}")
    assert (err <= bound).all(), (T, np.argwhere(err > bound)[:4], float((err / bound).max()))


_BARS = {}


def check_bar(run, n):
    """form 1 keeps all six partial products: normalised rms against f64 <= sqrt(rms of six x smallest rms of five), both emulated"""
    ops, case = real_case(n)
    if n not in _BARS:
        _BARS[n] = E.bar(case)
    six, five, bar, _ = _BARS[n]
    rms = case.rms(launch(run, 1, 0, ops))
    print(f"rec small n={n}: measured rms {rms:.3g}  emulated six {six:.3g}  five {five:.3g}  bar {bar:.3g}")
    assert rms <= bar, (n, rms, bar)


# ---- R5, R6 --------------------------------------------------------------------------------------------------------------------

NAN_CROPS = (0, 4, 8)      # of n = 9: first of a pair, first of a workgroup (T = 4) or of a pair (T = 2), last and ragged - re-read by its workgroup


def check_nan_crop(run, form, T, k, n=9):
    ops, _ = real_case(n)
    clean = launch(run, form, T, ops)
    crops = ops[0].copy()
    crops[k] = np.nan
    got = launch(run, form, T, (crops,) + ops[1:], nan_crop=k)
    others = np.arange(n) != k
    assert np.array_equal(_bits(got[others]), _bits(clean[others])), (T, k, np.argwhere(_bits(got) != _bits(clean))[:4])


def check_refusals(run, error):
    ops, _ = placement_case(2)
    empty = (np.zeros((0, 784), f32),) + ops[1:]
    for what, form, T, o in (("three crops per workgroup", 0, 3, ops), ("five", 0, 5, ops), ("negative", 0, -1, ops),
                             ("crops per workgroup with the small-batch form", 1, 2, ops), ("an empty batch", 0, 0, empty),
                             ("an empty batch, small form", 1, 0, empty)):
        try:
            run(form, T, o, 0)
        except error:
            continue
        raise AssertionError(f"{what} was not refused")


# ---- a numpy model of the kernels' data movement (tests/test_rec_conv_cases.py) ---------------------------------------------------

BUGS = ("swap_pair", "store_ragged", "swap_halves", "drop_tap", "pad_tap", "copy_last", "lead_read")


class Refused(Exception):
    pass


def model(form, T, ops, poison=0, bug=None):
    """What the hook returns, from a numpy restatement of the kernels: per workgroup of t crops the crops are staged pair by pair (a crop past
    the batch re-reads the last one), conv1 + pool fill p1[crop_local], conv2 + pool give row tile rt = 2 crop_local + tp, stored to crop
    crop0 + crop_local, half 8 tp, if that crop exists.  Arithmetic: f64 products summed in f64, rounded to f32 once.  bug = one of BUGS:
      swap_pair     the two crops of a staged pair land in each other's slot
      store_ragged  the ragged workgroup stores the crops past the batch as well
      swap_halves   a crop's row tiles are stored to each other's 8 tp half
      drop_tap      conv2 loses tap 13
      pad_tap       conv1's zero pad tap carries the weight of tap 24 (and reads the window's first pixel)
      copy_last     the last crop's features are stored over crop n - 2 as well
      lead_read     conv1's pad tap, weight 0, reads the float in front of the crops"""
    crops, w1, b1, w2, b2 = [np.asarray(a, f32) for a in ops]
    crops = crops.reshape(-1, 784)
    n = crops.shape[0]
    if form not in (0, 1) or n <= 0 or (form == 1 and T != 0) or T not in (0, 1, 2, 4):
        raise Refused((form, T, n))
    lead = np.full((4, 784), np.nan if poison else 0.0, f32)
    buf = np.concatenate([lead, crops, lead])
    rows = n + GUARD if form == 0 else 16 * ((n + 15) // 16 + 1)
    out = np.full((rows, 1024), SENTINEL, f32)
    # every crop's features, once
    x = crops.reshape(n, 28, 28, 1).astype(f64)
    c1 = _windows(x)[..., 0] @ w1.T.astype(f64)
    if bug == "pad_tap":
        c1 = c1 + x[:, :24, :24] * w1[:, 24].astype(f64)
    if bug == "lead_read":
        c1 = c1 + 0.0 * f64(buf[3, 783])
    p1 = (_pool2(c1.astype(f32))[0] + b1).astype(f32)
    B = w2.transpose(2, 1, 0).astype(f64)          # [tap][ci][co]
    if bug == "drop_tap":
        B = B.copy()
        B[13] = 0
    c2 = _windows(p1.astype(f64)).reshape(n, 8, 8, 800) @ B.reshape(800, 64)
    feats = (_pool2(c2.astype(f32))[0] + b2).astype(f32).transpose(0, 3, 1, 2).reshape(n, 64, 16)
    o = out.reshape(rows, 64, 16)
    if form == 1:
        o[:n] = feats
        return out[:n], out[n:]
    t = T or (1 if n <= 768 else 2 if n <= 3072 else 4)
    for crop0 in range(0, n, t):
        src = {}
        for pr in range(max(1, t // 2)):
            slots = [min(crop0 + 2 * pr + c, n - 1) for c in range(min(t, 2))]
            if bug == "swap_pair":
                slots.reverse()
            for c, g in enumerate(slots):
                src[2 * pr + c] = g
        for rt in range(2 * t):
            crop_local, tp = rt >> 1, rt & 1
            crop = crop0 + crop_local
            if crop < n or (bug == "store_ragged" and crop < rows):
                dst = 1 - tp if bug == "swap_halves" else tp
                o[crop, :, 8 * dst:8 * dst + 8] = feats[src[crop_local], :, 8 * tp:8 * tp + 8]
    if bug == "copy_last" and n >= 2:
        o[n - 2] = o[n - 1]
    return out[:n], out[n:]
