"""Kernel-level tests of the stem (stem_tail.hip), the fused head (tail_fused.hip) and the recogniser's conv stage (rec_net.hip) through
the ocr_test_stem_run / ocr_test_head_run / ocr_test_rec_features hooks: one launch of the shipped launcher on caller data.

C1  placement, by equality: one-hot weights over integer data - every form computes exactly, so a wrong tap, pixel, channel or
    output position is an inequality, not a tolerance.
C2  the split stem's per-tile decision "this tile is raw luma, skip the products of mid and lo": lone fractional pixels at the
    edges of a tile's staged window must switch the tile to six products (a miss costs 1.4e-3 of sum |a||b|; the bar is 1e-5).
C3  the dropped-product bar: normalised rms error against f64 <= sqrt(rms of six products x smallest rms of five), both emulated on
    the CPU from the operands of the case (tests/split_bf16_emul.py; tests/test_split_bf16_emul.py holds the families to a
    separation of 5 x).  A kernel that loses lo.hi, hi.lo or mid.mid fails here and nowhere else.  docs/split_bf16_error.md
    records the measured values (run with -s to print them).
C4  the bf16-precision forms against f64 on the rounded operands.
C5  memory discipline of the stem and the head (the recogniser's conv stage: tests/test_gpu_rec_conv_kernels.py): the hooks put the
    frames / y between two leads and guard rows behind every output.  Nothing is written behind an output; leads of NaN (u8 frames: 255)
    change no bit of the result - the padded MFMA rows and the zero-weight pad taps read zeros or nothing, M = 1 leaves 127 padded rows of
    a head workgroup -; a frame or image of NaN (u8: 255 among frames of 0) leaves its neighbours' bits alone.
"""
import functools
import itertools

import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from ocr_rs_amd import weights as W
from tests import split_bf16_emul as E
from tests.test_gpu_conv_kernel import _check

pytestmark = pytest.mark.gpu

FORM_NAMES = {0: "f32", 1: "bf16", 2: "split_bf16"}


@pytest.fixture(scope="module")
def det():
    d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def rec():
    r = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    yield r
    r.close()


# ---- C1: placement ---------------------------------------------------------------------------------------------------------

# (n, h, w): Wp = 8 one-column last tile of the 8 x 7 form; 16; 8; 24 = one workgroup of the 4 x 6 forms; 32 = a workgroup whose tile loop
# breaks early; 56 = no ragged column, two full workgroups of 4 x 7-wide tiles; 64; from 96 rows up interior tiles without validity test
STEM_SHAPES = [(1, 32, 32), (2, 32, 64), (2, 64, 32), (1, 96, 96), (1, 96, 128), (2, 96, 224), (1, 128, 256)]


def _luma_frames(n, h, w):
    """integer luma, distinct inside every aligned 16 x 16 block, blocks and frames offset against each other"""
    y, x = np.mgrid[0:h, 0:w]
    base = 16 * (y % 16) + (x % 16) + 5 * (y // 16) + 11 * (x // 16)
    return np.stack([(base + 97 * i) % 256 for i in range(n)]).astype(np.uint8)


def _stem_onehot_expected(frames, sign, bias):
    """channel c < 49 = relu(sign * frame shifted by tap c (zero padded) + bias) at stride 2, then max pool 3x3 s2 p1 from zero;
    channels 49 .. 63 have no weight"""
    n, h, w = frames.shape
    xp = np.zeros((n, h + 6, w + 6), np.float64)
    xp[:, 3:3 + h, 3:3 + w] = frames
    conv = np.full((n, h // 2, w // 2, 64), float(bias))
    for c in range(49):
        kh, kw = divmod(c, 7)
        conv[..., c] += sign * xp[:, kh:kh + h:2, kw:kw + w:2]
    conv = np.maximum(conv, 0)
    hc, wc = h // 2, w // 2
    cp = np.zeros((n, hc + 2, wc + 2, 64))
    cp[:, 1:-1, 1:-1] = conv
    out = np.zeros((n, hc // 2, wc // 2, 64))
    for py in range(hc // 2):
        for px in range(wc // 2):
            out[:, py, px] = cp[:, 2 * py:2 * py + 3, 2 * px:2 * px + 3].max(axis=(1, 2))
    return out.astype(np.float32)


@pytest.mark.parametrize("form", [0, 1, 2], ids=FORM_NAMES.get)
@pytest.mark.parametrize("shape", STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_places_every_tap_pixel_and_channel(det, shape, form):
    frames = _luma_frames(*shape)
    w = np.zeros((64, 49), np.float32)
    w[np.arange(49), np.arange(49)] = 1.0
    # +1 / bias 0: shifted copies of the frame.  -1 / bias 300: every conv value is >= 45, so neither ReLU nor the pool's zero
    # initial value can stand in for a wrong pixel
    for sign, bias in ((1.0, 0.0), (-1.0, 300.0)):
        want = _stem_onehot_expected(frames, sign, bias)
        if form == 1:
            want = E.bf16_round(want)      # bf16 output: integers above 256 round (the f32 value in front of the rounding is exact)
        for x in (frames, frames.astype(np.float32)):
            got = det.debug_stem_run(form, x, sign * w, np.ones(64, np.float32), np.full(64, bias, np.float32))
            assert np.array_equal(got, want), (sign, x.dtype, np.argwhere(got != want)[:4])


# (n, h4, w4): M = 1, 127, 129 (below, at -1 / +1 of and across the 128-pixel workgroup), non-power-of-two w4 and h4 * w4 for the magic divisions
HEAD_SHAPES = [(1, 1, 1), (1, 1, 127), (1, 3, 43), (3, 5, 7), (2, 8, 24), (1, 24, 40)]
_PERMS = list(itertools.permutations(range(4)))


def _head_onehot(n, h4, w4):
    """Pixel (n, i, j) has the single input 2.0 at channel k (a hash of its position).  Tap t sends channel k to output channel
    co_t(k) = 16 ((t + k) % 4) + (k // 4 + 3 t) % 16 with weight 1; s4 / b4 turn the 2.0 into exactly 1 and everything else into 0
    (even co: 2 * 1 - 1, odd co: 2 * 0.5 + 0; elsewhere relu(0 * s - 1) or relu(0)); row co of w2t holds the four values of group
    co // 16 (-8..-5, -4..-1, 0..3, 4..7) in the permutation co % 16.  The four taps of a pixel fall into four different groups: its
    16 logits are 16 different integers of -8 .. 7, + bias2 = 1, in an arrangement that differs between pixels whose k differs."""
    ni, ii, jj = np.meshgrid(np.arange(n), np.arange(h4), np.arange(w4), indexing="ij")
    k = (jj + 5 * ii + 7 * (jj // 64) + 11 * ni) % 64
    y = np.zeros((n, h4, w4, 64), np.float32)
    np.put_along_axis(y, k[..., None], 2.0, axis=3)
    ci = np.arange(64)
    wt1 = np.zeros((4, 64, 64), np.float32)
    co_of = np.stack([16 * ((t + ci) % 4) + (ci // 4 + 3 * t) % 16 for t in range(4)])     # [t][ci]
    for t in range(4):
        wt1[t, co_of[t], ci] = 1.0
    co = np.arange(64)
    s4 = np.tile(np.where(co % 2 == 0, 1.0, 0.5), 4).astype(np.float32)
    b4 = np.tile(np.where(co % 2 == 0, -1.0, 0.0), 4).astype(np.float32)
    w2t = np.array([[4 * (c // 16) - 8 + _PERMS[c % 16][u] for u in range(4)] for c in range(64)], np.float32)
    logits = w2t[co_of[:, k]].transpose(1, 2, 3, 0, 4).astype(np.float64) + 1.0      # [n][i][j][t][u], exact integers
    return y, wt1, s4, b4, w2t, 1.0, logits


@pytest.mark.parametrize("form", [0, 1, 2], ids=FORM_NAMES.get)
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_places_every_tap_phase_and_pixel(det, shape, form):
    n, h4, w4 = shape
    y, wt1, s4, b4, w2t, bias2, logits = _head_onehot(n, h4, w4)
    assert np.abs(logits).max() <= 8 and all(len(set(v)) == 16 for v in logits.reshape(-1, 16)[:64])
    want = np.zeros((n, 4 * h4, 4 * w4))
    for a in range(2):
        for b in range(2):
            for c in range(2):
                for d in range(2):
                    want[:, 2 * a + c::4, 2 * b + d::4] = 1.0 / (1.0 + np.exp(-logits[:, :, :, 2 * a + b, 2 * c + d]))
    prob, bitmap = det.debug_head_run(form, y, wt1, s4, b4, w2t, bias2, 0.5)
    # expf is within 1 ulp, then one add and one divide: 4 ulps of p
    ulps = np.abs(prob.astype(np.float64) - want) / np.spacing(want.astype(np.float32)).astype(np.float64)
    assert ulps.max() <= 4, (float(ulps.max()), np.argwhere(ulps > 4)[:4])
    assert np.array_equal(bitmap, (prob > np.float32(0.5)).astype(np.uint8))
    assert bitmap.any() and not bitmap.all()
    prob2, none = det.debug_head_run(form, y, wt1, s4, b4, w2t, bias2, 0.5, want_bitmap=False)
    assert none is None and np.array_equal(prob2, prob)


@pytest.mark.parametrize("form", [0, 1], ids=["f32", "small_split_bf16"])
@pytest.mark.parametrize("n", [1, 5, 17])
def test_rec_features_place_every_tap_channel_and_crop(rec, n, form):
    """one-hot conv1 and conv2 weights over integer crops: feat[crop][co * 16 + p] is a 2x2 max of a shifted pooled map, exactly;
    17 crops cross a 16-crop tile of the small-batch kernel's operand order"""
    rng = np.random.default_rng(n)
    crops = rng.integers(0, 256, (n, 784)).astype(np.float32)
    b1 = rng.integers(-3, 4, 32).astype(np.float32)
    p1, w1 = E.rec_pooled_onehot(crops, (3 * np.arange(32)) % 25, np.ones(32, np.float32), b1)
    co = np.arange(64)
    ci_of, tap_of, sign = (5 * co + 1) % 32, (7 * co + 2) % 25, np.where(co % 2 == 0, 1.0, -1.0)
    w2 = np.zeros((64, 32, 25), np.float32)
    w2[co, ci_of, tap_of] = sign
    b2 = np.where(co % 2 == 0, 0.0, 300.0).astype(np.float32) + (co % 5)
    want = np.zeros((n, 64, 4, 4), np.float32)
    for c in co:
        ky, kx = divmod(int(tap_of[c]), 5)
        v = sign[c] * p1[:, ky:ky + 8, kx:kx + 8, ci_of[c]]
        want[:, c] = v.reshape(n, 4, 2, 4, 2).max(axis=(2, 4)) + b2[c]
    got = rec.debug_rec_features(form, crops, w1, b1, w2, b2)
    assert np.array_equal(got, want.reshape(n, 1024)), np.argwhere(got != want.reshape(n, 1024))[:4]


# ---- C2: the tile-exactness decision of the split stem -----------------------------------------------------------------------

def test_split_stem_decides_per_tile_whether_mid_and_lo_exist(det):
    """8 x 7 pooled pixels per tile: tile (ty, tx) stages input rows 32 ty - 5 .. + 38 and columns 28 tx - 5 .. + 34 (+ one zero-weight
    column), two pixels per word.  Frame 0 is raw luma (every tile takes the short path), frame 1 fractional everywhere; frames 2 .. 5
    are raw luma but for ONE pixel + 0.3: the first staged word of tile (1, 1), its last staged word, a pixel that tile (1, 1) sees only
    in its halo (the columns it shares with tile (1, 2)), a pixel of the ragged fifth tile of a row (W / 4 = 32 = 4 x 7 + 4)."""
    n, h, w = 6, 96, 128
    rng = np.random.default_rng(42)
    frames = rng.integers(0, 256, (n, h, w)).astype(np.float32)
    frames[1] += rng.random((h, w)).astype(np.float32)
    r0, c0 = 32 * 1 - 5, 28 * 1 - 5
    for f, (r, c) in zip(range(2, 6), [(r0, c0), (r0 + 38, c0 + 34), (r0 + 20, 28 * 2 - 3), (40, 121)]):
        frames[f, r, c] += np.float32(0.3)
    wgt, scale, bias = E.stem_weights(2)
    case = E.StemCase(frames, wgt, scale, bias)
    got = det.debug_stem_run(2, frames, wgt, scale, bias)
    err = np.abs(got.astype(np.float64) - case.ref) / case.norm
    print("split stem, lone fractional pixels: max error / sum|a||b||scale| per frame", [f"{e:.2e}" for e in err.reshape(n, -1).max(axis=1)])
    assert err.max() <= 1e-5, np.argwhere(err > 1e-5)[:4]
    q = np.floor(frames)
    assert np.array_equal(det.debug_stem_run(2, q.astype(np.uint8), wgt, scale, bias), det.debug_stem_run(2, q, wgt, scale, bias))


# ---- C3: the dropped-product bar ---------------------------------------------------------------------------------------------

def _held_to_the_bar(name, case, got):
    six, five, bar, _ = _bars(name, case)
    rms = case.rms(got)
    print(f"{name}: measured rms {rms:.3g}  emulated six {six:.3g}  five {five:.3g}  bar {bar:.3g}")
    assert rms <= bar, (name, rms, bar)


_BARS = {}


def _bars(name, case):
    key = name.split(" form")[0]     # the forms of a kernel share operands, reference and bar
    if key not in _BARS:
        _BARS[key] = E.bar(case)
    return _BARS[key]


@functools.lru_cache(None)
def _stem_case(family):
    w, scale, bias = E.stem_weights(1)
    frames = E.stem_family(family)
    return frames, w, scale, bias, E.StemCase(frames, w, scale, bias)


@pytest.mark.parametrize("form", [0, 2], ids=FORM_NAMES.get)
@pytest.mark.parametrize("family", E.STEM_FAMILIES)
def test_stem_loses_none_of_its_six_products(det, family, form):
    frames, w, scale, bias, case = _stem_case(family)
    _held_to_the_bar(f"stem {family} form {form}", case, det.debug_stem_run(form, frames, w, scale, bias))


@functools.lru_cache(None)
def _head_case(shape):
    ops = E.head_family(*shape)
    return ops, E.HeadCase(*ops)


@pytest.mark.parametrize("form", [0, 2], ids=FORM_NAMES.get)
@pytest.mark.parametrize("shape", [(2, 8, 24), (1, 3, 43)], ids=lambda s: "x".join(map(str, s)))
def test_head_loses_none_of_its_six_products(det, shape, form):
    ops, case = _head_case(shape)
    prob, _ = det.debug_head_run(form, *ops)
    _held_to_the_bar(f"head {shape} form {form}", case, prob)


@functools.lru_cache(None)
def _rec_case():
    crops, w1, b1, w2, b2, p1 = E.rec_family(64)
    return (crops, w1, b1, w2, b2), E.RecCase(p1, w2, b2)


@pytest.mark.parametrize("form", [0, 1], ids=["f32", "small_split_bf16"])
def test_rec_conv2_loses_none_of_its_six_products(rec, form):
    ops, case = _rec_case()
    _held_to_the_bar(f"rec n=64 form {form}", case, rec.debug_rec_features(form, *ops))


@pytest.mark.parametrize("conv", E.CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_igemm_split_loses_none_of_its_six_products(det, conv):
    x, wg, stride = E.conv_family(conv)
    out, _ = det.debug_conv_run(x, wg, stride, variant=2)
    _held_to_the_bar(f"conv_igemm {conv} variant 2", E.ConvCase(x, wg, stride), out)


# ---- C4: the bf16-precision forms ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ["u8", "f32"])
@pytest.mark.parametrize("shape", STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_bf16_matches_f64_on_rounded_operands(det, shape, entry):
    w, scale, bias = E.stem_weights(3)
    frames = E.stem_family("luma_u8" if entry == "u8" else "fraction", *shape, seed=sum(shape))
    ref = E.StemCase(E.bf16_round(frames), E.bf16_round(w), scale, bias).ref
    _check(det.debug_stem_run(1, frames, w, scale, bias), ref.astype(np.float32), True)


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_bf16_matches_f64_on_rounded_operands(det, shape):
    y, wt1, s4, b4, w2t, bias2 = E.head_family(*shape, seed=sum(shape))
    ref = E.HeadCase(E.bf16_round(y), E.bf16_round(wt1), s4, b4, w2t, bias2).ref
    prob, _ = det.debug_head_run(1, y, wt1, s4, b4, w2t, bias2)
    assert float(np.abs(prob - ref).max()) <= 1e-5


# ---- C5: guards, poisoned leads, isolation of the items of a batch ---------------------------------------------------------------

GUARD = 8
STEM_GUARD_SHAPES = [(3, 32, 32), (2, 64, 32), (1, 96, 224)]     # one-tile frames with a neighbour on both sides; two tile rows; a ragged tile column
HEAD_GUARD_SHAPES = [(1, 1, 1), (1, 1, 127), (1, 3, 43), (3, 5, 7)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _stem_guarded(det, form, frames, ops, poison):
    out, guard = det.debug_stem_run(form, frames, *ops, poison=poison, guard=GUARD)
    assert guard.shape == (GUARD, 64) and np.array_equal(guard, np.full_like(guard, -7.0)), ("rows behind the stem's output were written", poison)
    return out


@pytest.mark.parametrize("entry", ["u8", "f32"])
@pytest.mark.parametrize("form", [0, 1, 2], ids=FORM_NAMES.get)
@pytest.mark.parametrize("shape", STEM_GUARD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_stays_inside_its_frames_and_its_output(det, shape, form, entry):
    ops = E.stem_weights(1)
    frames = E.stem_family("luma_u8" if entry == "u8" else "fraction", *shape, seed=sum(shape))
    clean = _stem_guarded(det, form, frames, ops, 0)
    assert not np.isnan(clean).any() and clean.any()
    for poison in (1, 2):      # f32: quiet NaN, +inf; u8: 255 both times
        got = _stem_guarded(det, form, frames, ops, poison)
        assert np.array_equal(_bits(got), _bits(clean)), (poison, np.argwhere(_bits(got) != _bits(clean))[:4])
    if shape[0] == 3:
        if entry == "u8":      # no NaN in u8: the loudest frame among silent ones
            base = np.zeros(shape, np.uint8)
            clean = _stem_guarded(det, form, base, ops, 0)
            bad = base.copy()
            bad[1] = 255
        else:
            bad = frames.copy()
            bad[1] = np.nan
        got = _stem_guarded(det, form, bad, ops, 0)
        assert np.array_equal(_bits(got[[0, 2]]), _bits(clean[[0, 2]])), np.argwhere(_bits(got[[0, 2]]) != _bits(clean[[0, 2]]))[:4]


def _head_guarded(det, form, ops, poison, want_bitmap=True):
    prob, bm, gp, gb = det.debug_head_run(form, *ops, want_bitmap=want_bitmap, poison=poison, guard=GUARD)
    w = prob.shape[2]
    assert gp.shape == (GUARD, w) and np.array_equal(gp, np.full_like(gp, -7.0)), ("rows behind prob were written", poison)
    if want_bitmap:
        assert gb.shape == (GUARD, w) and np.array_equal(gb, np.full_like(gb, 9)), ("rows behind the bitmap were written", poison)
        assert np.isin(bm, (0, 1)).all()
    else:
        assert bm is None and gb is None
    return prob, bm


@pytest.mark.parametrize("form", [0, 1, 2], ids=FORM_NAMES.get)
@pytest.mark.parametrize("shape", HEAD_GUARD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_stays_inside_its_pixels_and_its_outputs(det, shape, form):
    ops = E.head_family(*shape, seed=sum(shape))
    prob, bm = _head_guarded(det, form, ops, 0)
    assert not np.isnan(prob).any()
    for poison in (1, 2):      # rows past M read as zeros: not as what lies behind y
        p2, b2 = _head_guarded(det, form, ops, poison)
        assert np.array_equal(_bits(p2), _bits(prob)) and np.array_equal(b2, bm), (poison, np.argwhere(_bits(p2) != _bits(prob))[:4])
    p3, none = _head_guarded(det, form, ops, 1, want_bitmap=False)
    assert none is None and np.array_equal(_bits(p3), _bits(prob))
    if shape[0] == 3:
        y = ops[0].copy()
        y[1] = np.nan
        p4, b4 = _head_guarded(det, form, (y,) + tuple(ops[1:]), 0)
        assert np.array_equal(_bits(p4[[0, 2]]), _bits(prob[[0, 2]])) and np.array_equal(b4[[0, 2]], bm[[0, 2]])
