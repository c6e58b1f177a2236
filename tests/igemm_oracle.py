"""conv_igemm's launches with a SRC_PLAIN / SRC_CAT4 source and a STORE_NHWC / STORE_SHUFFLE2 store - the convs of the trunk, the laterals with
their top-down sum, bin_conv1 over the concat, the transposed conv's pixel shuffle and the batched GEMM - stated without a GPU.

  * the operation by definition in f64 (`conv`, `concat4`, `shuffle2`, `accumulate`, `finish`): conv -> acc scale + bias -> + residual ->
    ReLU; out2 = value + nearest_up2(up_residual); the shuffle sends column (2 a + b) 64 + co of pixel (i, j) to out[n][2 i + a][2 j + b][co];
    the CAT4 source is [up8(p5), up4(p4), up2(p3), p2]; the batched GEMM is B independent products.  The same functions on absolute values give
    sum |a||b| carried through the epilogue, the magnitude the f32 bars are written in.  tests/test_igemm_oracle.py holds them to
    torch.nn.functional.conv2d / conv_transpose2d in f64;
  * integer families (`operands`): "signed" / "nonneg" - small integers on both sides, scales powers of two, integer biases and residuals:
    every partial sum is an integer number of quanta below 2^24 in any order in any accumulator, so the result is determined bit for bit for
    the f32, the split-bf16 and the bf16 form (bf16 results: ONE rounding of the exact value).  For the split form three more, in which an
    operand has more than 8 significant bits and the three products the kernel drops (mid.lo, lo.mid, lo.lo) are zero: "wide_w" - dense
    {-1, 0, 1} activations against sparse weights of up to 21 bits (hi.hi, hi.mid, hi.lo); "wide_x" - the mirror image (lo.hi, mid.hi, hi.hi);
    "mid" - sparse 11-bit activations against dense 11-bit weights (mid.mid with hi.mid, mid.hi, hi.hi).  (A, B) = (activations, weights);
  * `standin`, a numpy model with the signature of Detector.debug_igemm_run that follows the kernel's structure - the source inside an
    allocation with lead regions (CAT4: a region between the levels), rows as a linear run of output pixels with every tap masked per row, the
    split weights as three planes, the epilogue in f32, rows of the last tile dropped beyond M - and, on request, commits one of `FAULTS`;
  * the assertions of tests/test_gpu_igemm_kernels.py (`check_g1` .. `check_g5`) as functions of a `run` callable, so that
    tests/test_igemm_oracle.py can show that the model passes every one of them and that every fault fails at least one.

`run(form, x, wgt, out_bf16=, stride=, src_mode=, store_mode=, scale=, bias=, residual=, up_residual=, want_out=, want_out2=, relu=, tile=,
poison=, guard=, sentinel=) -> (out | None, out2 | None, guard rows)`."""
import functools
from typing import NamedTuple

import numpy as np

from tests import split_bf16_emul as E

f32, f64 = np.float32, np.float64
F32, SPLIT, BF16 = 0, 1, 2
FORM_NAMES = {F32: "f32", SPLIT: "split", BF16: "bf16"}
PLAIN, CAT4 = 0, 2
NHWC, SHUFFLE2 = 0, 1
TILE_ROWS = {1: 128, 2: 128, 3: 64}
SENTINEL = -7.0       # below every ReLU output, exact in bf16
LIMIT = 1 << 24
IMAGE_SCALES = (1.0, 16.0, 1.0 / 16.0)


def bf16(a):
    """f32 -> nearest-even bf16, widened back to f32 (of a copy: the cases' arrays are read-only)"""
    return E.bf16_round(np.array(a, f32))


class Launch(NamedTuple):
    """one launch: grid = (N, H, W) of the input (CAT4: of p2; batched: (1, 1, M))"""
    form: int
    out_bf16: bool
    ks: int
    stride: int
    grid: tuple
    cin: int
    cout: int
    src: int = PLAIN
    store: int = NHWC
    batch: int = 1
    tile: int = 0

    def out_grid(self):
        pad = (self.ks - 1) // 2
        n, h, w = self.grid
        return n, (h + 2 * pad - self.ks) // self.stride + 1, (w + 2 * pad - self.ks) // self.stride + 1

    def shape_key(self):
        """what the operands and the f64 sums depend on"""
        return self._replace(form=BF16 if self.form == BF16 else F32, out_bf16=False, tile=0)

    def name(self):
        return (f"{FORM_NAMES[self.form]}->{'bf16' if self.out_bf16 else 'f32'} k{self.ks} s{self.stride} {'CAT4' if self.src == CAT4 else 'PLAIN'} "
                f"{'SHUFFLE2' if self.store == SHUFFLE2 else 'NHWC'} {self.grid} {self.cin}->{self.cout} batch {self.batch} tile {self.tile}")


# ---- the operation by definition --------------------------------------------------------------------------------------------------------------

def conv(x, w, stride=1):
    """x [n][H][W][C], w [K][ks ks][C] (tap = ks ky + kx) -> [n][Ho][Wo][K] in f64: zero padding (ks - 1) / 2, output pixel (oh, ow) sums the
    taps at (stride oh - pad + ky, stride ow - pad + kx)"""
    x, w = np.asarray(x, f64), np.asarray(w, f64)
    n, H, W, C = x.shape
    ks = {1: 1, 9: 3}[w.shape[1]]
    pad = (ks - 1) // 2
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    xp = np.zeros((n, H + 2 * pad, W + 2 * pad, C), f64)
    xp[:, pad:pad + H, pad:pad + W] = x
    out = np.zeros((n, Ho, Wo, w.shape[0]), f64)
    for ky in range(ks):
        for kx in range(ks):
            out += xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride] @ w[:, ks * ky + kx].T
    return out


def up_nearest(a, f):
    return np.repeat(np.repeat(a, f, axis=1), f, axis=2)


def concat4(levels):
    """(p5, p4, p3, p2) -> [up8(p5), up4(p4), up2(p3), p2] along the channels"""
    return np.concatenate([up_nearest(np.asarray(a, f64), 8 >> i) for i, a in enumerate(levels)], axis=3)


def shuffle2(v):
    """[n][h][w][256], column (2 a + b) 64 + co -> [n][2 h][2 w][64] at (2 i + a, 2 j + b, co): conv_transpose2d k 2 s 2 as a 1x1 conv"""
    n, h, w, _ = v.shape
    return np.ascontiguousarray(v.reshape(n, h, w, 2, 2, 64).transpose(0, 1, 3, 2, 4, 5)).reshape(n, 2 * h, 2 * w, 64)


def accumulate(l, x, w):
    """the sums of a launch in f64: [n][Ho][Wo][Cout], batched [B][n][Ho][Wo][Cout]"""
    if l.batch > 1:
        return np.stack([conv(xb, wb) for xb, wb in zip(np.asarray(x, f64), np.asarray(w, f64))])
    return conv(concat4(x) if l.src == CAT4 else x, w, l.stride)


def finish(l, acc, scale=None, bias=None, residual=None, up_residual=None, relu=False, magnitude=False):
    """-> (out, out2 | None) in f64; magnitude: acc is sum |a||b| and every term enters by its absolute value (no ReLU)"""
    a = np.abs if magnitude else (lambda t: t)
    v = np.asarray(acc, f64)
    if scale is not None:
        v = v * a(np.asarray(scale, f64))
    if bias is not None:
        v = v + a(np.asarray(bias, f64))
    if residual is not None:
        v = v + a(np.asarray(residual, f64)).reshape(v.shape)
    if relu and not magnitude:
        v = np.maximum(v, 0)
    out2 = None if up_residual is None else v + up_nearest(a(np.asarray(up_residual, f64)), 2)
    return (shuffle2(v) if l.store == SHUFFLE2 else v), out2


# ---- operands -----------------------------------------------------------------------------------------------------------------------------------

# name -> the terms of the epilogue; "both": out and out2, "up" alone: out2 only
EPILOGUES = {"none": (), "sbr": ("scale", "bias", "relu"), "sbrr": ("scale", "bias", "res", "relu"), "out2": ("scale", "bias", "up", "both"),
             "out2_only": ("scale", "bias", "up"), "out2_res": ("scale", "bias", "res", "relu", "up", "both")}
INT_FAMILIES = ("signed", "nonneg")
SPLIT_FAMILIES = ("wide_w", "wide_x", "mid")
# the products (plane of A, plane of B) a split family pins: dropping any of them changes the result
PINNED = {"wide_w": ("hi.hi", "hi.mid", "hi.lo"), "wide_x": ("lo.hi", "mid.hi", "hi.hi"), "mid": ("mid.mid", "mid.hi", "hi.mid", "hi.hi")}
WIDE_BITS, MID_BITS, NONZERO = 21, 11, 3
SCALES = {"signed": (0.25, 0.5, 1.0), "nonneg": (0.25, 0.5, 1.0), "wide_w": (0.5, 1.0), "wide_x": (0.5, 1.0), "mid": (1.0,)}


def epilogues_of(l):
    if l.store == SHUFFLE2 or l.batch > 1:
        return ("none", "sbr")
    _, ho, wo = l.out_grid()
    return ("none", "sbr", "sbrr") + (("out2", "out2_only", "out2_res") if not (ho | wo) & 1 else ())


class Ops:
    """x (CAT4: the four levels), w, scale, bias, res, up of one case; acc / mag: the f64 sums of the operands and of their absolute values"""


def _source_shapes(l):
    n, h, w = l.grid
    if l.src == CAT4:
        return [(n, h >> (3 - i), w >> (3 - i), 64) for i in range(4)]
    return [((l.batch,) if l.batch > 1 else ()) + (n, h, w, l.cin)]


def _wide(rng, shape, bits):
    """signed integers of exactly `bits` significant bits with the lowest set: all three bf16 terms (21 bits) or two (11 bits) in use"""
    m = rng.integers(1 << (bits - 1), 1 << bits, shape) | 1
    return (m * rng.choice([-1, 1], shape)).astype(f64)


def _sparse_pixels(rng, shape, ks, bits):
    """activations that are zero except NONZERO channels of the pixels of a lattice of step ks: a window of the conv sees one such pixel"""
    x = np.zeros(shape, f64)
    H, W, C = shape[-3:]
    lead = shape[:-3]
    y0, x0 = int(rng.integers(0, ks)), int(rng.integers(0, ks))
    for idx in np.ndindex(*lead):
        for y in range(y0 % max(min(ks, H), 1), H, ks):
            for xx in range(x0 % max(min(ks, W), 1), W, ks):
                ch = rng.choice(C, NONZERO, replace=False)
                x[idx + (y, xx, ch)] = _wide(rng, NONZERO, bits)
    return x


@functools.lru_cache(maxsize=32)
def operands(key, kind):
    """The operands of a launch's shape (key = Launch.shape_key()) for kind "real" or an integer family: computed once, shared, never modified.
    For an integer family it asserts per epilogue what makes equality a fair demand: every partial sum below 2^24 quanta in any order."""
    l = key
    rng = np.random.default_rng([l.ks, l.stride, l.cin, l.cout, l.src, l.store, l.batch, *l.grid, sum(map(ord, kind))])
    o = Ops()
    shapes = _source_shapes(l)
    wshape = ((l.batch,) if l.batch > 1 else ()) + (l.cout, l.ks * l.ks, l.cin)
    K = l.ks * l.ks * l.cin
    n, ho, wo = l.out_grid()
    oshape = ((l.batch,) if l.batch > 1 else ()) + (n, ho, wo, l.cout)
    if kind == "real":
        def act(shape):
            a = rng.standard_normal(shape)
            if not a.size:      # a 1 x 1 output has no half-resolution pixel
                return a.astype(f32)
            img = a.reshape((-1,) + shape[-4:])
            for b in range(img.shape[0]):
                for i in range(shape[-4]):
                    img[b, i] *= IMAGE_SCALES[i % 3]
            return a.astype(f32)
        xs = [act(s) for s in shapes]
        o.w = (rng.standard_normal(wshape) / np.sqrt(K)).astype(f32)
        o.scale = ((0.5 + rng.random(l.cout)) * rng.choice([-1.0, 1.0], l.cout)).astype(f32)
        o.bias = rng.standard_normal(l.cout).astype(f32)
        o.res, o.up = act(oshape), act((n, ho // 2, wo // 2, l.cout))
    else:
        if kind in INT_FAMILIES:
            xs = [rng.integers(-15 if kind == "signed" else 0, 16, s).astype(f64) for s in shapes]
            o.w = rng.integers(-7, 8, wshape).astype(f64)
        elif kind == "wide_w":
            xs = [rng.integers(-1, 2, s).astype(f64) for s in shapes]
            o.w = np.zeros(wshape, f64).reshape(-1, K)
            for row in o.w:
                at = rng.choice(K, NONZERO, replace=False)
                row[at] = _wide(rng, NONZERO, WIDE_BITS)
            o.w = o.w.reshape(wshape)
        elif kind == "wide_x":
            xs = [_sparse_pixels(rng, s, l.ks, WIDE_BITS) for s in shapes]
            o.w = rng.integers(-1, 2, wshape).astype(f64)
        else:
            assert kind == "mid", kind
            xs = [_sparse_pixels(rng, s, l.ks, MID_BITS) for s in shapes]
            o.w = _wide(rng, wshape, MID_BITS)
        xs, o.w = [a.astype(f32) for a in xs], o.w.astype(f32)
        o.scale = rng.choice(SCALES[kind], l.cout).astype(f32)
        o.res, o.up = rng.integers(-256, 257, oshape).astype(f32), rng.integers(-256, 257, (n, ho // 2, wo // 2, l.cout)).astype(f32)
    o.x = xs if l.src == CAT4 else xs[0]
    q = bf16 if l.form == BF16 else (lambda a: a)
    xq = [q(a) for a in xs] if l.src == CAT4 else q(xs[0])
    o.acc = accumulate(l, xq, q(o.w))
    o.mag = accumulate(l, [np.abs(a) for a in xq] if l.src == CAT4 else np.abs(xq), np.abs(q(o.w)))
    if kind != "real":
        spread = int(min(max(np.abs(o.acc).max(), 300), 4096))
        o.bias = rng.integers(-spread, spread + 1, l.cout).astype(f32)
        quantum = min(SCALES[kind])
        for epi in epilogues_of(l):
            t = EPILOGUES[epi]
            terms = {k: getattr(o, k) if k in t else None for k in ("scale", "bias", "res", "up")}
            big = finish(l, o.mag, terms["scale"], terms["bias"], terms["res"], terms["up"], magnitude=True)
            for m in big:
                assert m is None or m.max() / quantum < LIMIT, (l, kind, epi, float(m.max() / quantum))
            for v in finish(l, o.acc, terms["scale"], terms["bias"], terms["res"], terms["up"], "relu" in t):
                assert v is None or np.array_equal(v.astype(f32).astype(f64), v)
    for a in list(vars(o).values()) + xs:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return o


def terms_of(l, o, epi):
    """the epilogue's operands as the kernel sees them (residuals of the results' type) -> dict scale, bias, res, up (None where absent)"""
    t = EPILOGUES[epi]
    q = bf16 if l.out_bf16 else (lambda a: a)
    return {"scale": o.scale if "scale" in t else None, "bias": o.bias if "bias" in t else None, "res": q(o.res) if "res" in t else None,
            "up": q(o.up) if "up" in t else None}


def expected(l, o, epi):
    """-> (out, out2, mag of out, mag of out2) in f64; out is None for an epilogue that stores the sum only"""
    t = EPILOGUES[epi]
    k = terms_of(l, o, epi)
    out, out2 = finish(l, o.acc, k["scale"], k["bias"], k["res"], k["up"], "relu" in t)
    mag, mag2 = finish(l, o.mag, k["scale"], k["bias"], k["res"], k["up"], magnitude=True)
    if "up" in t and "both" not in t:
        out = mag = None
    return out, out2, mag, mag2


def guard_rows(l):
    _, _, wo = l.out_grid()
    return 2 * wo * (2 if l.store == SHUFFLE2 else 1) + 64      # more than two rows of the output


def launch(run, l, o, epi, **kw):
    """one launch of case o with a named epilogue -> (out, out2); the guard rows behind every output must come back untouched"""
    t = EPILOGUES[epi]
    sentinel = kw.pop("sentinel", SENTINEL)
    x = kw.pop("x", o.x)
    out, out2, guard = run(l.form, x, o.w, out_bf16=l.out_bf16, stride=l.stride, src_mode=l.src, store_mode=l.store, scale=o.scale if "scale" in t else None,
                           bias=o.bias if "bias" in t else None, residual=o.res if "res" in t else None, up_residual=o.up if "up" in t else None,
                           want_out="up" not in t or "both" in t, want_out2="up" in t, relu="relu" in t, tile=l.tile, guard=guard_rows(l),
                           sentinel=sentinel, **kw)
    row = 64 if l.store == SHUFFLE2 else l.cout
    assert guard.size == guard_rows(l) * row * ((out is not None) + (out2 is not None)) and (guard == sentinel).all(), \
        (l.name(), epi, "the launch wrote behind its output")
    return out, out2


# ---- the stand-in -------------------------------------------------------------------------------------------------------------------------------

class Refused(Exception):
    """what conv_igemm.hip's check() refuses"""


FAULTS = ("border_tap", "stride2_origin", "shuffle_swap", "out2_pixel", "row_beyond_m", "cat4_shift", "batch_weight0", "relu_before_residual",
          "split_slot")


def refuse(form, out_bf16, ks, stride, src_mode, store_mode, batch, grid, cin, cout, residual, want_out2, up_residual):
    """check()'s refusals for these source and store modes, by the arguments alone"""
    n, h, w = grid
    pad = (ks - 1) // 2
    ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    bad = []
    if form == SPLIT and (out_bf16 or src_mode == CAT4 or store_mode == SHUFFLE2):
        bad.append("the split form exists for f32 PLAIN convs with NHWC stores")
    if cin % (64 if form == BF16 else 32) or cout % 64:
        bad.append("channels")
    if batch > 1 and (ks != 1 or stride != 1 or src_mode != PLAIN or store_mode != NHWC or residual or want_out2 or form == BF16 or out_bf16):
        bad.append("batched GEMM needs a plain f32 1x1 s1 conv without residual")
    if src_mode == CAT4 and (cin != 256 or (h | w) & 7 or ks != 3 or stride != 1 or cout != 64):
        bad.append("CAT4 needs a 3x3 s1 256->64 conv on a grid divisible by 8")
    if store_mode == SHUFFLE2 and (cout != 256 or ks != 1 or stride != 1 or residual or want_out2 or form == BF16 or out_bf16):
        bad.append("SHUFFLE2 needs a plain f32 1x1 conv with Cout 4*64")
    if want_out2 and (not up_residual or (ho | wo) & 1):
        bad.append("out2 needs up_residual and an even grid")
    if form != BF16 and out_bf16:
        bad.append("f32 operands with bf16 output")
    if form == BF16 and not out_bf16 and src_mode != CAT4 and not (ks == 3 and stride == 1):
        bad.append("bf16 -> f32 exists for the CAT4 and 3x3 s1 convs only")
    return bad


def _lead_pixels(w, c):
    return -(-(w + 1) * c // 1024) * 1024 // c + 1


def _level_memory(a, poison):
    """a tensor [..][H][W][C] between two lead regions -> ([pixels][C], pixels in front)"""
    C = a.shape[-1]
    px = a.reshape(-1, C)
    lp = _lead_pixels(a.shape[-2], C)
    mem = np.full((2 * lp + len(px), C), np.nan if poison else 0.0, f32)
    mem[lp:lp + len(px)] = px
    return mem, lp


def _gather(mem, px, ok):
    d = mem[np.where(ok, np.clip(px, 0, len(mem) - 1), 0)]
    d[~ok] = 0
    return d


def standin(form, x, wgt, out_bf16=False, stride=1, src_mode=PLAIN, store_mode=NHWC, scale=None, bias=None, residual=None, up_residual=None,
            want_out=True, want_out2=False, relu=False, tile=0, poison=False, guard=64, sentinel=SENTINEL, fault=None):
    """The numpy model of Detector.debug_igemm_run.  fault: None or one of FAULTS:
      border_tap            the source column right of the image is not masked (it reads the next pixel in memory)
      stride2_origin        the window of a stride-2 conv starts one pixel further down and right
      shuffle_swap          the pixel shuffle with a and b swapped
      out2_pixel            out2 adds the up_residual pixel of column ow, not ow >> 1
      row_beyond_m          the first row beyond M of a partial last tile is stored
      cat4_shift            CAT4 reads p4 at p3's shift
      batch_weight0         every problem of the batched GEMM multiplies by the weights of problem 0
      relu_before_residual  ReLU acts on acc scale + bias, not on the sum with the residual
      split_slot            split form: the mid plane's 16-byte slots of rows 4 .. 7 of every 16 are swizzled with the slot pattern of rows 0 .. 3"""
    wg = np.asarray(wgt, f32)
    batch = wg.shape[0] if wg.ndim == 4 else 1
    cout, taps, cin = wg.shape[-3:]
    ks = {1: 1, 9: 3}[taps]
    q = bf16 if form == BF16 else (lambda a: np.asarray(a, f32))
    qo = bf16 if out_bf16 else (lambda a: np.asarray(a, f32))
    levels = [q(a) for a in x] if src_mode == CAT4 else [q(x)]
    n, H, W = levels[-1].shape[-4:-1]
    bad = refuse(form, out_bf16, ks, stride, src_mode, store_mode, batch, (n, H, W), cin, cout, residual is not None, want_out2, up_residual is not None)
    if bad or not (want_out or want_out2):
        raise Refused("; ".join(bad) or "no output")
    pad = (ks - 1) // 2
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    wq = q(wg).reshape(batch, cout, taps, cin)
    if form == SPLIT:
        planes = [p.reshape(batch * cout, taps * cin).copy() for p in E.split3(wq)]
        if fault == "split_slot":
            rows = np.flatnonzero((np.arange(batch * cout) % 16) >> 2 == 1)
            planes[1][rows] = planes[1][rows][:, np.arange(taps * cin) ^ 8]
        planes = [p.reshape(batch, cout, taps, cin) for p in planes]
    else:
        planes = [wq]
    b_of = (lambda b: 0) if fault == "batch_weight0" else (lambda b: b)
    off = 1 if (fault == "stride2_origin" and stride == 2) else 0
    acc = np.zeros((batch, n, Ho, Wo, cout), f64)
    img = np.arange(n)[:, None, None]
    for t in range(taps):
        kh, kw = divmod(t, ks)
        ih, iw = stride * np.arange(Ho) - pad + kh + off, stride * np.arange(Wo) - pad + kw + off
        col_ok = (iw >= 0) & (iw < W)
        if fault == "border_tap":
            col_ok |= iw == W
        ok = np.broadcast_to((((ih >= 0) & (ih < H))[None, :, None] & col_ok[None, None, :]), (n, Ho, Wo))
        for li, lv in enumerate(levels):
            s = (3 - li) if src_mode == CAT4 else 0
            if fault == "cat4_shift" and src_mode == CAT4 and li == 1:
                s = 1
            Hl, Wl, C = lv.shape[-3:]
            mem, lp = _level_memory(lv, poison)
            for b in range(batch):
                px = ((b * n + img) * Hl + (ih >> s)[None, :, None]) * Wl + (iw >> s)[None, None, :] + lp
                d = _gather(mem, px, ok).astype(f64)
                for p in planes:
                    acc[b] += d @ p[b_of(b), :, t, li * C:(li + 1) * C].astype(f64).T
    acc = acc.astype(f32)
    one, zero = f32(1), f32(0)
    v = (acc.astype(f64) * (one if scale is None else np.asarray(scale, f32)) + (zero if bias is None else np.asarray(bias, f32))).astype(f32)
    if fault == "relu_before_residual" and relu:
        v = np.maximum(v, zero)
    if residual is not None:
        v = (v + qo(residual).reshape(v.shape)).astype(f32)
    if relu:
        v = np.maximum(v, zero)
    M = batch * n * Ho * Wo
    bm = TILE_ROWS.get(tile, 128 if form == SPLIT or (form == BF16 and ks == 3) else 64)
    outs = []
    for want, plus in ((want_out, None), (want_out2, up_residual)):
        if not want:
            outs.append(None)
            continue
        val = v[0] if batch == 1 else v
        if plus is not None:
            up = qo(plus).reshape(n, Ho // 2, Wo // 2, cout)
            oh, ow = np.arange(Ho) >> 1, np.arange(Wo) >> 1
            if fault == "out2_pixel":
                ow = np.minimum(np.arange(Wo), Wo // 2 - 1)
            val = (val + up[:, oh][:, :, ow]).astype(f32)
        if store_mode == SHUFFLE2:
            if fault == "shuffle_swap":
                val = val.reshape(n, Ho, Wo, 2, 2, 64).transpose(0, 1, 2, 4, 3, 5).reshape(n, Ho, Wo, 256)
            val = shuffle2(val)
        rows, row = int(np.prod(val.shape[:-1])), val.shape[-1]
        io = np.full((rows + guard, row), sentinel, f32)
        io[:rows] = qo(val).reshape(rows, row)
        if fault == "row_beyond_m" and M % bm:
            io[rows] = 0
        outs.append((io, rows, val.shape))
    guards = np.concatenate([io[rows:] for io, rows, _ in filter(None, outs)])
    return tuple(None if e is None else e[0][:e[1]].reshape(e[2]) for e in outs) + (guards,)


# ---- the case lists of tests/test_gpu_igemm_kernels.py ----------------------------------------------------------------------------------------

# (form, bf16 results, tiles): every tile shape check() / pick_tile allow (128 x 128 needs Cout % 128 == 0)
FORMS = ((F32, False, (1, 2, 3)), (SPLIT, False, (1, 2)), (BF16, True, (1, 2, 3)))
KS_STRIDE = ((1, 1), (3, 1), (1, 2), (3, 2))
# M = 1, ragged, 306, rows of BM + 2 pixels, M = 65, 128, 129
GRIDS = ((1, 1, 1), (3, 5, 3), (2, 9, 17), (1, 3, 130), (1, 5, 13), (1, 8, 16), (1, 3, 43))
STRIDE2_GRIDS = GRIDS + ((2, 10, 18),)         # an even input grid: the last output row and column lose different taps
OUT2_GRIDS = ((1, 2, 2), (2, 6, 10), (1, 12, 22))   # of the output; (1, 12, 22): tiles split image rows
# Cin -> Cout: one K chunk per tap (32 f32 / 64 bf16 elements), four chunks, and one in between; Cout 64 and 192 are no multiple of 128
CHANNELS = {F32: ((32, 64), (128, 192), (64, 256), (256, 128)), SPLIT: ((32, 64), (128, 192), (64, 256), (256, 128)),
            BF16: ((64, 64), (256, 192), (128, 256), (256, 128))}
SHUFFLE_GRIDS = ((1, 1, 1), (2, 3, 5), (1, 9, 15))
CAT4_GRIDS = ((1, 8, 8), (2, 8, 16), (1, 16, 24))
BATCHED = tuple((m, k, c) for m in (1, 63, 130) for k, c in ((64, 64), (256, 128), (64, 128)))


def _tiles(tiles, cout):
    return [t for t in tiles if t != 1 or cout % 128 == 0]


def plain_launches(grids_per=None):
    """every form x tile x (ks, stride) x grid, the channel pairs dealt round over the grids (every pair meets every (ks, stride))"""
    out = []
    for form, obf, tiles in FORMS:
        for j, (ks, stride) in enumerate(KS_STRIDE):
            grids = STRIDE2_GRIDS if stride == 2 else GRIDS
            extra = [(g[0], stride * g[1], stride * g[2]) for g in OUT2_GRIDS]
            for i, g in enumerate(tuple(grids) + tuple(e for e in extra if e not in grids)):
                cin, cout = CHANNELS[form][(i + j) % len(CHANNELS[form])]
                for t in _tiles(tiles, cout):
                    out.append(Launch(form, obf, ks, stride, g, cin, cout, tile=t))
    # bf16 operands with f32 results: the 3x3 s1 conv only
    for i, g in enumerate(GRIDS):
        cin, cout = CHANNELS[BF16][i % 4]
        out += [Launch(BF16, False, 3, 1, g, cin, cout, tile=t) for t in _tiles((1, 2, 3), cout)]
    return out


def other_launches():
    out = [Launch(F32, False, 1, 1, g, cin, 256, store=SHUFFLE2, tile=t) for g, cin in zip(SHUFFLE_GRIDS, (64, 64, 64)) for t in (1, 2, 3)]
    out += [Launch(F32, False, 1, 1, (1, 5, 13), 32, 256, store=SHUFFLE2), Launch(F32, False, 1, 1, (1, 3, 43), 128, 256, store=SHUFFLE2)]
    for g in CAT4_GRIDS:
        out += [Launch(F32, False, 3, 1, g, 256, 64, src=CAT4, tile=t) for t in (2, 3)]
        out += [Launch(BF16, obf, 3, 1, g, 256, 64, src=CAT4, tile=t) for obf in (True, False) for t in (2, 3)]
    for m, k, c in BATCHED:
        out += [Launch(F32, False, 1, 1, (1, 1, m), k, c, batch=3, tile=t) for t in _tiles((1, 2, 3), c)]
        out += [Launch(SPLIT, False, 1, 1, (1, 1, m), k, c, batch=3, tile=t) for t in _tiles((1, 2), c)]
    return out


def all_launches():
    return plain_launches() + other_launches()


def split_launches():
    """the split form's launches of families (b): one grid per (ks, stride) and the batched GEMM, both tiles"""
    out = []
    for (ks, stride), g, (cin, cout) in zip(KS_STRIDE, ((2, 9, 17), (1, 3, 130), (2, 10, 18), (2, 10, 18)), ((64, 128), (32, 128), (128, 128), (64, 128))):
        out += [Launch(SPLIT, False, ks, stride, g, cin, cout, tile=t) for t in (1, 2)]
    return out + [Launch(SPLIT, False, 1, 1, (1, 1, 130), 64, 128, batch=3, tile=t) for t in (1, 2)]


def family_of(l):
    """the integer family of a launch in G1: both meet every form and (ks, stride)"""
    return INT_FAMILIES[(sum(l.grid) + l.cin // 32 + l.tile) % 2]


def refused_combinations():
    """(name, a fragment of check()'s message, keyword arguments of `run`) of what check() refuses for these source and store modes"""
    rng = np.random.default_rng(0)

    def t(*shape):
        return rng.integers(-3, 4, shape).astype(f32)

    def levels(n, h, w):
        return [t(n, h >> (3 - i), w >> (3 - i), 64) for i in range(4)]
    x64, w256 = t(2, 4, 6, 64), t(256, 1, 64)
    return [
        ("split with CAT4", "the split-bf16 form exists", dict(form=SPLIT, x=levels(1, 8, 8), wgt=t(64, 9, 256), src_mode=CAT4)),
        ("split with SHUFFLE2", "the split-bf16 form exists", dict(form=SPLIT, x=x64, wgt=w256, store_mode=SHUFFLE2)),
        ("split with bf16 results", "the split-bf16 form exists", dict(form=SPLIT, x=x64, wgt=t(64, 1, 64), out_bf16=True)),
        ("SHUFFLE2 with a residual", "SHUFFLE2 store needs", dict(form=F32, x=x64, wgt=w256, store_mode=SHUFFLE2, residual=t(2, 4, 6, 256))),
        ("SHUFFLE2 with out2", "SHUFFLE2 store needs", dict(form=F32, x=x64, wgt=w256, store_mode=SHUFFLE2, want_out2=True, up_residual=t(2, 2, 3, 256))),
        ("SHUFFLE2 in bf16", "SHUFFLE2 store needs", dict(form=BF16, x=x64, wgt=w256, store_mode=SHUFFLE2, out_bf16=True)),
        ("SHUFFLE2 with Cout 128", "SHUFFLE2 store needs", dict(form=F32, x=x64, wgt=t(128, 1, 64), store_mode=SHUFFLE2)),
        ("SHUFFLE2 with stride 2", "SHUFFLE2 store needs", dict(form=F32, x=x64, wgt=w256, store_mode=SHUFFLE2, stride=2)),
        ("SHUFFLE2 of a 3x3 conv", "SHUFFLE2 store needs", dict(form=F32, x=x64, wgt=t(256, 9, 64), store_mode=SHUFFLE2)),
        ("out2 on an odd grid", "out2 needs up_residual", dict(form=F32, x=t(1, 3, 6, 64), wgt=t(64, 1, 64), want_out2=True, up_residual=t(1, 1, 3, 64))),
        ("out2 without up_residual", "out2 needs up_residual", dict(form=F32, x=x64, wgt=t(64, 1, 64), want_out2=True)),
        ("f32 operands with bf16 results", "f32 operands with bf16 output", dict(form=F32, x=x64, wgt=t(64, 1, 64), out_bf16=True)),
        ("bf16 -> f32 of a 1x1 conv", "bf16 -> f32 exists", dict(form=BF16, x=x64, wgt=t(64, 1, 64))),
        ("batched with a residual", "batched GEMM needs", dict(form=F32, x=t(3, 1, 1, 5, 64), wgt=t(3, 64, 1, 64), residual=t(3, 1, 1, 5, 64))),
        ("batched in bf16", "batched GEMM needs", dict(form=BF16, x=t(3, 1, 1, 5, 64), wgt=t(3, 64, 1, 64), out_bf16=True)),
        ("batched 3x3", "batched GEMM needs", dict(form=F32, x=t(3, 1, 1, 5, 64), wgt=t(3, 64, 9, 64))),
        ("CAT4 off a grid divisible by 8", "CAT4 needs", dict(form=F32, x=levels(1, 12, 20), wgt=t(64, 9, 256), src_mode=CAT4)),
        ("CAT4 with Cout 128", "CAT4 needs", dict(form=F32, x=levels(1, 8, 8), wgt=t(128, 9, 256), src_mode=CAT4)),
        ("Cin no multiple of the K chunk", "Cin 32 not a multiple of 64", dict(form=BF16, x=t(2, 4, 6, 32), wgt=t(64, 1, 32), out_bf16=True)),
    ]


# ---- the assertions, as functions of `run` -------------------------------------------------------------------------------------------------------

def assert_equal(name, got, want):
    assert (got is None) == (want is None), name
    if got is None:
        return
    assert np.isfinite(got).all(), (name, int((~np.isfinite(got)).sum()), "not finite")
    bad = got != want
    assert not bad.any(), (name, int(bad.sum()), "elements differ, first at", tuple(int(i) for i in np.argwhere(bad)[0]), float(got[bad][0]), float(want[bad][0]))


def exact_results(l, o, epi):
    """the bits an integer case must give: the exact value, for bf16 results rounded ONCE"""
    out, out2, _, _ = expected(l, o, epi)
    r = (lambda v: None if v is None else (bf16(v.astype(f32)) if l.out_bf16 else v.astype(f32)))
    return r(out), r(out2)


def check_g1(run, l, family=None):
    """G1: equality with the exact result on an integer family, under every epilogue the launch can have"""
    family = family or family_of(l)
    o = operands(l.shape_key(), family)
    for epi in epilogues_of(l):
        got, want = launch(run, l, o, epi), exact_results(l, o, epi)
        for which, g, w in zip(("out", "out2"), got, want):
            assert_equal(f"{l.name()} {family} {epi} {which}", g, w)


def check_f32(name, got, ref, mag, report=print):
    err = np.abs(got.astype(f64) - ref)
    scale = float(np.abs(ref).max()) + 1e-12
    report(f"G2 {name}: max |err| / magnitude {float((err / mag).max()):.3g}  max |err| / scale {float(err.max()) / scale:.3g}")
    assert np.isfinite(got).all(), name
    assert (err <= 4e-6 * mag).all(), (name, float((err / mag).max()))
    assert float(err.max()) / scale < 2e-5, name


def check_bf16(name, got, ref, report=print):
    """tests/test_gpu_conv_kernel.py::_check for bf16 results: one bf16 ulp + 1e-5 of the scale, fewer than 1 % beyond 1e-5 of the scale"""
    scale = float(np.abs(ref).max()) + 1e-12
    refq = bf16(ref.astype(f32))
    tol = np.abs(refq) * 2.0 ** -7 + 1e-5 * scale
    diff = np.abs(got - refq)
    report(f"G2 {name}: max (diff - tol) {float((diff - tol).max()):.3g}  beyond 1e-5 of the scale {float((diff > 1e-5 * scale).mean()):.4f}")
    assert np.isfinite(got).all(), name
    assert (diff <= tol).all(), (name, float((diff - tol).max()))
    assert float((diff > 1e-5 * scale).mean()) < 0.01, name


def check_g2(run, l, report=print):
    """G2: real data against the f64 evaluation of the operands the kernel gets, under every epilogue"""
    o = operands(l.shape_key(), "real")
    for epi in epilogues_of(l):
        got = launch(run, l, o, epi)
        out, out2, mag, mag2 = expected(l, o, epi)
        for which, g, r, m in zip(("out", "out2"), got, (out, out2), (mag, mag2)):
            assert (g is None) == (r is None), (l.name(), epi, which)
            if g is None:
                continue
            if l.out_bf16:
                check_bf16(f"{l.name()} {epi} {which}", g, r, report)
            else:
                check_f32(f"{l.name()} {epi} {which}", g, r, m, report)


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def check_g3(run, l):
    """G3: two runs over different prefills give the same bits (an element that kept its prefill would differ); behind ReLU no element is the
    prefill; with out == null the sum alone is stored and has the bits of the run with both outputs"""
    o = operands(l.shape_key(), "real")
    epis = epilogues_of(l)
    for epi in ("sbr",) + (("out2", "out2_res") if "out2" in epis else ()):
        a, b = launch(run, l, o, epi), launch(run, l, o, epi, sentinel=-9.0)
        for which, u, v in zip(("out", "out2"), a, b):
            if u is not None:
                assert np.array_equal(_bits(u), _bits(v)), (l.name(), epi, which, "depends on what the buffer held")
        if epi == "sbr":
            assert (a[0] >= 0).all(), (l.name(), int((a[0] == SENTINEL).sum()), "elements kept their prefill")
        if epi == "out2":
            only = launch(run, l, o, "out2_only")
            assert only[0] is None and np.array_equal(_bits(only[1]), _bits(a[1])), (l.name(), "out2 alone differs from out2 beside out")


def check_g4_poison(run, l):
    """G4: NaN around the source (CAT4: between the levels) inside its allocation: finite results with the bits of the clean run"""
    o = operands(l.shape_key(), "real")
    # without an epilogue a NaN that was read is a NaN that is stored (behind ReLU fmaxf(NaN, 0) is 0 and only the bits would show it); then
    # the epilogue with the most terms
    for epi in ("none", "sbrr" if "sbrr" in epilogues_of(l) else "sbr"):
        clean, dirty = launch(run, l, o, epi), launch(run, l, o, epi, poison=True)
        assert np.isfinite(dirty[0]).all(), (l.name(), epi, int((~np.isfinite(dirty[0])).sum()), "results not finite")
        assert np.array_equal(_bits(clean[0]), _bits(dirty[0])), (l.name(), epi)


def _images(l, o, pick):
    """the source with pick(array [n]...) applied to every level"""
    return [pick(np.array(a)) for a in o.x] if l.src == CAT4 else pick(np.array(o.x))


def check_g4_batch(run, l):
    """G4: the middle image of three is NaN throughout: the other two keep their bits - a pixel of another image is selected away, not
    multiplied by zero"""
    assert l.grid[0] == 3 and l.batch == 1
    o = operands(l.shape_key(), "real")
    epi = "none"        # (fmaxf(NaN, 0) is 0: behind ReLU the poisoned image would not show that it was read)

    def nan1(a):
        a[1] = np.nan
        return a
    clean, dirty = launch(run, l, o, epi)[0], launch(run, l, o, epi, x=_images(l, o, nan1))[0]
    clean, dirty = [a.reshape(3, -1) for a in (clean, dirty)]
    assert np.isfinite(clean).all() and np.isnan(dirty[1]).any()
    for i in (0, 2):
        assert np.array_equal(_bits(clean[i]), _bits(dirty[i])), (l.name(), f"image {i} changed with image 1")


def check_g4_alone(run, l):
    """G4: image 1 alone gives the bits it has in the middle of a batch of three whose images are no multiple of the tile's rows: the
    order of a row's sums does not depend on where the row sits in its tile"""
    assert l.grid[0] == 3 and l.batch == 1 and l.store == NHWC
    o = operands(l.shape_key(), "real")
    batch = launch(run, l, o, "none")[0]
    one = l._replace(grid=(1,) + l.grid[1:])
    alone = launch(run, one, o, "none", x=_images(l, o, lambda a: a[1:2]))[0]
    assert np.array_equal(_bits(batch[1]), _bits(alone[0])), (l.name(), float(np.abs(batch[1] - alone[0]).max()))


G5_CASES = E.IGEMM_CASES     # (n, h, w, cin, cout, ks, stride, batch)


@functools.lru_cache(maxsize=None)
def g5_case(case):
    x, wg, stride = E.igemm_family(case)
    return x, wg, stride, E.ConvCase(x, wg, stride, kgroup=32)


@functools.lru_cache(maxsize=None)
def g5_bar(case):
    return E.bar(g5_case(case)[3])


def check_g5(run, case, form, tile, report=print):
    """G5: rms(kernel - f64) in units of sum |a||b| stays below sqrt(rms of six products x smallest rms of five), split and exact f32 alike"""
    x, wg, stride, cc = g5_case(case)
    n, h, w, cin, cout, ks, _, batch = case
    l = Launch(form, False, ks, stride, (n, h, w), cin, cout, batch=batch, tile=tile)
    out, _, guard = run(form, x, wg, stride=stride, tile=tile, guard=guard_rows(l), sentinel=SENTINEL)
    assert guard.size and (guard == SENTINEL).all(), (l.name(), "the launch wrote behind its output")
    six, five, bar, _ = g5_bar(case)
    rms = cc.rms(out)
    report(f"G5 {l.name()}: measured rms {rms:.3g}  emulated six {six:.3g}  five {five:.3g}  bar {bar:.3g}")
    assert rms <= bar, (l.name(), rms, bar)
    return rms
