"""The trunk convs of the bf16 precision - conv3x3_bf16_c64_kernel (form 0), basic_block_bf16_c64_kernel (form 1) and conv_igemm with bf16
operands and results (form 2) - stated without a GPU.  With bf16 operands a product is exact in f32 and a sum of small integers is exact below
2^24, so on the integer families the only rounding is the one f32 -> bf16 conversion of the output (and, in the block, of the intermediate):
the result is determined bit for bit whatever the order of the sums.

  * the operation by definition in f64 (`direct_conv`, `IntCase.reference`, `RealCase`): conv -> fma(acc, scale, bias) -> + residual -> ReLU ->
    ONE round-to-nearest-even to bf16; the block's intermediate is bf16(relu(fma(acc1, s1, b1))), zero outside the image;
  * integer families (`integer_case`): activations small integers (signed, or non-negative as behind a ReLU), weights small integers, scales
    powers of two in [1/4, 1], bias and residuals integers.  Per case and epilogue it asserts that every partial sum stays below 2^24 in units
    of the smallest quantum (for the block: conv2 over the ROUNDED intermediate), that some outputs exceed 256 (where bf16 no longer holds
    every integer), that some are exact ties of the rounding, and that at least a quarter survive ReLU;
  * `standin`, a numpy model with the signature of Detector.debug_bf16_trunk_run that follows the kernels' structure - the source inside an
    allocation with lead regions, 8 x 16 pixel blocks with their halo gathered by linear pixel index, the block's 10 x 18 intermediate, the
    persistent walks of both launchers, conv_igemm's rows as a linear run of pixels masked per tap - and, on request, commits one of `FAULTS`;
  * the assertions of tests/test_gpu_bf16_trunk_kernels.py (`check_b1` .. `check_b4`) as functions of a `run` callable, so that
    tests/test_bf16_conv_oracle.py can show that the model passes every one of them and that every fault fails at least one.

`run(form, x, wgt, scale=, bias=, residual=, relu=, stride=, up_residual=, want_out=, wgt2=, scale2=, bias2=, num_cus=, guard=, poison=,
sentinel=) -> (out | None, out2 | None, guard rows)`."""
import functools

import numpy as np

from tests import split_bf16_emul as E

f32, f64 = np.float32, np.float64
SENTINEL = -7.0       # a bf16 value
C64, BLOCK, IGEMM = 0, 1, 2
FORM_NAMES = {C64: "conv3x3_bf16_c64", BLOCK: "basic_block_bf16_c64", IGEMM: "conv_igemm bf16"}
LIMIT = 1 << 24


# ---- bf16 ------------------------------------------------------------------------------------------------------------------------------

def bf16_rne(a):
    """f32 -> bf16, round to nearest even, widened back to f32 (NaN stays NaN)"""
    a = np.ascontiguousarray(a, dtype=f32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(f32)
    return np.where(np.isnan(a), a, r)


def bf16_trunc(a):
    a = np.ascontiguousarray(a, dtype=f32)
    return (a.view(np.uint32) & np.uint32(0xffff0000)).view(f32)


def bf16_from_f64(v):
    """f64 -> bf16 in ONE rounding to nearest even (not through f32), as f32; normal range only"""
    m, e = np.frexp(np.asarray(v, f64))
    return np.ldexp(np.rint(m * 256.0) / 256.0, e).astype(f32)


def fma32(a, b, c):
    """a b + c of f32 values, rounded once (the product of two f32 is exact in f64)"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def bf16_step(v):
    """the distance from a positive bf16 value to the next one above it"""
    return np.ldexp(1.0, np.frexp(np.asarray(v, f64))[1] - 8)


def bf16_at_least(v):
    """the smallest bf16 value >= v (f64), as f32"""
    r = bf16_rne(np.asarray(v, f64).astype(f32))
    u = r.view(np.uint32)
    up = np.where(r > 0, u + np.uint32(0x10000), np.where(r < 0, u - np.uint32(0x10000), np.uint32(0x00800000))).astype(np.uint32).view(f32)
    return np.where(r.astype(f64) < v, up, r)


def is_tie(v):
    """f32 values exactly half way between two bf16 values"""
    return (np.ascontiguousarray(v, dtype=f32).view(np.uint32) & np.uint32(0xffff)) == 0x8000


def bf16_steps(a, b):
    """how many bf16 values a and b (bf16 values held in f32) lie apart"""
    def order(v):
        bits = (np.ascontiguousarray(v, dtype=f32).view(np.uint32) >> 16).astype(np.int64)
        return np.where(bits & 0x8000, -(bits & 0x7fff), bits & 0x7fff)
    return np.abs(order(a) - order(b))


# ---- the operation by definition ---------------------------------------------------------------------------------------------------------

def out_grid(h, w, ks, stride):
    pad = (ks - 1) // 2
    return (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1


def direct_conv(x, w, stride=1):
    """x [n][H][W][C], w [K][ks ks][C] (tap = ks ky + kx) -> [n][Ho][Wo][K] in f64: zero padding (ks - 1) / 2"""
    x, w = np.asarray(x, f64), np.asarray(w, f64)
    n, H, W, C = x.shape
    ks = {1: 1, 9: 3}[w.shape[1]]
    pad = (ks - 1) // 2
    Ho, Wo = out_grid(H, W, ks, stride)
    xp = np.zeros((n, H + 2 * pad, W + 2 * pad, C), f64)
    xp[:, pad:pad + H, pad:pad + W] = x
    out = np.zeros((n * Ho * Wo, w.shape[0]), f64)
    for t in range(ks * ks):
        ky, kx = divmod(t, ks)
        out += np.ascontiguousarray(xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]).reshape(-1, C) @ w[:, t].T
    return out.reshape(n, Ho, Wo, -1)


def upsample2(up, ho, wo):
    """[n][ho / 2][wo / 2][K] -> [n][ho][wo][K], nearest"""
    return np.repeat(np.repeat(up, 2, axis=1), 2, axis=2)[:, :ho, :wo]


# ---- the kernels' structure -----------------------------------------------------------------------------------------------------------------

def c64_walk(nblocks, num_cus):
    """launch_conv3x3_bf16_c64's grid and the kernel's walk: per workgroup the blocks it computes, in order"""
    grid = min(nblocks, 2 * (num_cus if num_cus > 0 else 256))
    return [list(range(wg, nblocks, grid)) for wg in range(grid)]


def block_walk(nblocks, num_cus):
    """launch_basic_block_bf16_c64's: a grid that is a multiple of 8 gives each XCD one contiguous eighth of the blocks"""
    grid = min(nblocks, num_cus if num_cus > 0 else 256)
    if grid % 8:
        return [list(range(wg, nblocks, grid)) for wg in range(grid)]
    return [list(range(nblocks * (wg & 7) // 8 + (wg >> 3), nblocks * ((wg & 7) + 1) // 8, grid >> 3)) for wg in range(grid)]


def _memory(x, poison):
    """the hook's allocation: the tensor between two lead regions of at least (W + 1) C elements -> ([pixels][C], pixels in front)"""
    n, H, W, C = x.shape
    lead = -(-(W + 1) * C // 1024) * 1024
    assert lead % C == 0
    mem = np.full((2 * lead + x.size) // C * C, np.nan if poison else 0.0, f32).reshape(-1, C)
    mem[lead // C:lead // C + n * H * W] = x.reshape(-1, C)
    return mem, lead // C


def _gather(mem, px, ok):
    d = mem[np.where(ok, np.clip(px, 0, len(mem) - 1), 0)]
    d[~ok] = 0
    return d


def _sum64(taps, w):
    """the conv of gathered taps ([rows][C] each) in f64, rounded to the f32 accumulator once"""
    return sum(t.astype(f64) @ w[:, i].astype(f64).T for i, t in enumerate(taps)).astype(f32)


def _chain32(taps, w):
    """the same as a sequential f32 chain, one fused multiply-add per k (split_bf16_emul.f32_chain), taps outer"""
    return E.f32_chain(np.concatenate(taps, axis=1), np.ascontiguousarray(w.reshape(w.shape[0], -1).T))


def _patch_conv(d, w, conv):
    """[B][R + 2][S + 2][C] -> [B][R][S][K]"""
    B, R, S, C = d.shape[0], d.shape[1] - 2, d.shape[2] - 2, d.shape[3]
    return conv([np.ascontiguousarray(d[:, ky:ky + R, kx:kx + S]).reshape(-1, C) for ky in range(3) for kx in range(3)], w).reshape(B, R, S, -1)


# what a kernel of this family could get wrong
FAULTS = ("top_halo", "halo_right", "mid_outside", "mid_f32", "round_before_residual", "relu_before_residual", "truncate", "ragged_row",
          "stale_block")


def standin(form, x, wgt, scale=None, bias=None, residual=None, relu=False, stride=1, up_residual=None, want_out=True, wgt2=None, scale2=None,
            bias2=None, num_cus=0, guard=64, poison=False, sentinel=SENTINEL, fault=None, chain=False):
    """The numpy model of Detector.debug_bf16_trunk_run.  chain: the sums as a sequential f32 chain instead of f64 rounded once (on the integer
    families both are exact).  fault: None or one of FAULTS:
      top_halo               the source row above image n > 0 is not masked (it reads the last row of image n - 1)
      halo_right             the source column right of the image is not masked (it reads the next row's first pixel)
      mid_outside            form 1: the intermediate's pixels outside the image are conv1 evaluated there, not zero padding
      mid_f32                form 1: the intermediate is not rounded to bf16
      round_before_residual  fma(acc, scale, bias) is rounded to bf16 before the residual is added
      relu_before_residual   ReLU acts on fma(acc, scale, bias), not on the sum with the residual
      truncate               f32 -> bf16 by truncation
      ragged_row             the last row of a ragged block (forms 0, 1: H no multiple of 8; form 2: M no multiple of the row tile) is not stored
      stale_block            forms 0, 1: the second block of a workgroup's walk is computed from the patch of its first"""
    to_bf16 = bf16_trunc if fault == "truncate" else bf16_rne
    conv = _chain32 if chain else _sum64
    x, wgt = bf16_rne(x), bf16_rne(wgt)
    n, H, W, C = x.shape
    K, ks = wgt.shape[0], {1: 1, 9: 3}[wgt.shape[1]]
    Ho, Wo = out_grid(H, W, ks, stride)
    mem, lp = _memory(x, poison)
    one, zero = f32(1), f32(0)
    sc, bi = (one if scale is None else np.asarray(scale, f32)), (zero if bias is None else np.asarray(bias, f32))
    res = None if residual is None else bf16_rne(residual).reshape(n, Ho, Wo, K)

    def finish(acc, s, b, r):
        """-> the f32 value the kernel rounds"""
        v = fma32(acc, s, b)
        if fault == "round_before_residual":
            v = to_bf16(v)
        if fault == "relu_before_residual" and relu:
            v = np.maximum(v, zero)
        if r is not None:
            v = (v + r).astype(f32)
        return np.maximum(v, zero) if relu else v

    if form == IGEMM:
        # rows = output pixels in linear order; tap (kh, kw) of row m = pixel (ih, iw) = a fixed distance in memory, masked per row
        pad = (ks - 1) // 2
        taps = []
        for t in range(ks * ks):
            kh, kw = divmod(t, ks)
            ih, iw = stride * np.arange(Ho) - pad + kh, stride * np.arange(Wo) - pad + kw
            row_ok = np.broadcast_to((ih >= 0) & (ih < H), (n, Ho)).copy()
            col_ok = (iw >= 0) & (iw < W)
            if fault == "top_halo":
                row_ok[1:] |= ih == -1
            if fault == "halo_right":
                col_ok |= iw == W
            ok = row_ok[:, :, None] & col_ok[None, None, :]
            px = (np.arange(n)[:, None, None] * H + ih[None, :, None]) * W + iw[None, None, :] + lp
            taps.append(_gather(mem, px, ok).reshape(-1, C))
        v = finish(conv(taps, wgt).reshape(n, Ho, Wo, K), sc, bi, res)
        M, bm = n * Ho * Wo, 128 if ks == 3 else 64
        rows = M - 1 if (fault == "ragged_row" and M % bm) else M
        outs = []
        for want, plus in ((want_out, None), (up_residual is not None, up_residual)):
            if not want:
                outs.append(None)
                continue
            io = np.full((M + guard, K), sentinel, f32)
            val = v if plus is None else (v + upsample2(bf16_rne(plus).reshape(n, Ho // 2, Wo // 2, K), Ho, Wo)).astype(f32)
            io[:rows] = to_bf16(val).reshape(M, K)[:rows]
            outs.append(io)
        return tuple(None if io is None else io[:M].reshape(n, Ho, Wo, K) for io in outs) + (np.concatenate([io[M:] for io in outs if io is not None]),)

    assert form in (C64, BLOCK) and (C, K, ks, stride) == (64, 64, 3, 1) and up_residual is None and want_out
    assert form == C64 or (residual is None and relu and wgt2 is not None)
    bh, bw = -(-H // 8), -(-W // 16)
    nb = n * bh * bw
    bb = np.arange(nb)
    img, y0, x0 = bb // (bh * bw), 8 * ((bb // bw) % bh), 16 * (bb % bw)
    halo = 2 if form == BLOCK else 1
    ys, xs = y0[:, None] - halo + np.arange(8 + 2 * halo)[None], x0[:, None] - halo + np.arange(16 + 2 * halo)[None]
    row_ok, col_ok = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    if fault == "top_halo":
        row_ok |= (ys == -1) & (img[:, None] > 0)
    if fault == "halo_right":
        col_ok |= xs == W
    ok = row_ok[:, :, None] & col_ok[:, None, :]
    d = _gather(mem, (img[:, None, None] * H + ys[:, :, None]) * W + xs[:, None, :] + lp, ok)        # [blocks][8 + 2 halo][16 + 2 halo][64]
    if fault == "stale_block":
        src = bb.copy()
        for walk in (block_walk if form == BLOCK else c64_walk)(nb, num_cus):
            if len(walk) > 1:
                src[walk[1]] = walk[0]
        d = d[src]
    oy, ox = y0[:, None] + np.arange(8)[None], x0[:, None] + np.arange(16)[None]
    inside = ((oy < H)[:, :, None] & (ox < W)[:, None, :])                                             # [blocks][8][16]
    opx = (img[:, None, None] * H + oy[:, :, None]) * W + ox[:, None, :]
    if form == C64:
        r = None if res is None else _gather(res.reshape(-1, K), opx, inside)
        v = finish(_patch_conv(d, wgt, conv), sc, bi, r)
    else:
        mid = np.maximum(fma32(_patch_conv(d, wgt, conv), sc, bi), zero)
        if fault != "mid_f32":
            mid = to_bf16(mid)
        my, mx = y0[:, None] - 1 + np.arange(10)[None], x0[:, None] - 1 + np.arange(18)[None]
        if fault != "mid_outside":
            mid[~(((my >= 0) & (my < H))[:, :, None] & ((mx >= 0) & (mx < W))[:, None, :])] = 0
        sc2, bi2 = (one if scale2 is None else np.asarray(scale2, f32)), (zero if bias2 is None else np.asarray(bias2, f32))
        v = finish(_patch_conv(mid, bf16_rne(wgt2), conv), sc2, bi2, d[:, 2:10, 2:18])
    stored = inside.copy()
    if fault == "ragged_row" and H % 8:
        stored &= (oy != H - 1)[:, :, None]
    io = np.full((n * H * W + guard, K), sentinel, f32)
    io[opx[stored]] = to_bf16(v)[stored]
    return io[:n * H * W].reshape(n, H, W, K), None, io[n * H * W:]


# ---- integer families -------------------------------------------------------------------------------------------------------------------------

FAMILIES = ("signed", "nonneg")
EPILOGUES = ("none", "scale_bias", "residual")       # residual: scale + bias + residual, as a block ends
BLOCK_EPILOGUES = ("none", "scale_bias")             # the block adds x and applies ReLU whatever its scales
# largest |x|, largest |w|: a one-pixel image of 64 channels still reaches outputs beyond 256; the block's second conv multiplies the first's
# magnitudes once more and takes the smaller pair
MAGNITUDES = {C64: (15, 7), IGEMM: (15, 7), BLOCK: (7, 3)}


class IntCase:
    """x, w and the epilogue operands of one integer case (spec = shape, cin, cout, ks, stride, lateral)"""

    def operands(self, epi):
        """-> the keyword arguments of `run` for a named epilogue"""
        kw = {"stride": self.stride}
        if self.form == BLOCK:
            kw.update(wgt2=self.w2)
            if epi == "scale_bias":
                kw.update(scale=self.scale, bias=self.bias, scale2=self.scale2, bias2=self.bias2)
            return kw
        if epi != "none":
            kw.update(scale=self.scale, bias=self.bias)
        if epi == "residual":
            kw.update(residual=self.res)
        if self.lateral:
            kw.update(up_residual=self.up, want_out=self.lateral == "both")
        return kw

    def exact(self, epi, relu):
        """-> (the value the kernel rounds, in f64 - exact; the largest partial sum in units of the smallest quantum)"""
        on = epi != "none"
        sc, bi = (self.scale.astype(f64), self.bias.astype(f64)) if on else (1.0, 0.0)
        q = float(np.min(sc))
        if self.form == BLOCK:
            sc2, bi2 = (self.scale2.astype(f64), self.bias2.astype(f64)) if on else (1.0, 0.0)
            q2 = q * float(np.min(sc2))
            mid = bf16_rne(np.maximum(self.acc * sc + bi, 0)).astype(f64)
            v = direct_conv(mid, self.w2) * sc2 + bi2 + self.x
            big = max(((self.mag * sc + np.abs(bi)) / q).max(), (direct_conv(mid, np.abs(self.w2)) / q).max(),
                      ((direct_conv(mid, np.abs(self.w2)) * sc2 + np.abs(bi2) + np.abs(self.x)) / q2).max())
            return np.maximum(v, 0), float(big)
        v, big = self.acc * sc + bi, self.mag * sc + np.abs(bi)
        if epi == "residual":
            v, big = v + self.res, big + np.abs(self.res)
        v = np.maximum(v, 0) if relu else v
        return v, float(((big + (256 if self.lateral else 0)) / q).max())

    def reference(self, epi, relu):
        """-> (out, out2): bf16 values in f32, None where the case has no such output"""
        v = self.exact(epi, relu)[0].astype(f32)
        if not self.lateral:
            return bf16_rne(v), None
        ho, wo = v.shape[1:3]
        return (bf16_rne(v) if self.lateral == "both" else None), bf16_rne(v + upsample2(self.up, ho, wo))


@functools.lru_cache(maxsize=8)
def integer_case(form, spec, family):
    """One integer case (computed once, shared, never modified).  Asserts per epilogue what makes equality a fair and a sharp demand: every
    partial sum below 2^24 quanta, the value representable in f32, outputs beyond 256, exact ties, a quarter of the outputs behind ReLU."""
    shape, cin, cout, ks, stride, lateral = spec
    n, H, W = shape
    ax, aw = MAGNITUDES[form]
    rng = np.random.default_rng(1000003 * FAMILIES.index(family) + 7919 * cin + 31 * cout + 10007 * n + 101 * H + W + 13 * ks + 17 * stride + form)
    c = IntCase()
    c.form, c.spec, c.shape, c.stride, c.lateral = form, spec, shape, stride, lateral
    c.x = rng.integers(-ax if family == "signed" else 0, ax + 1, (n, H, W, cin)).astype(f32)
    c.w = rng.integers(-aw, aw + 1, (cout, ks * ks, cin)).astype(f32)
    c.acc, c.mag = direct_conv(c.x, c.w, stride), direct_conv(np.abs(c.x), np.abs(c.w), stride)

    def epilogue_operands(acc):
        spread = int(min(max(np.abs(acc).max(), 300), 4096))
        return rng.choice([0.25, 0.5, 1.0], cout).astype(f32), rng.integers(-spread, spread + 1, cout).astype(f32)

    c.scale, c.bias = epilogue_operands(c.acc)
    ho, wo = c.acc.shape[1:3]
    c.res = rng.integers(-256, 257, (n, ho, wo, cout)).astype(f32)
    c.up = rng.integers(-256, 257, (n, ho // 2, wo // 2, cout)).astype(f32) if lateral else None
    if form == BLOCK:
        c.w2 = rng.integers(-aw, aw + 1, (cout, 9, cin)).astype(f32)
        mid = bf16_rne(np.maximum(c.acc * c.scale.astype(f64) + c.bias.astype(f64), 0))
        c.scale2, c.bias2 = epilogue_operands(direct_conv(mid, c.w2))
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            assert np.array_equal(a, np.rint(a)) or a is c.scale or a is getattr(c, "scale2", None)
            a.setflags(write=False)
    for a in (c.x, c.w, c.res, c.up, getattr(c, "w2", None)):
        assert a is None or np.array_equal(bf16_rne(a), a)
    for epi in (BLOCK_EPILOGUES if form == BLOCK else EPILOGUES):
        v, big = c.exact(epi, True)
        assert big < LIMIT, (form, spec, family, epi, big)
        assert np.array_equal(v.astype(f32).astype(f64), v)
        assert (v > 256).any() and is_tie(v.astype(f32)).any(), (form, spec, family, epi, float(v.max()), int(is_tie(v.astype(f32)).sum()))
        assert (v > 0).mean() >= 0.25, (form, spec, family, epi, float((v > 0).mean()))
    return c


# ---- real-valued cases --------------------------------------------------------------------------------------------------------------------------

FLOOR = 2.0 ** -7


def gamma(k):
    """the a-priori relative bound of any f32 summation of k terms (+ the fma of the epilogue and the residual add)"""
    return (k + 2) * 2.0 ** -24


class RealCase:
    """relu(N(0,1)) activations and N(0,1) / sqrt(K) weights, rounded to bf16; scale in [0.5, 1.5], bias N(0, 0.3^2), ReLU.  exact: f64 on the
    rounded operands; ref: exact rounded ONCE to bf16 (the block's intermediate likewise).

    err: per element an a-priori bound on |v - exact| for the f32 value v that ANY correct kernel rounds: gamma(K) (sum |x||w| |scale| + |bias|
    + |residual|).  For the block it also carries what its bf16 intermediate may do: an element of the intermediate whose f64 value lies
    within gamma(K) (sum |x||w1| |s1| + |b1|) of a rounding boundary (or of zero, under ReLU) may come out one step away in a correct kernel,
    and moves every output it feeds by |w2| |s2| times that step; all others are determined.  `assert_close` holds every element to
    |out - exact| <= err + 2^-8 (|exact| + err) - the bound on v plus half a bf16 step at v - and, where |ref| >= 2^10 err (err is below a
    quarter of a step, so v cannot leave the two rounding intervals next to exact's), to the reference or one of its two bf16 neighbours.

    natural=False (the cases of the share bar): forms 0 and 2 take the residual that cancels fma(acc, scale, bias) as far as a bf16 value
    can without going below FLOOR = 2^-7: res = the smallest bf16 value >= FLOOR - value.  The output then lies in [2^-7, 2^-7 + 2^-4)
    (asserted), where one bf16 step of the OUTPUT is 2^-15 .. 2^-11.  The f32 accumulation error of these sums is about 3e-8 (measured on
    the CPU emulation): the smallest step is a thousand times the typical error - near enough to a rounding boundary for hundreds of elements
    in 4e5 to fall on its other side, far enough that a correct kernel never moves an element by two steps: these cases are held to the
    neighbour demand in EVERY element.  (With outputs of order 1, a step of 2^-7, the same emulation differs from the reference in 4e-5 of the
    elements - 16 of the largest case; and where outputs cross zero the smallest have steps below the accumulation error.)
    natural=True: form 0 without a residual, form 2 with a relu(N(0,1)) residual - outputs of order 1 that ReLU clamps in part.
    The block adds x itself and is natural either way."""

    def __init__(self, form, spec, natural=False):
        shape, cin, cout, ks, stride, lateral = spec
        assert not lateral
        n, H, W = shape
        rng = np.random.default_rng(5300 + 7 * cin + 11 * cout + 13 * H + W + 1000 * form + 77 * natural)
        self.form, self.spec, self.stride, self.natural = form, spec, stride, natural or form == BLOCK
        self.x = bf16_rne(np.maximum(rng.standard_normal((n, H, W, cin)), 0))
        g = gamma(ks * ks * cin)

        def conv_operands():
            return (bf16_rne(rng.standard_normal((cout, ks * ks, cin)) / np.sqrt(ks * ks * cin)), (0.5 + rng.random(cout)).astype(f32),
                    (0.3 * rng.standard_normal(cout)).astype(f32))

        self.w, self.scale, self.bias = conv_operands()
        sc, bi = self.scale.astype(f64), self.bias.astype(f64)
        pre = direct_conv(self.x, self.w, stride) * sc + bi
        mag = direct_conv(self.x, np.abs(self.w), stride) * sc + np.abs(bi)
        self.kw = dict(scale=self.scale, bias=self.bias, relu=True, stride=stride)
        if form == BLOCK:
            self.w2, self.scale2, self.bias2 = conv_operands()
            self.kw.update(wgt2=self.w2, scale2=self.scale2, bias2=self.bias2)
            sc2, bi2 = self.scale2.astype(f64), self.bias2.astype(f64)
            m, delta = np.maximum(pre, 0), g * mag
            mid = bf16_from_f64(m).astype(f64)
            up = bf16_step(np.where(mid > 0, mid, 1.0))
            down = np.where(np.frexp(mid)[0] == 0.5, up / 2, up)      # below a power of two the steps are half as long
            room = np.where(m >= mid, up / 2 - (m - mid), down / 2 - (mid - m))
            self.slack = np.where((mid > 0) & (room <= delta), up, 0.0) + np.where(np.abs(pre) <= delta, 2 * delta, 0.0)
            v = direct_conv(mid, self.w2) * sc2 + bi2 + self.x
            self.err = direct_conv(self.slack, np.abs(self.w2)) * sc2 * (1 + g) + g * (direct_conv(mid, np.abs(self.w2)) * sc2 + np.abs(bi2) + self.x)
        else:
            if natural:
                self.res = None if form == C64 else bf16_rne(np.maximum(rng.standard_normal(pre.shape), 0))
            else:
                self.res = bf16_at_least(FLOOR - pre)
            v = pre if self.res is None else pre + self.res
            self.err = g * (mag + (0 if self.res is None else self.res))
            if self.res is not None:
                self.kw.update(residual=self.res)
            assert natural or (v.min() >= FLOOR and v.max() < FLOOR + 2.0 ** -4), (float(v.min()), float(v.max()))
        self.exact = np.maximum(v, 0)
        self.ref = bf16_from_f64(self.exact)
        for a in vars(self).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)

    def run(self, run, **kw):
        out, _, guard = run(self.form, self.x, self.w, guard=_guard_rows(self.x.shape[2]), sentinel=SENTINEL, **self.kw, **kw)
        assert guard.size and (guard == SENTINEL).all(), "the launch wrote behind its output"
        return out

    def share(self, out):
        """the share of elements that differ from the reference"""
        return float((out != self.ref).mean())

    def assert_close(self, out, report=None):
        """-> (largest |out - exact| in units of its bound, elements held to the neighbour demand, the furthest of them in steps)"""
        name = (FORM_NAMES[self.form], self.spec, "natural" if self.natural else "cancelling")
        assert np.isfinite(out).all(), name
        ratio = np.abs(out.astype(f64) - self.exact) / (self.err + 2.0 ** -8 * (self.exact + self.err))
        held = (np.abs(self.ref) >= 2.0 ** 10 * self.err) if self.natural else np.ones(out.shape, bool)
        steps = bf16_steps(out, self.ref)
        furthest = int(steps[held].max()) if held.any() else 0
        if report:
            report(f"B4 {name}: largest |out - exact| {float(ratio.max()):.3f} of its bound; {int(held.sum())} of {out.size} elements held to the neighbour demand, "
                   f"furthest {furthest} steps (anywhere: {int(steps.max())})")
        assert ratio.max() <= 1, (name, int((ratio > 1).sum()), "elements beyond the bound, largest", float(ratio.max()), "at", tuple(int(i) for i in np.argwhere(ratio > 1)[0]))
        assert furthest <= 1, (name, int((steps[held] > 1).sum()), "elements are not the reference or a neighbour; furthest", furthest)
        return float(ratio.max()), int(held.sum()), furthest


@functools.lru_cache(maxsize=None)
def real_case(form, spec, natural=False):
    return RealCase(form, spec, natural)


@functools.lru_cache(maxsize=None)
def real_emulation(form, spec, fault=None, natural=False):
    """the CPU emulation of a case - a sequential f32 chain, the f32 epilogue, one rounding, the block's intermediate in bf16 - or, with
    fault="round_before_residual", the same with the sum rounded to bf16 before the residual is added"""
    out = real_case(form, spec, natural).run(standin, chain=True, fault=fault)
    out.setflags(write=False)
    return out


def real_bar(form, spec):
    """(differing elements of the CPU emulation, their share) of a case"""
    case, emul = real_case(form, spec), real_emulation(form, spec)
    return int((emul != case.ref).sum()), case.share(emul)


# ---- the case lists and the assertions of tests/test_gpu_bf16_trunk_kernels.py, as functions of `run` -----------------------------------------------

def c64_spec(shape):
    return (shape, 64, 64, 3, 1, None)


# at and around the block (8 x 16) and patch edges
C64_SHAPES = ((3, 1, 1), (1, 8, 16), (1, 9, 17), (2, 7, 15), (1, 16, 32), (2, 17, 33), (1, 5, 40), (1, 33, 17))
# conv_igemm: the launches of the bf16 graph at their smallest hazardous sizes.  3x3 s1 runs the tap-sharing loop - 128 -> 128 on 128 x 64 tiles,
# 256 -> 256 and 512 -> 512 on 128 x 128 -; (1, 3, 130) has image rows of BM + 2 pixels; then the stride-2 convs, the laterals (1x1, with the
# top-down sum as second or as only output), 3x3 256 -> 64
IGEMM_SPECS = tuple((shape, c, c, 3, 1, None) for c in (128, 256, 512) for shape in ((1, 1, 1), (3, 5, 3), (2, 9, 17), (1, 3, 130))) + (
    ((2, 18, 22), 64, 128, 3, 2, None), ((2, 18, 22), 64, 128, 1, 2, None), ((2, 6, 10), 128, 256, 1, 1, "both"), ((2, 6, 10), 128, 256, 1, 1, "sum"),
    ((2, 9, 17), 256, 64, 3, 1, None))


def _guard_rows(wo):
    return 2 * wo + 64      # more than two output rows


def run_int(run, case, epi, relu, **kw):
    ho, wo = out_grid(case.shape[1], case.shape[2], {1: 1, 9: 3}[case.w.shape[1]], case.stride)
    out, out2, guard = run(case.form, case.x, case.w, relu=relu, guard=_guard_rows(wo), sentinel=SENTINEL, **case.operands(epi), **kw)
    assert guard.size == (_guard_rows(wo) * case.w.shape[0]) * ((out is not None) + (out2 is not None)) and (guard == SENTINEL).all(), \
        "the launch wrote behind its output"
    return out, out2


def assert_equal(name, got, want):
    for which, g, w in zip(("out", "out2"), got, want):
        assert (g is None) == (w is None), (name, which)
        if g is None:
            continue
        assert np.isfinite(g).all(), (name, which, int((~np.isfinite(g)).sum()), "not finite")
        bad = g != w
        assert not bad.any(), (name, which, int(bad.sum()), "elements differ, first at", tuple(int(i) for i in np.argwhere(bad)[0]),
                               float(g[bad][0]), float(w[bad][0]))


def epilogues(form):
    """(epilogue, relu) of every launch a form can make"""
    return [(e, True) for e in BLOCK_EPILOGUES] if form == BLOCK else [(e, r) for e in EPILOGUES for r in (False, True)]


def check_b1(run, form, spec, family):
    """equality with the reference for every epilogue of the graph, ReLU on and off"""
    case = integer_case(form, spec, family)
    for epi, relu in epilogues(form):
        assert_equal(f"{FORM_NAMES[form]} {spec} {family} {epi} relu {relu}", run_int(run, case, epi, relu), case.reference(epi, relu))


# 60 blocks: num_cus 1, 2, 3 walk them linearly with the next patch in flight; 8 and 16 make the block kernel's grid a multiple of 8 (one
# contiguous run per XCD, 60 = 8 x 7 + 4); 29 leaves a last round of two blocks; 64 clips the block kernel's grid to the block count
B2_SHAPE, B2_CUS = (3, 40, 56), (1, 2, 3, 8, 16, 29, 64)


def check_b2(run, form, cus=B2_CUS):
    """the persistent walk under every grid: equal to the reference on integers, with a residual and without; the same bits on real values"""
    case = integer_case(form, c64_spec(B2_SHAPE), "signed")
    for epi in (BLOCK_EPILOGUES if form == BLOCK else ("residual", "scale_bias")):
        for nc in cus:
            assert_equal(f"{FORM_NAMES[form]} {B2_SHAPE} {epi} num_cus {nc}", run_int(run, case, epi, True, num_cus=nc), case.reference(epi, True))
    real = real_case(form, c64_spec(B2_SHAPE))
    outs = [real.run(run, num_cus=nc) for nc in cus]
    for nc, o in zip(cus[1:], outs[1:]):
        assert np.array_equal(outs[0].view(np.uint32), o.view(np.uint32)), f"num_cus {nc} differs from num_cus {cus[0]}"


B3_SPECS = {C64: tuple(c64_spec(s) for s in ((2, 7, 15), (1, 16, 32), (2, 17, 33))), BLOCK: tuple(c64_spec(s) for s in ((2, 7, 15), (1, 16, 32), (2, 17, 33))),
            IGEMM: (((3, 5, 3), 128, 128, 3, 1, None), ((1, 3, 130), 256, 256, 3, 1, None), ((2, 9, 17), 512, 512, 3, 1, None), ((2, 18, 22), 64, 128, 3, 2, None),
                    ((2, 6, 10), 128, 256, 1, 1, "both"))}


def check_b3_poison(run, form, spec):
    """NaN in front of and behind the source inside its allocation: still equal, no NaN, every guard row untouched (run_int)"""
    case = integer_case(form, spec, "nonneg")
    for epi in (BLOCK_EPILOGUES if form == BLOCK else ("scale_bias", "residual")):
        assert_equal(f"poisoned {FORM_NAMES[form]} {spec} {epi}", run_int(run, case, epi, True, poison=True), case.reference(epi, True))


B3_BATCH_SPECS = {C64: (c64_spec((3, 9, 17)),), BLOCK: (c64_spec((3, 9, 17)),),
                  IGEMM: (((3, 5, 3), 128, 128, 3, 1, None), ((3, 5, 3), 256, 256, 3, 1, None), ((3, 6, 6), 64, 128, 3, 2, None))}


class _Image1NaN:
    """an integer case with image 1 of its batch replaced by NaN"""

    def __init__(self, case):
        self.__dict__.update(vars(case))
        x = case.x.copy()
        x[1] = np.nan
        self.x = x

    operands = IntCase.operands


def check_b3_batch(run, form, spec):
    """image 1 of three is NaN throughout: images 0 and 2 come out as from the clean batch, bit for bit - a pixel of another image has to be
    selected away, not multiplied by zero"""
    case = integer_case(form, spec, "signed")
    epi = "scale_bias" if form == BLOCK else "residual"
    clean = run_int(run, case, epi, True)
    assert_equal(f"{FORM_NAMES[form]} {spec} clean batch", clean, case.reference(epi, True))
    dirty = run_int(run, _Image1NaN(case), epi, True)
    for c, d in zip(clean, dirty):
        if c is not None:
            for i in (0, 2):
                assert np.array_equal(c[i].view(np.uint32), d[i].view(np.uint32)), (FORM_NAMES[form], spec, f"image {i} changed with image 1")


SHARE_FACTOR = 2.0     # the bar over the emulated share: the emulation is no model of the MFMA's internal order (the factor of the rec_fc tests)
# sized so that the emulation differs from the reference in at least 100 elements (tests/test_bf16_conv_oracle.py); the largest is 3 x 40 x 56 x 64
B4_SPECS = {C64: (c64_spec((3, 40, 56)),), BLOCK: (c64_spec((3, 40, 56)),),
            IGEMM: (((2, 20, 30), 128, 128, 3, 1, None), ((2, 16, 20), 256, 256, 3, 1, None), ((2, 9, 17), 512, 512, 3, 1, None),
                    ((3, 40, 56), 64, 128, 3, 2, None), ((2, 20, 28), 128, 256, 1, 1, None), ((2, 24, 40), 256, 64, 3, 1, None))}
MIN_FLIPS, TWICE_FACTOR = 100, 5.0


# natural magnitudes: one small case per form (the block's own case above is natural already)
B4_NATURAL_SPECS = {C64: (c64_spec((2, 17, 33)),), IGEMM: (((2, 9, 17), 256, 256, 3, 1, None), ((2, 18, 22), 64, 128, 3, 2, None))}


def check_b4(run, form, spec, report=print):
    """RealCase.assert_close - every element within its a-priori bound of the f64 value, and the reference or one of its two bf16 neighbours
    (forms 0 and 2: every element; the block: above its floor) - and the share of elements that differ stays under SHARE_FACTOR x the share
    of the CPU emulation.  Returns (emulated share, measured share)."""
    case = real_case(form, spec)
    flips, emulated = real_bar(form, spec)
    out = case.run(run)
    share = case.share(out)
    report(f"B4 {FORM_NAMES[form]} {spec}: emulated {flips} of {out.size} = {emulated:.3e}  bar {SHARE_FACTOR * emulated:.3e}  measured {share:.3e} "
           f"({share / (SHARE_FACTOR * emulated):.2f} of the bar)")
    case.assert_close(out, report)
    assert share <= SHARE_FACTOR * emulated, (FORM_NAMES[form], spec, share, SHARE_FACTOR * emulated)
    return emulated, share


def check_b4_natural(run, form, spec, report=print):
    """outputs of order 1 with ReLU at work (form 0 without a residual): RealCase.assert_close.  No share bar - these sizes show a handful of
    differing elements."""
    case = real_case(form, spec, True)
    return case.assert_close(case.run(run), report)
