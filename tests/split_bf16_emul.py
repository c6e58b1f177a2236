"""CPU emulation (numpy / torch-CPU, no GPU) of the split-bf16 arithmetic of the f32 engine's default kernels, as a statistical
yardstick: how large is the error of six partial products against f64, and how large does it get when one of them is lost?

A split-bf16 kernel writes every f32 operand as hi + mid + lo (three bf16 terms, round to nearest even at every level, exact)
and accumulates lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi - small terms first - in f32, one MFMA per product and K group.
`emulate` does the same with each product of a K group summed in f64 and added to an f32 accumulator.  This is NOT a bit-exact
model of the MFMA's internal order; it gives the error LEVEL (rms over many outputs, normalised by sum |a||b|), which separates
six products from five by a factor of 8 - 30 while the accumulation order moves it by a small factor only.

Per kernel a *Case class im2cols the operands, runs the kernel's epilogue in f32 the way the kernel does, and measures any
output of the same layout (an emulation's or the GPU's) against the same pipeline in f64:
  rms(out) = sqrt(mean(((out - ref) / norm)^2)),  norm = sum |a||b| * |scale| carried through the epilogue.
`bar(case)` = (rms of six products, smallest rms of five among the drops that change anything, their geometric mean).
The *_family functions are the inputs of tests/test_gpu_stem_head_kernels.py, tests/test_gpu_phase_kernels.py and
tests/test_gpu_igemm_kernels.py;
tests/test_split_bf16_emul.py and tests/test_phase_conv_oracle.py check on the CPU
that each of them separates five products from six by at least 5 x."""
import numpy as np
import torch

# (plane of A, plane of B) with 0 = hi, 1 = mid, 2 = lo, in the kernels' order
PRODUCTS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
PRODUCT_NAMES = ("lo.hi", "hi.lo", "mid.mid", "mid.hi", "hi.mid", "hi.hi")
f32, f64 = np.float32, np.float64


def bf16_round(a):
    """f32 -> nearest-even bf16, widened back to f32."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(torch.bfloat16).to(torch.float32).numpy()


def split3(a):
    """hi, mid, lo (bf16 values held in f32) with hi + mid + lo == a exactly: the remainders are exact in f32."""
    a = np.ascontiguousarray(a, dtype=f32)
    hi = bf16_round(a)
    r = (a - hi).astype(f32)
    mid = bf16_round(r)
    lo = bf16_round((r - mid).astype(f32))
    return hi, mid, lo


def emulate(A, B, products=PRODUCTS, kgroup=16):
    """A [M][K] x B [K][N] (f32) -> f32 [M][N]: per K group the chosen products in order, each summed in f64 and added to the f32 accumulator."""
    a, b = [p.astype(f64) for p in split3(A)], [p.astype(f64) for p in split3(B)]
    acc = np.zeros((A.shape[0], B.shape[1]), f32)
    for k0 in range(0, A.shape[1], kgroup):
        for i, j in products:
            acc = (acc.astype(f64) + a[i][:, k0:k0 + kgroup] @ b[j][k0:k0 + kgroup]).astype(f32)
    return acc


def f32_chain(A, B):
    """The exact-f32 kernels: one fused multiply-add per k, sequentially (a f64 product of two f32 is exact; the sum is rounded to f32)."""
    A64, B64 = A.astype(f64), B.astype(f64)
    acc = np.zeros((A.shape[0], B.shape[1]), f32)
    for k in range(A.shape[1]):
        acc = (acc.astype(f64) + A64[:, k:k + 1] * B64[k:k + 1]).astype(f32)
    return acc


def _fma32(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


class _Case:
    """A [M][K], B [K][N], kgroup; subclasses give epilogue(acc, dtype) -> output and norm / keep."""
    keep = None

    def rms(self, out):
        e = (np.asarray(out, f64) - self.ref) / self.norm
        if self.keep is not None:
            e = e[self.keep]
        return float(np.sqrt(np.mean(e * e)))

    def emulated(self, products=PRODUCTS):
        return self.epilogue(emulate(self.A, self.B, products, self.kgroup), f32)

    def chain(self):
        return self.epilogue(f32_chain(self.A, self.B), f32)

    def _finish(self):
        self.ref = self.epilogue(self.A.astype(f64) @ self.B.astype(f64), f64)
        self.mag = np.abs(self.A).astype(f64) @ np.abs(self.B).astype(f64)


def bar(case):
    """(six-product rms, smallest five-product rms among the drops whose emulation differs from the six-product one, sqrt of their
    product, names of the drops that qualified)."""
    full = case.emulated()
    six = case.rms(full)
    fives, names = [], []
    for d in range(6):
        out = case.emulated(tuple(p for q, p in enumerate(PRODUCTS) if q != d))
        if not np.array_equal(out, full):
            fives.append(case.rms(out))
            names.append(PRODUCT_NAMES[d])
    five = min(fives)
    return six, five, float(np.sqrt(six * five)), names


def pool3x3s2(c):
    """max pool 3x3 stride 2 pad 1 of [n][H][W][C] with ZERO padding (the stem pools ReLU outputs from a zero initial value)."""
    n, H, W, ch = c.shape
    p = np.zeros((n, H + 2, W + 2, ch), c.dtype)
    p[:, 1:-1, 1:-1] = c
    out = np.zeros((n, H // 2, W // 2, ch), c.dtype)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, p[:, dy:dy + H - 1:2, dx:dx + W - 1:2])
    return out


class StemCase(_Case):
    """stem_tail.hip: conv 7x7 s2 p3 (1 -> 64) as K = 8 kh + kw over an 8 x 8 window (row / column 7: zero weight), one MFMA step
    = two window rows = 16 k; acc * scale + bias (one fused multiply-add), ReLU, max pool 3x3 s2 p1.  Output [n][h/4][w/4][64]."""
    kgroup = 16

    def __init__(self, frames, w64x49, scale, bias):
        x = np.asarray(frames).astype(f32)
        n, h, w = x.shape
        self.shape = (n, h // 2, w // 2, 64)
        xp = np.zeros((n, h + 8, w + 8), f32)
        xp[:, 3:3 + h, 3:3 + w] = x
        A = np.zeros((n, h // 2, w // 2, 8, 8), f32)
        for kh in range(7):
            for kw in range(7):
                A[..., kh, kw] = xp[:, kh:kh + h:2, kw:kw + w:2]
        self.A = A.reshape(-1, 64)
        B = np.zeros((8, 8, 64), f32)
        B[:7, :7] = np.asarray(w64x49, f32).reshape(64, 7, 7).transpose(1, 2, 0)
        self.B = B.reshape(64, 64)
        self.scale, self.bias = np.asarray(scale, f32), np.asarray(bias, f32)
        self._finish()
        self.norm = pool3x3s2((self.mag * np.abs(self.scale).astype(f64)).reshape(self.shape))

    def epilogue(self, acc, dt):
        if dt == f32:
            v = _fma32(acc, self.scale, self.bias)
        else:
            v = acc * self.scale.astype(f64) + self.bias.astype(f64)
        return pool3x3s2(np.maximum(v, 0).astype(dt).reshape(self.shape))


def head_place(v):
    """[n][h4][w4][4 taps a*2+b][4 u = c'*2+d'] -> [n][4 h4][4 w4] with element (a, b, c', d') of pixel (i, j) at row 4i + 2a + c', column 4j + 2b + d'."""
    n, h4, w4 = v.shape[:3]
    v = v.reshape(n, h4, w4, 2, 2, 2, 2)            # n i j a b c' d'
    return np.ascontiguousarray(v.transpose(0, 1, 3, 5, 2, 4, 6)).reshape(n, 4 * h4, 4 * w4)   # n i a c' j b d'


class HeadCase(_Case):
    """tail_fused.hip: four taps of convT 2x2 s2 64 -> 64 as one [M][64] x [64][256] product (K groups of 16), fmax(acc * s4 + b4, 0),
    the 64-long f32 contraction with w2t (a lane's 32 channels as one fused multiply-add chain, the two halves added, + bias2),
    f32 sigmoid.  Output [n][4 h4][4 w4]; elements whose reference |logit| >= 4 are left out (keep), the rest are divided by p (1 - p)."""
    kgroup = 16

    def __init__(self, y, wt1, s4, b4, w2t, bias2):
        y = np.asarray(y, f32)
        self.nhw = y.shape[:3]
        self.A = y.reshape(-1, 64)
        self.B = np.ascontiguousarray(np.asarray(wt1, f32).reshape(256, 64).T)       # column = tap * 64 + co
        self.s4, self.b4 = np.asarray(s4, f32).reshape(256), np.asarray(b4, f32).reshape(256)
        self.w2t, self.bias2 = np.asarray(w2t, f32).reshape(64, 4), f32(bias2)
        self._logits = None
        self._finish()
        lg = self._logits
        magt = np.einsum("mtc,cu->mtu", (self.mag * np.abs(self.s4).astype(f64)).reshape(-1, 4, 64), np.abs(self.w2t).astype(f64))
        self.keep = head_place((np.abs(lg) < 4).reshape(self.nhw + (4, 4)))
        self.norm = head_place(magt.reshape(self.nhw + (4, 4))) * self.ref * (1 - self.ref)
        self.left_out = 1.0 - float(self.keep.mean())

    def epilogue(self, acc, dt):
        m = acc.shape[0]
        if dt == f64:
            z = np.maximum(acc * self.s4.astype(f64) + self.b4.astype(f64), 0).reshape(m, 4, 64)
            lg = np.einsum("mtc,cu->mtu", z, self.w2t.astype(f64)) + f64(self.bias2)
            self._logits = lg
            p = 1.0 / (1.0 + np.exp(-lg))
        else:
            z = np.maximum(_fma32(acc, self.s4, self.b4), f32(0)).reshape(m, 4, 64)
            part = np.zeros((2, m, 4, 4), f32)
            for half in range(2):
                for ct in range(2):
                    for e in range(16):
                        co = 32 * ct + (e & 3) + 8 * (e >> 2) + 4 * half
                        part[half] = _fma32(z[:, :, co, None], self.w2t[co], part[half])
            sm = ((part[0] + part[1]).astype(f32) + self.bias2).astype(f32)
            p = (f32(1) / (f32(1) + np.exp(-sm).astype(f32)).astype(f32)).astype(f32)
        return head_place(p.reshape(self.nhw + (4, 4)))


def rec_pooled_onehot(crops, tap, gain, b1):
    """The recogniser's pooled conv1 map [n][12][12][32] when channel c of conv1 has the single weight gain[c] (a power of two) at
    tap[c] = 5 ky + kx: gain * (2x2 max of the shifted crop) + b1, one f32 rounding (the add) whatever the kernel's order - the
    operand of conv2 is then known exactly on the host.  Also returns conv1's weights [32][25]."""
    x = np.asarray(crops, f32).reshape(-1, 28, 28)
    w1 = np.zeros((32, 25), f32)
    p1 = np.zeros((x.shape[0], 12, 12, 32), f32)
    for c in range(32):
        w1[c, tap[c]] = gain[c]
        ky, kx = divmod(int(tap[c]), 5)
        s = (x[:, ky:ky + 24, kx:kx + 24] * f32(gain[c])).astype(f32)
        p1[..., c] = s.reshape(-1, 12, 2, 12, 2).max(axis=(2, 4))
    return (p1 + np.asarray(b1, f32)).astype(f32), w1


class RecCase(_Case):
    """rec_net.hip's conv2 (valid 5x5, 32 -> 64) over the pooled map p1 [n][12][12][32]: K = tap * 32 + ci, one K group per tap
    (the small-batch kernel's 16x16x32 MFMA); 2x2 max of the accumulators, + bias.  Output [n][1024] as co * 16 + 4 py + px."""
    kgroup = 32

    def __init__(self, p1, w2, b2):
        p1 = np.asarray(p1, f32)
        self.n = p1.shape[0]
        A = np.zeros((self.n, 8, 8, 25, 32), f32)
        for t in range(25):
            ky, kx = divmod(t, 5)
            A[:, :, :, t] = p1[:, ky:ky + 8, kx:kx + 8]
        self.A = A.reshape(-1, 800)
        self.B = np.ascontiguousarray(np.asarray(w2, f32).reshape(64, 32, 25).transpose(2, 1, 0)).reshape(800, 64)
        self.b2 = np.asarray(b2, f32)
        self._finish()
        self.norm = self._pool(self.mag)

    def _pool(self, a):
        return a.reshape(self.n, 4, 2, 4, 2, 64).max(axis=(2, 4)).transpose(0, 3, 1, 2).reshape(self.n, 1024)

    def epilogue(self, acc, dt):
        return (self._pool(acc.astype(dt)) + np.repeat(self.b2.astype(dt), 16)[None, :]).astype(dt)


class ConvCase(_Case):
    """conv_igemm's plain conv (debug_conv_run(variant=2), debug_igemm_run) without epilogue terms: x NHWC, wg [cout][ks*ks][cin],
    K = tap * cin + ci in groups of `kgroup` - 16, one MFMA, or 32, the kernel's K-step.  Output [n][ho][wo][cout].  x [B][n][h][w][cin]
    with wg [B][cout][1][cin] is the batched GEMM: B products, each emulated on its own, output [B][n][h][w][cout]."""

    def __init__(self, x, wg, stride, kgroup=16):
        x, wg = np.asarray(x, f32), np.asarray(wg, f32)
        self.kgroup = kgroup
        self.batched = x.ndim == 5
        self.blocks = [self._im2col(xb, wb, stride) for xb, wb in (zip(x, wg) if self.batched else ((x, wg),))]
        self.A, self.B = self.blocks[0]
        self.ref = self._place([A.astype(f64) @ B.astype(f64) for A, B in self.blocks], f64)
        self.mag = self._place([np.abs(A).astype(f64) @ np.abs(B).astype(f64) for A, B in self.blocks], f64)
        self.norm = self.mag

    def _im2col(self, x, wg, stride):
        n, h, w, cin = x.shape
        cout, kk, _ = wg.shape
        ks = int(round(kk ** 0.5))
        pad = (ks - 1) // 2
        ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
        xp = np.zeros((n, h + 2 * pad, w + 2 * pad, cin), f32)
        xp[:, pad:pad + h, pad:pad + w] = x
        A = np.zeros((n, ho, wo, kk, cin), f32)
        for t in range(kk):
            ky, kx = divmod(t, ks)
            A[:, :, :, t] = xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
        self.shape = (n, ho, wo, cout)
        return A.reshape(-1, kk * cin), np.ascontiguousarray(wg.reshape(cout, kk * cin).T)

    def _place(self, per_block, dt):
        out = np.stack([np.asarray(v, dt).reshape(self.shape) for v in per_block])
        return out if self.batched else out[0]

    def emulated(self, products=PRODUCTS):
        return self._place([emulate(A, B, products, self.kgroup) for A, B in self.blocks], f32)

    def chain(self):
        return self._place([f32_chain(A, B) for A, B in self.blocks], f32)


class _PhasedCase(_Case):
    """A launch that is one GEMM per output phase (conv_igemm's STORE_PHASE forms): blocks of (A [cells][K], B [K][cout], a, b) with the
    result of block (a, b) at out[:, a::up, b::up]; K differs between the phases, so every block is emulated on its own.  No epilogue terms."""
    kgroup = 16

    def _place(self, per_block, dt):
        n, h, w, cout = self.grid
        out = np.zeros((n, self.up * h, self.up * w, cout), dt)
        for (A, B, a, b), v in zip(self.blocks, per_block):
            out[:, a::self.up, b::self.up] = np.asarray(v, dt).reshape(n, h, w, cout)
        return out

    def emulated(self, products=PRODUCTS):
        return self._place([emulate(A, B, products, self.kgroup) for A, B, a, b in self.blocks], f32)

    def chain(self):
        return self._place([f32_chain(A, B) for A, B, a, b in self.blocks], f32)

    def _finish(self):
        self.ref = self._place([A.astype(f64) @ B.astype(f64) for A, B, a, b in self.blocks], f64)
        self.norm = self._place([np.abs(A).astype(f64) @ np.abs(B).astype(f64) for A, B, a, b in self.blocks], f64)


class PhaseCase(_PhasedCase):
    """conv_igemm STORE_PHASE / SRC_PLAIN (debug_phase_conv_run, win 0 or 1: the same products in the same order): x [n][h][w][cin],
    wphase [up*up][cout][2x2][cin] as built; per phase K = tap * cin + c over its active taps, in groups of 16.  Output [n][up h][up w][cout]."""

    def __init__(self, x, wphase, up):
        from tests import phase_conv_oracle as O
        x, wp = np.asarray(x, f32), np.asarray(wphase, f32)
        n, h, w, cin = x.shape
        cout = wp.shape[1]
        self.up, self.grid = up, (n, h, w, cout)
        self.blocks = []
        for a, b, A in O.phase_operands(x, up):
            nt = A.shape[1] // cin
            self.blocks.append((A.astype(f32), np.ascontiguousarray(wp[a * up + b, :, :nt].reshape(cout, nt * cin).T), a, b))
        self._finish()


class PyrCase(_PhasedCase):
    """conv_igemm SRC_PYR4 (debug_pyr4_conv_run; one launch or the phase blocks and the corner launch: the same products in the same
    order): levels (p5, p4, p3[, p2]), wpyr [64][64][21][64] as built; per phase K ordered (source, tap, channel) over the active slots, in
    groups of 16.  Output [n][8 h][8 w][64]."""

    def __init__(self, levels, wpyr, nsrc=3):
        from tests import phase_conv_oracle as O
        lv = [None if a is None else np.asarray(a, f32) for a in levels]
        wp = np.asarray(wpyr, f32)
        n, h, w, _ = lv[0].shape
        self.up, self.grid = 8, (n, h, w, 64)
        self.blocks = [(A.astype(f32), np.ascontiguousarray(wp[8 * a + b][:, slots].reshape(64, -1).T), a, b) for a, b, slots, A in O.pyr4_operands(lv, nsrc)]
        self._finish()


# ---- the input families of tests/test_gpu_stem_head_kernels.py -------------------------------------------------------------

STEM_FAMILIES = ("fraction", "luma_f32", "luma_u8")


def stem_weights(seed):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((64, 49)) / 7).astype(f32)
    scale = ((0.5 + rng.random(64)) * rng.choice([-1.0, 1.0], 64)).astype(f32)
    bias = (20 * rng.standard_normal(64)).astype(f32)
    return w, scale, bias


def stem_family(kind, n=2, h=96, w=128, seed=11):
    """frames of raw luma: with a fraction added to every pixel (all three bf16 terms in use), integers in f32 (the kernel decides per
    tile that mid and lo are zero), integers in u8 (statically so)."""
    rng = np.random.default_rng(seed)
    luma = rng.integers(0, 256, (n, h, w))
    if kind == "fraction":
        return (luma + rng.random((n, h, w))).astype(f32)
    return luma.astype(np.uint8 if kind == "luma_u8" else f32)


def head_family(n, h4, w4, seed=5):
    """y = relu(N(0,1)), wt1 ~ N(0,1)/8, s4 in +-[0.5, 1.5], b4 ~ 0.5 N(0,1), w2t ~ 0.25 N(0,1): logits of a spread at which the sigmoid
    neither saturates (|logit| < 4 nearly everywhere) nor hides the accumulator's error."""
    rng = np.random.default_rng(seed)
    y = np.maximum(rng.standard_normal((n, h4, w4, 64)), 0).astype(f32)
    wt1 = (rng.standard_normal((4, 64, 64)) / 8).astype(f32)
    s4 = ((0.5 + rng.random(256)) * rng.choice([-1.0, 1.0], 256)).astype(f32)
    b4 = (0.5 * rng.standard_normal(256)).astype(f32)
    w2t = (0.25 * rng.standard_normal((64, 4))).astype(f32)
    return y, wt1, s4, b4, w2t, f32(0.1)


def rec_family(n, seed=7):
    """crops ~ |N(0,1)| with one-hot conv1 weights (gain 1 or 2, tap c mod 25) so that conv2's operand is exact on the host (rec_pooled_onehot)
    and carries full 24-bit significands; conv2 ~ N(0,1)/28.  Returns crops, w1, b1, w2, b2, p1."""
    rng = np.random.default_rng(seed)
    crops = np.abs(rng.standard_normal((n, 784))).astype(f32)
    tap = np.arange(32) % 25
    gain = np.where(np.arange(32) % 3 == 0, 2.0, 1.0).astype(f32)
    b1 = (0.25 * rng.standard_normal(32)).astype(f32)
    p1, w1 = rec_pooled_onehot(crops, tap, gain, b1)
    w2 = (rng.standard_normal((64, 32, 25)) / 28).astype(f32)
    b2 = (0.5 * rng.standard_normal(64)).astype(f32)
    return crops, w1, b1, w2, b2, p1


CONV_CASES = ((2, 18, 22, 64, 128, 3, 2), (1, 9, 7, 256, 64, 3, 1))   # K = 576 and K = 2304


def conv_family(case, seed=3):
    n, h, w, cin, cout, ks, stride = case
    rng = np.random.default_rng(seed + cin)
    x = rng.standard_normal((n, h, w, cin)).astype(f32)
    wg = (rng.standard_normal((cout, ks * ks, cin)) / np.sqrt(ks * ks * cin)).astype(f32)
    return x, wg, stride


# (n, h, w, cin, cout, ks, stride, batch): one per (ks, stride), the batched GEMM; K = 32, 64, 576 and 2304
IGEMM_CASES = ((2, 9, 7, 32, 64, 1, 1, 1), (2, 10, 18, 64, 128, 1, 2, 1), (1, 9, 17, 64, 128, 3, 1, 1), (2, 10, 18, 64, 64, 3, 2, 1),
               (1, 9, 7, 256, 64, 3, 1, 1), (1, 1, 130, 64, 64, 1, 1, 3))


def igemm_family(case, seed=29):
    """the inputs of tests/test_gpu_igemm_kernels.py (group G5): case = (n, h, w, cin, cout, ks, stride, batch); N(0,1) activations, weights
    N(0,1) / sqrt(K); batch > 1: the batched GEMM's x [B][n][h][w][cin], wg [B][cout][1][cin]"""
    n, h, w, cin, cout, ks, stride, batch = case
    rng = np.random.default_rng(seed + cin + 7 * ks + stride)
    lead = (batch,) if batch > 1 else ()
    x = rng.standard_normal(lead + (n, h, w, cin)).astype(f32)
    wg = (rng.standard_normal(lead + (cout, ks * ks, cin)) / np.sqrt(ks * ks * cin)).astype(f32)
    return x, wg, stride


# ---- ... and of tests/test_gpu_phase_kernels.py (group K5): N(0,1) activations, taps N(0,1) / sqrt(9 cin) merged by the engine's builders
# (`build` = capi.phase_weights / capi.pyr4_weights, passed in so that this module stays free of the library)

PHASE_CASES = ((2, 6, 10, 128, 64, 2), (2, 6, 10, 256, 64, 2))   # n, h, w, cin, cout, up: K = 512 and 1024 per phase
PYR_CASES = ((2, 3, 5, 3),)                                     # n, h, w, nsrc: K = 192 .. 768 per phase


def phase_family(case, build, seed=21):
    n, h, w, cin, cout, up = case
    rng = np.random.default_rng(seed + cin)
    x = rng.standard_normal((n, h, w, cin)).astype(f32)
    t = rng.standard_normal((cout, 9, cin)) / np.sqrt(9 * cin)
    return x, build(t, up), up


def pyr_family(case, build, seed=23):
    n, h, w, nsrc = case
    rng = np.random.default_rng(seed)
    levels = [rng.standard_normal((n, h << i, w << i, 64)).astype(f32) for i in range(4)]
    wg = (rng.standard_normal((64, 9, 256)) / np.sqrt(9 * 256)).astype(f32)
    scale = (0.5 + rng.random(64)).astype(f32)
    return levels, build(wg, scale), nsrc
