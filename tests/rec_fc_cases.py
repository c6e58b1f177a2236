"""References and case builders (numpy, no GPU) for the kernel-level tests of the recogniser's fc1, fc2, softmax and top-1
(tests/test_gpu_rec_fc_kernels.py; rec_net.hip's rec_fc1_ksplit_kernel, rec_fc2_small_kernel, rec_fc2_softmax_kernel and the
large-batch fc1, a conv_igemm GEMM).  tests/test_rec_fc_cases.py checks on the CPU the conditions the GPU tests lean on.

  fc_int_case       small integers: every partial sum is an integer below 2^24, so ANY f32 summation order is exact and the int64
                    product is the one right answer - a wrong row, column or k is an inequality, not a tolerance
  inject_logits     hid / w / bias that make fc2's logits a given f32 array, exactly: the softmax and top-1 tails see chosen logits
  softmax_top1_ref  np.argmax (first index of the maximum) and 1 / sum exp(L - max) in long double
  fc_real_case      hidden-layer-like real operands with the f64 result and the norm sum |a||w| + |b| of every element
  FcCase            a real case with the normalised error measures of tests/split_bf16_emul.py: the rms of a GPU result, of the
                    sequential f32 chain (the bar's yardstick) and of two degraded computations the bar must keep out"""
import numpy as np

from tests import split_bf16_emul as E

f32, f64 = np.float32, np.float64
RMS_FACTOR = 2.0      # the rms bar of an exact-f32 kernel: this many times the rms of a sequential K-long f32 chain on the same operands


def fc_int_case(n, K, N, seed, relu=False):
    """a [n][K] in 0 .. 15, w [N][K] in -3 .. 3, b [N] in -50 .. 50, all integers held in f32, and the int64 result a w^T + b
    (ReLU'd for fc1).  Rows are distinct; the product's spread (about 18 sqrt(K)) dwarfs the bias, so either sign is as likely
    and ReLU clamps about half of the outputs."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 16, (n, K))
    w = rng.integers(-3, 4, (N, K))
    b = rng.integers(-50, 51, N)
    want = a.astype(np.int64) @ w.astype(np.int64).T + b
    if relu:
        want = np.maximum(want, 0)
    return a.astype(f32), w.astype(f32), b.astype(f32), want


def int_case_bound(a, w, b):
    """max over the outputs of sum |a||w| + |b|: below 2^24 every partial sum of every order is an exactly representable integer"""
    return float((np.abs(a).astype(f64) @ np.abs(w).astype(f64).T + np.abs(b)).max())


def inject_logits(L):
    """hid [n][512], w [62][512], bias [62] with fc2(hid) == L bit for bit: w[o][o] = 1 and zero elsewhere, hid[:, :62] = L, bias 0.
    Column o's sum holds the single product L[o] * 1 (exact) among products that are +-0: only the first K quarter contributes,
    and the other partial tiles add exact zeros.  L must be finite."""
    L = np.ascontiguousarray(L, dtype=f32).reshape(-1, 62)
    assert np.isfinite(L).all()
    hid = np.zeros((L.shape[0], 512), f32)
    hid[:, :62] = L
    w = np.zeros((62, 512), f32)
    w[np.arange(62), np.arange(62)] = 1.0
    return hid, w, np.zeros(62, f32)


def softmax_top1_ref(L):
    """(label, p) of f32 logits [n][62]: label = first index of the maximum, p = softmax's value there = 1 / sum exp(L - max),
    summed in long double and returned as f64."""
    L = np.asarray(L, dtype=f32).reshape(-1, 62)
    x = L.astype(np.longdouble)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return np.argmax(L, axis=1).astype(np.int32), (np.longdouble(1) / e.sum(axis=1)).astype(f64)


def fc_real_case(n, K, N, seed):
    """a = max(N(0,1) - 1.5, 0) [n][K] (a ReLU output: mostly zero, one in fifteen is not), w ~ N(0, 1/sqrt(K)) [N][K], b ~ 0.1 N(0,1) [N];
    returns a, w, b, the f64 result a w^T + b (no ReLU) and the norm sum |a||w| + |b| of every element.
    Why the shift: with a = max(N(0,1), 0), half of it non-zero, a three-product split-bf16 computation sits only 5.5 x (K = 1024) and
    7.7 x (K = 512) above twice the f32 chain's rms - an error per product averages out as 1 / sqrt(non-zero terms) of the norm while the
    chain's rounding error, which grows with the partial sums, stays at about 2.8e-8 of it.  At one non-zero term in fifteen the same
    bar has 15 x and 20 x (tests/test_rec_fc_cases.py holds it to 10 x)."""
    rng = np.random.default_rng(seed)
    a = np.maximum(rng.standard_normal((n, K)) - 1.5, 0).astype(f32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(f32)
    b = (0.1 * rng.standard_normal(N)).astype(f32)
    ref = a.astype(f64) @ w.astype(f64).T + b.astype(f64)
    norm = np.abs(a).astype(f64) @ np.abs(w).astype(f64).T + np.abs(b).astype(f64)
    return a, w, b, ref, norm


class FcCase:
    """A real case of fc1 (relu: only the elements whose reference is > 0 count) or fc2, held against f64."""

    def __init__(self, n, K, N, seed, relu):
        self.a, self.w, self.b, self.ref, self.norm = fc_real_case(n, K, N, seed)
        self.K = K
        self.keep = self.ref > 0 if relu else np.ones_like(self.ref, bool)

    def errors(self, out):
        return (np.abs(np.asarray(out, f64) - self.ref) / self.norm)[self.keep]

    def rms(self, out):
        e = self.errors(out)
        return float(np.sqrt(np.mean(e * e)))

    def max_bound(self):
        """the a-priori bound of any f32 summation of K products, a bias and the final rounding, relative to sum |a||w| + |b|"""
        return (self.K + 2) * 2.0 ** -24

    def _with_bias(self, acc):
        return (acc + self.b).astype(f32)

    def chain(self):
        """one sequential K-long chain of f32 fused multiply-adds, then + bias in f32"""
        return self._with_bias(E.f32_chain(self.a, np.ascontiguousarray(self.w.T)))

    def bar(self):
        return RMS_FACTOR * self.rms(self.chain())

    def bf16_activation(self):
        """what a kernel that rounded its activations to bf16 would give (everything else in f64)"""
        return E.bf16_round(self.a).astype(f64) @ self.w.astype(f64).T + self.b.astype(f64)

    def three_products(self):
        """a split-bf16 kernel with only mid.hi, hi.mid and hi.hi"""
        return self._with_bias(E.emulate(self.a, np.ascontiguousarray(self.w.T), products=E.PRODUCTS[3:]))


# (name, n, K, N, seed, relu): fc1 on one 16-row tile family (48: three tiles of the small kernel) and across conv_igemm's row tiles (130), fc2 alike
REAL_CASES = (("fc1 n=48", 48, 1024, 512, 21, True), ("fc1 n=130", 130, 1024, 512, 22, True),
              ("fc2 n=48", 48, 512, 62, 23, False), ("fc2 n=130", 130, 512, 62, 24, False))
_REAL = {}


def real_case(name):
    """the cases are built once and shared, unchanged, by every test that needs them"""
    if name not in _REAL:
        _REAL[name] = FcCase(*next(c[1:] for c in REAL_CASES if c[0] == name))
    return _REAL[name]
