"""CPU oracle (numpy / torch-CPU in f64, no GPU) of the low-resolution forms of "3x3 conv of a nearest-upsampled tensor" that the
detector's composed FPN runs: conv_igemm's STORE_PHASE (up 2, 4, 8) and SRC_PYR4 launches and their weight builders in engine.hip.

Two independent descriptions of the same operation:

  *_ref   the DEFINITION: nearest upsample by `up`, then a 3x3 pad-1 conv with the original taps [cout][9][cin]
          (pyr4_ref: the same over the concat [up8(p5), up4(p4), up2(p3), p2] with bin_conv1's OHWI weights and bin_bn1's scale);
  *_eval  the low-res evaluation from the BUILT f32 weights, by the layout the comments in common.hpp and engine.hip state:
          phase (a, b) = (row, column) mod up of the output pixel; its 2 x 2 window of the low-res grid starts at row i - 1 for a = 0
          and at row i otherwise (columns alike); a phase on the rim of a cell (a = 0 or up - 1) has two taps in that direction, the
          others one; the active taps are the prefix t = th * nw + tw (nw = taps per window row of this phase) of the four tap slots.
          PYR4: slots 4 s + t for the upsampled sources s = 0 (p5, up 8), 1 (p4, up 4), 2 (p3, up 2), slots 12 + 3 dy + dx for p2.

tests/test_phase_conv_oracle.py holds the two against each other (what the builders must satisfy); tests/test_gpu_phase_kernels.py
holds the kernels to *_eval of their own operands, so the rounding of the merged weights to f32 is no part of a kernel's tolerance.

Everything is NHWC.  *_operands yield, per phase, the GEMM the kernel runs for it - A [low-res cells][K] and the tap slots K walks, K
ordered (source, tap, channel) - which tests/split_bf16_emul.py's PhaseCase / PyrCase emulate group by group."""
import numpy as np
import torch
import torch.nn.functional as F

f64 = np.float64


def _conv3x3(x, taps):
    """x [n][H][W][cin], taps [cout][9][cin] -> [n][H][W][cout], 3x3 pad 1, f64."""
    cout, _, cin = taps.shape
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=f64)).permute(0, 3, 1, 2)
    wt = torch.from_numpy(np.ascontiguousarray(taps, dtype=f64)).reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    return F.conv2d(xt, wt, None, 1, 1).permute(0, 2, 3, 1).contiguous().numpy()


def upsample(x, up):
    return np.repeat(np.repeat(np.asarray(x), up, axis=1), up, axis=2)


def upsampled_conv_ref(x, taps, up):
    """The definition: nearest upsample of x [n][h][w][cin] by `up`, then the 3x3 pad-1 conv with taps [cout][9][cin] -> [n][up h][up w][cout]."""
    return _conv3x3(upsample(np.asarray(x, f64), up), np.asarray(taps, f64))


def pyr4_ref(levels, w_ohwi, scale):
    """bin_conv1 (w_ohwi [64][9][256], input channels p5 | p4 | p3 | p2) times bin_bn1's scale [64] over cat[up8(p5), up4(p4), up2(p3), p2]."""
    cat = np.concatenate([upsample(np.asarray(a, f64), 8 >> i) for i, a in enumerate(levels)], axis=3)
    return _conv3x3(cat, np.asarray(w_ohwi, f64) * np.asarray(scale, f64)[:, None, None])


def taps_of(a, up):
    """taps a phase has along one direction"""
    return 2 if a in (0, up - 1) else 1


def _padded(x):
    x = np.asarray(x, f64)
    n, h, w, c = x.shape
    p = np.zeros((n, h + 2, w + 2, c), f64)
    p[:, 1:-1, 1:-1] = x
    return p


def _window_rows(xp, a, up, h, step, first, fault=None):
    """Per tap th the row slice of the zero-padded level xp that phase `a` of the cells first, first + step, ... (h of them) reads:
    the window starts at row r - 1 for a = 0 and at r otherwise (index r, r + 1 of the padded tensor)."""
    start = first + (0 if a == 0 and fault != "window0" else 1)
    return [slice(start + th, start + th + step * (h - 1) + 1, step) for th in range(taps_of(a, up))]


def phase_operands(x, up, fault=None):
    """Per phase (a, b): A [n h w][nt * cin] with K = t * cin + c over the nt active taps t = th * nw + tw."""
    xp = _padded(x)
    n, h, w, cin = np.asarray(x).shape
    for a in range(up):
        rows = _window_rows(xp, a, up, h, 1, 0, fault)
        for b in range(up):
            cols = _window_rows(xp, b, up, w, 1, 0, fault)
            A = np.concatenate([xp[:, r, c].reshape(n * h * w, cin) for r in rows for c in cols], axis=1)
            yield a, b, A


def phase_eval(x, wphase, up, fault=None):
    """x [n][h][w][cin], wphase [up*up][cout][2x2][cin] (the built f32 weights, or their absolute values for sum |a||b|) ->
    [n][up h][up w][cout] in f64.  fault = "window0" evaluates a wrong layout on purpose (phase 0's window started at i): what
    tests/test_phase_conv_oracle.py uses to show that the comparison rejects it."""
    w = np.asarray(wphase, f64)
    n, h, wd, cin = np.asarray(x).shape
    cout = w.shape[1]
    assert w.shape == (up * up, cout, 4, cin), w.shape
    out = np.zeros((n, up * h, up * wd, cout), f64)
    for a, b, A in phase_operands(x, up, fault):
        nt = A.shape[1] // cin
        out[:, a::up, b::up] = (A @ w[a * up + b, :, :nt].reshape(cout, nt * cin).T).reshape(n, h, wd, cout)
    return out


def pyr4_operands(levels, nsrc=4):
    """Per phase (a, b) of the 8 x 8 phases of a p5 cell: (a, b, slots, A [n h w][len(slots) * 64]) with K ordered (source, tap, channel)."""
    n, h, w, _ = np.asarray(levels[0]).shape
    xp = [_padded(a) if a is not None and i < nsrc else None for i, a in enumerate(levels)]
    for a in range(8):
        for b in range(8):
            slots, parts = [], []
            for s in range(3):
                up = 8 >> s
                rows = _window_rows(xp[s], a & (up - 1), up, h, 1 << s, a >> (3 - s))
                cols = _window_rows(xp[s], b & (up - 1), up, w, 1 << s, b >> (3 - s))
                for t, (r, c) in enumerate((r, c) for r in rows for c in cols):
                    slots.append(4 * s + t)
                    parts.append(xp[s][:, r, c].reshape(n * h * w, 64))
            if nsrc == 4:
                for dy in range(3):
                    for dx in range(3):
                        slots.append(12 + 3 * dy + dx)
                        parts.append(xp[3][:, a + dy:a + dy + 8 * (h - 1) + 1:8, b + dx:b + dx + 8 * (w - 1) + 1:8].reshape(n * h * w, 64))
            yield a, b, slots, np.concatenate(parts, axis=1)


def pyr4_eval(levels, wpyr, nsrc=4):
    """levels (p5, p4, p3, p2) as [n][h << i][w << i][64], wpyr [64 phases][64][21 slots][64] (built f32 weights) -> [n][8h][8w][64] in f64;
    nsrc = 3 leaves p2's term out (the kernel then never touches p2 or slots 12 - 20)."""
    w = np.asarray(wpyr, f64)
    assert w.shape == (64, 64, 21, 64), w.shape
    n, h, wd, _ = np.asarray(levels[0]).shape
    out = np.zeros((n, 8 * h, 8 * wd, 64), f64)
    for a, b, slots, A in pyr4_operands(levels, nsrc):
        out[:, a::8, b::8] = (A @ w[8 * a + b][:, slots].reshape(64, -1).T).reshape(n, h, wd, 64)
    return out


def epilogue(acc, bias=None, residual=None, relu=False):
    """the kernels' epilogue in f64: + bias per channel, + residual, ReLU"""
    v = np.asarray(acc, f64)
    if bias is not None:
        v = v + np.asarray(bias, f64)
    if residual is not None:
        v = v + np.asarray(residual, f64)
    return np.maximum(v, 0) if relu else v


def magnitude(mag, bias=None, residual=None):
    """sum |a||b| + |bias| + |residual|: what f32 rounding of the sum works on"""
    v = np.asarray(mag, f64)
    if bias is not None:
        v = v + np.abs(np.asarray(bias, f64))
    if residual is not None:
        v = v + np.abs(np.asarray(residual, f64))
    return v


# ---- inputs shared by the CPU and GPU tests ------------------------------------------------------------------------------------

IMAGE_SCALES = (1.0, 16.0, 1.0 / 16.0)


def activations(rng, n, h, w, c):
    """N(0,1), the images of a batch scaled 1, 16, 1/16 in turn: a read across an image border or a store into the neighbour's rows
    is not lost in a tolerance that follows the values"""
    x = rng.standard_normal((n, h, w, c))
    for i in range(n):
        x[i] *= IMAGE_SCALES[i % 3]
    return x.astype(np.float32)


def taps(rng, cout, cin):
    return rng.standard_normal((cout, 9, cin)) / np.sqrt(9 * cin)
