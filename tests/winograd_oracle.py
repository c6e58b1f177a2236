"""The 3x3 s1 p1 conv (+ scale, bias, residual, ReLU) of the detector's trunk as the Winograd kernels compute it, stated without a GPU:

  * twice in f64 - by definition (`direct_conv`, `epilogue`) and by the documented matrices (`by_matrices`: B^T d B, G g G^T, the (m+2)^2
    element-wise products, A^T M A) for F(4x4,3x3) and F(2x2,3x3);
  * integer families (`integer_case`) on which every value of the F(4x4) pipeline is an integer below 2^24, so that a kernel must EQUAL the
    direct conv whatever its summation order: activations are small integers, weights integer multiples of 576 (24 G is integral), scales
    powers of two, bias and residual integers;
  * `WinoCase`, the rms yardstick of docs/split_bf16_error.md for the real-valued families, normalised per element by the Winograd-domain
    |A^T| (sum_c |V||U|) |A| |scale| (rounding acts on V and U, not on x and w);
  * `standin`, a numpy model with the signature of Detector.debug_winograd_run that follows the kernels' order of operations in f32 - V by
    the kernels' bt6, the GEMMs as six split-bf16 products or as an f32 chain, the output by the kernels' at6, v * sc + bi + res - and, on
    request, commits one of the `FAULTS` a kernel of this family could commit;
  * the assertions of tests/test_gpu_winograd_kernels.py (`check_w1` .. `check_w4`) as functions of a `run` callable, so that
    tests/test_winograd_oracle.py can show that the model passes every one of them and that every fault fails at least one.

`run(form, x, wgt, scale=, bias=, residual=, relu=, inplace=, num_cus=, guard=, poison=, sentinel=) -> (out, guard rows)`; forms: 0 the
fused F(4x4) kernel, 1 three launches with the 36 split-bf16 GEMMs, 2 three launches with exact-f32 GEMMs, 3 three launches of F(2x2)."""
import functools

import numpy as np

from tests import split_bf16_emul as E

f32, f64 = np.float32, np.float64
SENTINEL = -7.0
FUSED, SPLIT3, F32_3, F22 = 0, 1, 2, 3
FORM_NAMES = {FUSED: "fused", SPLIT3: "3-launch split", F32_3: "3-launch f32", F22: "3-launch F(2x2)"}

# Lavin & Gray's matrices as winograd.hip and engine.hip document them
BT = {4: np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], f64),
      2: np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], f64)}
G = {4: np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], f64),
     2: np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], f64)}
AT = {4: np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], f64),
      2: np.array([[1, 1, 1, 0], [0, 1, -1, -1]], f64)}


def form_tile(form):
    return 2 if form == F22 else 4


# ---- the operation, twice in f64 ------------------------------------------------------------------------------------------------------

def direct_conv(x, w, dt=f64):
    """x [n][H][W][C], w [K][9][C] (tap = 3 ky + kx) -> [n][H][W][K]: zero padding 1, stride 1, summed in `dt`."""
    x, w = np.asarray(x).astype(dt), np.asarray(w).astype(dt)
    n, H, W, C = x.shape
    xp = np.zeros((n, H + 2, W + 2, C), dt)
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((n * H * W, w.shape[0]), dt)
    for t in range(9):
        ky, kx = divmod(t, 3)
        out += np.ascontiguousarray(xp[:, ky:ky + H, kx:kx + W]).reshape(-1, C) @ w[:, t].T
    return out.reshape(n, H, W, -1)


def epilogue(acc, scale=None, bias=None, residual=None, relu=False):
    v = np.asarray(acc, f64)
    if scale is not None:
        v = v * np.asarray(scale, f64)
    if bias is not None:
        v = v + np.asarray(bias, f64)
    if residual is not None:
        v = v + np.asarray(residual, f64).reshape(v.shape)
    return np.maximum(v, 0) if relu else v


def patches(x, m):
    """[n][H][W][C] -> the (m+2) x (m+2) input patches of the m x m output tiles, [n][th][tw][m+2][m+2][C], zeros outside the image."""
    n, H, W, C = x.shape
    th, tw = -(-H // m), -(-W // m)
    xp = np.zeros((n, m * th + 2, m * tw + 2, C), x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    d = np.empty((n, th, tw, m + 2, m + 2, C), x.dtype)
    for i in range(m + 2):
        for j in range(m + 2):
            d[:, :, :, i, j] = xp[:, i:i + m * th:m, j:j + m * tw:m]
    return d


def weight_transform(w, m):
    """U = G g G^T in f64, [(m+2)^2 = (m+2) i + j][K][C]."""
    w = np.asarray(w, f64)
    K, _, C = w.shape
    t = np.tensordot(G[m], w.reshape(K, 3, 3, C), axes=([1], [1]))      # [i][K][q][C]
    return np.tensordot(G[m], t, axes=([1], [2])).transpose(1, 0, 2, 3).reshape((m + 2) ** 2, K, C)      # [j][i][K][C] -> [i][j][K][C]


def weight_transform_576(w, m):
    """the same for weights that are integer multiples of 576 = 24^2, exactly: (24 G) (w / 576) (24 G)^T is integer arithmetic"""
    w = np.asarray(w, f64)
    K, _, C = w.shape
    g24, k = np.rint(24 * G[m]), w / 576
    assert np.array_equal(g24, 24 * G[m]) and np.array_equal(k, np.rint(k))
    t = np.tensordot(g24, k.reshape(K, 3, 3, C), axes=([1], [1]))
    return np.tensordot(g24, t, axes=([1], [2])).transpose(1, 0, 2, 3).reshape((m + 2) ** 2, K, C)


def _components(v):
    """[n][th][tw][a][a][C] -> [a a][T][C]"""
    a, C = v.shape[3], v.shape[5]
    return np.ascontiguousarray(v.transpose(3, 4, 0, 1, 2, 5)).reshape(a * a, -1, C)


def _untile(y, H, W):
    """[n][th][tw][m][m][K] -> [n][H][W][K]"""
    n, th, tw, m, _, K = y.shape
    return np.ascontiguousarray(y.transpose(0, 1, 3, 2, 4, 5)).reshape(n, m * th, m * tw, K)[:, :H, :W]


def by_matrices(x, w, m, absolute=False, u=None):
    """The conv by the documented matrices in f64.  absolute: |A^T| (sum_c |V||U|) |A| instead - the magnitude that rounding acts on;
    u: the weights already transformed ([(m+2)^2][K][C]) instead of G g G^T of w."""
    x = np.asarray(x, f64)
    n, H, W, C = x.shape
    d = patches(x, m)
    V = np.einsum("ip,ntspqc,jq->ntsijc", BT[m], d, BT[m])
    U = weight_transform(w, m) if u is None else np.asarray(u, f64)
    a = AT[m]
    if absolute:
        V, U, a = np.abs(V), np.abs(U), np.abs(a)
    M = np.matmul(_components(V), U.transpose(0, 2, 1))
    M = M.reshape(m + 2, m + 2, n, d.shape[1], d.shape[2], -1).transpose(2, 3, 4, 0, 1, 5)
    return _untile(np.einsum("ai,ntsijk,bj->ntsabk", a, M, a), H, W)


# ---- the kernels' arithmetic in f32 -----------------------------------------------------------------------------------------------------

def bt6(d):
    """winograd.hip's / winograd43_fused.hip's bt6 on six arrays, in the arrays' type"""
    d0, d1, d2, d3, d4, d5 = d
    a, b, c, e = d4 - 4 * d2, d3 - 4 * d1, d4 - d2, 2 * (d3 - d1)
    return [4 * d0 - 5 * d2 + d4, a + b, a - b, c + e, c - e, 4 * d1 - 5 * d3 + d5]


def at6(mm):
    m0, m1, m2, m3, m4, m5 = mm
    s12, d12, s34, d34 = m1 + m2, m1 - m2, m3 + m4, m3 - m4
    return [m0 + s12 + s34, d12 + 2 * d34, s12 + 4 * s34, d12 + 8 * d34 + m5]


def bt4(d):
    d0, d1, d2, d3 = d
    return [d0 - d2, d1 + d2, d2 - d1, d1 - d3]


def at4(mm):
    m0, m1, m2, m3 = mm
    return [m0 + m1 + m2, m1 - m2 - m3]


def _both_ways(v, step):
    """a transform step along axis 3 (the kernels' column pass), then along axis 4"""
    v = np.stack(step([v[:, :, :, i] for i in range(v.shape[3])]), axis=3)
    return np.stack(step([v[:, :, :, :, j] for j in range(v.shape[4])]), axis=4)


def gemm_exact(A, B):
    """[b][M][K] x [b][K][N]: f64 accumulation, rounded once"""
    return np.matmul(A.astype(f64), B.astype(f64)).astype(f32)


def gemm_chain(A, B):
    """split_bf16_emul.f32_chain, batched: one fused multiply-add per k"""
    A64, B64 = A.astype(f64), B.astype(f64)
    acc = np.zeros((A.shape[0], A.shape[1], B.shape[2]), f32)
    for k in range(A.shape[2]):
        acc = (acc.astype(f64) + A64[:, :, k:k + 1] * B64[:, k:k + 1, :]).astype(f32)
    return acc


def gemm_split(A, B, products=E.PRODUCTS, kgroup=16, memo=None):
    """split_bf16_emul.emulate, batched: per K group the chosen products in order, each summed in f64 and added to the f32 accumulator.
    memo: a dict of the caller's that keeps the split of B between calls with the SAME B (the weights of a case)"""
    bt, M, K = A.shape
    N, groups = B.shape[2], K // kgroup
    a = [p.astype(f64).reshape(bt, M, groups, kgroup).transpose(0, 2, 1, 3) for p in E.split3(A)]      # [b][g][M][16]
    b = None if memo is None else memo.get("b")
    if b is None:
        b = [p.astype(f64).reshape(bt, groups, kgroup, N) for p in E.split3(B)]                        # [b][g][16][N]
        if memo is not None:
            memo["b"] = b
    part = [np.matmul(a[i], b[j]) for i, j in products]                                                # every group's sum of every product
    acc = np.zeros((bt, M, N), f32)
    for g in range(groups):
        for q in part:
            acc = (acc.astype(f64) + q[:, g]).astype(f32)
    return acc


def gemm_v_bf16(A, B):
    """what a kernel that rounded V to bf16 would give (the bf16 precision's error level, for scale)"""
    return gemm_exact(E.bf16_round(A), B)


def fused_walk(pixel_blocks, kblocks, num_cus):
    """launch_winograd43_fused's grid and winograd43_fused_kernel's walk: per workgroup the list of blocks (pixel block * kblocks + kb) it
    computes, in order."""
    blocks = pixel_blocks * kblocks
    grid = min(blocks, 2 * (num_cus if num_cus > 0 else 256))
    unit = 8 * kblocks
    xcd = grid >= unit
    grid = grid // unit * unit if xcd else max(kblocks, grid // kblocks * kblocks)
    walks = []
    for wg in range(grid):
        first, count, q, stride = 0, blocks, wg, grid
        if xcd:
            j, sb = wg & 7, blocks // kblocks
            c, rem = sb >> 3, sb & 7
            q, stride = wg >> 3, grid >> 3
            first, count = (j * c + min(j, rem)) * kblocks, (c + (1 if j < rem else 0)) * kblocks
        walks.append([first + lb for lb in range(q, count, stride)])
    return walks


# what a kernel of this family could get wrong; ("drop", d) loses product d of split_bf16_emul.PRODUCTS in the 36 GEMMs
FAULTS = ("halo_right", "top_halo", "stale_patch", "ragged_row", "inplace_late", ("drop", 0), ("drop", 1), ("drop", 2), "kb_block0")


def standin(form, x, wgt, scale=None, bias=None, residual=None, relu=False, inplace=False, num_cus=0, guard=64, poison=False,
            sentinel=SENTINEL, fault=None, gemm=None):
    """The numpy model of Detector.debug_winograd_run.  gemm: None = the form's own (six products for form 1, the f32 chain otherwise), or
    one of the gemm_* functions / a tuple of products.  fault: None or one of FAULTS:
      halo_right    the patch column right of the image is not masked (it reads the next pixel in memory)
      top_halo      the patch row above image n > 0 is not masked (it reads the last row of image n - 1)
      stale_patch   form 0: a workgroup's block after its first is computed from the patch of the block it computed before
      ragged_row    the last tile row is not stored when H is no multiple of the tile
      inplace_late  in place, the residual is read after the result has been stored
      ("drop", d)   form 1: product d is missing from the GEMMs
      kb_block0     output channels 64 kb .. 64 kb + 63, kb > 0, are written over channels 0 .. 63"""
    m = form_tile(form)
    x, wgt = np.asarray(x, f32), np.asarray(wgt, f32)
    n, H, W, C = x.shape
    K = wgt.shape[0]
    th, tw = -(-H // m), -(-W // m)
    if form == FUSED:   # whole 16 x 16 blocks of 4 x 4 tiles
        th, tw = 4 * -(-H // 16), 4 * -(-W // 16)
    # the hook's allocation: the tensor between two guard regions of at least (W + 1) C floats
    lead = -(-(W + 1) * C // 1024) * 1024
    mem = np.full(2 * lead + x.size, np.nan if poison else 0.0, f32)
    mem[lead:lead + x.size] = x.ravel()
    mem = mem.reshape(-1, C)
    ys = m * np.arange(th)[:, None] - 1 + np.arange(m + 2)[None, :]     # [th][i]
    xs = m * np.arange(tw)[:, None] - 1 + np.arange(m + 2)[None, :]     # [tw][j]
    row_ok = np.broadcast_to(((ys >= 0) & (ys < H))[None], (n, th, m + 2)).copy()
    col_ok = (xs >= 0) & (xs < W)
    if fault == "halo_right":
        col_ok |= xs == W
    if fault == "top_halo":
        row_ok[1:] |= (ys == -1)[None]
    ok = row_ok[:, :, None, :, None] & col_ok[None, None, :, None, :]    # [n][th][tw][i][j]
    px = (np.arange(n)[:, None, None, None, None] * H + ys[None, :, None, :, None]) * W + xs[None, None, :, None, :] + lead // C
    d = mem[np.where(ok, px, 0)]
    d[~ok] = 0
    u = weight_transform(wgt, m).astype(f32)
    if gemm is None:
        gemm = gemm_split if form == SPLIT3 else gemm_chain
    if isinstance(fault, tuple) and form == SPLIT3:
        gemm = tuple(p for q, p in enumerate(E.PRODUCTS) if q != fault[1])
    if isinstance(gemm, tuple):
        gemm = functools.partial(gemm_split, products=gemm)

    def results(dd, k0, k1):
        v = _both_ways(dd, bt6 if m == 4 else bt4)
        mm = gemm(_components(v), np.ascontiguousarray(u[:, k0:k1].transpose(0, 2, 1)))
        mm = mm.reshape(m + 2, m + 2, n, th, tw, k1 - k0).transpose(2, 3, 4, 0, 1, 5)
        return _untile(_both_ways(mm, at6 if m == 4 else at4), H, W)

    if fault == "stale_patch" and form == FUSED:
        bh, bw, kblocks = th // 4, tw // 4, K // 64
        blk = d.reshape(n, bh, 4, bw, 4, m + 2, m + 2, C).transpose(0, 1, 3, 2, 4, 5, 6, 7).reshape(n * bh * bw, 4, 4, m + 2, m + 2, C)
        y = np.empty((n, H, W, K), f32)
        for kb in range(kblocks):
            src = np.arange(n * bh * bw)
            for walk in fused_walk(n * bh * bw, kblocks, num_cus):
                for prev, cur in zip(walk, walk[1:]):
                    if cur % kblocks == kb:
                        src[cur // kblocks] = prev // kblocks
            dd = blk[src].reshape(n, bh, bw, 4, 4, m + 2, m + 2, C).transpose(0, 1, 3, 2, 4, 5, 6, 7).reshape(d.shape)
            y[..., 64 * kb:64 * kb + 64] = results(np.ascontiguousarray(dd), 64 * kb, 64 * kb + 64)
    else:
        y = results(d, 0, K)

    io = np.full((n * H * W + guard, K), sentinel, f32)
    out = io[:n * H * W].reshape(n, H, W, K)
    res = None
    if residual is not None:
        res = np.asarray(residual, f32).reshape(n, H, W, K)
        if inplace:
            out[:] = res
    sc = f32(1) if scale is None else np.asarray(scale, f32)
    bi = f32(0) if bias is None else np.asarray(bias, f32)

    def finish(r):
        v = ((y * sc).astype(f32) + bi).astype(f32)
        if r is not None:
            v = (v + r).astype(f32)
        return np.maximum(v, f32(0)) if relu else v

    val = finish(finish(None) if (fault == "inplace_late" and inplace) else res)
    rows = H if not (fault == "ragged_row" and H % m) else m * (H // m)
    if fault == "kb_block0":
        for kb in range(K // 64):
            out[:, :rows, :, :64] = val[:, :rows, :, 64 * kb:64 * kb + 64]
    else:
        out[:, :rows] = val[:, :rows]
    return out, io[n * H * W:]


# ---- integer families -----------------------------------------------------------------------------------------------------------------------

# per Cin: (largest |x|, non-zero share of x, non-zero share of w / 576), chosen so that |A^T| (sum_c |V||U|) |A| stays below 2^24 with
# the epilogue's terms on top (asserted per case by integer_case); Cin 128 takes the family of 256; images of at most 4 pixels take
# x of Cin 64 whatever their Cin
INT_FAMILIES = {64: (3, 0.5, 0.5), 128: (2, 0.25, 0.25), 256: (2, 0.25, 0.25), 512: (1, 0.125, 0.25)}
EPILOGUES = ("none", "scale_bias", "residual", "inplace")
LIMIT = 1 << 24


class IntCase:
    """x, w and the epilogue operands of one integer case; acc = the direct conv as int64; bound = the Winograd-domain magnitude"""

    def operands(self, epi):
        """-> scale, bias, residual, inplace of a named epilogue"""
        if epi == "none":
            return None, None, None, False
        if epi == "scale_bias":
            return self.scale, self.bias, None, False
        return None, None, self.res, epi == "inplace"

    def reference(self, epi, relu):
        sc, bi, rs, _ = self.operands(epi)
        v = self.acc.copy()
        if sc is not None:
            v = v * sc.astype(np.int64) + bi.astype(np.int64)
        if rs is not None:
            v = v + rs.astype(np.int64)
        return np.maximum(v, 0) if relu else v


@functools.lru_cache(maxsize=4)
def integer_case(shape, cin, cout, seed=0):
    """One integer case (computed once, shared, never modified).  Asserts, in int64, the condition that makes equality a fair demand -
    |A^T| (sum_c |V||U|) |A| |scale| + |bias| + |res| < 2^24 for every element (with 2 % on top: the split-bf16 GEMMs add |hi| and |mid|
    products separately) - and that at least 90 % of the reference outputs are non-zero before ReLU, for every epilogue."""
    n, H, W = shape
    amax, px, pw = INT_FAMILIES[cin]
    if H * W <= 4:      # a patch that is nearly all padding: the sparse families would leave too many outputs zero, and the bound is far away
        amax, px = 3, 0.5
    rng = np.random.default_rng(1000003 * seed + 7919 * cin + 31 * cout + 10007 * n + 101 * H + W)
    x = rng.integers(1, amax + 1, (n, H, W, cin)) * rng.choice([-1, 1], (n, H, W, cin)) * (rng.random((n, H, W, cin)) < px)
    w = 576 * rng.choice([-1, 1], (cout, 9, cin)) * (rng.random((cout, 9, cin)) < pw)
    c = IntCase()
    c.shape, c.cin, c.cout = shape, cin, cout
    c.x, c.w = x.astype(f32), w.astype(f32)
    acc = direct_conv(x, w)        # f64 sums of integers far below 2^53 are exact
    c.acc = np.rint(acc).astype(np.int64)
    assert np.array_equal(c.acc, acc)
    u4 = weight_transform_576(w, 4)
    assert np.abs(u4 - weight_transform(w, 4)).max() < 1e-9 and np.abs(u4).max() < 1 << 16
    bound = np.rint(by_matrices(x, w, 4, absolute=True, u=u4)).astype(np.int64)
    c.bound = int(bound.max())
    spread = min(max(int(np.abs(c.acc).max()), 576), 1 << 20)
    c.bias = rng.integers(-spread, spread + 1, cout).astype(f32)
    c.res = rng.integers(-spread, spread + 1, (n, H, W, cout)).astype(f32)
    # per channel the largest of 4, 2, 1 that keeps the condition below, with either sign
    room = (LIMIT - 1 - spread) * 100 // (102 * np.maximum(bound.reshape(-1, cout).max(axis=0), 1))
    c.scale = (np.select([room >= 4, room >= 2], [4.0, 2.0], 1.0) * rng.choice([-1.0, 1.0], cout)).astype(f32)
    for epi in EPILOGUES:
        sc, bi, rs, _ = c.operands(epi)
        total = bound * (1 if sc is None else np.abs(sc).astype(np.int64)) * 102 // 100
        total = total + (0 if bi is None else np.abs(bi).astype(np.int64)) + (0 if rs is None else np.abs(rs).astype(np.int64))
        assert int(total.max()) < LIMIT, (shape, cin, cout, epi, int(total.max()))
        nz = float((c.reference(epi, False) != 0).mean())
        assert nz >= 0.9, (shape, cin, cout, epi, nz)
    for a in (c.x, c.w, c.acc, c.scale, c.bias, c.res):
        a.setflags(write=False)
    return c


# ---- rms cases ---------------------------------------------------------------------------------------------------------------------------------

class WinoCase:
    """One real-valued conv with scale, bias and ReLU, in the style of split_bf16_emul._Case: ref = the f64 definition, norm = the
    Winograd-domain |A^T| (sum_c |V||U|) |A| |scale| with U as the kernels read it (f32), keep = the elements ReLU does not clamp."""

    def __init__(self, x, w, scale, bias, m=4):
        self.x, self.w, self.scale, self.bias, self.m = np.asarray(x, f32), np.asarray(w, f32), np.asarray(scale, f32), np.asarray(bias, f32), m
        pre = epilogue(direct_conv(self.x, self.w), self.scale, self.bias)
        self.ref = np.maximum(pre, 0)
        self.keep = pre > 0
        self.left_out = 1.0 - float(self.keep.mean())
        u = weight_transform(self.w, m).astype(f32)
        self.norm = by_matrices(self.x, self.w, m, absolute=True, u=u) * np.abs(self.scale).astype(f64)
        self._memo = {}
        self.direct_norm = direct_conv(np.abs(self.x), np.abs(self.w)) * np.abs(self.scale).astype(f64)
        for a in (self.x, self.w, self.scale, self.bias, self.ref, self.keep, self.norm):
            a.setflags(write=False)

    def _err(self, out, other=None):
        return ((np.asarray(out, f64) - (self.ref if other is None else np.asarray(other, f64))) / self.norm)[self.keep]

    def rms(self, out, other=None):
        e = self._err(out, other)
        return float(np.sqrt(np.mean(e * e)))

    def largest(self, out):
        return float(np.abs(self._err(out)).max())

    def run(self, run, form, **kw):
        out, guard = run(form, self.x, self.w, scale=self.scale, bias=self.bias, relu=True, **kw)
        assert guard.size and (guard == SENTINEL).all(), "the launch wrote behind its output"
        return out

    def emulated(self, products=E.PRODUCTS):
        return self.run(standin, SPLIT3 if self.m == 4 else F22, gemm=functools.partial(gemm_split, products=tuple(products), memo=self._memo))

    def chain(self):
        return self.run(standin, F32_3 if self.m == 4 else F22)

    def v_bf16(self):
        return self.run(standin, F32_3, gemm=gemm_v_bf16)


# form(s), cin, cout, (n, H, W)
W4_CASES = (((FUSED,), 64, 64, (2, 20, 24)), ((FUSED,), 128, 64, (1, 13, 37)), ((FUSED,), 256, 64, (1, 16, 16)),
            ((SPLIT3, F32_3), 256, 256, (2, 9, 21)), ((SPLIT3, F32_3), 512, 512, (1, 8, 8)))
W4_FAMILIES = ("relu", "offset")


@functools.lru_cache(maxsize=None)
def wino_case(cin, cout, shape, family):
    """relu: x = relu(N(0,1)); offset: x = 0.1 N(0,1) + 3, a common offset that B^T cancels.  w ~ N(0,1) / sqrt(9 cin), scale in +-[0.5, 1.5];
    the bias puts the 30 % quantile of every channel's reference at zero, so that ReLU clamps about 30 % whatever the family."""
    n, H, W = shape
    rng = np.random.default_rng(4300 + cin + 7 * cout + H + 1000 * W4_FAMILIES.index(family))
    g = rng.standard_normal((n, H, W, cin))
    x = (np.maximum(g, 0) if family == "relu" else 0.1 * g + 3).astype(f32)
    w = (rng.standard_normal((cout, 9, cin)) / np.sqrt(9 * cin)).astype(f32)
    scale = ((0.5 + rng.random(cout)) * rng.choice([-1.0, 1.0], cout)).astype(f32)
    pre = direct_conv(x, w) * scale.astype(f64)
    bias = (-np.quantile(pre.reshape(-1, cout), 0.3, axis=0)).astype(f32)
    return WinoCase(x, w, scale, bias)


@functools.lru_cache(maxsize=None)
def wino_bar(cin, cout, shape, family):
    """(six, smallest five, bar, names of the drops that change anything, f32 chain rms, largest element of the six-product emulation,
    of the chain) of a case - everything the GPU test needs from the CPU"""
    case = wino_case(cin, cout, shape, family)
    six, five, bar, names = E.bar(case)
    chain = case.chain()
    return six, five, bar, names, case.rms(chain), case.largest(case.emulated()), case.largest(chain)


# ---- the assertions of tests/test_gpu_winograd_kernels.py, as functions of `run` ----------------------------------------------------------------

def _guard_rows(shape):
    return 2 * shape[2] + 64      # more than two output rows


def run_int(run, form, case, epi, relu, **kw):
    sc, bi, rs, inplace = case.operands(epi)
    out, guard = run(form, case.x, case.w, scale=sc, bias=bi, residual=rs, relu=relu, inplace=inplace, guard=_guard_rows(case.shape),
                     sentinel=SENTINEL, **kw)
    assert guard.size and (guard == SENTINEL).all(), "the launch wrote behind its output"
    return out


def assert_equal_int(name, got, want):
    assert np.isfinite(got).all(), (name, int((~np.isfinite(got)).sum()), "not finite")
    bad = got != want
    assert not bad.any(), (name, int(bad.sum()), "elements differ, first at", tuple(int(i) for i in np.argwhere(bad)[0]),
                           float(got[bad][0]), int(want[bad][0]))


def check_w1(run, form, shape, cin, cout):
    """equality with the int64 direct conv for every epilogue of the graph, ReLU on and off"""
    case = integer_case(shape, cin, cout)
    for epi in EPILOGUES:
        for relu in (False, True):
            got = run_int(run, form, case, epi, relu)
            assert_equal_int(f"{FORM_NAMES[form]} {shape} {cin} -> {cout} {epi} relu {relu}", got, case.reference(epi, relu))


W2_SHAPE, W2_CUS = (3, 33, 17), (1, 2, 3, 4, 8, 9, 40)


def check_w2(run, cin, cout):
    """the fused kernel's walk: 18 pixel blocks under every grid the launcher forms for them - equal to the reference and bit-identical"""
    case = integer_case(W2_SHAPE, cin, cout)
    outs = []
    for cus in W2_CUS:
        got = run_int(run, FUSED, case, "inplace", True, num_cus=cus)
        assert_equal_int(f"fused {W2_SHAPE} {cin} -> {cout} num_cus {cus}", got, case.reference("inplace", True))
        outs.append(got)
    real = wino_case(cin, cout, W2_SHAPE, "relu")     # real values: on integers every order of the sums gives the same bits
    outs = [real.run(run, FUSED, num_cus=cus) for cus in W2_CUS]
    for cus, o in zip(W2_CUS[1:], outs[1:]):
        assert np.array_equal(outs[0].view(np.uint32), o.view(np.uint32)), f"num_cus {cus} differs from num_cus {W2_CUS[0]}"


def w3_shapes(form):
    """one ragged case, then H and W one past a block edge (fused) and one past a tile edge"""
    m = form_tile(form)
    return ((2, 15, 17), (1, 17, 17), (2, m + 1, m + 1)) if form == FUSED else ((3, 3, 5), (2, m + 1, m + 1), (1, 2 * m + 1, m + 1))


def check_w3(run, form, shape, cin, cout):
    """NaN around the source: still equal, no NaN anywhere, every guard row untouched (run_int)"""
    case = integer_case(shape, cin, cout)
    for epi in ("scale_bias", "inplace"):
        got = run_int(run, form, case, epi, False, poison=True)
        assert_equal_int(f"poisoned {FORM_NAMES[form]} {shape} {cin} -> {cout} {epi}", got, case.reference(epi, False))


MAX_FACTOR = 10.0     # the largest element against the CPU emulation's: what another summation order does to a maximum over ~1e5 elements


def check_w4(run, forms, cin, cout, shape, family, report=print):
    """rms(kernel - f64) <= sqrt(rms_six x min rms_five) for every form of the case, the largest element within MAX_FACTOR of the emulation's,
    and forms 1 and 2 apart by no more than the same bar.  Returns the measured figures per form."""
    case = wino_case(cin, cout, shape, family)
    six, five, bar, names, chain, big_six, big_chain = wino_bar(cin, cout, shape, family)
    assert case.left_out < 0.6, case.left_out
    outs, figures = {}, {}
    for form in forms:
        out = outs[form] = case.run(run, form)
        rms, big = case.rms(out), case.largest(out)
        limit = MAX_FACTOR * (big_six if form == SPLIT3 else big_chain)
        figures[form] = (rms, big)
        report(f"W4 {FORM_NAMES[form]} {cin} -> {cout} {shape} {family}: six {six:.3g}  five {five:.3g} ({five / six:.1f} x)  chain {chain:.3g}  bar {bar:.3g}  "
               f"measured {rms:.3g} ({rms / bar:.2f} of the bar)  largest element {big:.3g} (limit {limit:.3g})  left out {case.left_out:.2f}")
        assert np.isfinite(out).all()
        assert rms <= bar, (FORM_NAMES[form], rms, bar)
        assert big <= limit, (FORM_NAMES[form], big, limit)
    if SPLIT3 in outs and F32_3 in outs:
        apart = case.rms(outs[SPLIT3], outs[F32_3])
        report(f"W4 forms 1 and 2 apart {apart:.3g} (bar {bar:.3g})")
        assert apart <= bar, (apart, bar)
    return figures
