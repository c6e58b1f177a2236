// Winograd F(2x2, 3x3) transforms for the deep 3x3 s1 p1 convs of the detector trunk (layer3 / layer4,
// /root/reference/src/text_detection/model.rs:40-55): y = A^T [ (G g G^T) . (B^T d B) ] A per 2x2 output tile,
// 16 multiplies instead of 36 per (tile, cin, cout).  The 16 element-wise products over all tiles and channels
// are 16 independent GEMMs [T x C] x [C x K] and run on the matrix cores through conv_igemm's batched mode;
// the kernels here are the HBM-bound ends: d -> V = B^T d B and M -> Y = A^T M A (+ folded BN, residual, ReLU).
//
//   B^T = | 1  0 -1  0 |     G = | 1    0    0  |     A^T = | 1 1  1  0 |
//         | 0  1  1  0 |         | 1/2  1/2  1/2|           | 0 1 -1 -1 |
//         | 0 -1  1  0 |         | 1/2 -1/2  1/2|
//         | 0  1  0 -1 |         | 0    0    1  |
//
// Only additions and subtractions of f32 values happen here (the 1/2 factors live in the host-side weight
// transform, engine.hip), so the results differ from the direct convolution by summation order / a few ulp.
#include "common.hpp"

namespace ocr {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// one thread = one tile x 4 channels; consecutive threads walk the channels of a tile (coalesced 16-byte
// accesses on both sides).  v layout [16][T][C].
__global__ __launch_bounds__(256) void winograd_input_kernel(const float* __restrict__ x, float* __restrict__ v, int H, int W,
                                                             int C, int th, int tw, long long T) {
  const int c4n = C >> 2;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= T * c4n) return;
  const long long t = gid / c4n;
  const int c = (int)(gid - t * c4n) * 4;
  const int tx = (int)(t % tw);
  const long long r = t / tw;
  const int ty = (int)(r % th);
  const long long n = r / th;
  const int y0 = 2 * ty - 1, x0 = 2 * tx - 1;
  f32x4 d[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int yy = y0 + i, xx = x0 + j;
      const bool ok = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      d[i][j] = ok ? *reinterpret_cast<const f32x4*>(x + ((n * H + yy) * W + xx) * C + c) : zero;
    }
  f32x4 r4[4][4];  // B^T d
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r4[0][j] = d[0][j] - d[2][j];
    r4[1][j] = d[1][j] + d[2][j];
    r4[2][j] = d[2][j] - d[1][j];
    r4[3][j] = d[1][j] - d[3][j];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // (B^T d) B
    const f32x4 v0 = r4[i][0] - r4[i][2];
    const f32x4 v1 = r4[i][1] + r4[i][2];
    const f32x4 v2 = r4[i][2] - r4[i][1];
    const f32x4 v3 = r4[i][1] - r4[i][3];
    float* o = v + ((size_t)(4 * i) * T + t) * C + c;
    const size_t step = (size_t)T * C;
    *reinterpret_cast<f32x4*>(o) = v0;
    *reinterpret_cast<f32x4*>(o + step) = v1;
    *reinterpret_cast<f32x4*>(o + 2 * step) = v2;
    *reinterpret_cast<f32x4*>(o + 3 * step) = v3;
  }
}

// one thread = one tile x 4 output channels.  m layout [16][T][K]; y NHWC.
__global__ __launch_bounds__(256) void winograd_output_kernel(const float* __restrict__ m, const float* __restrict__ scale,
                                                              const float* __restrict__ bias, const float* __restrict__ residual,
                                                              int relu, float* __restrict__ y, int H, int W, int K, int th,
                                                              int tw, long long T) {
  const int k4n = K >> 2;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= T * k4n) return;
  const long long t = gid / k4n;
  const int k = (int)(gid - t * k4n) * 4;
  const int tx = (int)(t % tw);
  const long long r = t / tw;
  const int ty = (int)(r % th);
  const long long n = r / th;
  const size_t step = (size_t)T * K;
  const float* src = m + (size_t)t * K + k;
  f32x4 a[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) a[i][j] = *reinterpret_cast<const f32x4*>(src + (size_t)(4 * i + j) * step);
  f32x4 u[2][4];  // A^T M
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    u[0][j] = a[0][j] + a[1][j] + a[2][j];
    u[1][j] = a[1][j] - a[2][j] - a[3][j];
  }
  f32x4 sc = {1.f, 1.f, 1.f, 1.f}, bi = {0.f, 0.f, 0.f, 0.f};
  if (scale) sc = *reinterpret_cast<const f32x4*>(scale + k);
  if (bias) bi = *reinterpret_cast<const f32x4*>(bias + k);
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const f32x4 o0 = u[p][0] + u[p][1] + u[p][2];
    const f32x4 o1 = u[p][1] - u[p][2] - u[p][3];
    const int yy = 2 * ty + p;
    if (yy >= H) continue;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int xx = 2 * tx + q;
      if (xx >= W) continue;
      const size_t o = ((n * H + yy) * W + xx) * (size_t)K + k;
      f32x4 val = (q ? o1 : o0) * sc + bi;
      if (residual) val += *reinterpret_cast<const f32x4*>(residual + o);
      if (relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) val[e] = fmaxf(val[e], 0.f);
      }
      *reinterpret_cast<f32x4*>(y + o) = val;
    }
  }
}

// ---- F(4x4, 3x3): 36 multiplies per 4x4 output tile (2.25 per output instead of 4) for the grids where the transforms are
// cheap beside the GEMMs (layer4's 512 channels at H/32).  Lavin & Gray's matrices; the weight transform carries the
// fractions of G (engine.hip, f64 rounded once), so the device side multiplies by 2, 4, 5 and 8 only:
//
//   B^T = | 4  0 -5  0  1  0 |     A^T = | 1  1  1  1  1  0 |
//         | 0 -4 -4  1  1  0 |           | 0  1 -1  2 -2  0 |
//         | 0  4 -4 -1  1  0 |           | 0  1  1  4  4  0 |
//         | 0 -2 -1  2  1  0 |           | 0  1 -1  8 -8  1 |
//         | 0  2 -1 -2  1  0 |
//         | 0  4  0 -5  0  1 |
//
// The products are larger and cancel more than F(2x2)'s: ~1e-6 relative error of a conv output instead of ~1e-7.
template <typename V>
__device__ __forceinline__ void bt6(const V d0, const V d1, const V d2, const V d3, const V d4, const V d5, V* t) {
  const V a = d4 - 4.f * d2, b = d3 - 4.f * d1, c = d4 - d2, e = 2.f * (d3 - d1);
  t[0] = 4.f * d0 - 5.f * d2 + d4;
  t[1] = a + b;
  t[2] = a - b;
  t[3] = c + e;
  t[4] = c - e;
  t[5] = 4.f * d1 - 5.f * d3 + d5;
}

// one thread = one tile x 2 channels (36 loads of 8 bytes; consecutive threads walk the channels).  v layout [36][T][C].
// Addresses through buffer descriptors: lane part (the tile's first pixel, this channel pair) in the voffset, tap / component
// part a scalar - no 64-bit index arithmetic and no branch per element (the first form spent ~10 integer instructions and
// an exec-mask branch on each of its 36 loads); taps outside the image get an out-of-range voffset and read as zero.
// The input descriptor starts one row and one pixel BEFORE the tensor so that the tap offsets (i W + j) C are non-negative.
constexpr unsigned WOOB = 0x80000000u;
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256) void winograd43_input_kernel(const float* __restrict__ x, float* __restrict__ v, int H, int W,
                                                               int C, int th, int tw, long long T, unsigned x_bytes, unsigned v_bytes) {
  const int c2n = C >> 1;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= T * c2n) return;
  const long long t = gid / c2n;
  const int c = (int)(gid - t * c2n) * 2;
  const int tx = (int)(t % tw);
  const long long r = t / tw;
  const int ty = (int)(r % th);
  const int n = (int)(r / th);
  const unsigned lead = (unsigned)(W + 1) * C * 4;
  const auto x_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x) - (size_t)(W + 1) * C, 0, x_bytes + lead, 0x00020000);
  const auto v_rsrc = __builtin_amdgcn_make_buffer_rsrc(v, 0, v_bytes, 0x00020000);
  const unsigned voff0 = (unsigned)((((n * H + 4 * ty) * W + 4 * tx) * C + c) * 4);
  bool row_ok[6], col_ok[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    row_ok[i] = (unsigned)(4 * ty - 1 + i) < (unsigned)H;
    col_ok[i] = (unsigned)(4 * tx - 1 + i) < (unsigned)W;
  }
  f32x2 rt[6][6];  // B^T d, column by column
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    f32x2 d[6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
      d[i] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(x_rsrc, (row_ok[i] && col_ok[j]) ? voff0 : WOOB,
                                                                            (i * W + j) * C * 4, 0));
    f32x2 tcol[6];
    bt6(d[0], d[1], d[2], d[3], d[4], d[5], tcol);
#pragma unroll
    for (int i = 0; i < 6; ++i) rt[i][j] = tcol[i];
  }
  const unsigned step = (unsigned)(T * C) * 4u;              // bytes between components (36 x step < 2^31: checked by the launcher)
  const unsigned voff_v = (unsigned)((t * C + c) * 4);
#pragma unroll
  for (int i = 0; i < 6; ++i) {  // (B^T d) B
    f32x2 o[6];
    bt6(rt[i][0], rt[i][1], rt[i][2], rt[i][3], rt[i][4], rt[i][5], o);
#pragma unroll
    for (int j = 0; j < 6; ++j) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o[j]), v_rsrc, voff_v, (6 * i + j) * step, 0);
  }
}

// winograd43_input_kernel with the FPN's top-down add on load: d = up2(low)(y, x) + x(y, x) before bt6, low [N][H/2][W/2][C] (H and W even).
// The engine runs out4 this way (top_side): in4 stores its plain conv, and the one f32 add that conv_igemm's epilogue
// made of the same two values (up + v) happens here - the same bits in V.  A tile starts at a multiple of 4, so the low pixel of tap
// (i, j) is (2 ty - 1 + (i + 1) / 2, 2 tx - 1 + (j + 1) / 2): a 4 x 4 patch of low values per tile, each requested once.  The low tensor has
// its own descriptor (it, too, starts one row and one pixel before the tensor) and its own out-of-range voffset; with H and W even a low
// pixel is inside exactly where the taps it covers are, so a tap outside the image is 0 + 0.
__global__ __launch_bounds__(256) void winograd43_input_up2_kernel(const float* __restrict__ x, const float* __restrict__ low, float* __restrict__ v,
                                                                   int H, int W, int C, int th, int tw, long long T, unsigned x_bytes,
                                                                   unsigned low_bytes, unsigned v_bytes) {
  const int c2n = C >> 1;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= T * c2n) return;
  const long long t = gid / c2n;
  const int c = (int)(gid - t * c2n) * 2;
  const int tx = (int)(t % tw);
  const long long r = t / tw;
  const int ty = (int)(r % th);
  const int n = (int)(r / th);
  const int Hl = H >> 1, Wl = W >> 1;
  const unsigned lead = (unsigned)(W + 1) * C * 4, lead_l = (unsigned)(Wl + 1) * C * 4;
  const auto x_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x) - (size_t)(W + 1) * C, 0, x_bytes + lead, 0x00020000);
  const auto l_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(low) - (size_t)(Wl + 1) * C, 0, low_bytes + lead_l, 0x00020000);
  const auto v_rsrc = __builtin_amdgcn_make_buffer_rsrc(v, 0, v_bytes, 0x00020000);
  const unsigned voff0 = (unsigned)((((n * H + 4 * ty) * W + 4 * tx) * C + c) * 4);
  const unsigned voff0_l = (unsigned)((((n * Hl + 2 * ty) * Wl + 2 * tx) * C + c) * 4);
  bool row_ok[6], col_ok[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    row_ok[i] = (unsigned)(4 * ty - 1 + i) < (unsigned)H;
    col_ok[i] = (unsigned)(4 * tx - 1 + i) < (unsigned)W;
  }
  f32x2 lo[4][4];   // low row li covers the taps i = 2 li - 1, 2 li: inside with tap 2 li (li < 3) / tap 5
#pragma unroll
  for (int li = 0; li < 4; ++li)
#pragma unroll
    for (int lj = 0; lj < 4; ++lj) {
      const bool ok = row_ok[li < 3 ? 2 * li : 5] && col_ok[lj < 3 ? 2 * lj : 5];
      lo[li][lj] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(l_rsrc, ok ? voff0_l : WOOB, (li * Wl + lj) * C * 4, 0));
    }
  f32x2 rt[6][6];  // B^T d, column by column
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    f32x2 d[6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
      d[i] = lo[(i + 1) >> 1][(j + 1) >> 1] +
             __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(x_rsrc, (row_ok[i] && col_ok[j]) ? voff0 : WOOB, (i * W + j) * C * 4, 0));
    f32x2 tcol[6];
    bt6(d[0], d[1], d[2], d[3], d[4], d[5], tcol);
#pragma unroll
    for (int i = 0; i < 6; ++i) rt[i][j] = tcol[i];
  }
  const unsigned step = (unsigned)(T * C) * 4u;              // bytes between components (36 x step < 2^31: checked by the launcher)
  const unsigned voff_v = (unsigned)((t * C + c) * 4);
#pragma unroll
  for (int i = 0; i < 6; ++i) {  // (B^T d) B
    f32x2 o[6];
    bt6(rt[i][0], rt[i][1], rt[i][2], rt[i][3], rt[i][4], rt[i][5], o);
#pragma unroll
    for (int j = 0; j < 6; ++j) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o[j]), v_rsrc, voff_v, (6 * i + j) * step, 0);
  }
}

template <typename V>
__device__ __forceinline__ void at6(const V m0, const V m1, const V m2, const V m3, const V m4, const V m5, V* y) {
  const V s12 = m1 + m2, d12 = m1 - m2, s34 = m3 + m4, d34 = m3 - m4;
  y[0] = m0 + s12 + s34;
  y[1] = d12 + 2.f * d34;
  y[2] = s12 + 4.f * s34;
  y[3] = d12 + 8.f * d34 + m5;
}

// one thread = one tile x 2 output channels.  m layout [36][T][K]; y NHWC.  Buffer addressing as in the input kernel; the
// residual block is requested first: its 16 loads are in flight under the 36 loads and the arithmetic of the transform
// (requested where they are consumed, behind per-pixel bounds checks, they cost 0.024 ms per layer3 conv for 52 MB - half
// the kernel); pixels beyond the image read as zero and are not stored (out-of-range voffset).
__global__ __launch_bounds__(256) void winograd43_output_kernel(const float* __restrict__ m, const float* __restrict__ scale,
                                                                const float* __restrict__ bias, const float* __restrict__ residual,
                                                                int relu, float* __restrict__ y, int H, int W, int K, int th,
                                                                int tw, long long T, unsigned m_bytes, unsigned y_bytes) {
  const int k2n = K >> 1;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= T * k2n) return;
  const long long t = gid / k2n;
  const int k = (int)(gid - t * k2n) * 2;
  const int tx = (int)(t % tw);
  const long long r = t / tw;
  const int ty = (int)(r % th);
  const int n = (int)(r / th);
  const auto m_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(m), 0, m_bytes, 0x00020000);
  const auto y_rsrc = __builtin_amdgcn_make_buffer_rsrc(y, 0, y_bytes, 0x00020000);
  const auto r_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(residual ? residual : y), 0, residual ? y_bytes : 0u, 0x00020000);
  const unsigned voff0 = (unsigned)((((n * H + 4 * ty) * W + 4 * tx) * K + k) * 4);
  unsigned pv[4][4];   // this lane's offset of pixel (p, q) of the tile: the tile origin, or out of range beyond the image
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) pv[p][q] = (4 * ty + p < H && 4 * tx + q < W) ? voff0 : WOOB;
  f32x2 res[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      res[p][q] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r_rsrc, pv[p][q], (p * W + q) * K * 4, 0));   // (no residual: 0 records, zeros)
  const unsigned step = (unsigned)(T * K) * 4u;
  const unsigned voff_m = (unsigned)((t * K + k) * 4);
  f32x2 u[4][6];  // A^T M, column by column
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    f32x2 a[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) a[i] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(m_rsrc, voff_m, (6 * i + j) * step, 0));
    f32x2 col[4];
    at6(a[0], a[1], a[2], a[3], a[4], a[5], col);
#pragma unroll
    for (int p = 0; p < 4; ++p) u[p][j] = col[p];
  }
  f32x2 sc = {1.f, 1.f}, bi = {0.f, 0.f};
  if (scale) sc = *reinterpret_cast<const f32x2*>(scale + k);
  if (bias) bi = *reinterpret_cast<const f32x2*>(bias + k);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    f32x2 o4[4];
    at6(u[p][0], u[p][1], u[p][2], u[p][3], u[p][4], u[p][5], o4);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x2 val = o4[q] * sc + bi + res[p][q];
      if (relu) {
        val[0] = fmaxf(val[0], 0.f);
        val[1] = fmaxf(val[1], 0.f);
      }
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, val), y_rsrc, pv[p][q], (p * W + q) * K * 4, 0);
    }
  }
}

}  // namespace

void launch_winograd_input_up2(const float* x, const float* low, float* v, int N, int H, int W, int C, hipStream_t s) {
  if (!x || !low || !v || N <= 0 || H <= 0 || W <= 0 || ((H | W) & 1) || C <= 0 || C % 4)
    fail(OCR_ERR_INVALID, "winograd input + top-down: bad shape N=%d H=%d W=%d C=%d (H and W even, C a multiple of 4)", N, H, W, C);
  const int th = (H + 3) / 4, tw = (W + 3) / 4;
  const long long T = (long long)N * th * tw;
  const long long threads = T * (C / 2);
  if (threads >= (1ll << 31) * 256) fail(OCR_ERR_INVALID, "winograd input + top-down: too large");
  const unsigned long long xb = (unsigned long long)N * H * W * C * 4, lb = xb / 4, vb = 36ull * T * C * 4;
  if (xb + (unsigned long long)(W + 1) * C * 4 >= (1ull << 31) || vb >= (1ull << 31)) fail(OCR_ERR_INVALID, "winograd input + top-down: tensors beyond 2 GB");
  hipLaunchKernelGGL(winograd43_input_up2_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, x, low, v, H, W, C, th, tw, T, (unsigned)xb,
                     (unsigned)lb, (unsigned)vb);
  OCR_HIP(hipGetLastError());
}

void launch_winograd_input(const float* x, float* v, int N, int H, int W, int C, int m, hipStream_t s) {
  if (N <= 0 || H <= 0 || W <= 0 || C % 4 || (m != 2 && m != 4)) fail(OCR_ERR_INVALID, "winograd input: bad shape N=%d H=%d W=%d C=%d m=%d", N, H, W, C, m);
  if (m == 4) {
    const int th = (H + 3) / 4, tw = (W + 3) / 4;
    const long long T = (long long)N * th * tw;
    const long long threads = T * (C / 2);
    if (threads >= (1ll << 31) * 256) fail(OCR_ERR_INVALID, "winograd input: too large");
    const unsigned long long xb = (unsigned long long)N * H * W * C * 4, vb = 36ull * T * C * 4;
    if (xb + (unsigned long long)(W + 1) * C * 4 >= (1ull << 31) || vb >= (1ull << 31)) fail(OCR_ERR_INVALID, "winograd input: tensors beyond 2 GB");
    hipLaunchKernelGGL(winograd43_input_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, x, v, H, W, C, th, tw, T, (unsigned)xb, (unsigned)vb);
    OCR_HIP(hipGetLastError());
    return;
  }
  const int th = (H + 1) / 2, tw = (W + 1) / 2;
  const long long T = (long long)N * th * tw;
  const long long threads = T * (C / 4);
  if (threads >= (1ll << 31) * 256) fail(OCR_ERR_INVALID, "winograd input: too large");
  hipLaunchKernelGGL(winograd_input_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, x, v, H, W, C, th, tw, T);
  OCR_HIP(hipGetLastError());
}

void launch_winograd_output(const float* m, const float* scale, const float* bias, const float* residual, int relu, float* y,
                            int N, int H, int W, int K, int m_tile, hipStream_t s) {
  if (N <= 0 || H <= 0 || W <= 0 || K % 4 || (m_tile != 2 && m_tile != 4)) fail(OCR_ERR_INVALID, "winograd output: bad shape N=%d H=%d W=%d K=%d m=%d", N, H, W, K, m_tile);
  if (m_tile == 4) {
    const int th = (H + 3) / 4, tw = (W + 3) / 4;
    const long long T = (long long)N * th * tw;
    const long long threads = T * (K / 2);
    if (threads >= (1ll << 31) * 256) fail(OCR_ERR_INVALID, "winograd output: too large");
    const unsigned long long yb = (unsigned long long)N * H * W * K * 4, mb = 36ull * T * K * 4;
    if (yb >= (1ull << 31) || mb >= (1ull << 31)) fail(OCR_ERR_INVALID, "winograd output: tensors beyond 2 GB");
    hipLaunchKernelGGL(winograd43_output_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, m, scale, bias, residual,
                       relu, y, H, W, K, th, tw, T, (unsigned)mb, (unsigned)yb);
    OCR_HIP(hipGetLastError());
    return;
  }
  const int th = (H + 1) / 2, tw = (W + 1) / 2;
  const long long T = (long long)N * th * tw;
  const long long threads = T * (K / 4);
  if (threads >= (1ll << 31) * 256) fail(OCR_ERR_INVALID, "winograd output: too large");
  hipLaunchKernelGGL(winograd_output_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, m, scale, bias, residual,
                     relu, y, H, W, K, th, tw, T);
  OCR_HIP(hipGetLastError());
}

}  // namespace ocr
