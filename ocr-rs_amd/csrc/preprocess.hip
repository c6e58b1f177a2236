// preprocess_image as HIP image kernels.
//   /root/reference/src/image_ops.rs:188-220: decode -> RGBA -> DynamicImage::resize(W, H, Triangle)
//   (aspect preserving) -> to_luma -> zero-pad to W x H; adjust = resized / original.
// The sampling arithmetic is that of the un-vendored crate image 0.23.11 (imageops::resize =
// vertical_sample then horizontal_sample, f32 weights normalised per output index, every pass
// truncated to u8; luma = trunc(0.2126 R + 0.7152 G + 0.0722 B)).  Weight tables are built on the
// host with the same f32 operation order; the kernels accumulate with separately rounded multiply
// and add (no FMA contraction), so the result equals oracle/preprocess_oracle.py bit for bit.
// HBM-bound: one pass reads the RGBA source, the second writes the padded gray frame (+ f32 copy).
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include "common.hpp"

namespace ocr {
namespace {

// image 0.23.11 sample.rs, Triangle filter (support 1.0); every step in f32 like the crate
AxisTable build_axis(int in_size, int out_size) {
  AxisTable t;
  const float ratio = (float)in_size / (float)out_size;
  const float sratio = ratio < 1.0f ? 1.0f : ratio;
  const float support = 1.0f * sratio;
  std::vector<std::vector<float>> ws(out_size);
  t.left.resize(out_size);
  t.count.resize(out_size);
  for (int o = 0; o < out_size; ++o) {
    float inp = ((float)o + 0.5f) * ratio;
    long left = (long)std::floor(inp - support);
    left = std::min<long>(std::max<long>(left, 0), in_size - 1);
    long right = (long)std::ceil(inp + support);
    right = std::min<long>(std::max<long>(right, left + 1), in_size);
    inp = inp - 0.5f;
    float sum = 0.0f;
    for (long i = left; i < right; ++i) {
      const float x = ((float)i - inp) / sratio;
      const float ax = std::fabs(x);
      const float w = ax < 1.0f ? 1.0f - ax : 0.0f;
      ws[o].push_back(w);
      sum += w;
    }
    for (float& w : ws[o]) w /= sum;
    t.left[o] = (int)left;
    t.count[o] = (int)ws[o].size();
    t.maxk = std::max(t.maxk, t.count[o]);
  }
  t.w.assign((size_t)out_size * t.maxk, 0.0f);
  for (int o = 0; o < out_size; ++o)
    for (int k = 0; k < t.count[o]; ++k) t.w[(size_t)o * t.maxk + k] = ws[o][k];
  return t;
}

__device__ __forceinline__ unsigned char to_u8(float t) { return (unsigned char)fminf(fmaxf(t, 0.f), 255.f); }  // clamp, truncate

// vertical_sample: src h x w RGBA -> tmp nh x w RGBA; one thread per output pixel (4 channels)
__global__ __launch_bounds__(256) void resize_vertical_kernel(const uchar4* __restrict__ src, uchar4* __restrict__ tmp, int w,
                                                              int nh, const int* __restrict__ left, const int* __restrict__ cnt,
                                                              const float* __restrict__ wts, int maxk) {
  const int x = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y;
  if (x >= w || oy >= nh) return;
  const int l = left[oy], c = cnt[oy];
  float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
  for (int k = 0; k < c; ++k) {
    const uchar4 p = src[(size_t)(l + k) * w + x];
    const float wk = wts[oy * maxk + k];
    t0 = __fadd_rn(t0, __fmul_rn((float)p.x, wk));
    t1 = __fadd_rn(t1, __fmul_rn((float)p.y, wk));
    t2 = __fadd_rn(t2, __fmul_rn((float)p.z, wk));
    t3 = __fadd_rn(t3, __fmul_rn((float)p.w, wk));
  }
  tmp[(size_t)oy * w + x] = make_uchar4(to_u8(t0), to_u8(t1), to_u8(t2), to_u8(t3));
}

// horizontal_sample + to_luma + zero padding: tmp nh x w RGBA -> gray H x W u8 (and f32 copy)
__global__ __launch_bounds__(256) void resize_horizontal_luma_kernel(const uchar4* __restrict__ tmp, unsigned char* __restrict__ gray,
                                                                     float* __restrict__ gray_f32, int w, int nw, int nh, int W,
                                                                     int H, const int* __restrict__ left, const int* __restrict__ cnt,
                                                                     const float* __restrict__ wts, int maxk) {
  const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y;
  if (ox >= W || oy >= H) return;
  unsigned char g = 0;  // zero padding right of / below the resized image (image_ops.rs:204-214)
  if (ox < nw && oy < nh) {
    const int l = left[ox], c = cnt[ox];
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
    for (int k = 0; k < c; ++k) {
      const uchar4 p = tmp[(size_t)oy * w + l + k];
      const float wk = wts[ox * maxk + k];
      t0 = __fadd_rn(t0, __fmul_rn((float)p.x, wk));
      t1 = __fadd_rn(t1, __fmul_rn((float)p.y, wk));
      t2 = __fadd_rn(t2, __fmul_rn((float)p.z, wk));
    }
    const float r = (float)to_u8(t0), gg = (float)to_u8(t1), b = (float)to_u8(t2);
    const float lum = __fadd_rn(__fadd_rn(__fmul_rn(0.2126f, r), __fmul_rn(0.7152f, gg)), __fmul_rn(0.0722f, b));
    g = (unsigned char)lum;  // NumCast: truncation
  }
  gray[(size_t)oy * W + ox] = g;
  if (gray_f32) gray_f32[(size_t)oy * W + ox] = (float)g;  // convert_image_to_tensor(..).to_kind(Float): raw 0..255
}


// ---- the batched form (ocr_preprocess_batch): one launch over the output tiles of every image of a chunk.
// A tile is kPreTR output rows x kPreTC output columns, one output pixel per lane.  Phase 1 (vertical_sample) runs over the source
// columns the tile's output columns need - `left` and `left + count` are monotone in the output index, so that is one contiguous
// span - and leaves truncated R, G, B in LDS (alpha never reaches the luma); phase 2 (horizontal_sample + luma) reads them back.
// The span is walked in chunks of kPreCH columns, left to right, with every lane's three accumulators in registers across the
// chunks: the taps of a pixel are added in ascending k whatever the ratio (16384 columns may go into one), and the loop runs once
// for ordinary ratios.  The nh x w RGBA intermediate of the two kernels above never exists in HBM.
constexpr int kPreTR = 8, kPreTC = 32, kPreCH = 512;   // 256 lanes; LDS kPreTR * kPreCH * 4 = 16 KiB: eight waves per SIMD
static_assert(kPreTR * kPreTC == 256, "one output pixel per lane");

__global__ __launch_bounds__(256) void preprocess_batch_kernel(const uint32_t* __restrict__ plan, int n_images, int W, int H,
                                                               unsigned char* __restrict__ gray, float* __restrict__ gray_f32) {
  __shared__ uint32_t lds[kPreTR * kPreCH];   // [row][column of the chunk]: R | G << 8 | B << 16 after the vertical pass
  const PreImage* __restrict__ imgs = reinterpret_cast<const PreImage*>(plan);
  // the image of this tile: the last one whose first tile is not after it (uniform: scalar loads)
  const int tile = blockIdx.x;
  int lo = 0, hi = n_images - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (imgs[mid].tile0 <= tile) lo = mid;
    else hi = mid - 1;
  }
  const PreImage im = imgs[lo];
  const int t = tile - im.tile0, tiles_x = (W + kPreTC - 1) / kPreTC;
  const int oy0 = (t / tiles_x) * kPreTR, ox0 = (t % tiles_x) * kPreTC;
  const int tid = threadIdx.x, r = tid / kPreTC, oy = oy0 + r, ox = ox0 + tid % kPreTC;
  const bool inside = oy < H && ox < W;
  const size_t o = ((size_t)im.frame * H + (inside ? oy : 0)) * W + (inside ? ox : 0);
  if (oy0 >= im.nh || ox0 >= im.nw) {   // a tile wholly in the padding right of / below the resized image (image_ops.rs:204-214)
    if (inside) {
      if (gray) gray[o] = 0;
      if (gray_f32) gray_f32[o] = 0.f;
    }
    return;
  }
  const int *ly = reinterpret_cast<const int*>(plan + im.ty), *cy = ly + im.nh;
  const float* wy = reinterpret_cast<const float*>(cy + im.nh);
  const int *lx = reinterpret_cast<const int*>(plan + im.tx), *cx = lx + im.nw;
  const float* wx = reinterpret_cast<const float*>(cx + im.nw);
  const int rows = min(kPreTR, im.nh - oy0), oxl = min(ox0 + kPreTC, im.nw) - 1;
  const int s0 = lx[ox0], s1 = lx[oxl] + cx[oxl];   // the tile's span of source columns
  const bool live = oy < im.nh && ox < im.nw;
  const int l = live ? lx[ox] : 0, c = live ? cx[ox] : 0;
  const float* wk = wx + (size_t)(live ? ox : 0) * im.maxk_x;
  float t0 = 0.f, t1 = 0.f, t2 = 0.f;
  for (int c0 = s0; c0 < s1; c0 += kPreCH) {
    const int cw = min(kPreCH, s1 - c0);
    // vertical_sample of columns [c0, c0 + cw) for the tile's rows; consecutive lanes read consecutive source pixels
    for (int i = tid; i < rows * cw; i += 256) {
      const int rr = i / cw, col = i - rr * cw;
      const int yl = ly[oy0 + rr], yc = cy[oy0 + rr];
      const float* wv = wy + (size_t)(oy0 + rr) * im.maxk_y;
      const unsigned char* p = im.src + (int64_t)yl * im.stride + (int64_t)(c0 + col) * 4;
      float v0 = 0.f, v1 = 0.f, v2 = 0.f;
      for (int k = 0; k < yc; k += 4, p += 4 * im.stride) {
        // four taps' loads in flight, added in ascending k.  A tap past the count is pixel 0 x weight 0: the sums are never
        // negative, and adding +0 to such a sum changes no bit
        uint32_t px[4];
        float w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool on = k + j < yc;
          px[j] = on ? *reinterpret_cast<const uint32_t*>(p + j * im.stride) : 0u;
          w[j] = on ? wv[k + j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v0 = __fadd_rn(v0, __fmul_rn((float)(px[j] & 255u), w[j]));
          v1 = __fadd_rn(v1, __fmul_rn((float)((px[j] >> 8) & 255u), w[j]));
          v2 = __fadd_rn(v2, __fmul_rn((float)((px[j] >> 16) & 255u), w[j]));
        }
      }
      lds[rr * kPreCH + col] = (uint32_t)to_u8(v0) | (uint32_t)to_u8(v1) << 8 | (uint32_t)to_u8(v2) << 16;
    }
    __syncthreads();
    // horizontal_sample: the taps of this lane's pixel that lie in the chunk, k ascending
    const int k0 = max(0, c0 - l), k1 = min(c, c0 + cw - l);
    for (int k = k0; k < k1; ++k) {
      const uint32_t px = lds[r * kPreCH + (l + k - c0)];
      const float w = wk[k];
      t0 = __fadd_rn(t0, __fmul_rn((float)(px & 255u), w));
      t1 = __fadd_rn(t1, __fmul_rn((float)((px >> 8) & 255u), w));
      t2 = __fadd_rn(t2, __fmul_rn((float)((px >> 16) & 255u), w));
    }
    __syncthreads();
  }
  if (!inside) return;
  unsigned char g = 0;
  if (live) {
    const float rf = (float)to_u8(t0), gf = (float)to_u8(t1), bf = (float)to_u8(t2);
    const float lum = __fadd_rn(__fadd_rn(__fmul_rn(0.2126f, rf), __fmul_rn(0.7152f, gf)), __fmul_rn(0.0722f, bf));
    g = (unsigned char)lum;  // NumCast: truncation
  }
  if (gray) gray[o] = g;
  if (gray_f32) gray_f32[o] = (float)g;
}
}  // namespace

void resize_dimensions(int width, int height, int nwidth, int nheight, int* ow, int* oh) {
  const unsigned long long ratio = (unsigned long long)width * nheight, nratio = (unsigned long long)nwidth * height;
  const bool use_width = nratio <= ratio;
  unsigned long long inter = use_width ? (unsigned long long)height * nwidth / width : (unsigned long long)width * nheight / height;
  if (inter < 1) inter = 1;
  *ow = use_width ? nwidth : (int)inter;
  *oh = use_width ? (int)inter : nheight;
}

// rgba_dev: h x w x 4 u8 on the device.  scratch must hold nh*w*4 bytes (tmp) + the tables.
void launch_preprocess(const unsigned char* rgba_dev, int w, int h, int W, int H, unsigned char* gray_dev, float* gray_f32_dev,
                       void* scratch, size_t scratch_bytes, double* adj_xy, hipStream_t s) {
  if (w < 1 || h < 1 || W < 1 || H < 1) fail(OCR_ERR_INVALID, "preprocess: bad dimensions");
  int nw, nh;
  resize_dimensions(w, h, W, H, &nw, &nh);
  const AxisTable ty = build_axis(h, nh), tx = build_axis(w, nw);
  auto al = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t o_tmp = 0, o_ly = al((size_t)nh * w * 4), o_cy = o_ly + al((size_t)nh * 4), o_wy = o_cy + al((size_t)nh * 4);
  const size_t o_lx = o_wy + al(ty.w.size() * 4), o_cx = o_lx + al((size_t)nw * 4), o_wx = o_cx + al((size_t)nw * 4);
  const size_t total = o_wx + al(tx.w.size() * 4);
  if (total > scratch_bytes) fail(OCR_ERR_INTERNAL, "preprocess: scratch of %zu bytes needed, %zu given", total, scratch_bytes);
  char* sc = static_cast<char*>(scratch);
  OCR_HIP(hipMemcpyAsync(sc + o_ly, ty.left.data(), (size_t)nh * 4, hipMemcpyHostToDevice, s));
  OCR_HIP(hipMemcpyAsync(sc + o_cy, ty.count.data(), (size_t)nh * 4, hipMemcpyHostToDevice, s));
  OCR_HIP(hipMemcpyAsync(sc + o_wy, ty.w.data(), ty.w.size() * 4, hipMemcpyHostToDevice, s));
  OCR_HIP(hipMemcpyAsync(sc + o_lx, tx.left.data(), (size_t)nw * 4, hipMemcpyHostToDevice, s));
  OCR_HIP(hipMemcpyAsync(sc + o_cx, tx.count.data(), (size_t)nw * 4, hipMemcpyHostToDevice, s));
  OCR_HIP(hipMemcpyAsync(sc + o_wx, tx.w.data(), tx.w.size() * 4, hipMemcpyHostToDevice, s));
  OCR_HIP(hipStreamSynchronize(s));  // the host tables go out of scope
  hipLaunchKernelGGL(resize_vertical_kernel, dim3((w + 255) / 256, nh), dim3(256), 0, s, reinterpret_cast<const uchar4*>(rgba_dev),
                     reinterpret_cast<uchar4*>(sc + o_tmp), w, nh, reinterpret_cast<const int*>(sc + o_ly),
                     reinterpret_cast<const int*>(sc + o_cy), reinterpret_cast<const float*>(sc + o_wy), ty.maxk);
  OCR_HIP(hipGetLastError());
  hipLaunchKernelGGL(resize_horizontal_luma_kernel, dim3((W + 255) / 256, H), dim3(256), 0, s,
                     reinterpret_cast<const uchar4*>(sc + o_tmp), gray_dev, gray_f32_dev, w, nw, nh, W, H,
                     reinterpret_cast<const int*>(sc + o_lx), reinterpret_cast<const int*>(sc + o_cx),
                     reinterpret_cast<const float*>(sc + o_wx), tx.maxk);
  OCR_HIP(hipGetLastError());
  if (adj_xy) {
    adj_xy[0] = (double)nw / (double)w;  // image_ops.rs:200-202
    adj_xy[1] = (double)nh / (double)h;
  }
}

// The plan of one launch of preprocess_batch_kernel: n PreImage descriptors, then the weight tables they point to (per table:
// left[out], count[out], w[out][maxk]; offsets in 4-byte words from the start of the plan).  A table is built once per distinct
// (in, out) pair of the CALL (PrePlanner::tables) and stored once per plan.
long long PrePlanner::plan(const PreSource* src, int n, int first_frame, std::vector<uint32_t>& blob) {
  static_assert(sizeof(PreImage) % 16 == 0, "descriptors are read as an array");
  const long long tiles_per_image = (long long)((W + kPreTC - 1) / kPreTC) * ((H + kPreTR - 1) / kPreTR);
  blob.assign((size_t)n * sizeof(PreImage) / 4, 0u);
  std::map<std::pair<int, int>, std::pair<uint32_t, int>> placed;   // (in, out) -> word offset in this plan, maxk
  auto place = [&](int in, int out) {
    const std::pair<int, int> key(in, out);
    auto hit = placed.find(key);
    if (hit != placed.end()) return hit->second;
    auto tab = tables.find(key);
    if (tab == tables.end()) tab = tables.emplace(key, build_axis(in, out)).first;
    const AxisTable& t = tab->second;
    if (blob.size() + 2 * (size_t)out + t.w.size() > (size_t)0x7fffffff) fail(OCR_ERR_INVALID, "preprocess_batch: weight tables of more than 8 GiB");
    const uint32_t off = (uint32_t)blob.size();
    blob.insert(blob.end(), t.left.begin(), t.left.end());
    blob.insert(blob.end(), t.count.begin(), t.count.end());
    const uint32_t* w = reinterpret_cast<const uint32_t*>(t.w.data());
    blob.insert(blob.end(), w, w + t.w.size());
    return placed.emplace(key, std::make_pair(off, t.maxk)).first->second;
  };
  for (int i = 0; i < n; ++i) {
    PreImage im{};
    im.src = src[i].dev;
    im.stride = src[i].stride;
    im.w = src[i].w;
    im.h = src[i].h;
    resize_dimensions(im.w, im.h, W, H, &im.nw, &im.nh);
    im.tile0 = (int32_t)(i * tiles_per_image);
    im.frame = first_frame + i;
    const auto ty = place(im.h, im.nh), tx = place(im.w, im.nw);
    im.ty = ty.first;
    im.maxk_y = ty.second;
    im.tx = tx.first;
    im.maxk_x = tx.second;
    std::memcpy(reinterpret_cast<char*>(blob.data()) + (size_t)i * sizeof(PreImage), &im, sizeof im);
  }
  return n * tiles_per_image;
}

int PrePlanner::max_images() const {
  const long long tiles_per_image = (long long)((W + kPreTC - 1) / kPreTC) * ((H + kPreTR - 1) / kPreTR);
  return (int)std::max<long long>(1, std::min<long long>(1 << 20, ((1ll << 31) - 1) / tiles_per_image));
}

void launch_preprocess_batch(const void* plan_dev, int n, long long tiles, int W, int H, unsigned char* gray_dev, float* gray_f32_dev,
                             hipStream_t s) {
  if (n < 1 || tiles < 1 || tiles > 0x7fffffffll) fail(OCR_ERR_INTERNAL, "preprocess_batch: %d images, %lld tiles in one launch", n, tiles);
  hipLaunchKernelGGL(preprocess_batch_kernel, dim3((unsigned)tiles), dim3(256), 0, s, static_cast<const uint32_t*>(plan_dev), n, W, H,
                     gray_dev, gray_f32_dev);
  OCR_HIP(hipGetLastError());
}

size_t preprocess_scratch_bytes(int w, int h, int W, int H) {
  int nw, nh;
  resize_dimensions(w, h, W, H, &nw, &nh);
  // tmp + generous room for the weight tables (support grows with the down-scaling ratio)
  const size_t ky = (size_t)(2.0 * std::max(1.0, (double)h / nh) + 3), kx = (size_t)(2.0 * std::max(1.0, (double)w / nw) + 3);
  return (size_t)nh * w * 4 + (size_t)nh * (ky + 2) * 4 + (size_t)nw * (kx + 2) * 4 + 16 * 256;
}

}  // namespace ocr
