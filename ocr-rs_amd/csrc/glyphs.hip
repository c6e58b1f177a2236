// Glyph segmentation detect -> recognise: every detected word (polygon) is cut into glyph boxes, and every glyph into one 28 x 28
// crop for the single-glyph recogniser.
// BUILD-DEFINED (the reference lists "Character Segmentation" in its pipeline, README.md:20-26, but never built it): the rule is
// written down in include/ocr_amd.h (ocr_segment_glyphs) and restated in tests/glyph_oracle.py; these kernels meet it bit for bit
// (f32 separately rounded: this file is compiled with -ffp-contract=off).
//
// segment_kernel, one 256-thread workgroup per word:
//   1. histogram of q = (int)clamp(v, 0, 255) over the word box: one 256-bin LDS histogram per wave, integer atomics (order-free);
//   2. wave 0 runs Otsu: prefix sums over the 256 bins (4 per lane + a wave scan), the f64 score per t, argmax -> smaller t on ties
//      (1 and 2 live in glyph_levels.hpp, shared with glyph_cc.hip);
//   3. column profile, CHUNK columns at a time: per column the ink count and the first / last ink row, accumulated in registers over a
//      row slice and merged with LDS atomics (min / max / add: order-free);
//   4. wave 0 finds the spans of the chunk with a ballot per 64 columns; a span open at the chunk's end carries over.  Per span the
//      pixel count and row extent are masked wave reductions over its columns;
//   5. results go to a fixed record per word (max_glyphs slots); the host compacts the records into CSR.
//   The box is read from the frame once per pass (histogram, profile): words are small next to the frame and stay in the caches, so
//   no u8 copy of the box is staged in LDS.
// glyph_crop_kernel, one 256-thread workgroup per glyph: 784 bilinear samples of the normalised word levels, written to the caller's
// buffer.  glyph_crop_masked_kernel (ocr_extract_glyph_crops_masked) is the same sampling with a tap that first asks the word's label
// plane (glyph_cc.hip) whose ink the pixel is: a kerned neighbour's ink inside the glyph's box reads as background.
// Out of scope of the rule: touching or kerned glyphs (they stay one glyph), rotated or curved words (the word box is axis-aligned and
// pixels are not masked by the polygon), lexicons.  Spaces inside a polygon are word_breaks.hip's, on the block this rule returns.
#include "common.hpp"
#include "glyph_levels.hpp"

namespace ocr {
namespace {

using glyph_dev::kThreads;
using glyph_dev::kWaves;
using glyph_dev::quantise;
using glyph_dev::wave_max;
using glyph_dev::wave_min;
using glyph_dev::wave_sum;
constexpr int kChunk = 1024;   // columns of the profile held in LDS at a time
constexpr int kMaxSlots = 256;

__global__ __launch_bounds__(kThreads) void segment_kernel(const float* __restrict__ frames, int H, int W, const WordBox* __restrict__ words,
                                                           GlyphSegParams prm, int32_t* __restrict__ rec) {
  __shared__ unsigned hist[kWaves][256];
  __shared__ int ccnt[kChunk], cmin[kChunk], cmax[kChunk];
  __shared__ int s_t, s_pol;
  __shared__ int4 s_box[kMaxSlots];
  __shared__ int s_nkept, s_trunc;

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const WordBox wb = words[blockIdx.x];
  const float* img = frames + (size_t)wb.frame * H * W;
  const int bw = wb.x1 - wb.x0;
  int32_t* out = rec + (size_t)blockIdx.x * glyph_record_ints(prm.max_glyphs);

  glyph_dev::box_histogram(hist, img, W, wb);
  glyph_dev::otsu_levels(hist, wb, prm.polarity, out, &s_t, &s_pol);
  __syncthreads();
  const int t = s_t, pol = s_pol;
  if (t < 0) {   // flat box: no glyphs
    if (tid == 0) { out[3] = 0; out[6] = 0; }
    return;
  }

  // span scan state (meaningful in wave 0 only; uniform across its lanes)
  bool open = false;
  int xs = 0, pix = 0, ylo = 0x7fffffff, yhi = -1, nkept = 0, trunc = 0;
  auto close_span = [&](int xe) {
    if (pix >= prm.min_glyph_pixels) {
      if (nkept < prm.max_glyphs) {
        if (lane == 0) s_box[nkept] = make_int4(xs, ylo, xe, yhi + 1);
        ++nkept;
      } else {
        trunc = 1;
      }
    }
    open = false;
  };

  for (int c0 = 0; c0 < bw && !trunc; c0 += kChunk) {
    const int cw = min(kChunk, bw - c0);
    for (int i = tid; i < cw; i += kThreads) { ccnt[i] = 0; cmin[i] = 0x7fffffff; cmax[i] = -1; }
    __syncthreads();
    // work item = (column, row slice): narrow chunks split their rows over several threads
    const int rg = max(1, kThreads / cw);
    for (int it = tid; it < cw * rg; it += kThreads) {
      const int cx = it % cw, r = it / cw;
      const float* colp = img + wb.x0 + c0 + cx;
      int n = 0, lo = 0x7fffffff, hi = -1;
      for (int y = wb.y0 + r; y < wb.y1; y += rg) {
        const int q = quantise(colp[(size_t)y * W]);
        const bool inkp = pol == 1 ? q <= t : q > t;
        if (inkp) { ++n; lo = min(lo, y); hi = y; }
      }
      if (n) {
        atomicAdd(&ccnt[cx], n);
        atomicMin(&cmin[cx], lo);
        atomicMax(&cmax[cx], hi);
      }
    }
    __syncthreads();
    if (wv == 0) {
      for (int b0 = 0; b0 < cw && !trunc; b0 += 64) {
        const int cx = b0 + lane;
        const bool valid = cx < cw;
        const int n = valid ? ccnt[cx] : 0;
        const bool inkc = valid && n >= prm.min_col_ink;
        const unsigned long long m = __ballot(inkc);
        const unsigned long long vmask = cw - b0 >= 64 ? ~0ull : ((1ull << (cw - b0)) - 1);
        const int lo = inkc ? cmin[cx] : 0x7fffffff, hi = inkc ? cmax[cx] : -1;
        // events in lane order: a start where an ink column follows a non-ink one, an end where a non-ink column follows ink
        const unsigned long long prev = (m << 1) | (open ? 1ull : 0ull);
        unsigned long long starts = m & ~prev, ends = ~m & prev & vmask;
        int seg = 0;   // first lane of the open span inside this block
        while ((starts | ends) && !trunc) {
          const int ls = starts ? __builtin_ctzll(starts) : 64, le = ends ? __builtin_ctzll(ends) : 64;
          if (ls < le) {
            open = true;
            xs = wb.x0 + c0 + b0 + ls;
            pix = 0; ylo = 0x7fffffff; yhi = -1;
            seg = ls;
            starts &= starts - 1;
          } else {
            const bool in = lane >= seg && lane < le;
            pix += wave_sum(in ? n : 0);
            ylo = min(ylo, wave_min(in ? lo : 0x7fffffff));
            yhi = max(yhi, wave_max(in ? hi : -1));
            close_span(wb.x0 + c0 + b0 + le);
            ends &= ends - 1;
          }
        }
        if (open && !trunc) {   // the span runs on past this block: fold in its lanes here
          const bool in = lane >= seg;
          pix += wave_sum(in ? n : 0);
          ylo = min(ylo, wave_min(in ? lo : 0x7fffffff));
          yhi = max(yhi, wave_max(in ? hi : -1));
        }
      }
      if (c0 + cw == bw && open && !trunc) close_span(wb.x1);
      if (lane == 0) { s_nkept = nkept; s_trunc = trunc; }
    }
    __syncthreads();
    // every thread needs the stop flag of the chunk loop
    trunc = s_trunc;
  }
  __syncthreads();
  const int nk = s_nkept;
  for (int k = tid; k < nk; k += kThreads) {
    const int4 b = s_box[k];
    out[8 + 4 * k] = b.x;
    out[8 + 4 * k + 1] = b.y;
    out[8 + 4 * k + 2] = b.z;
    out[8 + 4 * k + 3] = b.w;
  }
  if (tid == 0) {
    out[3] = s_trunc;
    out[6] = nk;
  }
}

__device__ __forceinline__ float level(const float* img, int W, int x, int y, const GlyphJob& g, float den) {
  if (x < g.x0 || x >= g.x1 || y < g.y0 || y >= g.y1) return 0.f;
  const float r = (img[(size_t)y * W + x] - g.bg) / den;
  return r > 0.f ? (r < 1.f ? r : 1.f) : 0.f;   // NaN -> 0, -0 -> +0
}

// the 784 samples of one glyph, shared by both crop kernels: tap(x, y) is the level of frame pixel (x, y)
template <class Tap>
__device__ __forceinline__ void sample_crop(const GlyphJob& g, int glyph_box, int ink_high, float* __restrict__ crop, Tap tap) {
  const float s = (float)max(g.x1 - g.x0, g.y1 - g.y0) / (float)glyph_box;
  const float cx = (float)(g.x0 + g.x1) * 0.5f, cy = (float)(g.y0 + g.y1) * 0.5f;
  for (int o = threadIdx.x; o < 784; o += kThreads) {
    const int i = o / 28, j = o - i * 28;
    const float sy = (cy + (((float)i + 0.5f) - 14.0f) * s) - 0.5f;
    const float sx = (cx + (((float)j + 0.5f) - 14.0f) * s) - 0.5f;
    const float fsy = floorf(sy), fsx = floorf(sx);
    const int iy0 = (int)fsy, ix0 = (int)fsx;
    const float fy = sy - (float)iy0, fx = sx - (float)ix0;
    const float a = tap(ix0, iy0), b = tap(ix0 + 1, iy0);
    const float c = tap(ix0, iy0 + 1), d = tap(ix0 + 1, iy0 + 1);
    const float top = a + fx * (b - a), bot = c + fx * (d - c);
    const float v = top + fy * (bot - top);
    crop[o] = ink_high ? v : 1.0f - v;
  }
}

__global__ __launch_bounds__(kThreads) void glyph_crop_kernel(const float* __restrict__ frames, int H, int W, const GlyphJob* __restrict__ jobs,
                                                              int glyph_box, int ink_high, float* __restrict__ crops) {
  const GlyphJob g = jobs[blockIdx.x];
  const float* img = frames + (size_t)g.frame * H * W;
  const float den = g.ink - g.bg;
  sample_crop(g, glyph_box, ink_high, crops + (size_t)blockIdx.x * 784, [&](int x, int y) { return level(img, W, x, y, g, den); });
}

// The masked tap (include/ocr_amd.h, ocr_extract_glyph_crops_masked): integer tests on the word's label plane in front of level(), so
// whatever passes them is level()'s f32, bit for bit.  The glyph box lies inside the word box (the host checks it), so a pixel that
// passed level()'s box test has a label; its neighbours may lie outside the word box and read as 0.
__device__ __forceinline__ float masked_level(const float* img, int W, int x, int y, const GlyphMaskJob& j, float den, int halo) {
  const GlyphJob& g = j.g;
  if (x < g.x0 || x >= g.x1 || y < g.y0 || y >= g.y1) return 0.f;
  const int bw = j.wx1 - j.wx0, m = j.m;
  const uint16_t* row = j.plane + (size_t)(y - j.wy0) * bw + (x - j.wx0);   // the label of (x, y)
  const int l = *row;
  if (l != 0 && l != m) return 0.f;
  if (l == 0 && halo) {
    bool foreign = false, own = false;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if (dx == 0 && dy == 0) continue;
        const int nx = x + dx, ny = y + dy;
        if (nx < j.wx0 || nx >= j.wx1 || ny < j.wy0 || ny >= j.wy1) continue;
        const int v = row[dy * bw + dx];
        foreign |= v != 0 && v != m;
        own |= v == m;
      }
    if (foreign && !own) return 0.f;
  }
  return level(img, W, x, y, g, den);
}

__global__ __launch_bounds__(kThreads) void glyph_crop_masked_kernel(const float* __restrict__ frames, int H, int W,
                                                                     const GlyphMaskJob* __restrict__ jobs, int glyph_box, int ink_high, int halo,
                                                                     float* __restrict__ crops) {
  const GlyphMaskJob j = jobs[blockIdx.x];
  const float* img = frames + (size_t)j.g.frame * H * W;
  const float den = j.g.ink - j.g.bg;
  sample_crop(j.g, glyph_box, ink_high, crops + (size_t)blockIdx.x * 784, [&](int x, int y) { return masked_level(img, W, x, y, j, den, halo); });
}

}  // namespace

void launch_segment(const float* frames_dev, int H, int W, const WordBox* words_dev, int n_words, const GlyphSegParams& p,
                    int32_t* records_dev, hipStream_t s) {
  if (n_words <= 0) return;
  hipLaunchKernelGGL(segment_kernel, dim3(n_words), dim3(kThreads), 0, s, frames_dev, H, W, words_dev, p, records_dev);
  OCR_HIP(hipGetLastError());
}

void launch_glyph_crops(const float* frames_dev, int H, int W, const GlyphJob* jobs_dev, int n_glyphs, int glyph_box, int ink_high,
                        float* crops_dev, hipStream_t s) {
  if (n_glyphs <= 0) return;
  hipLaunchKernelGGL(glyph_crop_kernel, dim3(n_glyphs), dim3(kThreads), 0, s, frames_dev, H, W, jobs_dev, glyph_box, ink_high, crops_dev);
  OCR_HIP(hipGetLastError());
}

void launch_glyph_crops_masked(const float* frames_dev, int H, int W, const GlyphMaskJob* jobs_dev, int n_glyphs, int glyph_box, int ink_high,
                               int halo, float* crops_dev, hipStream_t s) {
  if (n_glyphs <= 0) return;
  hipLaunchKernelGGL(glyph_crop_masked_kernel, dim3(n_glyphs), dim3(kThreads), 0, s, frames_dev, H, W, jobs_dev, glyph_box, ink_high, halo,
                     crops_dev);
  OCR_HIP(hipGetLastError());
}

}  // namespace ocr
