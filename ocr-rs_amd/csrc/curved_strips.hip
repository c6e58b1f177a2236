// Curved strips: every atlas pixel samples its word along the normal of the word's own centreline (BUILD-DEFINED; rule in
// include/ocr_amd.h at ocr_plan_curved_strips, oracle tests/curved_strip_oracle.py).  f32, separately rounded: this file is compiled
// with -ffp-contract=off.  A gather like strip_kernel: one thread per atlas pixel, 256 consecutive columns of one row per workgroup
// (coalesced stores), four taps from the frames.  The two knots of a pixel are 32 consecutive bytes of a table all rows share.
// No LDS, no scratch.
#include "common.hpp"

namespace ocr {
namespace {

__global__ __launch_bounds__(256) void curved_strip_kernel(const float* __restrict__ frames, int H, int W,
                                                           const CurveWord* __restrict__ words, const float4* __restrict__ knots,
                                                           const int32_t* __restrict__ col_word, int height, int total_width,
                                                           float* __restrict__ atlas) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= total_width) return;
  const int i = blockIdx.y;
  const int k = col_word[j];
  const CurveWord cw = words[k];
  const float* img = frames + (size_t)cw.frame * H * W;
  const float t = ((float)(j - cw.c0) + 0.5f) * cw.tscale;
  const int r = max(min((int)t, 31), 0);   // t >= 0 in every planned block; the lower bound keeps a foreign block inside the table
  const float f = t - (float)r;
  const float4 k0 = knots[(size_t)k * 33 + r], k1 = knots[(size_t)k * 33 + r + 1];
  const float px = k0.x + f * (k1.x - k0.x), py = k0.y + f * (k1.y - k0.y);
  const float nx = k0.z + f * (k1.z - k0.z), ny = k0.w + f * (k1.w - k0.w);
  const float o = ((float)i + 0.5f) - 0.5f * (float)height;
  float sx = (px + o * nx) - 0.5f;
  float sy = (py + o * ny) - 0.5f;
  sx = fminf(fmaxf(sx, 0.f), (float)(W - 1));
  sy = fminf(fmaxf(sy, 0.f), (float)(H - 1));
  const int iy0 = (int)floorf(sy), iy1 = min(iy0 + 1, H - 1);
  const float fy = sy - (float)iy0;
  const int ix0 = (int)floorf(sx), ix1 = min(ix0 + 1, W - 1);
  const float fx = sx - (float)ix0;
  const float a = img[(size_t)iy0 * W + ix0], b = img[(size_t)iy0 * W + ix1];
  const float c = img[(size_t)iy1 * W + ix0], d = img[(size_t)iy1 * W + ix1];
  const float top = a + fx * (b - a), bot = c + fx * (d - c);
  atlas[(size_t)i * total_width + j] = top + fy * (bot - top);
}

}  // namespace

void launch_curved_strips(const float* frames_dev, int H, int W, const CurveWord* words_dev, const float* knots_dev,
                          const int32_t* col_word_dev, int height, int total_width, float* atlas_dev, hipStream_t s) {
  if (height <= 0 || total_width <= 0) return;
  hipLaunchKernelGGL(curved_strip_kernel, dim3((total_width + 255) / 256, height), dim3(256), 0, s, frames_dev, H, W, words_dev,
                     reinterpret_cast<const float4*>(knots_dev), col_word_dev, height, total_width, atlas_dev);
  OCR_HIP(hipGetLastError());
}

}  // namespace ocr
