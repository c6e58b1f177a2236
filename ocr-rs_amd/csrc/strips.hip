// Word strips: every atlas pixel samples its word's rotated rectangle in the frame (BUILD-DEFINED; rule in include/ocr_amd.h at
// ocr_plan_word_strips, oracle tests/strip_oracle.py).  f32, separately rounded: this file is compiled with -ffp-contract=off.
// A gather: one thread per atlas pixel, 256 consecutive columns of one row per workgroup (coalesced stores), four taps from the frames.
// No LDS, no scratch.
#include "common.hpp"

namespace ocr {
namespace {

__global__ __launch_bounds__(256) void strip_kernel(const float* __restrict__ frames, int H, int W, const StripWord* __restrict__ words,
                                                    const int32_t* __restrict__ col_word, int total_width, float* __restrict__ atlas) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= total_width) return;
  const int i = blockIdx.y;
  const StripWord sw = words[col_word[j]];
  const float* img = frames + (size_t)sw.frame * H * W;
  const float fc = (float)(j - sw.c0) + 0.5f, fi = (float)i + 0.5f;
  float sx = ((sw.ox + fc * sw.ux) + fi * sw.vx) - 0.5f;
  float sy = ((sw.oy + fc * sw.uy) + fi * sw.vy) - 0.5f;
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

void launch_word_strips(const float* frames_dev, int H, int W, const StripWord* words_dev, const int32_t* col_word_dev, int height,
                        int total_width, float* atlas_dev, hipStream_t s) {
  if (height <= 0 || total_width <= 0) return;
  hipLaunchKernelGGL(strip_kernel, dim3((total_width + 255) / 256, height), dim3(256), 0, s, frames_dev, H, W, words_dev, col_word_dev,
                     total_width, atlas_dev);
  OCR_HIP(hipGetLastError());
}

}  // namespace ocr
