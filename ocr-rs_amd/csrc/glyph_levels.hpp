// Device code shared by the two glyph segmentation kernels (glyphs.hip segment_kernel, glyph_cc.hip segment_cc_kernel): steps 2-5 of
// the rule in include/ocr_amd.h (quantise, histogram, Otsu, polarity, levels) for one word per 256-thread workgroup.  Both files are
// compiled with -ffp-contract=off.
#pragma once
#include "common.hpp"

namespace ocr {
namespace glyph_dev {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ int quantise(float v) {
  // (int)min(max(v, 0), 255) with NaN -> 0, spelt with comparisons so that no min/max NaN convention enters
  return v >= 0.f ? (v <= 255.f ? (int)v : 255) : 0;
}

__device__ __forceinline__ int wave_min(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// histogram of q over the word box: one 256-bin LDS histogram per wave, integer atomics (order-free).  Every thread of the workgroup
// calls it; the histograms are complete when it returns.
__device__ __forceinline__ void box_histogram(unsigned (*hist)[256], const float* img, int W, const WordBox& wb) {
  const int tid = threadIdx.x, wv = tid >> 6;
  const int bw = wb.x1 - wb.x0, area = bw * (wb.y1 - wb.y0);
  for (int i = tid; i < kWaves * 256; i += kThreads) (&hist[0][0])[i] = 0;
  __syncthreads();
  for (int i = tid; i < area; i += kThreads) {
    const int y = i / bw, x = i - y * bw;
    atomicAdd(&hist[wv][quantise(img[(size_t)(wb.y0 + y) * W + wb.x0 + x])], 1u);
  }
  __syncthreads();
}

// Otsu, polarity and levels from the histograms, by wave 0 (the other waves skip it): lane 0 leaves t (-1: a flat box) and the
// polarity used in *s_t / *s_pol and writes out[0], [1], [2], [4], [5] of the word's record.  The caller synchronises afterwards.
__device__ __forceinline__ void otsu_levels(unsigned (*hist)[256], const WordBox& wb, int polarity, int32_t* out, int* s_t, int* s_pol) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (wv != 0) return;
  // lane owns bins 4*lane .. 4*lane+3: local counts / sums, then an inclusive wave scan of the lane totals
  long long hc[4], hs[4], c = 0, s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int bin = 4 * lane + k;
    hc[k] = (long long)hist[0][bin] + hist[1][bin] + hist[2][bin] + hist[3][bin];
    hs[k] = hc[k] * bin;
    c += hc[k];
    s += hs[k];
  }
  long long ic = c, is = s;
  for (int o = 1; o < 64; o <<= 1) {
    const long long pc = __shfl_up(ic, o), ps = __shfl_up(is, o);
    if (lane >= o) { ic += pc; is += ps; }
  }
  const long long Wt = __shfl(ic, 63), St = __shfl(is, 63);
  long long w0 = ic - c, s0 = is - s;   // exclusive prefix: bins below 4*lane
  double best = -1.0;
  int bt = -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    w0 += hc[k];
    s0 += hs[k];
    const int t = 4 * lane + k;
    const long long w1 = Wt - w0, s1 = St - s0;
    if (t < 255 && w0 > 0 && w1 > 0) {
      const double d = (double)(s1 * w0 - s0 * w1);
      const double sc = (d * d) / ((double)w0 * (double)w1);
      if (sc > best) { best = sc; bt = t; }   // k ascending: ties keep the smaller t
    }
  }
  // argmax over the wave: the higher score, the smaller t on ties (bt = -1 carries best = -1 and never beats a valid t)
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o);
    const int ot = __shfl_xor(bt, o);
    if (ob > best || (ob == best && ot >= 0 && (bt < 0 || ot < bt))) { best = ob; bt = ot; }
  }
  if (lane == 0) {
    int pol = 0;
    float bg = 0.f, ink = 0.f;
    if (bt >= 0) {
      long long W0 = 0, S0 = 0;
      for (int b = 0; b <= bt; ++b) {
        const long long h = (long long)hist[0][b] + hist[1][b] + hist[2][b] + hist[3][b];
        W0 += h;
        S0 += h * b;
      }
      const long long W1 = Wt - W0, S1 = St - S0;
      pol = polarity != 0 ? polarity : (W0 <= W1 ? 1 : 2);
      const float mu0 = (float)((double)S0 / (double)W0), mu1 = (float)((double)S1 / (double)W1);
      bg = pol == 1 ? mu1 : mu0;
      ink = pol == 1 ? mu0 : mu1;
    }
    *s_t = bt;
    *s_pol = pol;
    out[0] = wb.frame;
    out[1] = bt;
    out[2] = pol;
    out[4] = __float_as_int(bg);
    out[5] = __float_as_int(ink);
  }
}

}  // namespace glyph_dev
}  // namespace ocr
