// Wide glyphs cut into pieces at ink minima (BUILD-DEFINED; rule in include/ocr_amd.h at ocr_split_glyphs, oracle
// tests/glyph_split_oracle.py).  All integer; compiled with -ffp-contract=off like its neighbours (the only float is the quantised pixel).
//   split_kernel  one wave per glyph, kSplitGlyphs glyphs per workgroup, no LDS and no barrier.  The host has worked out n (pieces asked
//                 for) per glyph.  n = 1: lane 0 copies the box.  Otherwise, per cut j, the lanes take the columns of the window, count
//                 the ink of their column over the glyph's rows, and one wave minimum over the packed key cnt << 40 | |x - c_j| << 20 |
//                 x names the cut; then, per piece, the lanes take its columns for the first and last ink row.  A glyph's record is
//                 17 ints: the pieces kept, then their boxes; the host scans the records into the block (and applies max_word_pieces).
#include <algorithm>
#include <cstring>
#include <memory>

#include "api_internal.hpp"
#include "glyph_levels.hpp"
#include "lattice_host.hpp"

namespace ocr {
namespace {

using glyph_dev::quantise;
using glyph_dev::wave_max;
using glyph_dev::wave_min;
constexpr int kSplitGlyphs = 4;
constexpr int kSplitRec = 17;

struct SplitJob {
  int frame, x0, y0, x1, y1, t, pol, n;
};

__device__ inline unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    const unsigned long long u = ((unsigned long long)hi << 32) | lo;
    v = u < v ? u : v;
  }
  return v;
}

__global__ __launch_bounds__(kSplitGlyphs * 64) void split_kernel(const float* __restrict__ frames, int H, int W, const SplitJob* __restrict__ jobs,
                                                                  int n_glyphs, int32_t* __restrict__ recs) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * kSplitGlyphs + (threadIdx.x >> 6);
  if (g >= n_glyphs) return;
  const SplitJob jb = jobs[g];
  int32_t* rec = recs + (size_t)g * kSplitRec;
  if (jb.n <= 1) {
    if (lane == 0) {
      rec[0] = 1;
      rec[1] = jb.x0;
      rec[2] = jb.y0;
      rec[3] = jb.x1;
      rec[4] = jb.y1;
    }
    return;
  }
  const float* img = frames + (size_t)jb.frame * H * W;
  const int gw = jb.x1 - jb.x0, n = jb.n;
  int r = gw / (4 * n);
  r = r < 1 ? 1 : r;
  int cut[4];
  cut[0] = jb.x0;
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    cut[j] = jb.x1;
    if (j < n) {   // uniform
      const int c = jb.x0 + (j * gw) / n;
      const int lo = max(c - r, jb.x0 + 1), hi = min(c + r, jb.x1 - 1);
      unsigned long long key = ~0ull;
      for (int x = lo + lane; x <= hi; x += 64) {
        int cnt = 0;
        for (int y = jb.y0; y < jb.y1; ++y) {
          const int q = quantise(img[(size_t)y * W + x]);
          cnt += (jb.pol == 1 ? q <= jb.t : q > jb.t) ? 1 : 0;
        }
        const int d = x < c ? c - x : x - c;
        const unsigned long long k = ((unsigned long long)cnt << 40) | ((unsigned long long)d << 20) | (unsigned)x;
        key = k < key ? k : key;
      }
      key = wave_min_u64(key);
      cut[j] = (int)(key & 0xFFFFF);   // the window is never empty: lo <= c <= hi since x0 < c < x1
    }
  }
  int kept = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < n) {   // uniform
      const int xa = cut[i], xb = i + 1 < n ? cut[i + 1] : jb.x1;
      int lo = INT32_MAX, hi = -1;
      for (int x = xa + lane; x < xb; x += 64)
        for (int y = jb.y0; y < jb.y1; ++y) {
          const int q = quantise(img[(size_t)y * W + x]);
          if (jb.pol == 1 ? q <= jb.t : q > jb.t) {
            lo = min(lo, y);
            hi = max(hi, y);
          }
        }
      lo = wave_min(lo);
      hi = wave_max(hi);
      if (hi >= 0) {   // uniform: a piece without an ink pixel is dropped
        if (lane == 0) {
          rec[1 + 4 * kept] = xa;
          rec[2 + 4 * kept] = lo;
          rec[3 + 4 * kept] = xb;
          rec[4 + 4 * kept] = hi + 1;
        }
        ++kept;
      }
    }
  }
  if (lane == 0) rec[0] = kept;
}

struct PieceMapOwned {   // the library-owned storage behind an ocr_piece_map_t* (released by ocr_piece_map_free)
  ocr_piece_map_t view{};
  std::vector<int32_t> glyph, rank;
};

}  // namespace
}  // namespace ocr

extern "C" {

void ocr_split_default_params(ocr_split_params_t* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->aspect_pct = 100;
  p->max_pieces = 3;
  p->min_piece_w = 3;
  p->max_word_pieces = 32;
}

int ocr_split_glyphs(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_glyphs_t* glyphs,
                     const ocr_split_params_t* params, ocr_glyphs_t** pieces, ocr_piece_map_t** map) {
  return ocr::guard([&] {
    using namespace ocr;
    if (pieces) *pieces = nullptr;
    if (map) *map = nullptr;
    if (!det || !frames || !glyphs || !pieces || !map) fail(OCR_ERR_INVALID, "split_glyphs: null argument");
    if (mem_kind != OCR_MEM_HOST && mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "split_glyphs: mem_kind %d", mem_kind);
    if (n < 0 || h < 1 || w < 1 || h >= (1 << 20) || w >= (1 << 20)) fail(OCR_ERR_INVALID, "split_glyphs: N=%d H=%d W=%d", n, h, w);
    if (glyphs->n_images != n) fail(OCR_ERR_INVALID, "split_glyphs: glyph block holds %d images, frames %d", glyphs->n_images, n);
    ocr_split_params_t p;
    ocr_split_default_params(&p);
    if (params) p = *params;
    split_check_params(p);
    const int nw = glyphs->n_words, ng = glyphs->n_glyphs;
    if (nw < 0 || ng < 0) fail(OCR_ERR_INVALID, "split_glyphs: %d words, %d glyphs", nw, ng);
    if (!glyphs->img_offsets || !glyphs->word_offsets || (nw > 0 && (!glyphs->word_info || !glyphs->word_levels)) || (ng > 0 && !glyphs->boxes))
      fail(OCR_ERR_INVALID, "split_glyphs: null array in the glyph block");
    if (glyphs->word_offsets[0] != 0 || glyphs->word_offsets[nw] != ng) fail(OCR_ERR_INVALID, "split_glyphs: word offsets do not span the glyphs");
    std::vector<SplitJob> jobs;
    jobs.reserve(ng);
    for (int i = 0; i < nw; ++i) {   // every box is checked against the frames: the kernel reads inside them only
      const int32_t* info = glyphs->word_info + 4 * (size_t)i;
      const int k0 = glyphs->word_offsets[i], k1 = glyphs->word_offsets[i + 1];
      if (k1 < k0 || k1 > ng) fail(OCR_ERR_INVALID, "split_glyphs: word %d glyph range [%d, %d)", i, k0, k1);
      if (k1 == k0) continue;
      if (info[0] < 0 || info[0] >= n) fail(OCR_ERR_INVALID, "split_glyphs: word %d on frame %d of %d", i, info[0], n);
      if (info[1] < 0 || info[1] > 254 || info[2] < 1 || info[2] > 2)
        fail(OCR_ERR_INVALID, "split_glyphs: word %d has glyphs, t = %d and polarity %d", i, info[1], info[2]);
      int hw = 0;
      for (int k = k0; k < k1; ++k) {
        const int32_t* b = glyphs->boxes + 4 * (size_t)k;
        if (b[0] < 0 || b[1] < 0 || b[2] > w || b[3] > h || b[0] >= b[2] || b[1] >= b[3])
          fail(OCR_ERR_INVALID, "split_glyphs: glyph %d box (%d, %d, %d, %d) outside the %d x %d frame", k, b[0], b[1], b[2], b[3], w, h);
        hw = std::max(hw, b[3] - b[1]);
      }
      for (int k = k0; k < k1; ++k) {
        const int32_t* b = glyphs->boxes + 4 * (size_t)k;
        const int64_t gw = b[2] - b[0], den = (int64_t)2 * hw * p.aspect_pct;
        int64_t np = (200 * gw + (int64_t)hw * p.aspect_pct) / den;
        np = std::max<int64_t>(1, std::min<int64_t>({np, p.max_pieces, gw / p.min_piece_w}));
        jobs.push_back({info[0], b[0], b[1], b[2], b[3], info[1], info[2], (int)np});
      }
    }
    std::vector<int32_t> rec((size_t)ng * kSplitRec);
    if (ng > 0) {
      OCR_HIP(hipSetDevice(det->impl.device()));
      hipStream_t s = det->impl.stream();
      const size_t jb_bytes = jobs.size() * sizeof(SplitJob), rec_bytes = rec.size() * 4, fr_bytes = (size_t)n * h * w * 4;
      Carve c;
      const size_t o_jb = c.take(jb_bytes), o_rec = c.take(rec_bytes);
      char* sc = static_cast<char*>(det->impl.scratch(1, c.end));
      const float* d_fr = frames;
      if (mem_kind == OCR_MEM_HOST) {
        float* f = static_cast<float*>(det->impl.scratch(0, fr_bytes));
        OCR_HIP(hipMemcpyAsync(f, frames, fr_bytes, hipMemcpyHostToDevice, s));
        d_fr = f;
      }
      OCR_HIP(hipMemcpyAsync(sc + o_jb, jobs.data(), jb_bytes, hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(split_kernel, dim3((ng + kSplitGlyphs - 1) / kSplitGlyphs), dim3(kSplitGlyphs * 64), 0, s, d_fr, h, w,
                         at<const SplitJob>(sc, o_jb), ng, at<int32_t>(sc, o_rec));
      OCR_HIP(hipGetLastError());
      OCR_HIP(hipMemcpyAsync(rec.data(), sc + o_rec, rec_bytes, hipMemcpyDeviceToHost, s));
      OCR_HIP(hipStreamSynchronize(s));
    }
    std::unique_ptr<GlyphsOwned> g(new GlyphsOwned());
    std::unique_ptr<PieceMapOwned> pm(new PieceMapOwned());
    g->img_offsets.assign(glyphs->img_offsets, glyphs->img_offsets + n + 1);
    g->word_info.assign(glyphs->word_info, glyphs->word_info + (size_t)4 * nw);
    g->word_levels.assign(glyphs->word_levels, glyphs->word_levels + (size_t)2 * nw);
    g->word_offsets.push_back(0);
    for (int i = 0; i < nw; ++i) {   // the per-glyph records -> CSR
      const int k0 = glyphs->word_offsets[i], k1 = glyphs->word_offsets[i + 1];
      int64_t total = 0;
      for (int k = k0; k < k1; ++k) {
        const int kept = rec[(size_t)k * kSplitRec];
        if (kept < 0 || kept > 4) fail(OCR_ERR_INTERNAL, "split_glyphs: glyph %d reports %d pieces", k, kept);
        total += kept;
      }
      const bool pass = total > p.max_word_pieces;
      if (pass) g->word_info[4 * (size_t)i + 3] |= 4;
      for (int k = k0; k < k1; ++k) {
        const int32_t* r = &rec[(size_t)k * kSplitRec];
        if (pass) {
          g->boxes.insert(g->boxes.end(), glyphs->boxes + 4 * (size_t)k, glyphs->boxes + 4 * (size_t)k + 4);
          pm->glyph.push_back(k);
          pm->rank.push_back(0);
          continue;
        }
        g->boxes.insert(g->boxes.end(), r + 1, r + 1 + 4 * r[0]);
        for (int q = 0; q < r[0]; ++q) {
          pm->glyph.push_back(k);
          pm->rank.push_back(q);
        }
      }
      g->word_offsets.push_back((int32_t)(g->boxes.size() / 4));
    }
    g->finish();
    pm->view.n_pieces = (int32_t)pm->glyph.size();
    pm->view.glyph = pm->glyph.data();
    pm->view.rank = pm->rank.data();
    *pieces = &g.release()->view;
    *map = &pm.release()->view;
  });
}

void ocr_piece_map_free(ocr_piece_map_t* m) {
  if (!m) return;
  delete reinterpret_cast<ocr::PieceMapOwned*>(reinterpret_cast<char*>(m) - offsetof(ocr::PieceMapOwned, view));
}

}  // extern "C"
