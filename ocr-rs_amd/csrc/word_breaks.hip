// Word breaks inside a polygon: the words of a glyph block re-cut at their inter-word gaps (BUILD-DEFINED; rule in include/ocr_amd.h
// at ocr_break_words, oracle tests/word_break_oracle.py).  All integer except the f64 score of the adaptive rule, every operation of
// which is separately rounded: this file is compiled with -ffp-contract=off, and the f64 divide is correctly rounded on gfx950 (as
// lines.hip relies on).
//   word_break_kernel    one wave per source word, kBreakWaves words per workgroup.  Glyph i sits in lane i % 64, slot i / 64, so the
//                        256 glyphs of the largest word are four registers a lane.  The prefix maximum of x1 and the int64 prefix sums
//                        of the sorted gaps are wave scans (__shfl_up) with a carry across the slots.  Both sorts are rank counts over
//                        an LDS copy of the wave's keys, every lane reading the same key (a broadcast) and comparing it with its four
//                        own by (value, index); the heights need only the element of rank G / 2, the gaps are scattered to their
//                        ranks.  The arg-max of the score is a butterfly over (score, c), ties to the smaller c.
// A wave shares its LDS rows with no other wave and a workgroup passes no barrier: a wave past the last word leaves at once.  The
// kernel decides every break; the host scans the per-glyph records into offsets and copies the block.
#include <climits>
#include <cstddef>
#include <cstring>
#include <memory>

#include "api_internal.hpp"

namespace ocr {
namespace {

constexpr int kBreakWaves = 4;                          // source words per workgroup
constexpr int kBreakSlots = OCR_BREAK_MAX_GLYPHS / 64;  // glyphs per lane
constexpr int kCoordMax = 1 << 22;
static_assert(OCR_BREAK_MAX_GLYPHS % 64 == 0, "slot layout");

struct BreakParams {
  int32_t mode, space_pct, min_space_pct, sep_pct, min_gaps;
};

// rec[g]: -1 when no sub-word starts at glyph g, else the gap_pct in front of it (the first glyph of a source word is -1: the host
// starts a sub-word there anyway).  info[4k..]: hw, rule, threshold, flags.
__global__ __launch_bounds__(kBreakWaves * 64) void word_break_kernel(const int4* __restrict__ boxes, const int32_t* __restrict__ word_off,
                                                                       int n_source, BreakParams p, int32_t* __restrict__ rec,
                                                                       int32_t* __restrict__ info) {
  __shared__ int32_t key_s[kBreakWaves][OCR_BREAK_MAX_GLYPHS];
  __shared__ int32_t sorted_s[kBreakWaves][OCR_BREAK_MAX_GLYPHS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = blockIdx.x * kBreakWaves + wave;
  if (k >= n_source) return;
  int32_t* key = key_s[wave];
  int32_t* sorted = sorted_s[wave];
  const int g0 = word_off[k], G = word_off[k + 1] - g0;
  if (G == 0 || G > OCR_BREAK_MAX_GLYPHS) {   // rule 0
    for (int i = lane; i < G; i += 64) rec[(size_t)g0 + i] = -1;
    if (lane == 0) *reinterpret_cast<int4*>(info + 4 * (size_t)k) = make_int4(0, 0, 0, G > 0 ? 2 : 0);
    return;
  }

  int x0[kBreakSlots], x1[kBreakSlots], h[kBreakSlots];
#pragma unroll
  for (int e = 0; e < kBreakSlots; ++e) {
    const int i = lane + 64 * e;
    x0[e] = x1[e] = h[e] = 0;
    if (i < G) {
      const int4 b = boxes[(size_t)g0 + i];
      x0[e] = b.x;
      x1[e] = b.z;
      h[e] = b.w - b.y;
      key[i] = h[e];
    }
  }
  __builtin_amdgcn_wave_barrier();

  // ---- hw: the height of rank G / 2 by (height, index)
  int rank[kBreakSlots];
#pragma unroll
  for (int e = 0; e < kBreakSlots; ++e) rank[e] = 0;
  for (int j = 0; j < G; ++j) {
    const int v = key[j];
#pragma unroll
    for (int e = 0; e < kBreakSlots; ++e) rank[e] += (v < h[e] || (v == h[e] && j < lane + 64 * e)) ? 1 : 0;
  }
  int hw = 0;   // heights are positive and one glyph has the rank: the maximum over the wave is its height
#pragma unroll
  for (int e = 0; e < kBreakSlots; ++e)
    if (lane + 64 * e < G && rank[e] == G / 2) hw = h[e];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hw = max(hw, __shfl_xor(hw, o, 64));

  // ---- gaps: x0 against the prefix maximum of x1 (coordinates are >= 0: 0 is the identity)
  int gap[kBreakSlots];
  int carry = 0;
#pragma unroll
  for (int e = 0; e < kBreakSlots; ++e) {
    const int i = lane + 64 * e;
    int inc = x1[e];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(inc, o, 64);
      if (lane >= o) inc = max(inc, v);
    }
    inc = max(inc, carry);
    int before = __shfl_up(inc, 1, 64);
    if (lane == 0) before = carry;
    carry = __shfl(inc, 63, 64);
    gap[e] = (i >= 1 && i < G) ? max(0, x0[e] - before) : 0;
  }

  // ---- the fixed rule, and the adaptive rule in front of it
  const int n = G - 1;
  int rule = 1;
  const int64_t fixed_lim = (int64_t)p.space_pct * hw;
  int thr = (int)((fixed_lim + 99) / 100);
  if (p.mode == 1 && n >= p.min_gaps) {   // (uniform over the wave)
    __builtin_amdgcn_wave_barrier();      // the heights have been read
#pragma unroll
    for (int e = 0; e < kBreakSlots; ++e) {
      const int i = lane + 64 * e;
      if (i >= 1 && i < G) key[i - 1] = gap[e];
      rank[e] = 0;
    }
    __builtin_amdgcn_wave_barrier();
    for (int j = 0; j < n; ++j) {
      const int v = key[j];
#pragma unroll
      for (int e = 0; e < kBreakSlots; ++e) rank[e] += (v < gap[e] || (v == gap[e] && j < lane + 64 * e - 1)) ? 1 : 0;
    }
#pragma unroll
    for (int e = 0; e < kBreakSlots; ++e) {
      const int i = lane + 64 * e;
      if (i >= 1 && i < G) sorted[min(rank[e], n - 1)] = gap[e];   // (a rank is below n; the bound keeps a store in its row)
    }
    __builtin_amdgcn_wave_barrier();
    // position c = lane + 64 e of the sorted gaps: S0 = s_0 + .. + s_(c-1) from the inclusive scan
    int64_t below[kBreakSlots];
    int s[kBreakSlots];
    int64_t run = 0;
#pragma unroll
    for (int e = 0; e < kBreakSlots; ++e) {
      const int c = lane + 64 * e;
      s[e] = c < n ? sorted[c] : 0;
      int64_t inc = s[e];
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int64_t v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
      }
      inc += run;
      below[e] = inc - s[e];
      run = __shfl(inc, 63, 64);
    }
    const int64_t total = run;
    double best = 0.0;
    int best_c = 0;   // 0: no valid c
#pragma unroll
    for (int e = 0; e < kBreakSlots; ++e) {   // ascending c, strict improvement: the smaller c keeps a tie
      const int c = lane + 64 * e;
      if (c >= 1 && c < n && sorted[c - 1] < s[e]) {
        const int64_t S0 = below[e], S1 = total - S0, n0 = c, n1 = n - c;
        const double d = (double)(S1 * n0 - S0 * n1);
        const double score = d * d / ((double)n0 * (double)n1);
        if (best_c == 0 || score > best) {
          best = score;
          best_c = c;
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double os = __shfl_xor(best, o, 64);
      const int oc = __shfl_xor(best_c, o, 64);
      if (oc != 0 && (best_c == 0 || os > best || (os == best && oc < best_c))) {
        best = os;
        best_c = oc;
      }
    }
    if (best_c != 0) {
      const int64_t T = sorted[best_c], L = sorted[best_c - 1];
      if (T * 100 >= (int64_t)p.min_space_pct * hw && T * 100 >= (int64_t)p.sep_pct * L) {
        rule = 2;
        thr = (int)T;
      }
    }
  }

#pragma unroll
  for (int e = 0; e < kBreakSlots; ++e) {
    const int i = lane + 64 * e;
    if (i < G) {
      const int64_t g100 = (int64_t)gap[e] * 100;   // (gap <= 2^22: below 2^31)
      const bool brk = i >= 1 && (rule == 2 ? gap[e] >= thr : g100 >= fixed_lim);
      rec[(size_t)g0 + i] = brk ? (int)min(g100 / hw, (int64_t)INT32_MAX) : -1;
    }
  }
  if (lane == 0) *reinterpret_cast<int4*>(info + 4 * (size_t)k) = make_int4(hw, rule, thr, 0);
}

struct WordBreaksOwned {   // the library-owned storage behind an ocr_word_breaks_t* (released by ocr_word_breaks_free)
  ocr_word_breaks_t view{};
  std::vector<int32_t> source, sub_offsets, gap_pct, source_info;
};

}  // namespace
}  // namespace ocr

extern "C" {

void ocr_break_default_params(ocr_break_params_t* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->mode = 1;
  p->space_pct = 35;
  p->min_space_pct = 25;
  p->sep_pct = 200;
  p->min_gaps = 3;
}

int ocr_break_words(ocr_det_t* det, const ocr_glyphs_t* glyphs, const ocr_break_params_t* params, ocr_glyphs_t** words,
                    ocr_word_breaks_t** breaks) {
  return ocr::guard([&] {
    using namespace ocr;
    if (words) *words = nullptr;
    if (breaks) *breaks = nullptr;
    if (!det || !glyphs || !words || !breaks) fail(OCR_ERR_INVALID, "break_words: null argument");
    ocr_break_params_t p;
    ocr_break_default_params(&p);
    if (params) p = *params;
    if (p.mode < 0 || p.mode > 1 || p.space_pct < 1 || p.space_pct > 1000 || p.min_space_pct < 1 || p.min_space_pct > 1000 || p.sep_pct < 100 ||
        p.sep_pct > 1000 || p.min_gaps < 3 || p.min_gaps > 255 || p.reserved[0] || p.reserved[1] || p.reserved[2])
      fail(OCR_ERR_INVALID, "break_words: params mode=%d space_pct=%d min_space_pct=%d sep_pct=%d min_gaps=%d reserved=(%d, %d, %d) (limits: "
           "mode 0..1, space_pct and min_space_pct 1..1000, sep_pct 100..1000, min_gaps 3..255, reserved 0)", p.mode, p.space_pct,
           p.min_space_pct, p.sep_pct, p.min_gaps, p.reserved[0], p.reserved[1], p.reserved[2]);
    const int ni = glyphs->n_images, nw = glyphs->n_words, ng = glyphs->n_glyphs;
    if (ni < 0 || nw < 0 || ng < 0) fail(OCR_ERR_INVALID, "break_words: %d images, %d words, %d glyphs", ni, nw, ng);
    if (!glyphs->img_offsets || !glyphs->word_offsets || (nw > 0 && (!glyphs->word_info || !glyphs->word_levels)) || (ng > 0 && !glyphs->boxes))
      fail(OCR_ERR_INVALID, "break_words: null array in the glyph block");
    if (glyphs->img_offsets[0] != 0 || glyphs->img_offsets[ni] != nw) fail(OCR_ERR_INVALID, "break_words: image offsets do not span the words");
    for (int b = 0; b < ni; ++b)
      if (glyphs->img_offsets[b + 1] < glyphs->img_offsets[b]) fail(OCR_ERR_INVALID, "break_words: image offsets decrease at image %d", b);
    if (glyphs->word_offsets[0] != 0 || glyphs->word_offsets[nw] != ng) fail(OCR_ERR_INVALID, "break_words: word offsets do not span the glyphs");
    for (int k = 0; k < nw; ++k)
      if (glyphs->word_offsets[k + 1] < glyphs->word_offsets[k]) fail(OCR_ERR_INVALID, "break_words: word offsets decrease at word %d", k);
    for (int g = 0; g < ng; ++g) {   // the kernel's int32 differences and int64 sums rest on these bounds
      const int32_t* b = glyphs->boxes + 4 * (size_t)g;
      if (b[0] < 0 || b[1] < 0 || b[2] > kCoordMax || b[3] > kCoordMax || b[0] >= b[2] || b[1] >= b[3])
        fail(OCR_ERR_INVALID, "break_words: glyph %d box (%d, %d, %d, %d) is empty or outside 0..%d", g, b[0], b[1], b[2], b[3], kCoordMax);
    }

    std::vector<int32_t> rec(ng);
    std::unique_ptr<WordBreaksOwned> wb(new WordBreaksOwned());
    wb->source_info.assign((size_t)4 * nw, 0);
    if (ng > 0) {
      OCR_HIP(hipSetDevice(det->impl.device()));
      hipStream_t s = det->impl.stream();
      const size_t box_bytes = (size_t)ng * 16, off_bytes = ((size_t)nw + 1) * 4, rec_bytes = (size_t)ng * 4, info_bytes = (size_t)nw * 16;
      Carve c;
      const size_t o_box = c.take(box_bytes), o_off = c.take(off_bytes), o_rec = c.take(rec_bytes), o_info = c.take(info_bytes);
      char* sc = static_cast<char*>(det->impl.scratch(1, c.end));
      OCR_HIP(hipMemcpyAsync(sc + o_box, glyphs->boxes, box_bytes, hipMemcpyHostToDevice, s));
      OCR_HIP(hipMemcpyAsync(sc + o_off, glyphs->word_offsets, off_bytes, hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(word_break_kernel, dim3((nw + kBreakWaves - 1) / kBreakWaves), dim3(kBreakWaves * 64), 0, s, at<const int4>(sc, o_box),
                         at<const int32_t>(sc, o_off), nw, BreakParams{p.mode, p.space_pct, p.min_space_pct, p.sep_pct, p.min_gaps},
                         at<int32_t>(sc, o_rec), at<int32_t>(sc, o_info));
      OCR_HIP(hipGetLastError());
      OCR_HIP(hipMemcpyAsync(rec.data(), sc + o_rec, rec_bytes, hipMemcpyDeviceToHost, s));
      OCR_HIP(hipMemcpyAsync(wb->source_info.data(), sc + o_info, info_bytes, hipMemcpyDeviceToHost, s));
      OCR_HIP(hipStreamSynchronize(s));
    }

    // the per-glyph records -> sub-word offsets; everything else of the block is copied
    std::unique_ptr<GlyphsOwned> g(new GlyphsOwned());
    g->boxes.assign(glyphs->boxes, glyphs->boxes + (size_t)4 * ng);
    g->img_offsets.assign(1, 0);
    wb->sub_offsets.assign(1, 0);
    int img = 0;
    for (int k = 0; k < nw; ++k) {
      for (; glyphs->img_offsets[img + 1] <= k; ++img) g->img_offsets.push_back((int32_t)wb->source.size());
      const int k0 = glyphs->word_offsets[k], k1 = glyphs->word_offsets[k + 1];
      for (int i = k0; i < k1 || i == k0; ++i) {   // (a source word without glyphs is one sub-word without glyphs)
        const bool first = i == k0;
        if (!first && rec[i] < 0) continue;
        g->word_offsets.push_back(i);
        wb->source.push_back(k);
        wb->gap_pct.push_back(first ? 0 : rec[i]);
        g->word_info.insert(g->word_info.end(), glyphs->word_info + 4 * (size_t)k, glyphs->word_info + 4 * (size_t)k + 4);
        g->word_levels.insert(g->word_levels.end(), glyphs->word_levels + 2 * (size_t)k, glyphs->word_levels + 2 * (size_t)k + 2);
      }
      wb->sub_offsets.push_back((int32_t)wb->source.size());
    }
    for (; img < ni; ++img) g->img_offsets.push_back((int32_t)wb->source.size());
    g->word_offsets.push_back(ng);
    g->finish();
    wb->view.n_source = nw;
    wb->view.n_words = (int32_t)wb->source.size();
    wb->view.source = wb->source.data();
    wb->view.sub_offsets = wb->sub_offsets.data();
    wb->view.gap_pct = wb->gap_pct.data();
    wb->view.source_info = wb->source_info.data();
    *words = &g.release()->view;
    *breaks = &wb.release()->view;
  });
}

void ocr_word_breaks_free(ocr_word_breaks_t* b) {
  if (!b) return;
  delete reinterpret_cast<ocr::WordBreaksOwned*>(reinterpret_cast<char*>(b) - offsetof(ocr::WordBreaksOwned, view));
}

}  // extern "C"
