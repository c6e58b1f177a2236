// Segmentation lattice: the pieces of a word decoded as the cheapest (segmentation, classes) pairs under span cost plus transition cost
// (BUILD-DEFINED; rule in include/ocr_amd.h at ocr_lattice_decode, oracle tests/lattice_oracle.py).  f64, every operation separately
// rounded, adds and mins only: this file is compiled with -ffp-contract=off.
//   lattice_decode_kernel<K>  lm_decode_kernel's shape (char_lm.hip): one wave per word, class c in lane c, kLatWords words per workgroup
//                        which share the model in LDS (lane c reads T[p][c], bank c), the greedy pass first - here the all-singletons
//                        path, and the check of every span row of the word -, the lists of a lane sorted in registers, the previous
//                        lists read by v_readlane under the uniform p, the wave leaving p's list together (__any).
//                        New: a step e first merges L_e[c] out of the last min(M, e) lists A_(e-m)[c] of the same lane (no cross-lane
//                        traffic: candidates arrive in (m, a) order and are inserted behind their equals, the key (value, m, a)), then
//                        relaxes A_e[c] out of L_e[p] once; the up to M later steps that read A_e reuse it.  The ring of the last
//                        4 lists A is a register array with compile-time indices only: it is rotated by moves after every step (96
//                        v_mov at K = 8, against up to 62 x 8 insertions of 8 stages), so nothing goes to scratch.  The ring always
//                        has 4 slots; max_span only bounds the uniform loop over m.
//                        A list entry carries the link (p, r) of its A entry; L_e's link adds m: (m - 1) << 9 | r << 6 | p as uint16,
//                        to a per-call device buffer [piece e - 1][rank][64].  The end is lm_decode_kernel's: top_k rounds of a wave
//                        argmin over (value, c, r), then lane k walks hypothesis k back and stores class and length at the first
//                        piece of every segment.  The butterflies, the list insertion and the f64 readlane are word_search.hpp's.
// LDS: 16 KB per workgroup.  Registers and scratch: DESIGN.md 3.22 and docs/vmcnt_audit.md.
// Also here: ocr_glyph_spans, the C entry of the host-only span table (lattice_host.cpp).
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>

#include "api_internal.hpp"
#include "lattice_host.hpp"
#include "word_search.hpp"

namespace ocr {
namespace {

struct LatSpanCost {
  double v[kLatMaxSpan];
};

template <int K>
__global__ __launch_bounds__(kLatWords * 64) void lattice_decode_kernel(const float* __restrict__ costs, const int32_t* __restrict__ span_off,
                                                                        const int32_t* __restrict__ piece_off, int n_words, int n_pieces,
                                                                        const float* __restrict__ trans, int M, int top_k, LatSpanCost sc,
                                                                        uint16_t* __restrict__ links, int32_t* __restrict__ labels,
                                                                        int32_t* __restrict__ seg_len, int32_t* __restrict__ n_chars,
                                                                        double* __restrict__ out_cost, double* __restrict__ raw,
                                                                        int32_t* __restrict__ bad_word) {
  __shared__ float T[kLmStride][kLmStride];
  for (int t = threadIdx.x; t < kLmStride * kLmStride; t += kLatWords * 64) (&T[0][0])[t] = trans[t];
  __syncthreads();   // the only barrier: whole waves leave behind it
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * kLatWords + (threadIdx.x >> 6);
  if (w >= n_words) return;
  const int s0 = span_off[w], p0 = piece_off[w], G = piece_off[w + 1] - p0;
  const bool cls = lane < kLmClasses;

  // the all-singletons reading and the check of every span row (a word of any length)
  {
    double acc = 0.0;
    int prev = kLmBegin;
    bool bad = false;
    size_t row = (size_t)s0;
    for (int e = 1; e <= G; ++e) {
      const int ms = e < M ? e : M;
      float v = INFINITY;
      if (cls) {
        v = costs[row * kLmClasses + lane];
        bad |= !(v >= 0.0f && v <= FLT_MAX);   // NaN, +-inf or negative
        for (int m = 1; m < ms; ++m) {
          const float u = costs[(row + m) * kLmClasses + lane];
          bad |= !(u >= 0.0f && u <= FLT_MAX);
        }
      }
      int c = lane;
      wave_argmin(v, c);   // the first minimum: by (cost, class)
      acc = acc + (double)T[prev][c];
      acc = acc + sc.v[0];
      acc = acc + (double)v;
      prev = c;
      row += ms;
    }
    if (G > 0) acc = acc + (double)T[prev][kLmEnd];
    if (lane == 0) raw[w] = acc;
    if (bad) atomicMin(bad_word, w);
    if (G < 1 || G > kLatMaxPieces || __any(bad)) {   // uniform: not decoded (labels, lengths and counts were preset)
      if (lane < top_k) out_cost[(size_t)w * top_k + lane] = INFINITY;
      return;
    }
  }

  double rv[kLatMaxSpan][K];   // the ring: rv[d] is the list A_(e-1-d) of class `lane`, values ascending, +inf past its length
  int rc[kLatMaxSpan][K];      // p | r << 6 of the link
#pragma unroll
  for (int d = 0; d < kLatMaxSpan; ++d)
#pragma unroll
    for (int t = 0; t < K; ++t) {
      rv[d][t] = INFINITY;
      rc[d][t] = 0;
    }
  rv[0][0] = (double)T[kLmBegin][lane];
  rc[0][0] = kLmBegin;
  double bv[K];   // L_e of class `lane`
  int bc[K];      // its links: the A entry's p | r << 6, and (m - 1) << 9

  size_t row = (size_t)s0;
  for (int e = 1;; ++e) {
    const int ms = e < M ? e : M;
#pragma unroll
    for (int t = 0; t < K; ++t) {
      bv[t] = INFINITY;
      bc[t] = 0;
    }
#pragma unroll
    for (int m = 1; m <= kLatMaxSpan; ++m) {
      if (m > ms) break;   // uniform
      const double gc = (double)(cls ? costs[(row + (m - 1)) * kLmClasses + lane] : 0.0f);
#pragma unroll
      for (int a = 0; a < K; ++a) {
        if (a >= top_k) break;   // uniform
        const double nv = (rv[m - 1][a] + sc.v[m - 1]) + gc;
        const int nc = rc[m - 1][a] | ((m - 1) << 9);
        if constexpr (K == 1) {
          const bool ins = nv < bv[0];   // the first minimum: m ascends
          bv[0] = ins ? nv : bv[0];
          bc[0] = ins ? nc : bc[0];
        } else {
          list_insert(bv, bc, nv, nc);
        }
      }
    }
    row += ms;
#pragma unroll
    for (int t = 0; t < K; ++t)
      if (t < top_k) links[((size_t)(p0 + e - 1) * top_k + t) * kLmStride + lane] = (uint16_t)bc[t];
    if (e == G) break;   // uniform

    // the ring moves on, and A_e is relaxed out of L_e once
#pragma unroll
    for (int d = kLatMaxSpan - 1; d > 0; --d)
#pragma unroll
      for (int t = 0; t < K; ++t) {
        rv[d][t] = rv[d - 1][t];
        rc[d][t] = rc[d - 1][t];
      }
#pragma unroll
    for (int t = 0; t < K; ++t) {
      rv[0][t] = INFINITY;
      rc[0][t] = 0;
    }
    if constexpr (K == 1) {
      // one value per class: no list to leave early, so the loop is branch-free, in groups of 8 whose LDS reads are in flight together
      auto relax = [&](int p) {
        const double nv = readlane_f64(bv[0], p) + (double)T[p][lane];
        const bool ins = nv < rv[0][0];   // the first minimum: p ascends
        rv[0][0] = ins ? nv : rv[0][0];
        rc[0][0] = ins ? p : rc[0][0];
      };
#pragma unroll 1
      for (int q = 0; q < 56; q += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) relax(q + j);
      }
#pragma unroll
      for (int p = 56; p < kLmClasses; ++p) relax(p);
    }
    for (int p = 0; K > 1 && p < kLmClasses; ++p) {
      const double tr = (double)T[p][lane];
#pragma unroll
      for (int r = 0; r < K; ++r) {
        if (r >= top_k) break;                  // uniform
        const double s = readlane_f64(bv[r], p);
        if (s == INFINITY) break;               // uniform: the end of p's list
        const double nv = s + tr;
        if (!__any(cls && nv < rv[0][K - 1])) break;   // uniform: enters no list, and neither does a later rank
        list_insert(rv[0], rc[0], nv, p | (r << 6));
      }
    }
  }

  const double end = (double)T[cls ? lane : 0][kLmEnd];
#pragma unroll
  for (int t = 0; t < K; ++t) bv[t] = cls ? bv[t] + end : INFINITY;
  int popped = 0, my_c = 0, my_r = 0;
  for (int k = 0; k < top_k; ++k) {
    double v = bv[0];
    int c = lane;
    wave_argmin(v, c);   // by (value, class); the rank is the winner's own
    const int r = __shfl(popped, c, 64);
    if (lane == 0) out_cost[(size_t)w * top_k + k] = v;
    if (lane == k) {
      my_c = c;
      my_r = r;
    }
    if (lane == c) {
#pragma unroll
      for (int t = 0; t + 1 < K; ++t) bv[t] = bv[t + 1];
      bv[K - 1] = INFINITY;
      ++popped;
    }
  }
  __threadfence();   // the links of this wave, written by other lanes, before lane k reads them
  if (lane < top_k) {
    int c = my_c, r = my_r, e = G, n = 0;
    while (e > 0) {
      const int code = links[((size_t)(p0 + e - 1) * top_k + r) * kLmStride + c];
      int m = (code >> 9) + 1;
      m = m < e ? m : e;   // a link never reaches in front of the word: m <= min(M, e) by construction
      const size_t at = (size_t)lane * n_pieces + p0 + (e - m);
      labels[at] = c;
      seg_len[at] = m;
      c = code & 63;
      r = (code >> 6) & 7;
      e -= m;
      ++n;
    }
    n_chars[(size_t)w * top_k + lane] = n;
  }
}

}  // namespace
}  // namespace ocr

// ---- the C surface (include/ocr_amd.h)
namespace {
struct LatticePathsOwned {   // the library-owned storage behind an ocr_lattice_paths_t* (released by ocr_lattice_paths_free)
  ocr_lattice_paths_t view{};
  std::vector<int32_t> labels, seg_len, n_chars, word_flags;
  std::vector<double> costs, raw_costs;
  void finish(int n_words, int top_k, int n_pieces) {
    view.n_words = n_words;
    view.top_k = top_k;
    view.n_pieces = n_pieces;
    view.labels = labels.data();
    view.seg_len = seg_len.data();
    view.n_chars = n_chars.data();
    view.costs = costs.data();
    view.raw_costs = raw_costs.data();
    view.word_flags = word_flags.data();
  }
};
struct SpanTableOwned {   // behind an ocr_span_table_t* (released by ocr_span_table_free)
  ocr_span_table_t view{};
  std::vector<int32_t> span_word, span_end, span_len, piece_offsets;
};
constexpr int32_t kLatNone = 0x7F7F7F7F;   // what a byte memset of 0x7F leaves: above every word index
}  // namespace

extern "C" {

void ocr_lattice_default_params(ocr_lattice_params_t* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->max_span = 2;
  p->top_k = 1;
}

int ocr_glyph_spans(const ocr_glyphs_t* pieces, int max_span, ocr_glyphs_t** spans, ocr_span_table_t** table) {
  return ocr::guard([&] {
    using namespace ocr;
    if (spans) *spans = nullptr;
    if (table) *table = nullptr;
    if (!pieces || !spans || !table) fail(OCR_ERR_INVALID, "glyph_spans: null argument");
    SpanBlock sb;
    lat_spans(*pieces, max_span, sb);
    const int nw = pieces->n_words, ni = pieces->n_images;
    if (ni < 0 || !pieces->img_offsets || (nw > 0 && (!pieces->word_info || !pieces->word_levels)))
      fail(OCR_ERR_INVALID, "glyph_spans: %d images, or a null array in the piece block", ni);
    std::unique_ptr<GlyphsOwned> g(new GlyphsOwned());
    std::unique_ptr<SpanTableOwned> t(new SpanTableOwned());
    g->img_offsets.assign(pieces->img_offsets, pieces->img_offsets + ni + 1);
    g->word_info.assign(pieces->word_info, pieces->word_info + (size_t)4 * nw);
    g->word_levels.assign(pieces->word_levels, pieces->word_levels + (size_t)2 * nw);
    g->word_offsets = sb.span_offsets;
    g->boxes.swap(sb.boxes);
    g->finish();
    t->piece_offsets.assign(pieces->word_offsets, pieces->word_offsets + nw + 1);
    t->span_word.swap(sb.span_word);
    t->span_end.swap(sb.span_end);
    t->span_len.swap(sb.span_len);
    t->view.n_words = nw;
    t->view.n_spans = (int32_t)t->span_word.size();
    t->view.n_pieces = pieces->n_glyphs;
    t->view.max_span = max_span;
    t->view.span_word = t->span_word.data();
    t->view.span_end = t->span_end.data();
    t->view.span_len = t->span_len.data();
    t->view.piece_offsets = t->piece_offsets.data();
    *spans = &g.release()->view;
    *table = &t.release()->view;
  });
}

void ocr_span_table_free(ocr_span_table_t* t) {
  if (!t) return;
  delete reinterpret_cast<SpanTableOwned*>(reinterpret_cast<char*>(t) - offsetof(SpanTableOwned, view));
}

int ocr_lattice_decode(ocr_rec_t* rec, const ocr_char_lm_t* lm, const float* costs, int n_spans, int mem_kind, const int32_t* span_offsets,
                       const int32_t* piece_offsets, int n_words, const ocr_lattice_params_t* params, ocr_lattice_paths_t** out) {
  return ocr::guard([&] {
    using namespace ocr;
    if (!rec || !lm || !span_offsets || !piece_offsets || !out) fail(OCR_ERR_INVALID, "lattice_decode: null argument");
    *out = nullptr;
    if (mem_kind != OCR_MEM_HOST && mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "lattice_decode: mem_kind %d", mem_kind);
    if (lm->device != rec->impl.device())
      fail(OCR_ERR_INVALID, "lattice_decode: model on device %d, handle on device %d", lm->device, rec->impl.device());
    ocr_lattice_params_t p;
    ocr_lattice_default_params(&p);
    if (params) p = *params;
    lat_check_params(p);
    LatPlan plan;
    lat_plan(span_offsets, piece_offsets, n_words, n_spans, p.max_span, p.top_k, plan);
    if (n_spans > 0 && !costs) fail(OCR_ERR_INVALID, "lattice_decode: null costs");
    std::unique_ptr<LatticePathsOwned> m(new LatticePathsOwned());
    const int k = p.top_k, np = plan.n_pieces;
    const size_t nw = (size_t)n_words;
    m->word_flags.swap(plan.flags);
    m->labels.assign(plan.label_count, -1);
    m->seg_len.assign(plan.label_count, 0);
    m->n_chars.assign(nw * k, 0);
    m->costs.assign(nw * k, INFINITY);
    m->raw_costs.assign(nw, 0.0);
    if (n_words == 0) {
      m->finish(0, k, np);
      *out = &m.release()->view;
      return;
    }
    OCR_HIP(hipSetDevice(rec->impl.device()));
    hipStream_t s = rec->impl.stream();
    const size_t cost_bytes = (size_t)n_spans * kLmClasses * 4, lab_bytes = plan.label_count * 4;
    // the outputs lie end to end at the head of the workspace and come home in one copy; both offset arrays go up in one
    Carve c;
    const size_t o_bad = c.take(4), o_raw = c.take(nw * 8), o_oc = c.take(nw * k * 8), o_lab = c.take(lab_bytes), o_nc = c.take(nw * k * 4);
    const size_t o_seg = c.take(lab_bytes), out_bytes = c.end;
    const size_t o_off = c.take(2 * (nw + 1) * 4), o_cost = c.take(mem_kind == OCR_MEM_HOST ? cost_bytes : 0), o_link = c.take(plan.link_bytes);
    char* ws = lex_workspace(rec, c.end);
    int32_t* bad_dev = at<int32_t>(ws, o_bad);
    OCR_HIP(hipMemsetAsync(bad_dev, 0x7F, 4, s));
    if (lab_bytes) OCR_HIP(hipMemsetAsync(ws + o_lab, 0xFF, lab_bytes, s));   // -1: the rows of words that are not decoded, the pieces inside a segment
    OCR_HIP(hipMemsetAsync(ws + o_nc, 0, out_bytes - o_nc, s));                // counts and segment lengths
    const float* cost_dev = costs;
    if (mem_kind == OCR_MEM_HOST && n_spans > 0) {
      OCR_HIP(hipMemcpyAsync(ws + o_cost, costs, cost_bytes, hipMemcpyHostToDevice, s));
      cost_dev = at<const float>(ws, o_cost);
    }
    std::vector<int32_t> offs(span_offsets, span_offsets + nw + 1);
    offs.insert(offs.end(), piece_offsets, piece_offsets + nw + 1);
    OCR_HIP(hipMemcpyAsync(ws + o_off, offs.data(), offs.size() * 4, hipMemcpyHostToDevice, s));
    LatSpanCost sc;
    for (int i = 0; i < kLatMaxSpan; ++i) sc.v[i] = p.span_cost[i];
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(plan.blocks), dim3(kLatWords * 64), 0, s, cost_dev, at<const int32_t>(ws, o_off),
                         at<const int32_t>(ws, o_off) + (nw + 1), n_words, np, lm->dev, p.max_span, k, sc, at<uint16_t>(ws, o_link),
                         at<int32_t>(ws, o_lab), at<int32_t>(ws, o_seg), at<int32_t>(ws, o_nc), at<double>(ws, o_oc), at<double>(ws, o_raw), bad_dev);
    };
    if (k == 1) launch(lattice_decode_kernel<1>);
    else launch(lattice_decode_kernel<8>);
    OCR_HIP(hipGetLastError());
    std::vector<char> home(out_bytes);
    OCR_HIP(hipMemcpyAsync(home.data(), ws, out_bytes, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipStreamSynchronize(s));
    int32_t bad = kLatNone;
    std::memcpy(&bad, home.data() + o_bad, 4);
    std::memcpy(m->raw_costs.data(), home.data() + o_raw, nw * 8);
    std::memcpy(m->costs.data(), home.data() + o_oc, nw * k * 8);
    std::memcpy(m->n_chars.data(), home.data() + o_nc, nw * k * 4);
    if (lab_bytes) {
      std::memcpy(m->labels.data(), home.data() + o_lab, lab_bytes);
      std::memcpy(m->seg_len.data(), home.data() + o_seg, lab_bytes);
    }
    if (bad != kLatNone) fail(OCR_ERR_INVALID, "lattice_decode: word %d has a cost that is NaN, infinite or negative", bad);
    m->finish(n_words, k, np);
    *out = &m.release()->view;
  });
}

void ocr_lattice_paths_free(ocr_lattice_paths_t* p) {
  if (!p) return;
  delete reinterpret_cast<LatticePathsOwned*>(reinterpret_cast<char*>(p) - offsetof(LatticePathsOwned, view));
}

}  // extern "C"
