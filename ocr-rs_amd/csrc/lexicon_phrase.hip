// Phrase search: the glyphs of a line segmented into lexicon words and out-of-vocabulary words by one DP (BUILD-DEFINED; rule in
// include/ocr_amd.h at ocr_lexicon_phrase_match, oracle tests/phrase_oracle.py).  f64, every operation separately rounded, adds and
// mins only: this file is compiled with -ffp-contract=off.
//   phrase_raw_kernel    one wave per line: raw(i) of every glyph row (the row minimum by a butterfly in f32, which is exact), their
//                        sum in glyph order, and the check of every cost; the first bad line is kept by atomicMin.
//   phrase_match_kernel  the hot path.  Grid (window of 32 starts, lexicon chunk), 256 threads.  A chunk holds entries of ONE length M
//                        (the host cuts the sorted lexicon at its length boundaries), so the loop over the characters is uniform.
//                        The window's cost rows (up to 63) sit in LDS as rows of 64 floats, folded there; lane l holds one entry and
//                        reads tab[s + k][c_k] for its character k and every start s: 32 f64 accumulators, the starts unrolled in
//                        groups of 4 behind one scalar test, their LDS reads in flight together.  A workgroup makes `span` passes of
//                        256 entries; every lane keeps its best (cost, caller's index) per start.  The 32 minima of a wave come from
//                        32 butterflies by (cost, index), the waves meet in LDS, and the chunk's 32 slots are written (key_less,
//                        wave_argmin and slots_argmin of word_search.hpp, which states the tie rules).
//   phrase_seg_kernel    one thread per (start, M): L(i, M) as the minimum over the chunks of length M by (cost, index) - a total
//                        order, so the chunking does not show -, U and J summed in the association of the rule, T for both kinds.
//   phrase_dp_kernel     one wave per line, lane = kind * 32 + (M - 1): B and the boundary costs in LDS, the segment costs of eight
//                        steps loaded ahead of the steps (they do not depend on B), the arg-min by (v, lane) a butterfly, the
//                        backtrack in lane 0 and the words written out in glyph order by the wave.
// Lines are processed in groups of at most kPhraseGroupWindows windows, so the workspace is bounded whatever the batch.
// LDS: 16 KB table + 1.5 KB of merge slots (match), 5.0 KB (DP).  Registers and scratch: DESIGN.md 3.25 and docs/vmcnt_audit.md.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>

#include "api_internal.hpp"
#include "lexicon_handle.hpp"
#include "lexicon_host.hpp"
#include "word_search.hpp"

namespace ocr {
namespace {

constexpr int kPhraseMaxGlyphs = OCR_PHRASE_MAX_GLYPHS;
constexpr int kPhraseStarts = 32;              // starts per window
constexpr int kPhraseRows = 4;                 // starts per uniform branch
constexpr int kPhraseGroupWindows = 2048;      // windows per group of lines: bounds the workspace
constexpr int kPhraseMaxChunks = 64;           // chunks the lexicon is cut into: at most one more per length than kPhraseMaxChunks / 2
constexpr int kPhraseAhead = 8;                // DP steps whose segment costs are loaded together
static_assert(kPhraseStarts == kLexMaxLen && kPhraseStarts % kPhraseRows == 0, "a window has one start per length, in whole groups");
static_assert(kPhraseMaxGlyphs % kPhraseStarts == 0, "whole windows");

struct PhraseWindow {   // the match kernel's job: the line's first glyph row, its glyph count, the window's first start
  int32_t g0, G, i0, pad;
};
struct PhraseChunk {    // positions [p0, p1) of the sorted lexicon, all of length M
  int32_t p0, p1, M, pad;
};
struct PhraseLine {     // the DP kernel's job: glyph rows [g0, g0 + G), the line's first window in the group, its index in the call
  int32_t g0, G, win0, line;
};

__global__ __launch_bounds__(256) void phrase_raw_kernel(const float* __restrict__ costs, const int32_t* __restrict__ line_off, int n_lines,
                                                         double* __restrict__ raw, double* __restrict__ raw_line, int32_t* __restrict__ bad_line) {
  const int lane = threadIdx.x & 63;
  const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (l >= n_lines) return;   // a whole wave leaves; the kernel has no barrier
  const int g1 = line_off[l + 1];
  double acc = 0.0;
  bool bad = false;
  for (int g = line_off[l]; g < g1; ++g) {
    const float v = row_min_checked(costs, (size_t)g, lane, bad);
    acc = acc + (double)v;
    if (lane == 0) raw[g] = (double)v;
  }
  if (lane == 0) raw_line[l] = acc;
  if (bad) atomicMin(bad_line, l);
}

__global__ __launch_bounds__(kLexChunk) void phrase_match_kernel(const float* __restrict__ costs, const PhraseWindow* __restrict__ windows,
                                                                 const PhraseChunk* __restrict__ chunks, const uint32_t* __restrict__ codes,
                                                                 const int32_t* __restrict__ index, int n_entries, int fold,
                                                                 double* __restrict__ part_cost, int32_t* __restrict__ part_idx) {
  __shared__ float tab[2 * kPhraseStarts][64];   // rows 0..62 are read
  __shared__ double red_c[kLexChunk / 64][kPhraseStarts];
  __shared__ int32_t red_i[kLexChunk / 64][kPhraseStarts];
  const PhraseWindow win = windows[blockIdx.x];
  const PhraseChunk ch = chunks[blockIdx.y];
  const int tid = threadIdx.x, M = ch.M;
  const int left = win.G - win.i0;                              // glyph rows from the window's first start to the end of the line
  const int n_start = min(kPhraseStarts, left - M + 1);         // starts i with i + M <= G
  if (n_start <= 0) return;   // the whole workgroup leaves, before any barrier: phrase_seg_kernel reads no slot of such a pair

  const int n_rows = min(2 * kPhraseStarts - 1, left);
  stage_cost_rows(tab, costs, win.g0 + win.i0, n_rows, fold, tid, kLexChunk);
  __syncthreads();

  double best_c[kPhraseStarts];
  int best_i[kPhraseStarts];
#pragma unroll
  for (int s = 0; s < kPhraseStarts; ++s) {
    best_c[s] = INFINITY;
    best_i[s] = kNoIndex;
  }

  for (int p0 = ch.p0; p0 < ch.p1; p0 += kLexChunk) {
    const bool live = p0 + tid < ch.p1;
    const int e = live ? p0 + tid : ch.p1 - 1;   // a lane past the chunk reads its last entry and keeps nothing
    double acc[kPhraseStarts];
#pragma unroll
    for (int s = 0; s < kPhraseStarts; ++s) acc[s] = 0.0;
    for (int w = 0; 4 * w < M; ++w) {
      const uint32_t word = codes[(size_t)w * n_entries + e];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (4 * w + b < M) {   // uniform: a chunk has one length
          const float* col = &tab[4 * w + b][(word >> (8 * b)) & 0xFF];
#pragma unroll
          for (int s0 = 0; s0 < kPhraseStarts; s0 += kPhraseRows) {
            if (s0 < n_start) {   // uniform: kPhraseRows starts per scalar branch (rows past the line hold what nobody wrote; their
                                  // starts are never kept; s0 + 3 + M - 1 <= 62 stays inside the table)
#pragma unroll
              for (int s = s0; s < s0 + kPhraseRows; ++s) acc[s] = acc[s] + (double)col[s * 64];
            }
          }
        }
      }
    }
    const int ni = index[e];
#pragma unroll
    for (int s = 0; s < kPhraseStarts; ++s) {
      if (live && s < n_start && key_less(acc[s], ni, best_c[s], best_i[s])) {
        best_c[s] = acc[s];
        best_i[s] = ni;
      }
    }
  }

  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int s = 0; s < kPhraseStarts; ++s) {   // the wave's minimum of every start: a butterfly by (cost, index)
    double c = best_c[s];
    int x = best_i[s];
    wave_argmin(c, x);
    if (lane == 0) {
      red_c[wave][s] = c;
      red_i[wave][s] = x;
    }
  }
  __syncthreads();
  if (tid < n_start) {
    double c;
    int x;
    slots_argmin(&red_c[0][tid], &red_i[0][tid], kPhraseStarts, c, x);
    const size_t slot = ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * kPhraseStarts + tid;
    part_cost[slot] = c;
    part_idx[slot] = x;
  }
}

// seg_t[((window * 32 + s) * 32 + (M - 1)) * 2 + kind], seg_e[(window * 32 + s) * 32 + (M - 1)]
__global__ __launch_bounds__(256) void phrase_seg_kernel(const PhraseWindow* __restrict__ windows, int n_windows, int n_chunks,
                                                         const int32_t* __restrict__ chunk_first, const double* __restrict__ part_cost,
                                                         const int32_t* __restrict__ part_idx, const double* __restrict__ raw,
                                                         const float* __restrict__ join, double word_cost, double oov_word_cost,
                                                         double oov_glyph_cost, double* __restrict__ seg_t, int32_t* __restrict__ seg_e) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int w = t >> 10, s = (t >> 5) & 31, M = (t & 31) + 1;
  if (w >= n_windows) return;
  const PhraseWindow win = windows[w];
  const int i = win.i0 + s;
  if (i + M > win.G) return;   // no such segment: the DP never asks for it
  double c = INFINITY;
  int x = kNoIndex;
  for (int k = chunk_first[M]; k < chunk_first[M + 1]; ++k) {
    const size_t slot = ((size_t)w * n_chunks + k) * kPhraseStarts + s;
    const double pc = part_cost[slot];
    const int px = part_idx[slot];
    if (key_less(pc, px, c, x)) {
      c = pc;
      x = px;
    }
  }
  const int r = win.g0 + i;
  double u = oov_word_cost, jn = 0.0;
  for (int k = 0; k < M; ++k) {
    u = u + raw[r + k];
    u = u + oov_glyph_cost;
    if (k > 0) jn = jn + (double)join[r + k];
  }
  const size_t o = (size_t)t;   // ((w * 32 + s) * 32 + M - 1)
  seg_t[2 * o] = (c + word_cost) + jn;
  seg_t[2 * o + 1] = u + jn;
  seg_e[o] = x == kNoIndex ? -1 : x;
}

__global__ __launch_bounds__(64) void phrase_dp_kernel(const PhraseLine* __restrict__ lines, const float* __restrict__ bound,
                                                       const double* __restrict__ seg_t, const int32_t* __restrict__ seg_e,
                                                       int32_t* __restrict__ n_words, double* __restrict__ line_cost,
                                                       int32_t* __restrict__ word_len, int32_t* __restrict__ word_entry,
                                                       double* __restrict__ word_cost) {
  __shared__ double B[kPhraseMaxGlyphs + 1];
  __shared__ double bnd[kPhraseMaxGlyphs];
  __shared__ uint8_t choice[kPhraseMaxGlyphs + 1];
  __shared__ int16_t stk_start[kPhraseMaxGlyphs];
  __shared__ uint8_t stk_choice[kPhraseMaxGlyphs];
  __shared__ int32_t stk_n;
  const PhraseLine ln = lines[blockIdx.x];
  const int lane = threadIdx.x, G = ln.G;
  const int kind = lane >> 5, M = (lane & 31) + 1;
  for (int i = lane; i < G; i += 64) bnd[i] = i > 0 ? (double)bound[ln.g0 + i] : 0.0;
  if (lane == 0) B[0] = 0.0;
  __syncthreads();
  const double* tl = seg_t + (size_t)ln.win0 * kPhraseStarts * kPhraseStarts * 2;   // the line's windows are consecutive: start i at slot i

  for (int j0 = 1; j0 <= G; j0 += kPhraseAhead) {
    double t[kPhraseAhead];
#pragma unroll
    for (int a = 0; a < kPhraseAhead; ++a) {
      const int i = j0 + a - M;
      t[a] = (j0 + a <= G && i >= 0) ? tl[((size_t)i * kPhraseStarts + (M - 1)) * 2 + kind] : INFINITY;
    }
#pragma unroll
    for (int a = 0; a < kPhraseAhead; ++a) {
      const int j = j0 + a;
      if (j <= G) {   // uniform
        const int i = j - M;
        double v = INFINITY;
        if (i >= 0) v = (B[i] + bnd[i]) + t[a];
        int x = lane;
        wave_argmin(v, x);
        if (lane == 0) {
          B[j] = v;
          choice[j] = (uint8_t)x;
        }
        __syncthreads();   // one wave: the barrier orders the LDS write before the next step's reads
      }
    }
  }

  if (lane == 0) {
    int n = 0;
    for (int j = G; j > 0;) {
      const int c = choice[j];
      j -= (c & 31) + 1;
      stk_start[n] = (int16_t)j;
      stk_choice[n] = (uint8_t)c;
      ++n;
    }
    stk_n = n;
    n_words[ln.line] = n;
    line_cost[ln.line] = B[G];
  }
  __syncthreads();
  const int n = stk_n;
  for (int w = lane; w < n; w += 64) {   // word w of the line is entry n - 1 - w of the walk back
    const int i = stk_start[n - 1 - w], c = stk_choice[n - 1 - w];
    const size_t o = ((size_t)ln.win0 * kPhraseStarts + i) * kPhraseStarts + (c & 31);
    word_len[ln.g0 + w] = (c & 31) + 1;
    word_entry[ln.g0 + w] = (c >> 5) ? -1 : seg_e[o];
    word_cost[ln.g0 + w] = seg_t[2 * o + (c >> 5)];
  }
}

void check_phrase_params(const ocr_phrase_params_t& p) {
  // (written so that a NaN is out of range)
  if (!(p.word_cost >= 0 && std::isfinite(p.word_cost)) || !(p.oov_word_cost >= 0 && std::isfinite(p.oov_word_cost)) ||
      !(p.oov_glyph_cost >= 0 && std::isfinite(p.oov_glyph_cost)) || (p.fold_case != 0 && p.fold_case != 1) || p.reserved[0] ||
      p.reserved[1] || p.reserved[2])
    fail(OCR_ERR_INVALID, "lexicon_phrase_match: params word_cost=%g oov_word_cost=%g oov_glyph_cost=%g fold_case=%d reserved=(%d, %d, %d) "
         "(limits: costs finite and >= 0, fold_case 0 | 1, reserved 0)", p.word_cost, p.oov_word_cost, p.oov_glyph_cost, p.fold_case,
         p.reserved[0], p.reserved[1], p.reserved[2]);
}

// The lexicon cut into chunks of one length each: `per` positions a chunk, chosen so that the windows of a group times the chunks give
// a few thousand workgroups and the chunks stay at most kPhraseMaxChunks.  first[M]..first[M + 1] are the chunks of length M.
void plan_chunks(const int32_t* start, int n_entries, int n_windows, std::vector<PhraseChunk>& chunks, int32_t (&first)[kLexMaxLen + 2]) {
  const int want = std::max(1, std::min(kPhraseMaxChunks / 2, 4096 / std::max(n_windows, 1)));
  const int per = std::max(kLexChunk, (int)(((int64_t)n_entries + want - 1) / want + kLexChunk - 1) / kLexChunk * kLexChunk);
  chunks.clear();
  first[0] = 0;
  for (int M = 1; M <= kLexMaxLen; ++M) {
    first[M] = (int32_t)chunks.size();
    for (int p = start[M]; p < start[M + 1]; p += per) chunks.push_back({p, std::min(p + per, start[M + 1]), M, 0});
  }
  first[kLexMaxLen + 1] = (int32_t)chunks.size();
}

struct PhraseOwned {   // the library-owned storage behind an ocr_phrase_matches_t* (released by ocr_phrase_matches_free)
  ocr_phrase_matches_t view{};
  std::vector<int32_t> line_word_offsets, word_offsets, entries, line_flags;
  std::vector<double> word_costs, line_costs, raw_costs;
  void finish(int n_lines, int n_glyphs) {
    view.n_lines = n_lines;
    view.n_words = (int32_t)entries.size();
    view.n_glyphs = n_glyphs;
    view.line_word_offsets = line_word_offsets.data();
    view.word_offsets = word_offsets.data();
    view.entries = entries.data();
    view.word_costs = word_costs.data();
    view.line_costs = line_costs.data();
    view.raw_costs = raw_costs.data();
    view.line_flags = line_flags.data();
  }
};

constexpr int32_t kNone = 0x7F7F7F7F;   // what a byte memset of 0x7F leaves: above every line index

}  // namespace
}  // namespace ocr

extern "C" {

void ocr_phrase_default_params(ocr_phrase_params_t* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->word_cost = 1.0;
  p->oov_word_cost = 6.0;
  p->oov_glyph_cost = 1.0;
  p->fold_case = 1;
}

int ocr_lexicon_phrase_match(ocr_rec_t* rec, const ocr_lexicon_t* lex, const float* costs, int n_glyphs, int mem_kind,
                             const int32_t* line_offsets, int n_lines, const float* bound_cost, const float* join_cost,
                             const ocr_phrase_params_t* params, ocr_phrase_matches_t** out) {
  return ocr::guard([&] {
    using namespace ocr;
    if (!rec || !lex || !line_offsets || !out) fail(OCR_ERR_INVALID, "lexicon_phrase_match: null argument");
    *out = nullptr;
    if (mem_kind != OCR_MEM_HOST && mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "lexicon_phrase_match: mem_kind %d", mem_kind);
    if (lex->device != rec->impl.device())
      fail(OCR_ERR_INVALID, "lexicon_phrase_match: lexicon on device %d, handle on device %d", lex->device, rec->impl.device());
    ocr_phrase_params_t p;
    ocr_phrase_default_params(&p);
    if (params) p = *params;
    check_phrase_params(p);
    if (n_lines < 0 || n_glyphs < 0) fail(OCR_ERR_INVALID, "lexicon_phrase_match: %d lines, %d glyphs", n_lines, n_glyphs);
    if (line_offsets[0] != 0) fail(OCR_ERR_INVALID, "lexicon_phrase_match: line offsets start at %d", line_offsets[0]);
    for (int l = 0; l < n_lines; ++l)
      if (line_offsets[l + 1] < line_offsets[l]) fail(OCR_ERR_INVALID, "lexicon_phrase_match: line offsets decrease at line %d", l);
    if (line_offsets[n_lines] != n_glyphs)
      fail(OCR_ERR_INVALID, "lexicon_phrase_match: line offsets end at %d, not at the %d glyphs", line_offsets[n_lines], n_glyphs);
    if (n_glyphs > 0 && !costs) fail(OCR_ERR_INVALID, "lexicon_phrase_match: null costs");
    if ((bound_cost == nullptr) != (join_cost == nullptr))
      fail(OCR_ERR_INVALID, "lexicon_phrase_match: bound_cost and join_cost are given together or not at all");
    if (bound_cost)
      for (int g = 0; g < n_glyphs; ++g) {
        if (!(bound_cost[g] >= 0.0f && bound_cost[g] <= FLT_MAX)) fail(OCR_ERR_INVALID, "lexicon_phrase_match: bound_cost[%d] is NaN, infinite or negative", g);
        if (!(join_cost[g] >= 0.0f && join_cost[g] <= FLT_MAX)) fail(OCR_ERR_INVALID, "lexicon_phrase_match: join_cost[%d] is NaN, infinite or negative", g);
      }

    std::unique_ptr<PhraseOwned> m(new PhraseOwned());
    const size_t nl = (size_t)n_lines, ng = (size_t)n_glyphs;
    m->line_flags.assign(nl, 0);
    m->line_costs.assign(nl, 0.0);
    m->raw_costs.assign(nl, 0.0);
    m->line_word_offsets.assign(nl + 1, 0);
    if (n_lines == 0) {
      m->word_offsets.assign(1, 0);
      m->finish(0, n_glyphs);
      *out = &m.release()->view;
      return;
    }

    // the groups of lines: every line of 1..256 glyphs has ceil(G / 32) windows, consecutive in its group
    std::vector<PhraseWindow> windows;
    std::vector<PhraseLine> jobs;
    std::vector<int32_t> group_win{0}, group_job{0};   // where every group starts in `windows` and `jobs`
    for (int l = 0; l < n_lines; ++l) {
      const int32_t g0 = line_offsets[l], G = line_offsets[l + 1] - g0;
      if (G == 0) m->line_flags[l] = 1;
      else if (G > kPhraseMaxGlyphs) m->line_flags[l] = 2;
      if (m->line_flags[l]) continue;
      const int nw = (G + kPhraseStarts - 1) / kPhraseStarts;
      if ((int)windows.size() - group_win.back() + nw > kPhraseGroupWindows) {
        group_win.push_back((int32_t)windows.size());
        group_job.push_back((int32_t)jobs.size());
      }
      jobs.push_back({g0, G, (int32_t)windows.size() - group_win.back(), l});
      for (int k = 0; k < nw; ++k) windows.push_back({g0, G, k * kPhraseStarts, 0});
    }
    group_win.push_back((int32_t)windows.size());
    group_job.push_back((int32_t)jobs.size());
    const int n_groups = (int)group_win.size() - 1;
    int max_windows = 0;
    for (int g = 0; g < n_groups; ++g) max_windows = std::max(max_windows, group_win[g + 1] - group_win[g]);
    std::vector<PhraseChunk> chunks;
    int32_t first[kLexMaxLen + 2];
    plan_chunks(lex->host.start, lex->host.n, max_windows, chunks, first);
    const int n_chunks = (int)chunks.size();

    OCR_HIP(hipSetDevice(rec->impl.device()));
    hipStream_t s = rec->impl.stream();
    const size_t cost_bytes = ng * kLexClasses * 4, slots = (size_t)max_windows * n_chunks * kPhraseStarts;
    const size_t segs = (size_t)max_windows * kPhraseStarts * kPhraseStarts;
    Carve c;
    const size_t o_bad = c.take(4), o_cost = c.take(mem_kind == OCR_MEM_HOST ? cost_bytes : 0), o_off = c.take((nl + 1) * 4);
    const size_t o_bound = c.take(ng * 4), o_join = c.take(ng * 4), o_raw = c.take(ng * 8), o_rawl = c.take(nl * 8);
    const size_t o_win = c.take(windows.size() * sizeof(PhraseWindow)), o_jobs = c.take(jobs.size() * sizeof(PhraseLine));
    const size_t o_chunks = c.take(chunks.size() * sizeof(PhraseChunk)), o_first = c.take(sizeof first);
    const size_t o_nw = c.take(nl * 4), o_lc = c.take(nl * 8), o_wl = c.take(ng * 4), o_we = c.take(ng * 4), o_wc = c.take(ng * 8);
    const size_t o_pc = c.take(slots * 8), o_pi = c.take(slots * 4), o_st = c.take(segs * 16), o_se = c.take(segs * 4);
    char* ws = ocr::lex_workspace(rec, c.end);
    int32_t* bad_dev = at<int32_t>(ws, o_bad);
    OCR_HIP(hipMemsetAsync(bad_dev, 0x7F, 4, s));
    const float* cost_dev = costs;
    if (mem_kind == OCR_MEM_HOST && n_glyphs > 0) {
      OCR_HIP(hipMemcpyAsync(ws + o_cost, costs, cost_bytes, hipMemcpyHostToDevice, s));
      cost_dev = at<const float>(ws, o_cost);
    }
    OCR_HIP(hipMemcpyAsync(ws + o_off, line_offsets, (nl + 1) * 4, hipMemcpyHostToDevice, s));
    if (n_glyphs > 0) {
      if (bound_cost) {
        OCR_HIP(hipMemcpyAsync(ws + o_bound, bound_cost, ng * 4, hipMemcpyHostToDevice, s));
        OCR_HIP(hipMemcpyAsync(ws + o_join, join_cost, ng * 4, hipMemcpyHostToDevice, s));
      } else {
        OCR_HIP(hipMemsetAsync(ws + o_bound, 0, ng * 4, s));
        OCR_HIP(hipMemsetAsync(ws + o_join, 0, ng * 4, s));
      }
    }
    hipLaunchKernelGGL(phrase_raw_kernel, dim3((n_lines + 3) / 4), dim3(256), 0, s, cost_dev, at<const int32_t>(ws, o_off), n_lines,
                       at<double>(ws, o_raw), at<double>(ws, o_rawl), bad_dev);
    OCR_HIP(hipGetLastError());
    std::vector<int32_t> nw_host(nl, 0), wl(ng), we(ng);
    std::vector<double> wc(ng);
    if (!jobs.empty()) {
      OCR_HIP(hipMemcpyAsync(ws + o_win, windows.data(), windows.size() * sizeof(PhraseWindow), hipMemcpyHostToDevice, s));
      OCR_HIP(hipMemcpyAsync(ws + o_jobs, jobs.data(), jobs.size() * sizeof(PhraseLine), hipMemcpyHostToDevice, s));
      OCR_HIP(hipMemcpyAsync(ws + o_first, first, sizeof first, hipMemcpyHostToDevice, s));
      if (n_chunks > 0) OCR_HIP(hipMemcpyAsync(ws + o_chunks, chunks.data(), chunks.size() * sizeof(PhraseChunk), hipMemcpyHostToDevice, s));
      const char* d = static_cast<const char*>(lex->dev);
      for (int g = 0; g < n_groups; ++g) {   // in stream order: a group reuses the slots and the segment table of the one before it
        const int nwin = group_win[g + 1] - group_win[g], njob = group_job[g + 1] - group_job[g];
        if (njob == 0) continue;
        const PhraseWindow* win_dev = at<const PhraseWindow>(ws, o_win) + group_win[g];
        if (n_chunks > 0) {
          hipLaunchKernelGGL(phrase_match_kernel, dim3(nwin, n_chunks), dim3(kLexChunk), 0, s, cost_dev, win_dev,
                             at<const PhraseChunk>(ws, o_chunks), reinterpret_cast<const uint32_t*>(d + lex->o_codes),
                             reinterpret_cast<const int32_t*>(d + lex->o_index), lex->host.n, p.fold_case, at<double>(ws, o_pc),
                             at<int32_t>(ws, o_pi));
          OCR_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(phrase_seg_kernel, dim3(nwin * 4), dim3(256), 0, s, win_dev, nwin, n_chunks, at<const int32_t>(ws, o_first),
                           at<const double>(ws, o_pc), at<const int32_t>(ws, o_pi), at<const double>(ws, o_raw),
                           at<const float>(ws, o_join), p.word_cost, p.oov_word_cost, p.oov_glyph_cost, at<double>(ws, o_st),
                           at<int32_t>(ws, o_se));
        OCR_HIP(hipGetLastError());
        hipLaunchKernelGGL(phrase_dp_kernel, dim3(njob), dim3(64), 0, s, at<const PhraseLine>(ws, o_jobs) + group_job[g],
                           at<const float>(ws, o_bound), at<const double>(ws, o_st), at<const int32_t>(ws, o_se), at<int32_t>(ws, o_nw),
                           at<double>(ws, o_lc), at<int32_t>(ws, o_wl), at<int32_t>(ws, o_we), at<double>(ws, o_wc));
        OCR_HIP(hipGetLastError());
      }
      OCR_HIP(hipMemcpyAsync(nw_host.data(), ws + o_nw, nl * 4, hipMemcpyDeviceToHost, s));
      OCR_HIP(hipMemcpyAsync(m->line_costs.data(), ws + o_lc, nl * 8, hipMemcpyDeviceToHost, s));
      OCR_HIP(hipMemcpyAsync(wl.data(), ws + o_wl, ng * 4, hipMemcpyDeviceToHost, s));
      OCR_HIP(hipMemcpyAsync(we.data(), ws + o_we, ng * 4, hipMemcpyDeviceToHost, s));
      OCR_HIP(hipMemcpyAsync(wc.data(), ws + o_wc, ng * 8, hipMemcpyDeviceToHost, s));
    }
    int32_t bad = kNone;
    OCR_HIP(hipMemcpyAsync(&bad, bad_dev, 4, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(m->raw_costs.data(), ws + o_rawl, nl * 8, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipStreamSynchronize(s));
    if (bad != kNone) fail(OCR_ERR_INVALID, "lexicon_phrase_match: line %d has a cost that is NaN, infinite or negative", bad);

    // the words of every line in line order: what the DP wrote at the line's first glyph rows, or the one word of a flagged line
    m->word_offsets.push_back(0);
    for (int l = 0; l < n_lines; ++l) {
      const int32_t g0 = line_offsets[l], G = line_offsets[l + 1] - g0;
      if (m->line_flags[l]) {
        const double cost = m->line_flags[l] == 2 ? INFINITY : 0.0;
        m->word_offsets.push_back(g0 + G);
        m->entries.push_back(-1);
        m->word_costs.push_back(cost);
        m->line_costs[l] = cost;
      } else {
        int32_t g = g0;
        const int32_t n = nw_host[l];
        if (n < 1 || n > G) fail(OCR_ERR_INTERNAL, "lexicon_phrase_match: line %d came back with %d words for %d glyphs", l, n, G);
        for (int w = 0; w < n; ++w) {
          g += wl[(size_t)g0 + w];
          m->word_offsets.push_back(g);
          m->entries.push_back(we[(size_t)g0 + w]);
          m->word_costs.push_back(wc[(size_t)g0 + w]);
        }
        if (g != g0 + G) fail(OCR_ERR_INTERNAL, "lexicon_phrase_match: the words of line %d cover %d of %d glyphs", l, g - g0, G);
      }
      m->line_word_offsets[(size_t)l + 1] = (int32_t)m->entries.size();
    }
    m->finish(n_lines, n_glyphs);
    *out = &m.release()->view;
  });
}

void ocr_phrase_matches_free(ocr_phrase_matches_t* m) {
  if (!m) return;
  delete reinterpret_cast<ocr::PhraseOwned*>(reinterpret_cast<char*>(m) - offsetof(ocr::PhraseOwned, view));
}

}  // extern "C"
