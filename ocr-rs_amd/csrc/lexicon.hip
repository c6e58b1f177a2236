// Lexicon matching: the glyphs of a word read as a whole against a word list (BUILD-DEFINED; rule in include/ocr_amd.h at
// ocr_lexicon_match, oracle tests/lexicon_oracle.py).  f64, every operation separately rounded, adds and mins only: this file is
// compiled with -ffp-contract=off.
//   glyph_cost_kernel   one wave per glyph row: the negative log-softmax in f64, the sum of the exponentials taken in class order by
//                       every lane from LDS (the same value in all of them), one cost per lane.
//   lex_raw_kernel      one wave per word: the greedy reading's cost (the row minimum by a butterfly in f32, which is exact, added in
//                       glyph order in f64) and the check of every cost; the first bad word is kept by atomicMin.
//   lex_match_kernel    grid (word, lexicon chunk), 256 threads.  The word's G x 62 cost table is staged once in LDS as rows of 64
//                       floats (folded there when fold_case is set): lane l reads tab[i][c_l], class c in bank c, equal classes
//                       broadcast, so a read has no bank conflict.  A workgroup makes `span` passes of 256 entries of the word's
//                       candidate range, one entry per lane: the DP column D[0..G] lives in 33 f64 registers (the loop over the
//                       glyphs is unrolled in groups of 4 behind one scalar test of G each, so the LDS reads of a group are in
//                       flight together; the loop over the entry's characters is the lane's own, four
//                       characters per 32-bit load of the position-major code array, 256 bytes per wave).  Every lane keeps its best K
//                       (1 or 8) by the key (cost, caller's index); top_k rounds of a workgroup argmin pop the winners into the
//                       chunk's slots.
//   lex_merge_kernel    one wave per word over the slots of all its chunks (merge_slots of word_search.hpp).
// The key, the best K, the butterfly, the slot read-back, the staging and the checked row minimum are word_search.hpp's, which states
// the tie rules; lexicon_lattice.hip and lexicon_phrase.hip use the same functions.
// LDS: 8 KB table + 384 B of merge slots per workgroup.  Registers and scratch: DESIGN.md 3.19 and docs/vmcnt_audit.md.
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

constexpr int kLexRows = 4;            // glyph rows of the DP column per uniform branch
static_assert(kLexMaxLen % kLexRows == 0, "row groups");

__global__ __launch_bounds__(256) void glyph_cost_kernel(const float* __restrict__ logits, int n, float* __restrict__ costs,
                                                         int32_t* __restrict__ bad_row) {
  __shared__ double ex[4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  const bool live = row < n && lane < kLexClasses;
  const float x = live ? logits[(size_t)row * kLexClasses + lane] : -INFINITY;
  if (live && !(fabsf(x) <= FLT_MAX)) atomicMin(bad_row, row);   // NaN or +-inf
  const float m = wave_max(x);
  ex[wave][lane] = live ? exp((double)x - (double)m) : 0.0;
  __syncthreads();
  double sum = 0.0;
  for (int c = 0; c < kLexClasses; ++c) sum += ex[wave][c];
  const double lse = (double)m + log(sum);
  if (live) costs[(size_t)row * kLexClasses + lane] = (float)fmax(lse - (double)x, 0.0);
}

__global__ __launch_bounds__(256) void lex_raw_kernel(const float* __restrict__ costs, const int32_t* __restrict__ word_off, int n_words,
                                                      double* __restrict__ raw, int32_t* __restrict__ bad_word) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n_words) return;   // a whole wave leaves; the kernel has no barrier
  const int g1 = word_off[w + 1];
  double acc = 0.0;
  bool bad = false;
  for (int g = word_off[w]; g < g1; ++g) {
    acc = acc + (double)row_min_checked(costs, (size_t)g, lane, bad);
  }
  if (lane == 0) raw[w] = acc;
  if (bad) atomicMin(bad_word, w);
}

template <int K>
__global__ __launch_bounds__(kLexChunk) void lex_match_kernel(const float* __restrict__ costs, const LexWordJob* __restrict__ jobs,
                                                              const uint32_t* __restrict__ codes, const uint8_t* __restrict__ lens,
                                                              const int32_t* __restrict__ index, int n_entries, int span, int fold,
                                                              double ins, double del, int top_k, double* __restrict__ part_cost,
                                                              int32_t* __restrict__ part_idx) {
  __shared__ float tab[kLexMaxLen][64];
  __shared__ double red_c[8][4];
  __shared__ int32_t red_i[8][4];
  const LexWordJob job = jobs[blockIdx.x];
  const int G = job.G, tid = threadIdx.x;
  const int base = job.r0 + (int)blockIdx.y * span * kLexChunk;   // (below n_entries <= 2^22 for every chunk that stays)
  if (base >= job.r1) return;   // the whole workgroup leaves, before any barrier: the merge counts the chunks of a word itself

  stage_cost_rows(tab, costs, job.g0, G, fold, tid, kLexChunk);
  __syncthreads();

  double best_c[K];
  int best_i[K];
  best_clear(best_c, best_i);

  for (int pass = 0; pass < span; ++pass) {
    const int p0 = base + pass * kLexChunk;
    if (p0 >= job.r1) break;
    const int e = p0 + tid;
    if (e < job.r1) {
      const int M = lens[e];
      double D[kLexMaxLen + 1];
      D[0] = 0.0;
#pragma unroll
      for (int i = 1; i <= kLexMaxLen; ++i) D[i] = D[i - 1] + del;
      for (int w = 0; 4 * w < M; ++w) {
        const uint32_t word = codes[(size_t)w * n_entries + e];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          if (4 * w + b < M) {
            const float* col = &tab[0][(word >> (8 * b)) & 0xFF];
            double diag = D[0];
            D[0] = diag + ins;
#pragma unroll
            for (int i0 = 1; i0 <= kLexMaxLen; i0 += kLexRows) {
              if (i0 <= G) {   // uniform: kLexRows glyphs per scalar branch, their LDS reads in flight together
#pragma unroll
                for (int i = i0; i < i0 + kLexRows; ++i) {   // (rows past G compute on table rows nobody wrote; D[0..G] never reads them)
                  const double s = (double)col[(i - 1) * 64];
                  const double sub = diag + s;
                  diag = D[i];
                  const double gap = fmin(D[i - 1] + del, diag + ins);
                  D[i] = fmin(sub, gap);
                }
              }
            }
          }
        }
      }
      double nc = D[0];
#pragma unroll
      for (int i = 1; i <= kLexMaxLen; ++i)
        if (i == G) nc = D[i];
      best_insert(best_c, best_i, nc, index[e]);
    }
  }

  const int lane = tid & 63, wave = tid >> 6;
  const size_t slot = ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * top_k;
  for (int r = 0; r < top_k; ++r) {
    double c = best_c[0];
    int x = best_i[0];
    wave_argmin(c, x);
    if (lane == 0) {
      red_c[r][wave] = c;
      red_i[r][wave] = x;
    }
    __syncthreads();   // (a round has slots of its own: one barrier per round)
    slots_argmin(red_c[r], red_i[r], 1, c, x);
    if (tid == 0) {
      part_cost[slot + r] = c;
      part_idx[slot + r] = x == kNoIndex ? -1 : x;
    }
    if (x != kNoIndex && best_i[0] == x) best_pop(best_c, best_i);   // the winner's lane pops it: an index is in one lane only
  }
}

__global__ __launch_bounds__(64) void lex_merge_kernel(const LexWordJob* __restrict__ jobs, int n_chunks, int span, int top_k,
                                                       const double* __restrict__ part_cost, const int32_t* __restrict__ part_idx,
                                                       int32_t* __restrict__ entries, double* __restrict__ out_cost) {
  const LexWordJob job = jobs[blockIdx.x];
  merge_slots(job.r0, job.r1, n_chunks, span, top_k, part_cost, part_idx, entries, out_cost);
}

}  // namespace
}  // namespace ocr

// ---- the C surface of the three calls (include/ocr_amd.h; struct ocr_lexicon: lexicon_handle.hpp)
namespace {
struct MatchesOwned {   // the library-owned storage behind an ocr_lexicon_matches_t* (released by ocr_lexicon_matches_free)
  ocr_lexicon_matches_t view{};
  std::vector<int32_t> entries, n_candidates, word_flags;
  std::vector<double> costs, raw_costs;
  void finish(int n_words, int top_k) {
    view.n_words = n_words;
    view.top_k = top_k;
    view.entries = entries.data();
    view.costs = costs.data();
    view.raw_costs = raw_costs.data();
    view.n_candidates = n_candidates.data();
    view.word_flags = word_flags.data();
  }
};

constexpr int32_t kNone = 0x7F7F7F7F;   // what a byte memset of 0x7F leaves: above every row and word index
}  // namespace

extern "C" {

int ocr_rec_glyph_costs(ocr_rec_t* rec, const float* logits, int n, float* costs, int mem_kind) {
  return ocr::guard([&] {
    using namespace ocr;
    if (!rec || !logits || !costs) fail(OCR_ERR_INVALID, "rec_glyph_costs: null argument");
    if (mem_kind != OCR_MEM_HOST && mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "rec_glyph_costs: mem_kind %d", mem_kind);
    if (n < 0) fail(OCR_ERR_INVALID, "rec_glyph_costs: %d rows", n);
    if (n == 0) return;
    OCR_HIP(hipSetDevice(rec->impl.device()));
    hipStream_t s = rec->impl.stream();
    const size_t bytes = (size_t)n * kLexClasses * 4;
    Carve c;
    const size_t o_bad = c.take(4), o_in = c.take(mem_kind == OCR_MEM_HOST ? bytes : 0), o_out = c.take(mem_kind == OCR_MEM_HOST ? bytes : 0);
    char* ws = ocr::lex_workspace(rec, c.end);
    int32_t* bad_dev = at<int32_t>(ws, o_bad);
    OCR_HIP(hipMemsetAsync(bad_dev, 0x7F, 4, s));
    const float* in = logits;
    float* outp = costs;
    if (mem_kind == OCR_MEM_HOST) {
      OCR_HIP(hipMemcpyAsync(ws + o_in, logits, bytes, hipMemcpyHostToDevice, s));
      in = at<const float>(ws, o_in);
      outp = at<float>(ws, o_out);
    }
    hipLaunchKernelGGL(glyph_cost_kernel, dim3((n + 3) / 4), dim3(256), 0, s, in, n, outp, bad_dev);
    OCR_HIP(hipGetLastError());
    int32_t bad = kNone;
    OCR_HIP(hipMemcpyAsync(&bad, bad_dev, 4, hipMemcpyDeviceToHost, s));
    if (mem_kind == OCR_MEM_HOST) OCR_HIP(hipMemcpyAsync(costs, ws + o_out, bytes, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipStreamSynchronize(s));
    if (bad != kNone) fail(OCR_ERR_INVALID, "rec_glyph_costs: non-finite logit in row %d", bad);
  });
}

int ocr_lexicon_create(ocr_rec_t* rec, const char* bytes, const int32_t* offsets, int n_entries, ocr_lexicon_t** out) {
  return ocr::guard([&] {
    using namespace ocr;
    if (!rec || !out) fail(OCR_ERR_INVALID, "lexicon_create: null argument");
    *out = nullptr;
    std::unique_ptr<ocr_lexicon> lex(new ocr_lexicon());
    lex_pack(bytes, offsets, n_entries, lex->host);
    lex->device = rec->impl.device();
    OCR_HIP(hipSetDevice(lex->device));
    const size_t n = (size_t)n_entries;
    Carve c;
    lex->o_codes = c.take(n * kLexCodeWords * 4);
    lex->o_lens = c.take(n);
    lex->o_index = c.take(n * 4);
    OCR_HIP(hipMalloc(&lex->dev, c.end));
    char* d = static_cast<char*>(lex->dev);
    OCR_HIP(hipMemcpy(d + lex->o_codes, lex->host.codes.data(), n * kLexCodeWords * 4, hipMemcpyHostToDevice));
    OCR_HIP(hipMemcpy(d + lex->o_lens, lex->host.lens.data(), n, hipMemcpyHostToDevice));
    OCR_HIP(hipMemcpy(d + lex->o_index, lex->host.index.data(), n * 4, hipMemcpyHostToDevice));
    std::vector<uint32_t>().swap(lex->host.codes);
    std::vector<uint8_t>().swap(lex->host.lens);
    std::vector<int32_t>().swap(lex->host.index);
    *out = lex.release();
  });
}

int ocr_lexicon_size(const ocr_lexicon_t* lex, int32_t* n_entries) {
  return ocr::guard([&] {
    if (!lex || !n_entries) ocr::fail(OCR_ERR_INVALID, "lexicon_size: null argument");
    *n_entries = lex->host.n;
  });
}

void ocr_lexicon_destroy(ocr_lexicon_t* lex) { delete lex; }

void ocr_lexicon_default_params(ocr_lexicon_params_t* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->ins_cost = 4.0;
  p->del_cost = 4.0;
  p->max_len_diff = 2;
  p->fold_case = 1;
  p->top_k = 1;
}

int ocr_lexicon_match(ocr_rec_t* rec, const ocr_lexicon_t* lex, const float* costs, int n_glyphs, int mem_kind,
                      const int32_t* word_offsets, int n_words, const ocr_lexicon_params_t* params, ocr_lexicon_matches_t** out) {
  return ocr::guard([&] {
    using namespace ocr;
    if (!rec || !lex || !word_offsets || !out) fail(OCR_ERR_INVALID, "lexicon_match: null argument");
    *out = nullptr;
    if (mem_kind != OCR_MEM_HOST && mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "lexicon_match: mem_kind %d", mem_kind);
    if (lex->device != rec->impl.device()) fail(OCR_ERR_INVALID, "lexicon_match: lexicon on device %d, handle on device %d", lex->device, rec->impl.device());
    ocr_lexicon_params_t p;
    ocr_lexicon_default_params(&p);
    if (params) p = *params;
    lex_check_params(p);
    LexPlan plan;
    lex_plan(lex->host.start, word_offsets, n_words, n_glyphs, p.max_len_diff, plan);
    if (n_glyphs > 0 && !costs) fail(OCR_ERR_INVALID, "lexicon_match: null costs");
    std::unique_ptr<MatchesOwned> m(new MatchesOwned());
    const int k = p.top_k;
    const size_t nw = (size_t)n_words;
    m->n_candidates.swap(plan.n_candidates);
    m->word_flags.swap(plan.flags);
    m->entries.assign(nw * k, -1);
    m->costs.assign(nw * k, INFINITY);
    m->raw_costs.assign(nw, 0.0);
    if (n_words == 0) {
      m->finish(0, k);
      *out = &m.release()->view;
      return;
    }
    OCR_HIP(hipSetDevice(rec->impl.device()));
    hipStream_t s = rec->impl.stream();
    const int span = lex_span(n_words, plan.max_range);
    const int per = span * kLexChunk;
    const int n_chunks = plan.max_range > 0 ? (plan.max_range + per - 1) / per : 0;
    const size_t cost_bytes = (size_t)n_glyphs * kLexClasses * 4, slots = nw * (size_t)n_chunks * k;
    Carve c;
    const size_t o_bad = c.take(4), o_cost = c.take(mem_kind == OCR_MEM_HOST ? cost_bytes : 0), o_off = c.take((nw + 1) * 4);
    const size_t o_jobs = c.take(nw * sizeof(LexWordJob)), o_raw = c.take(nw * 8), o_ent = c.take(nw * k * 4), o_oc = c.take(nw * k * 8);
    const size_t o_pc = c.take(slots * 8), o_pi = c.take(slots * 4);
    char* ws = ocr::lex_workspace(rec, c.end);
    int32_t* bad_dev = at<int32_t>(ws, o_bad);
    OCR_HIP(hipMemsetAsync(bad_dev, 0x7F, 4, s));
    const float* cost_dev = costs;
    if (mem_kind == OCR_MEM_HOST && n_glyphs > 0) {
      OCR_HIP(hipMemcpyAsync(ws + o_cost, costs, cost_bytes, hipMemcpyHostToDevice, s));
      cost_dev = at<const float>(ws, o_cost);
    }
    OCR_HIP(hipMemcpyAsync(ws + o_off, word_offsets, (nw + 1) * 4, hipMemcpyHostToDevice, s));
    OCR_HIP(hipMemcpyAsync(ws + o_jobs, plan.jobs.data(), nw * sizeof(LexWordJob), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(lex_raw_kernel, dim3((n_words + 3) / 4), dim3(256), 0, s, cost_dev, at<const int32_t>(ws, o_off), n_words,
                       at<double>(ws, o_raw), bad_dev);
    OCR_HIP(hipGetLastError());
    if (n_chunks > 0) {
      const char* d = static_cast<const char*>(lex->dev);
      const dim3 grid(n_words, n_chunks);
      auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(kLexChunk), 0, s, cost_dev, at<const LexWordJob>(ws, o_jobs),
                           reinterpret_cast<const uint32_t*>(d + lex->o_codes), reinterpret_cast<const uint8_t*>(d + lex->o_lens),
                           reinterpret_cast<const int32_t*>(d + lex->o_index), lex->host.n, span, p.fold_case, p.ins_cost, p.del_cost, k,
                           at<double>(ws, o_pc), at<int32_t>(ws, o_pi));
      };
      if (k == 1) launch(lex_match_kernel<1>);
      else launch(lex_match_kernel<8>);
      OCR_HIP(hipGetLastError());
      hipLaunchKernelGGL(lex_merge_kernel, dim3(n_words), dim3(64), 0, s, at<const LexWordJob>(ws, o_jobs), n_chunks, span, k,
                         at<const double>(ws, o_pc), at<const int32_t>(ws, o_pi), at<int32_t>(ws, o_ent), at<double>(ws, o_oc));
      OCR_HIP(hipGetLastError());
      OCR_HIP(hipMemcpyAsync(m->entries.data(), ws + o_ent, nw * k * 4, hipMemcpyDeviceToHost, s));
      OCR_HIP(hipMemcpyAsync(m->costs.data(), ws + o_oc, nw * k * 8, hipMemcpyDeviceToHost, s));
    }
    int32_t bad = kNone;
    OCR_HIP(hipMemcpyAsync(&bad, bad_dev, 4, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(m->raw_costs.data(), ws + o_raw, nw * 8, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipStreamSynchronize(s));
    if (bad != kNone) fail(OCR_ERR_INVALID, "lexicon_match: word %d has a cost that is NaN, infinite or negative", bad);
    m->finish(n_words, k);
    *out = &m.release()->view;
  });
}

void ocr_lexicon_matches_free(ocr_lexicon_matches_t* m) {
  if (!m) return;
  delete reinterpret_cast<MatchesOwned*>(reinterpret_cast<char*>(m) - offsetof(MatchesOwned, view));
}

}  // extern "C"
