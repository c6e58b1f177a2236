// Joint lexicon and lattice search: the entries of a lexicon matched over the pieces of a word, a character reading a span of 1..M
// pieces (BUILD-DEFINED; rule in include/ocr_amd.h at ocr_lexicon_lattice_match, oracle tests/lexicon_lattice_oracle.py).  f64, every
// operation separately rounded, adds and mins only: this file is compiled with -ffp-contract=off.
//   lexlat_raw_kernel         one wave per word: the check of every span row and F, the cheapest free segmentation with every span
//                             read as its cheapest class (the row minimum by a butterfly in f32, which is exact; the last four F in
//                             scalars, so a word of any length is summed).
//   lexlat_match_kernel<K, MS, ZS>  lex_match_kernel's shape (lexicon.hip): grid (word, lexicon chunk), 256 threads, one entry per lane,
//                             the sorted codes / lens / index arrays of the lexicon read unchanged.  The word's table in LDS is its
//                             span rows (up to 122 rows of 64 floats, folded while staging, class c in bank c); with max_span a
//                             template parameter the row of span (i, m) is a compile-time offset from the lane's column pointer.
//                             The DP column D[0..G] lives in 33 f64 registers and is updated in place: the old values
//                             D[i-1..i-4][j-1] are carried in four scalars.  Rows are unrolled in groups of 4 behind one scalar
//                             test of G, so the up to 16 LDS reads of a group are in flight together.  Per-lane best K (1 or 8) by
//                             (cost, caller's index), then top_k rounds of a workgroup argmin into the chunk's slots: the functions
//                             lex_match_kernel calls (word_search.hpp, which states the tie rules).
//   lexlat_merge_kernel       one wave per word over the slots of its chunks (merge_slots of word_search.hpp, as lex_merge_kernel).
//   lexlat_trace_kernel       one wave per returned (word, rank): finds the entry's sorted position (lane L searches the bucket of
//                             length L for the caller's index, which ascends inside a bucket), stages the word's span rows, builds the
//                             full table in LDS along anti-diagonals with row i in lane i, and lane 0 walks it back by the rule's
//                             order.  D[G][L] goes home beside the match kernel's cost: the call holds them equal bit for bit.
// LDS: 31 232 B table + 384 B of merge slots (match), 31 232 B + 8 976 B table + 128 B (trace).  Registers and scratch: DESIGN.md
// 3.23 and docs/vmcnt_audit.md.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>
#include <type_traits>

#include "api_internal.hpp"
#include "lexicon_handle.hpp"
#include "lexicon_lattice_host.hpp"
#include "word_search.hpp"

namespace ocr {
namespace {

constexpr int kRowsPerBranch = 4;     // piece rows of the DP column per uniform branch
static_assert(kLexMaxLen % kRowsPerBranch == 0, "row groups");

struct LexLatSpanCost {
  double v[kLatMaxSpan];
};

// the spans of a word's first e pieces: sum over e' = 1..e of min(M, e') (lat_span_count, for the device)
__host__ __device__ constexpr int lexlat_rows(int e, int M) { return e <= M ? e * (e + 1) / 2 : M * (M + 1) / 2 + (e - M) * M; }

__global__ __launch_bounds__(256) void lexlat_raw_kernel(const float* __restrict__ costs, const int32_t* __restrict__ span_off,
                                                         const int32_t* __restrict__ piece_off, int n_words, int M, LexLatSpanCost sc,
                                                         double* __restrict__ raw, int32_t* __restrict__ bad_word) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n_words) return;   // a whole wave leaves; the kernel has no barrier
  const int G = piece_off[w + 1] - piece_off[w];
  size_t row = (size_t)span_off[w];
  double f1 = 0.0, f2 = INFINITY, f3 = INFINITY, f4 = INFINITY;   // F[e-1] .. F[e-4]
  bool bad = false;
  for (int e = 1; e <= G; ++e) {
    const int ms = e < M ? e : M;
    double best = INFINITY;
#pragma unroll
    for (int m = 1; m <= kLatMaxSpan; ++m) {
      if (m <= ms) {   // uniform
        const float v = row_min_checked(costs, row + (m - 1), lane, bad);
        const double f = m == 1 ? f1 : m == 2 ? f2 : m == 3 ? f3 : f4;
        best = fmin(best, (f + sc.v[m - 1]) + (double)v);
      }
    }
    row += ms;
    f4 = f3;
    f3 = f2;
    f2 = f1;
    f1 = best;
  }
  if (lane == 0) raw[w] = f1;
  if (bad) atomicMin(bad_word, w);
}

// ZS: every span_cost[0..MS-1] of the call is zero.  x + 0.0 = x in every bit for the x >= +0.0 (and +inf) of this table, so the add is
// left out, not rounded differently: with the default parameters a cell then takes the adds of lex_match_kernel's plus one per span.
template <int K, int MS, bool ZS>
__global__ __launch_bounds__(kLexChunk) void lexlat_match_kernel(const float* __restrict__ costs, const LexLatJob* __restrict__ jobs,
                                                                 const uint32_t* __restrict__ codes, const uint8_t* __restrict__ lens,
                                                                 const int32_t* __restrict__ index, int n_entries, int span, int fold,
                                                                 double ins, double del, LexLatSpanCost sc, int top_k,
                                                                 double* __restrict__ part_cost, int32_t* __restrict__ part_idx) {
  __shared__ float tab[kLexLatMaxRows][64];
  __shared__ double red_c[8][4];
  __shared__ int32_t red_i[8][4];
  const LexLatJob job = jobs[blockIdx.x];
  const int G = job.G, tid = threadIdx.x;
  const int base = job.r0 + (int)blockIdx.y * span * kLexChunk;   // (below n_entries <= 2^22 for every chunk that stays)
  if (base >= job.r1) return;   // the whole workgroup leaves, before any barrier: the merge counts the chunks of a word itself
                                // (a word with a flag has r0 == r1, so 1 <= G <= 32 from here on)
  stage_cost_rows(tab, costs, job.s0, min(lexlat_rows(G, MS), kLexLatMaxRows), fold, tid, kLexChunk);   // (the word's span rows)
  __syncthreads();

  double best_c[K];
  int best_i[K];
  best_clear(best_c, best_i);

  for (int pass = 0; pass < span; ++pass) {
    const int p0 = base + pass * kLexChunk;
    if (p0 >= job.r1) break;
    const int e = p0 + tid;
    if (e < job.r1) {
      const int L = lens[e];
      double D[kLexMaxLen + 1];
      D[0] = 0.0;
#pragma unroll
      for (int i = 1; i <= kLexMaxLen; ++i) D[i] = D[i - 1] + del;
      for (int w = 0; 4 * w < L; ++w) {
        const uint32_t word = codes[(size_t)w * n_entries + e];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          if (4 * w + b < L) {
            const float* col = &tab[0][(word >> (8 * b)) & 0xFF];
            double o1 = D[0], o2 = INFINITY, o3 = INFINITY, o4 = INFINITY;   // D[i-1..i-4][j-1], the column being overwritten
            D[0] = o1 + ins;
#pragma unroll
            for (int i0 = 1; i0 <= kLexMaxLen; i0 += kRowsPerBranch) {
              if (i0 <= G) {   // uniform: kRowsPerBranch pieces per scalar branch, their LDS reads in flight together
#pragma unroll
                for (int i = i0; i < i0 + kRowsPerBranch; ++i) {   // (rows past G compute on table rows nobody wrote; D[0..G] never reads them)
                  const float* r = col + lexlat_rows(i - 1, MS) * 64;   // row(i, 1); row(i, m) is m - 1 rows on
                  const double cur = D[i];
                  double seg = (ZS ? o1 : o1 + sc.v[0]) + (double)r[0];
                  if (MS >= 2 && i >= 2) seg = fmin(seg, (ZS ? o2 : o2 + sc.v[1]) + (double)r[64]);
                  if (MS >= 3 && i >= 3) seg = fmin(seg, (ZS ? o3 : o3 + sc.v[2]) + (double)r[128]);
                  if (MS >= 4 && i >= 4) seg = fmin(seg, (ZS ? o4 : o4 + sc.v[3]) + (double)r[192]);
                  const double gap = fmin(D[i - 1] + del, cur + ins);
                  D[i] = fmin(seg, gap);
                  o4 = o3;
                  o3 = o2;
                  o2 = o1;
                  o1 = cur;
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

__global__ __launch_bounds__(64) void lexlat_merge_kernel(const LexLatJob* __restrict__ jobs, int n_chunks, int span, int top_k,
                                                          const double* __restrict__ part_cost, const int32_t* __restrict__ part_idx,
                                                          int32_t* __restrict__ entries, double* __restrict__ out_cost) {
  const LexLatJob job = jobs[blockIdx.x];
  merge_slots(job.r0, job.r1, n_chunks, span, top_k, part_cost, part_idx, entries, out_cost);
}

__global__ __launch_bounds__(64) void lexlat_trace_kernel(const float* __restrict__ costs, const LexLatJob* __restrict__ jobs,
                                                          const uint32_t* __restrict__ codes, const uint8_t* __restrict__ lens,
                                                          const int32_t* __restrict__ index, const int32_t* __restrict__ start,
                                                          int n_entries, int M, int fold, double ins, double del, LexLatSpanCost sc,
                                                          int top_k, int n_pieces, const int32_t* __restrict__ entries,
                                                          int32_t* __restrict__ seg_len, int32_t* __restrict__ seg_char,
                                                          int32_t* __restrict__ n_ins, double* __restrict__ trace_cost) {
  __shared__ float tab[kLexLatMaxRows][64];
  __shared__ double D[kLexMaxLen + 1][kLexMaxLen + 2];
  __shared__ int cls[kLexMaxLen];
  const int w = blockIdx.x / top_k, k = blockIdx.x % top_k, lane = threadIdx.x;
  const int x = entries[(size_t)w * top_k + k];
  if (x < 0) return;   // uniform: an empty slot keeps its preset rows
  const LexLatJob job = jobs[w];
  const int G = job.G;   // 1..32: the word has candidates

  // the entry's position in the sorted order: the caller's index ascends inside a length bucket, and lane L searches bucket L
  int pos = -1;
  if (lane >= 1 && lane <= kLexMaxLen) {
    int lo = start[lane], hi = start[lane + 1];
    const int end = hi;
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (index[mid] < x) lo = mid + 1;
      else hi = mid;
    }
    if (lo < end && index[lo] == x) pos = lo;
  }
  const unsigned long long found = __ballot(pos >= 0);
  if (!found) return;   // uniform; every index is in the lexicon once, so this does not happen
  const int src = __ffsll((long long)found) - 1;
  const int p = __shfl(pos, src, 64);
  int L = lens[p];
  L = L < kLexMaxLen ? L : kLexMaxLen;
  if (lane < L) cls[lane] = (int)((codes[(size_t)(lane >> 2) * n_entries + p] >> (8 * (lane & 3))) & 0x3F);
  stage_cost_rows(tab, costs, job.s0, min(lexlat_rows(G, M), kLexLatMaxRows), fold, lane, 64);
  __syncthreads();

  // the full table, anti-diagonal t = i + j per step, row i in lane i
  for (int t = 0; t <= G + L; ++t) {
    const int i = lane, j = t - lane;
    if (i <= G && j >= 0 && j <= L) {
      double v;
      if (j == 0) {
        v = i == 0 ? 0.0 : D[i - 1][0] + del;
      } else if (i == 0) {
        v = D[0][j - 1] + ins;
      } else {
        const int c = cls[j - 1], r0 = lexlat_rows(i - 1, M);
        v = fmin(D[i - 1][j] + del, D[i][j - 1] + ins);
#pragma unroll
        for (int m = 1; m <= kLatMaxSpan; ++m)
          if (m <= M && m <= i) v = fmin(v, (D[i - m][j - 1] + sc.v[m - 1]) + (double)tab[r0 + m - 1][c]);
      }
      D[i][j] = v;
    }
    __syncthreads();
  }

  if (lane == 0) {
    int i = G, j = L, n = 0;
    const size_t out = (size_t)k * n_pieces + job.p0;
    while (i > 0 || j > 0) {
      const double v = D[i][j];
      int step = 0;   // m of a segment, -1 a deletion, -2 an insertion
      if (i >= 1 && j >= 1) {
        const int c = cls[j - 1], r0 = lexlat_rows(i - 1, M);
#pragma unroll
        for (int m = 1; m <= kLatMaxSpan; ++m)
          if (step == 0 && m <= M && m <= i && (D[i - m][j - 1] + sc.v[m - 1]) + (double)tab[r0 + m - 1][c] == v) step = m;
      }
      if (step == 0 && i >= 1 && D[i - 1][j] + del == v) step = -1;
      if (step == 0) step = j >= 1 ? -2 : -1;   // what is left is the insertion (every branch moves toward (0, 0))
      if (step > 0) {
        seg_len[out + (i - step)] = step;
        seg_char[out + (i - step)] = j - 1;
        i -= step;
        --j;
      } else if (step == -1) {
        seg_len[out + (i - 1)] = -1;
        --i;
      } else {
        ++n;
        --j;
      }
    }
    n_ins[(size_t)w * top_k + k] = n;
    trace_cost[(size_t)w * top_k + k] = D[G][L];
  }
}

}  // namespace
}  // namespace ocr

// ---- the C surface (include/ocr_amd.h)
namespace {
struct LexLatMatchesOwned {   // the library-owned storage behind an ocr_lexlat_matches_t* (released by ocr_lexlat_matches_free)
  ocr_lexlat_matches_t view{};
  std::vector<int32_t> entries, n_candidates, word_flags, seg_len, seg_char, n_ins;
  std::vector<double> costs, raw_costs;
  void finish(int n_words, int top_k, int n_pieces) {
    view.n_words = n_words;
    view.top_k = top_k;
    view.n_pieces = n_pieces;
    view.entries = entries.data();
    view.costs = costs.data();
    view.raw_costs = raw_costs.data();
    view.n_candidates = n_candidates.data();
    view.word_flags = word_flags.data();
    view.seg_len = seg_len.data();
    view.seg_char = seg_char.data();
    view.n_ins = n_ins.data();
  }
};
constexpr int32_t kLexLatNone = 0x7F7F7F7F;   // what a byte memset of 0x7F leaves: above every word index
}  // namespace

extern "C" {

void ocr_lexlat_default_params(ocr_lexlat_params_t* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->ins_cost = 4.0;
  p->del_cost = 4.0;
  p->max_span = 2;
  p->max_len_diff = 2;
  p->fold_case = 1;
  p->top_k = 1;
}

int ocr_lexicon_lattice_match(ocr_rec_t* rec, const ocr_lexicon_t* lex, const float* costs, int n_spans, int mem_kind,
                              const int32_t* span_offsets, const int32_t* piece_offsets, int n_words, const ocr_lexlat_params_t* params,
                              ocr_lexlat_matches_t** out) {
  return ocr::guard([&] {
    using namespace ocr;
    if (!rec || !lex || !span_offsets || !piece_offsets || !out) fail(OCR_ERR_INVALID, "lexicon_lattice_match: null argument");
    *out = nullptr;
    if (mem_kind != OCR_MEM_HOST && mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "lexicon_lattice_match: mem_kind %d", mem_kind);
    if (lex->device != rec->impl.device())
      fail(OCR_ERR_INVALID, "lexicon_lattice_match: lexicon on device %d, handle on device %d", lex->device, rec->impl.device());
    ocr_lexlat_params_t p;
    ocr_lexlat_default_params(&p);
    if (params) p = *params;
    lexlat_check_params(p);
    LexLatPlan plan;
    lexlat_plan(lex->host.start, span_offsets, piece_offsets, n_words, n_spans, p.max_span, p.max_len_diff, plan);
    if (n_spans > 0 && !costs) fail(OCR_ERR_INVALID, "lexicon_lattice_match: null costs");
    std::unique_ptr<LexLatMatchesOwned> m(new LexLatMatchesOwned());
    const int k = p.top_k, np = plan.n_pieces;
    const size_t nw = (size_t)n_words, seg_count = (size_t)k * (size_t)np;
    m->n_candidates.swap(plan.n_candidates);
    m->word_flags.swap(plan.flags);
    m->entries.assign(nw * k, -1);
    m->costs.assign(nw * k, INFINITY);
    m->raw_costs.assign(nw, 0.0);
    m->seg_len.assign(seg_count, 0);
    m->seg_char.assign(seg_count, -1);
    m->n_ins.assign(nw * k, 0);
    if (n_words == 0) {
      m->finish(0, k, np);
      *out = &m.release()->view;
      return;
    }
    OCR_HIP(hipSetDevice(rec->impl.device()));
    hipStream_t s = rec->impl.stream();
    const int span = lex_span(n_words, plan.max_range);
    const int per = span * kLexChunk;
    const int n_chunks = plan.max_range > 0 ? (plan.max_range + per - 1) / per : 0;
    const size_t cost_bytes = (size_t)n_spans * kLexClasses * 4, slots = nw * (size_t)n_chunks * k, seg_bytes = seg_count * 4;
    // the outputs lie end to end at the head of the workspace and come home in one copy; offsets and bucket starts go up in one
    Carve c;
    const size_t o_bad = c.take(4), o_raw = c.take(nw * 8), o_ent = c.take(nw * k * 4), o_oc = c.take(nw * k * 8), o_tc = c.take(nw * k * 8);
    const size_t o_ni = c.take(nw * k * 4), o_seg = c.take(seg_bytes), o_sch = c.take(seg_bytes), out_bytes = c.end;
    const size_t n_start = kLexMaxLen + 2;
    const size_t o_off = c.take((2 * (nw + 1) + n_start) * 4), o_jobs = c.take(nw * sizeof(LexLatJob));
    const size_t o_cost = c.take(mem_kind == OCR_MEM_HOST ? cost_bytes : 0), o_pc = c.take(slots * 8), o_pi = c.take(slots * 4);
    char* ws = lex_workspace(rec, c.end);
    int32_t* bad_dev = at<int32_t>(ws, o_bad);
    OCR_HIP(hipMemsetAsync(bad_dev, 0x7F, 4, s));
    OCR_HIP(hipMemsetAsync(ws + o_ni, 0, o_sch - o_ni, s));                    // inserted characters and segment lengths
    if (seg_bytes) OCR_HIP(hipMemsetAsync(ws + o_sch, 0xFF, seg_bytes, s));    // -1: no segment starts here
    const float* cost_dev = costs;
    if (mem_kind == OCR_MEM_HOST && n_spans > 0) {
      OCR_HIP(hipMemcpyAsync(ws + o_cost, costs, cost_bytes, hipMemcpyHostToDevice, s));
      cost_dev = at<const float>(ws, o_cost);
    }
    std::vector<int32_t> offs(span_offsets, span_offsets + nw + 1);
    offs.insert(offs.end(), piece_offsets, piece_offsets + nw + 1);
    offs.insert(offs.end(), lex->host.start, lex->host.start + n_start);
    OCR_HIP(hipMemcpyAsync(ws + o_off, offs.data(), offs.size() * 4, hipMemcpyHostToDevice, s));
    OCR_HIP(hipMemcpyAsync(ws + o_jobs, plan.jobs.data(), nw * sizeof(LexLatJob), hipMemcpyHostToDevice, s));
    const int32_t* off_dev = at<const int32_t>(ws, o_off);
    LexLatSpanCost sc;
    for (int i = 0; i < kLatMaxSpan; ++i) sc.v[i] = p.span_cost[i];
    hipLaunchKernelGGL(lexlat_raw_kernel, dim3((n_words + 3) / 4), dim3(256), 0, s, cost_dev, off_dev, off_dev + (nw + 1), n_words,
                       p.max_span, sc, at<double>(ws, o_raw), bad_dev);
    OCR_HIP(hipGetLastError());
    if (n_chunks > 0) {
      const char* d = static_cast<const char*>(lex->dev);
      const uint32_t* codes = reinterpret_cast<const uint32_t*>(d + lex->o_codes);
      const uint8_t* lens = reinterpret_cast<const uint8_t*>(d + lex->o_lens);
      const int32_t* index = reinterpret_cast<const int32_t*>(d + lex->o_index);
      const dim3 grid(n_words, n_chunks);
      auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(kLexChunk), 0, s, cost_dev, at<const LexLatJob>(ws, o_jobs), codes, lens, index, lex->host.n,
                           span, p.fold_case, p.ins_cost, p.del_cost, sc, k, at<double>(ws, o_pc), at<int32_t>(ws, o_pi));
      };
      bool zs = true;   // the span costs this call can read are all zero: the instantiation without their adds gives the same bits
      for (int i = 0; i < p.max_span; ++i) zs = zs && p.span_cost[i] == 0.0;
      auto pick = [&](auto ms) {
        constexpr int MS = decltype(ms)::value;
        if (k == 1) zs ? launch(lexlat_match_kernel<1, MS, true>) : launch(lexlat_match_kernel<1, MS, false>);
        else zs ? launch(lexlat_match_kernel<8, MS, true>) : launch(lexlat_match_kernel<8, MS, false>);
      };
      switch (p.max_span) {
        case 1: pick(std::integral_constant<int, 1>()); break;
        case 2: pick(std::integral_constant<int, 2>()); break;
        case 3: pick(std::integral_constant<int, 3>()); break;
        default: pick(std::integral_constant<int, 4>()); break;
      }
      OCR_HIP(hipGetLastError());
      hipLaunchKernelGGL(lexlat_merge_kernel, dim3(n_words), dim3(64), 0, s, at<const LexLatJob>(ws, o_jobs), n_chunks, span, k,
                         at<const double>(ws, o_pc), at<const int32_t>(ws, o_pi), at<int32_t>(ws, o_ent), at<double>(ws, o_oc));
      OCR_HIP(hipGetLastError());
      hipLaunchKernelGGL(lexlat_trace_kernel, dim3(n_words * k), dim3(64), 0, s, cost_dev, at<const LexLatJob>(ws, o_jobs), codes, lens,
                         index, off_dev + 2 * (nw + 1), lex->host.n, p.max_span, p.fold_case, p.ins_cost, p.del_cost, sc, k, np,
                         at<const int32_t>(ws, o_ent), at<int32_t>(ws, o_seg), at<int32_t>(ws, o_sch), at<int32_t>(ws, o_ni),
                         at<double>(ws, o_tc));
      OCR_HIP(hipGetLastError());
    }
    std::vector<char> home(out_bytes);
    OCR_HIP(hipMemcpyAsync(home.data(), ws, out_bytes, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipStreamSynchronize(s));
    int32_t bad = kLexLatNone;
    std::memcpy(&bad, home.data() + o_bad, 4);
    if (bad != kLexLatNone) fail(OCR_ERR_INVALID, "lexicon_lattice_match: word %d has a cost that is NaN, infinite or negative", bad);
    std::memcpy(m->raw_costs.data(), home.data() + o_raw, nw * 8);
    if (n_chunks > 0) {   // (without a candidate in the whole call nothing ran: the presets stand)
      std::memcpy(m->entries.data(), home.data() + o_ent, nw * k * 4);
      std::memcpy(m->costs.data(), home.data() + o_oc, nw * k * 8);
      std::memcpy(m->n_ins.data(), home.data() + o_ni, nw * k * 4);
      if (seg_bytes) {
        std::memcpy(m->seg_len.data(), home.data() + o_seg, seg_bytes);
        std::memcpy(m->seg_char.data(), home.data() + o_sch, seg_bytes);
      }
      const double* tc = reinterpret_cast<const double*>(home.data() + o_tc);
      for (size_t t = 0; t < nw * k; ++t)
        if (m->entries[t] >= 0 && std::memcmp(&tc[t], &m->costs[t], 8) != 0)
          fail(OCR_ERR_INTERNAL, "lexicon_lattice_match: word %zu rank %zu: the traced table ends at %.17g, the match at %.17g", t / k, t % k,
               tc[t], m->costs[t]);
    }
    m->finish(n_words, k, np);
    *out = &m.release()->view;
  });
}

void ocr_lexlat_matches_free(ocr_lexlat_matches_t* m) {
  if (!m) return;
  delete reinterpret_cast<LexLatMatchesOwned*>(reinterpret_cast<char*>(m) - offsetof(LexLatMatchesOwned, view));
}

}  // extern "C"
