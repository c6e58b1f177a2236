// Host side of the joint lexicon and lattice search (rule: include/ocr_amd.h at ocr_lexicon_lattice_match): the parameter check, the
// check of span and piece offsets and the per-word plan.  Plain C++ without a device call, so that it runs under ASan + UBSan with a
// main of its own (tools/fuzz/lexicon_lattice_host_fuzz.cpp).
#pragma once
#include "lattice_host.hpp"
#include "lexicon_host.hpp"

namespace ocr {

// the table rows of a word of kLatMaxPieces pieces at kLatMaxSpan: what the match kernel keeps in LDS
constexpr int kLexLatMaxRows = kLatMaxSpan * (kLatMaxSpan + 1) / 2 + (kLatMaxPieces - kLatMaxSpan) * kLatMaxSpan;
static_assert(kLatMaxPieces == kLexMaxLen, "the DP column of the match kernel is sized by both");

void lexlat_check_params(const ocr_lexlat_params_t& p);

// What the kernels read per word: its span rows [s0, s0 + lat_span_count(G, M)), its pieces [p0, p0 + G) and its candidates [r0, r1)
// in the lexicon's sorted order (r0 == r1 for a word with a flag).
struct LexLatJob {
  int32_t s0, p0, G, r0, r1;
};
struct LexLatPlan {
  std::vector<LexLatJob> jobs;
  std::vector<int32_t> n_candidates, flags;
  int32_t max_range = 0;   // the largest r1 - r0
  int32_t n_pieces = 0;
};
// the admissible entry lengths of a word of G pieces (1 <= G <= kLatMaxPieces): max(1, ceil(G / M) - d) .. min(32, G + d)
inline int lexlat_len_lo(int G, int M, int d) { const int lo = (G + M - 1) / M - d; return lo < 1 ? 1 : lo; }
inline int lexlat_len_hi(int G, int d) { return G + d > kLexMaxLen ? kLexMaxLen : G + d; }
// span_offsets must hold exactly lat_span_count(G, max_span) spans per word and end at n_spans; start is LexPacked::start
void lexlat_plan(const int32_t* start, const int32_t* span_offsets, const int32_t* piece_offsets, int n_words, int n_spans, int max_span,
                 int max_len_diff, LexLatPlan& out);

}  // namespace ocr
