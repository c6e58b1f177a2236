// Host side of the segmentation lattice (rules: include/ocr_amd.h at ocr_split_glyphs, ocr_glyph_spans and ocr_lattice_decode): the
// parameter checks, the span table of a piece block, the check of span and piece offsets and the per-call plan of the decode.  Plain
// C++ without a device call, so that it runs under ASan + UBSan with a main of its own (tools/fuzz/lattice_host_fuzz.cpp).
#pragma once
#include "char_lm_host.hpp"

namespace ocr {

constexpr int kLatMaxSpan = OCR_LATTICE_MAX_SPAN;
constexpr int kLatMaxPieces = OCR_LATTICE_MAX_PIECES;
constexpr int kLatWords = 4;   // words per workgroup of the decode kernel: one wave each, the model shared in LDS

// the spans of a word of G pieces: sum over e = 1..G of min(M, e)
inline int64_t lat_span_count(int64_t G, int M) { return G <= M ? G * (G + 1) / 2 : (int64_t)M * (M + 1) / 2 + (G - M) * M; }

void split_check_params(const ocr_split_params_t& p);
void lat_check_params(const ocr_lattice_params_t& p);

// the arrays of ocr_glyph_spans: the span block's word_offsets and boxes, and the table
struct SpanBlock {
  std::vector<int32_t> span_offsets;                     // [n_words+1]
  std::vector<int32_t> boxes;                            // [4*n_spans] the union of the pieces' boxes
  std::vector<int32_t> span_word, span_end, span_len;    // [n_spans]
};
// checks the block (counts, arrays, offsets) and fills `out`; spans ordered by (word, e, m)
void lat_spans(const ocr_glyphs_t& pieces, int max_span, SpanBlock& out);

struct LatPlan {
  std::vector<int32_t> flags;   // per word: 1 no pieces, 2 more than kLatMaxPieces pieces
  int32_t n_pieces = 0;
  int32_t blocks = 0;           // workgroups of the decode launch: every word gets a wave
  size_t link_bytes = 0;        // the back-pointers of the call: n_pieces x top_k x 64 uint16
  size_t label_count = 0;       // top_k x n_pieces
};
// span_offsets must hold exactly lat_span_count(G, max_span) spans per word and end at n_spans
void lat_plan(const int32_t* span_offsets, const int32_t* piece_offsets, int n_words, int n_spans, int max_span, int top_k, LatPlan& out);

}  // namespace ocr
