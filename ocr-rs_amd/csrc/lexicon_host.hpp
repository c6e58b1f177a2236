// Host side of lexicon matching (rule: include/ocr_amd.h at ocr_lexicon_match): the checks of every argument, the packer that turns a
// word list into the device layout, and the per-word plan of a match call.  Plain C++ without a device call, so that
// tools/sanitize_host.sh can run it under ASan + UBSan (tools/fuzz/lexicon_host_fuzz.cpp).
#pragma once
#include "common.hpp"

namespace ocr {

constexpr int kLexMaxLen = OCR_LEX_MAX_LEN;
constexpr int kLexClasses = 62;
constexpr int kLexCodeWords = kLexMaxLen / 4;   // 32-bit words of four class indices per entry
constexpr int kLexChunk = 256;                  // entries per pass of a match workgroup: one per lane

// The device layout, built on the host.  Entries are sorted by (length, caller's index): position p of the sorted order holds
// lens[p], index[p] (the caller's index) and its class indices codes[w * n + p] (characters 4w .. 4w+3, low byte first, 0 past the
// end).  start[m] is the first position of length m (m = 1..32), start[33] = n: the candidates of a word are one contiguous range.
struct LexPacked {
  int32_t n = 0;
  std::vector<uint32_t> codes;
  std::vector<uint8_t> lens;
  std::vector<int32_t> index;
  int32_t start[kLexMaxLen + 2] = {};
};
void lex_pack(const char* bytes, const int32_t* offsets, int n_entries, LexPacked& out);

void lex_check_params(const ocr_lexicon_params_t& p);

// What the match kernels read per word: its glyph rows [g0, g0 + G) and its candidates [r0, r1) in the sorted order (r0 == r1 for a
// word with a flag).
struct LexWordJob {
  int32_t g0, G, r0, r1;
};
struct LexPlan {
  std::vector<LexWordJob> jobs;
  std::vector<int32_t> n_candidates, flags;
  int32_t max_range = 0;   // the largest r1 - r0
};
void lex_plan(const int32_t* start, const int32_t* word_offsets, int n_words, int n_glyphs, int max_len_diff, LexPlan& out);

// Passes of kLexChunk entries one workgroup makes, so that about 4 096 workgroups cover n_words x max_range.
int lex_span(int n_words, int max_range);

}  // namespace ocr
