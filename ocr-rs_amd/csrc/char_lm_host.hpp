// Host side of the character language model (rule: include/ocr_amd.h at ocr_lm_decode): the check of a model, of the parameters and of
// the word offsets, and the per-call plan.  Plain C++ without a device call, so that it runs under ASan + UBSan with a main of its own
// (tools/fuzz/char_lm_host_fuzz.cpp).
#pragma once
#include "common.hpp"

namespace ocr {

constexpr int kLmMaxLen = OCR_LM_MAX_LEN;
constexpr int kLmClasses = 62;
constexpr int kLmStride = 64;    // rows and columns of a model: 62 classes, begin / end of word, one unused
constexpr int kLmBegin = 62;     // the row of begin-of-word
constexpr int kLmEnd = 62;       // the column of end-of-word
constexpr int kLmWords = 4;      // words per workgroup of the decode kernel: one wave each, the model shared in LDS

// every used value finite and >= 0, every unused cell 0; the message names the first offending cell
void lm_check_model(const float* trans);

void lm_check_params(const ocr_lm_params_t& p);

struct LmPlan {
  std::vector<int32_t> flags;   // per word: 1 no glyphs, 2 more than kLmMaxLen glyphs
  int32_t n_decoded = 0;        // words with 1..kLmMaxLen glyphs
  int32_t blocks = 0;           // workgroups of the decode launch: every word gets a wave (the greedy cost is summed for all of them)
  size_t link_bytes = 0;        // the back-pointers of the call: n_glyphs x 64 x top_k uint16
  size_t label_count = 0;       // top_k x n_glyphs
};
void lm_plan(const int32_t* word_offsets, int n_words, int n_glyphs, int top_k, LmPlan& out);

}  // namespace ocr
