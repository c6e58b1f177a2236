// Host side of the character language model: the checks of model, parameters and offsets, and the per-call plan (char_lm_host.hpp).
#include "char_lm_host.hpp"

#include <cmath>

namespace ocr {

void lm_check_model(const float* trans) {
  if (!trans) fail(OCR_ERR_INVALID, "char_lm_create: null argument");
  for (int p = 0; p < kLmStride; ++p)
    for (int c = 0; c < kLmStride; ++c) {
      const float v = trans[p * kLmStride + c];
      const bool used = p < kLmStride - 1 && c < kLmStride - 1 && !(p == kLmBegin && c == kLmEnd);
      if (used) {
        // (written so that a NaN is refused)
        if (!(v >= 0.0f && std::isfinite(v))) fail(OCR_ERR_INVALID, "char_lm_create: model cell [%d][%d] is %g (a used cell is finite and >= 0)", p, c, (double)v);
      } else if (!(v == 0.0f)) {
        fail(OCR_ERR_INVALID, "char_lm_create: model cell [%d][%d] is %g (an unused cell is 0)", p, c, (double)v);
      }
    }
}

void lm_check_params(const ocr_lm_params_t& p) {
  if (p.top_k < 1 || p.top_k > 8 || p.reserved[0] || p.reserved[1] || p.reserved[2])
    fail(OCR_ERR_INVALID, "lm_decode: params top_k=%d reserved=(%d, %d, %d) (limits: top_k 1..8, reserved 0)", p.top_k, p.reserved[0],
         p.reserved[1], p.reserved[2]);
}

void lm_plan(const int32_t* word_offsets, int n_words, int n_glyphs, int top_k, LmPlan& out) {
  if (!word_offsets) fail(OCR_ERR_INVALID, "lm_decode: null word offsets");
  if (n_words < 0 || n_glyphs < 0) fail(OCR_ERR_INVALID, "lm_decode: %d words, %d glyphs", n_words, n_glyphs);
  if (word_offsets[0] != 0) fail(OCR_ERR_INVALID, "lm_decode: word offsets start at %d", word_offsets[0]);
  for (int w = 0; w < n_words; ++w)
    if (word_offsets[w + 1] < word_offsets[w]) fail(OCR_ERR_INVALID, "lm_decode: word offsets decrease at word %d", w);
  if (word_offsets[n_words] != n_glyphs) fail(OCR_ERR_INVALID, "lm_decode: word offsets end at %d, not at the %d glyphs", word_offsets[n_words], n_glyphs);
  out.flags.assign((size_t)n_words, 0);
  out.n_decoded = 0;
  for (int w = 0; w < n_words; ++w) {
    const int32_t G = word_offsets[w + 1] - word_offsets[w];
    if (G == 0)
      out.flags[w] = 1;
    else if (G > kLmMaxLen)
      out.flags[w] = 2;
    else
      ++out.n_decoded;
  }
  out.blocks = (n_words + kLmWords - 1) / kLmWords;
  out.link_bytes = (size_t)n_glyphs * kLmStride * (size_t)top_k * 2;
  out.label_count = (size_t)top_k * (size_t)n_glyphs;
}

}  // namespace ocr
