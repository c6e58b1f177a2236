// Host side of lexicon matching: argument checks, the packer, the per-word plan (lexicon_host.hpp).
#include "lexicon_host.hpp"

#include <cmath>
#include <cstring>

namespace ocr {

void lex_pack(const char* bytes, const int32_t* offsets, int n_entries, LexPacked& out) {
  if (!bytes || !offsets) fail(OCR_ERR_INVALID, "lexicon_create: null argument");
  if (n_entries < 1 || n_entries > OCR_LEX_MAX_ENTRIES) fail(OCR_ERR_INVALID, "lexicon_create: %d entries (limits 1..%d)", n_entries, OCR_LEX_MAX_ENTRIES);
  if (offsets[0] != 0) fail(OCR_ERR_INVALID, "lexicon_create: offsets start at %d", offsets[0]);
  int8_t cls[256];
  std::memset(cls, -1, sizeof cls);
  const char* alphabet = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789";
  for (int c = 0; c < kLexClasses; ++c) cls[(unsigned char)alphabet[c]] = (int8_t)c;
  int32_t count[kLexMaxLen + 2] = {};
  for (int k = 0; k < n_entries; ++k) {
    const int64_t len = (int64_t)offsets[k + 1] - offsets[k];
    if (len < 1 || len > kLexMaxLen) fail(OCR_ERR_INVALID, "lexicon_create: entry %d has %lld characters (limits 1..%d)", k, (long long)len, kLexMaxLen);
    for (int32_t b = offsets[k]; b < offsets[k + 1]; ++b)
      if (cls[(unsigned char)bytes[b]] < 0) fail(OCR_ERR_INVALID, "lexicon_create: entry %d holds byte 0x%02x, which is not in the alphabet", k, (unsigned char)bytes[b]);
    ++count[len];
  }
  const size_t n = (size_t)n_entries;
  out.n = n_entries;
  out.codes.assign(n * kLexCodeWords, 0u);
  out.lens.assign(n, 0);
  out.index.assign(n, 0);
  out.start[0] = out.start[1] = 0;
  for (int m = 1; m <= kLexMaxLen; ++m) out.start[m + 1] = out.start[m] + count[m];
  int32_t next[kLexMaxLen + 2];
  std::memcpy(next, out.start, sizeof next);
  for (int k = 0; k < n_entries; ++k) {   // a counting sort: stable, so a bucket keeps the caller's order
    const int len = offsets[k + 1] - offsets[k];
    const size_t p = (size_t)next[len]++;
    out.lens[p] = (uint8_t)len;
    out.index[p] = k;
    for (int j = 0; j < len; ++j) out.codes[(size_t)(j / 4) * n + p] |= (uint32_t)cls[(unsigned char)bytes[offsets[k] + j]] << (8 * (j % 4));
  }
}

void lex_check_params(const ocr_lexicon_params_t& p) {
  // (written so that a NaN is out of range)
  if (!(p.ins_cost >= 0 && std::isfinite(p.ins_cost)) || !(p.del_cost >= 0 && std::isfinite(p.del_cost)) || p.max_len_diff < 0 ||
      p.max_len_diff > 8 || (p.fold_case != 0 && p.fold_case != 1) || p.top_k < 1 || p.top_k > 8 || p.reserved[0] || p.reserved[1] ||
      p.reserved[2])
    fail(OCR_ERR_INVALID, "lexicon_match: params ins_cost=%g del_cost=%g max_len_diff=%d fold_case=%d top_k=%d reserved=(%d, %d, %d) (limits: "
         "costs finite and >= 0, max_len_diff 0..8, fold_case 0 | 1, top_k 1..8, reserved 0)", p.ins_cost, p.del_cost, p.max_len_diff,
         p.fold_case, p.top_k, p.reserved[0], p.reserved[1], p.reserved[2]);
}

void lex_plan(const int32_t* start, const int32_t* word_offsets, int n_words, int n_glyphs, int max_len_diff, LexPlan& out) {
  if (!word_offsets) fail(OCR_ERR_INVALID, "lexicon_match: null word offsets");
  if (n_words < 0 || n_glyphs < 0) fail(OCR_ERR_INVALID, "lexicon_match: %d words, %d glyphs", n_words, n_glyphs);
  if (word_offsets[0] != 0) fail(OCR_ERR_INVALID, "lexicon_match: word offsets start at %d", word_offsets[0]);
  for (int w = 0; w < n_words; ++w)
    if (word_offsets[w + 1] < word_offsets[w]) fail(OCR_ERR_INVALID, "lexicon_match: word offsets decrease at word %d", w);
  if (word_offsets[n_words] != n_glyphs) fail(OCR_ERR_INVALID, "lexicon_match: word offsets end at %d, not at the %d glyphs", word_offsets[n_words], n_glyphs);
  out.jobs.resize((size_t)n_words);
  out.n_candidates.assign((size_t)n_words, 0);
  out.flags.assign((size_t)n_words, 0);
  out.max_range = 0;
  for (int w = 0; w < n_words; ++w) {
    const int32_t g0 = word_offsets[w], G = word_offsets[w + 1] - g0;
    LexWordJob j{g0, G, 0, 0};
    if (G == 0)
      out.flags[w] = 1;
    else if (G > kLexMaxLen)
      out.flags[w] = 2;
    else {
      const int lo = G - max_len_diff < 1 ? 1 : G - max_len_diff, hi = G + max_len_diff > kLexMaxLen ? kLexMaxLen : G + max_len_diff;
      j.r0 = start[lo];
      j.r1 = start[hi + 1];
      if (j.r1 == j.r0) out.flags[w] = 4;
    }
    out.n_candidates[w] = j.r1 - j.r0;
    if (j.r1 - j.r0 > out.max_range) out.max_range = j.r1 - j.r0;
    out.jobs[w] = j;
  }
}

int lex_span(int n_words, int max_range) {
  const int64_t blocks = ((int64_t)max_range + kLexChunk - 1) / kLexChunk;
  const int64_t span = (blocks * n_words + 4095) / 4096;
  return span < 1 ? 1 : (int)(span < blocks ? span : blocks);
}

}  // namespace ocr
