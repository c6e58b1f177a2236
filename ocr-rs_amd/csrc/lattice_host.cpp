// Host side of the segmentation lattice: parameter checks, the span table, the offsets check and the per-call plan (lattice_host.hpp).
#include "lattice_host.hpp"

#include <algorithm>
#include <cmath>

namespace ocr {

void split_check_params(const ocr_split_params_t& p) {
  if (p.aspect_pct < 25 || p.aspect_pct > 400 || p.max_pieces < 1 || p.max_pieces > 4 || p.min_piece_w < 3 || p.min_piece_w > 64 ||
      p.max_word_pieces < 1 || p.max_word_pieces > 256 || p.reserved[0] || p.reserved[1] || p.reserved[2] || p.reserved[3])
    fail(OCR_ERR_INVALID,
         "split_glyphs: params aspect_pct=%d max_pieces=%d min_piece_w=%d max_word_pieces=%d reserved=(%d, %d, %d, %d) (limits: aspect_pct "
         "25..400, max_pieces 1..4, min_piece_w 3..64, max_word_pieces 1..256, reserved 0)",
         p.aspect_pct, p.max_pieces, p.min_piece_w, p.max_word_pieces, p.reserved[0], p.reserved[1], p.reserved[2], p.reserved[3]);
}

void lat_check_params(const ocr_lattice_params_t& p) {
  if (p.max_span < 1 || p.max_span > kLatMaxSpan || p.top_k < 1 || p.top_k > 8 || p.reserved[0] || p.reserved[1])
    fail(OCR_ERR_INVALID, "lattice_decode: params max_span=%d top_k=%d reserved=(%d, %d) (limits: max_span 1..%d, top_k 1..8, reserved 0)",
         p.max_span, p.top_k, p.reserved[0], p.reserved[1], kLatMaxSpan);
  for (int m = 0; m < kLatMaxSpan; ++m)
    // (written so that a NaN is refused)
    if (!(p.span_cost[m] >= 0.0 && std::isfinite(p.span_cost[m])))
      fail(OCR_ERR_INVALID, "lattice_decode: span_cost[%d] is %g (finite and >= 0)", m, p.span_cost[m]);
}

void lat_spans(const ocr_glyphs_t& g, int M, SpanBlock& out) {
  if (M < 1 || M > kLatMaxSpan) fail(OCR_ERR_INVALID, "glyph_spans: max_span %d (limits: 1..%d)", M, kLatMaxSpan);
  const int nw = g.n_words, np = g.n_glyphs;
  if (nw < 0 || np < 0) fail(OCR_ERR_INVALID, "glyph_spans: %d words, %d pieces", nw, np);
  if (!g.word_offsets || (np > 0 && !g.boxes)) fail(OCR_ERR_INVALID, "glyph_spans: null array in the piece block");
  if (g.word_offsets[0] != 0) fail(OCR_ERR_INVALID, "glyph_spans: word offsets start at %d", g.word_offsets[0]);
  int64_t total = 0;
  for (int w = 0; w < nw; ++w) {
    if (g.word_offsets[w + 1] < g.word_offsets[w]) fail(OCR_ERR_INVALID, "glyph_spans: word offsets decrease at word %d", w);
    total += lat_span_count((int64_t)g.word_offsets[w + 1] - g.word_offsets[w], M);
  }
  if (g.word_offsets[nw] != np) fail(OCR_ERR_INVALID, "glyph_spans: word offsets end at %d, not at the %d pieces", g.word_offsets[nw], np);
  if (total > INT32_MAX) fail(OCR_ERR_INVALID, "glyph_spans: %lld spans (limit 2^31 - 1)", (long long)total);
  out.span_offsets.assign(1, 0);
  out.boxes.clear();
  out.span_word.clear();
  out.span_end.clear();
  out.span_len.clear();
  out.boxes.reserve((size_t)total * 4);
  for (int w = 0; w < nw; ++w) {
    const int p0 = g.word_offsets[w], G = g.word_offsets[w + 1] - p0;
    for (int e = 1; e <= G; ++e) {
      int32_t u[4] = {INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN};
      for (int m = 1; m <= std::min(M, e); ++m) {   // [e-m, e): one more piece on the left per m
        const int32_t* b = g.boxes + 4 * (size_t)(p0 + e - m);
        u[0] = std::min(u[0], b[0]);
        u[1] = std::min(u[1], b[1]);
        u[2] = std::max(u[2], b[2]);
        u[3] = std::max(u[3], b[3]);
        out.boxes.insert(out.boxes.end(), u, u + 4);
        out.span_word.push_back(w);
        out.span_end.push_back(e);
        out.span_len.push_back(m);
      }
    }
    out.span_offsets.push_back((int32_t)out.span_word.size());
  }
}

void lat_plan(const int32_t* span_offsets, const int32_t* piece_offsets, int n_words, int n_spans, int M, int top_k, LatPlan& out) {
  if (!span_offsets || !piece_offsets) fail(OCR_ERR_INVALID, "lattice_decode: null offsets");
  if (n_words < 0 || n_spans < 0) fail(OCR_ERR_INVALID, "lattice_decode: %d words, %d spans", n_words, n_spans);
  if (M < 1 || M > kLatMaxSpan || top_k < 1 || top_k > 8) fail(OCR_ERR_INVALID, "lattice_decode: max_span %d, top_k %d", M, top_k);
  if (span_offsets[0] != 0 || piece_offsets[0] != 0)
    fail(OCR_ERR_INVALID, "lattice_decode: offsets start at %d (spans) and %d (pieces)", span_offsets[0], piece_offsets[0]);
  out.flags.assign((size_t)n_words, 0);
  for (int w = 0; w < n_words; ++w) {
    const int64_t G = (int64_t)piece_offsets[w + 1] - piece_offsets[w], S = (int64_t)span_offsets[w + 1] - span_offsets[w];
    if (G < 0) fail(OCR_ERR_INVALID, "lattice_decode: piece offsets decrease at word %d", w);
    if (S != lat_span_count(G, M))
      fail(OCR_ERR_INVALID, "lattice_decode: word %d of %lld pieces holds %lld spans, max_span %d gives %lld", w, (long long)G, (long long)S, M,
           (long long)lat_span_count(G, M));
    out.flags[w] = G == 0 ? 1 : G > kLatMaxPieces ? 2 : 0;
  }
  if (span_offsets[n_words] != n_spans)
    fail(OCR_ERR_INVALID, "lattice_decode: span offsets end at %d, not at the %d spans", span_offsets[n_words], n_spans);
  out.n_pieces = piece_offsets[n_words];
  out.blocks = (n_words + kLatWords - 1) / kLatWords;
  out.link_bytes = (size_t)out.n_pieces * kLmStride * (size_t)top_k * 2;
  out.label_count = (size_t)top_k * (size_t)out.n_pieces;
}

}  // namespace ocr
