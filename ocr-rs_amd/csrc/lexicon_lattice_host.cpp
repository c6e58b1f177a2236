// Host side of the joint lexicon and lattice search: the parameter check, the offsets check and the per-word plan
// (lexicon_lattice_host.hpp).
#include "lexicon_lattice_host.hpp"

#include <cmath>

namespace ocr {

void lexlat_check_params(const ocr_lexlat_params_t& p) {
  // (written so that a NaN is out of range)
  if (!(p.ins_cost >= 0 && std::isfinite(p.ins_cost)) || !(p.del_cost >= 0 && std::isfinite(p.del_cost)) || p.max_span < 1 ||
      p.max_span > kLatMaxSpan || p.max_len_diff < 0 || p.max_len_diff > 8 || (p.fold_case != 0 && p.fold_case != 1) || p.top_k < 1 ||
      p.top_k > 8 || p.reserved[0] || p.reserved[1])
    fail(OCR_ERR_INVALID, "lexicon_lattice_match: params ins_cost=%g del_cost=%g max_span=%d max_len_diff=%d fold_case=%d top_k=%d "
         "reserved=(%d, %d) (limits: costs finite and >= 0, max_span 1..%d, max_len_diff 0..8, fold_case 0 | 1, top_k 1..8, reserved 0)",
         p.ins_cost, p.del_cost, p.max_span, p.max_len_diff, p.fold_case, p.top_k, p.reserved[0], p.reserved[1], kLatMaxSpan);
  for (int m = 0; m < kLatMaxSpan; ++m)
    if (!(p.span_cost[m] >= 0.0 && std::isfinite(p.span_cost[m])))
      fail(OCR_ERR_INVALID, "lexicon_lattice_match: span_cost[%d] is %g (finite and >= 0)", m, p.span_cost[m]);
}

void lexlat_plan(const int32_t* start, const int32_t* span_offsets, const int32_t* piece_offsets, int n_words, int n_spans, int M, int d,
                 LexLatPlan& out) {
  if (!start || !span_offsets || !piece_offsets) fail(OCR_ERR_INVALID, "lexicon_lattice_match: null offsets");
  if (n_words < 0 || n_spans < 0) fail(OCR_ERR_INVALID, "lexicon_lattice_match: %d words, %d spans", n_words, n_spans);
  if (M < 1 || M > kLatMaxSpan || d < 0 || d > 8) fail(OCR_ERR_INVALID, "lexicon_lattice_match: max_span %d, max_len_diff %d", M, d);
  if (span_offsets[0] != 0 || piece_offsets[0] != 0)
    fail(OCR_ERR_INVALID, "lexicon_lattice_match: offsets start at %d (spans) and %d (pieces)", span_offsets[0], piece_offsets[0]);
  out.jobs.resize((size_t)n_words);
  out.n_candidates.assign((size_t)n_words, 0);
  out.flags.assign((size_t)n_words, 0);
  out.max_range = 0;
  for (int w = 0; w < n_words; ++w) {
    const int64_t G = (int64_t)piece_offsets[w + 1] - piece_offsets[w], S = (int64_t)span_offsets[w + 1] - span_offsets[w];
    if (G < 0) fail(OCR_ERR_INVALID, "lexicon_lattice_match: piece offsets decrease at word %d", w);
    if (S != lat_span_count(G, M))
      fail(OCR_ERR_INVALID, "lexicon_lattice_match: word %d of %lld pieces holds %lld spans, max_span %d gives %lld", w, (long long)G,
           (long long)S, M, (long long)lat_span_count(G, M));
    LexLatJob j{span_offsets[w], piece_offsets[w], (int32_t)G, 0, 0};
    if (G == 0)
      out.flags[w] = 1;
    else if (G > kLatMaxPieces)
      out.flags[w] = 2;
    else {
      j.r0 = start[lexlat_len_lo((int)G, M, d)];
      j.r1 = start[lexlat_len_hi((int)G, d) + 1];
      if (j.r1 == j.r0) out.flags[w] = 4;
    }
    out.n_candidates[w] = j.r1 - j.r0;
    if (j.r1 - j.r0 > out.max_range) out.max_range = j.r1 - j.r0;
    out.jobs[w] = j;
  }
  if (span_offsets[n_words] != n_spans)
    fail(OCR_ERR_INVALID, "lexicon_lattice_match: span offsets end at %d, not at the %d spans", span_offsets[n_words], n_spans);
  out.n_pieces = piece_offsets[n_words];
}

}  // namespace ocr
