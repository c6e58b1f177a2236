// ASan/UBSan run of the host side of the joint lexicon and lattice search (csrc/lexicon_lattice_host.cpp): the parameter check on
// values in and out of range, and the plan on random lexicons (through lex_pack) and random offsets, valid and broken (a wrong span
// count, a wrong end, decreasing pieces, null pointers), checked against its definition: span rows, piece rows, flags, the candidate
// range under the length rule max(1, ceil(G / M) - d) .. min(32, G + d) counted entry by entry.  Every outcome of a broken input must
// be an ocr::Error.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>
#include "lexicon_lattice_host.hpp"

#define REQUIRE(cond, ...) do { if (!(cond)) { printf("iteration %d: ", it); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 3000;
  std::mt19937 rng(9731);
  int plans = 0, refused = 0;
  long candidates = 0;
  for (int it = 0; it < iters; ++it) {
    // ---- parameters
    {
      ocr_lexlat_params_t q{};
      q.ins_cost = (double)(rng() % 1000) / 64.0;
      q.del_cost = rng() % 7 == 0 ? 0.0 : (double)(rng() % 1000) / 32.0;
      for (double& v : q.span_cost) v = (rng() % 3 == 0) ? 0.0 : (rng() % 5 == 0 ? 1e30 : (rng() % 5 == 0 ? 4.9e-324 : (double)(rng() % 1000) / 64.0));
      q.max_span = 1 + (int32_t)(rng() % 4);
      q.max_len_diff = (int32_t)(rng() % 9);
      q.fold_case = (int32_t)(rng() % 2);
      q.top_k = 1 + (int32_t)(rng() % 8);
      const int h = (int)(rng() % 24);
      const double bads[5] = {NAN, INFINITY, -INFINITY, -0.5, -4.9e-324};
      if (h == 0) q.max_span = 0; else if (h == 1) q.max_span = 5; else if (h == 2) q.top_k = 0; else if (h == 3) q.top_k = 9;
      else if (h == 4) q.reserved[rng() % 2] = 3; else if (h == 5) q.span_cost[rng() % 4] = bads[rng() % 5]; else if (h == 6) q.top_k = INT32_MAX;
      else if (h == 7) q.ins_cost = bads[rng() % 5]; else if (h == 8) q.del_cost = bads[rng() % 5]; else if (h == 9) q.max_len_diff = -1;
      else if (h == 10) q.max_len_diff = 9; else if (h == 11) q.fold_case = rng() % 2 ? 2 : -1; else if (h == 12) q.max_span = INT32_MIN;
      try { ocr::lexlat_check_params(q); REQUIRE(h >= 13, "bad parameters accepted (%d)", h); }
      catch (const ocr::Error&) { REQUIRE(h < 13, "good parameters refused"); ++refused; }
    }

    // ---- a random lexicon, packed as ocr_lexicon_create packs it
    const int ne = 1 + (int)(rng() % 60), max_len = rng() % 3 == 0 ? 32 : 1 + (int)(rng() % 12);
    std::string bytes;
    std::vector<int32_t> eo(1, 0);
    std::vector<int> elen;
    for (int k = 0; k < ne; ++k) {
      const int len = 1 + (int)(rng() % max_len);
      for (int j = 0; j < len; ++j) bytes.push_back("ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789"[rng() % 62]);
      eo.push_back((int32_t)bytes.size());
      elen.push_back(len);
    }
    ocr::LexPacked lex;
    ocr::lex_pack(bytes.data(), eo.data(), ne, lex);

    // ---- the plan of a match
    const int nw = (int)(rng() % 12), M = 1 + (int)(rng() % 4), d = (int)(rng() % 9);
    std::vector<int32_t> po(1, 0), so(1, 0);
    for (int w = 0; w < nw; ++w) po.push_back(po.back() + (int32_t)(rng() % 4 == 0 ? rng() % 40 : rng() % 7));
    for (int w = 0; w < nw; ++w) so.push_back(so.back() + (int32_t)ocr::lat_span_count(po[w + 1] - po[w], M));
    ocr::LexLatPlan plan;
    ocr::lexlat_plan(lex.start, so.data(), po.data(), nw, so.back(), M, d, plan);
    ++plans;
    REQUIRE((int)plan.jobs.size() == nw && (int)plan.flags.size() == nw && (int)plan.n_candidates.size() == nw && plan.n_pieces == po.back(), "plan sizes");
    int32_t max_range = 0;
    for (int w = 0; w < nw; ++w) {
      const int G = po[w + 1] - po[w];
      const ocr::LexLatJob& j = plan.jobs[w];
      REQUIRE(j.s0 == so[w] && j.p0 == po[w] && j.G == G, "rows of word %d", w);
      int want = 0;
      if (G >= 1 && G <= ocr::kLatMaxPieces) {
        const int lo = std::max(1, (G + M - 1) / M - d), hi = std::min(32, G + d);
        for (int len : elen) want += len >= lo && len <= hi;
        REQUIRE(j.r0 >= 0 && j.r1 <= ne && j.r0 <= j.r1, "range of word %d", w);
        for (int p = j.r0; p < j.r1; ++p) REQUIRE(lex.lens[p] >= lo && lex.lens[p] <= hi, "an entry of length %d in the range of word %d", lex.lens[p], w);
      } else {
        REQUIRE(j.r0 == 0 && j.r1 == 0, "a flagged word %d has a range", w);
      }
      REQUIRE(j.r1 - j.r0 == want && plan.n_candidates[w] == want, "word %d: %d candidates, %d counted", w, j.r1 - j.r0, want);
      REQUIRE(plan.flags[w] == (G == 0 ? 1 : G > ocr::kLatMaxPieces ? 2 : want == 0 ? 4 : 0), "flag of word %d", w);
      REQUIRE(ocr::lat_span_count(G, M) <= ocr::kLexLatMaxRows || G > ocr::kLatMaxPieces, "rows of a matched word exceed the table");
      max_range = std::max(max_range, j.r1 - j.r0);
      candidates += want;
    }
    REQUIRE(plan.max_range == max_range, "max_range");
    {
      const int broke = (int)(rng() % 11);
      std::vector<int32_t> bs = so, bp = po;
      const int32_t *sp = bs.data(), *pp = bp.data(), *st = lex.start;
      int n_arg = nw, s_arg = so.back(), m_arg = M, d_arg = d;
      const int w = nw ? (int)(rng() % nw) : 0;
      if (broke == 0) sp = nullptr; else if (broke == 1) pp = nullptr; else if (broke == 2) bs[0] = 1; else if (broke == 3) bp[0] = 2;
      else if (broke == 4) s_arg += 1 + (int)(rng() % 3); else if (broke == 5) n_arg = -1 - (int)(rng() % 3);
      else if (broke == 6 && nw) { for (int k = w + 1; k <= nw; ++k) bs[k] += 1; s_arg += 1; }            // one span too many in word w
      else if (broke == 7 && nw) { for (int k = w + 1; k <= nw; ++k) bp[k] += 1; }                        // one piece more than the spans say
      else if (broke == 8 && nw >= 2) { const int k = 1 + (int)(rng() % (nw - 1)); bp[k] = bp[k + 1] + 1; }
      else if (broke == 9) st = nullptr;
      else if (rng() % 2) m_arg = rng() % 2 ? 0 : 5;
      else d_arg = rng() % 2 ? -1 : 9;
      try { ocr::lexlat_plan(st, sp, pp, n_arg, s_arg, m_arg, d_arg, plan); REQUIRE(false, "broken offsets (%d) were planned", broke); }
      catch (const ocr::Error&) { ++refused; }
    }
  }
  printf("%d plans, %ld candidates, %d refused\n", plans, candidates, refused);
  return 0;
}
