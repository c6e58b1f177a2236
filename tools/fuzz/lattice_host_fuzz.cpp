// ASan/UBSan run of the host side of the segmentation lattice (csrc/lattice_host.cpp): the two parameter checks on values in and out of
// range, the span table of random piece blocks checked against its definition (counts, order, union boxes), broken blocks, and the
// decode's plan on random offsets, valid and broken (a wrong span count, a wrong end, decreasing pieces, null pointers).  Every
// outcome of a broken input must be an ocr::Error.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "lattice_host.hpp"

#define REQUIRE(cond, ...) do { if (!(cond)) { printf("iteration %d: ", it); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 3000;
  std::mt19937 rng(4321);
  int tables = 0, plans = 0, refused = 0;
  for (int it = 0; it < iters; ++it) {
    // ---- parameters
    {
      ocr_split_params_t s{25 + (int32_t)(rng() % 376), 1 + (int32_t)(rng() % 4), 3 + (int32_t)(rng() % 62), 1 + (int32_t)(rng() % 256), {0, 0, 0, 0}};
      const int f = (int)(rng() % 14);
      if (f == 0) s.aspect_pct = 24; else if (f == 1) s.aspect_pct = 401; else if (f == 2) s.max_pieces = 0; else if (f == 3) s.max_pieces = 5;
      else if (f == 4) s.min_piece_w = 2; else if (f == 5) s.min_piece_w = 65; else if (f == 6) s.max_word_pieces = 0;
      else if (f == 7) s.max_word_pieces = 257; else if (f == 8) s.reserved[rng() % 4] = 1 + (int32_t)(rng() % 9); else if (f == 9) s.aspect_pct = INT32_MIN;
      try { ocr::split_check_params(s); REQUIRE(f >= 10, "bad split parameters accepted (%d)", f); }
      catch (const ocr::Error&) { REQUIRE(f < 10, "good split parameters refused"); ++refused; }
      ocr_lattice_params_t q{1 + (int32_t)(rng() % 4), 1 + (int32_t)(rng() % 8), {0, 0, 0, 0}, {0, 0}};
      for (double& v : q.span_cost) v = (rng() % 3 == 0) ? 0.0 : (rng() % 5 == 0 ? 1e30 : (double)(rng() % 1000) / 64.0);
      const int h = (int)(rng() % 14);
      const double bads[5] = {NAN, INFINITY, -INFINITY, -0.5, -4.9e-324};
      if (h == 0) q.max_span = 0; else if (h == 1) q.max_span = 5; else if (h == 2) q.top_k = 0; else if (h == 3) q.top_k = 9;
      else if (h == 4) q.reserved[rng() % 2] = 3; else if (h == 5 || h == 6) q.span_cost[rng() % 4] = bads[rng() % 5]; else if (h == 7) q.top_k = INT32_MAX;
      try { ocr::lat_check_params(q); REQUIRE(h >= 8, "bad lattice parameters accepted (%d)", h); }
      catch (const ocr::Error&) { REQUIRE(h < 8, "good lattice parameters refused"); ++refused; }
    }

    // ---- the span table of a random piece block
    const int nw = (int)(rng() % 12), M = 1 + (int)(rng() % 4);
    std::vector<int32_t> po(1, 0), boxes;
    for (int w = 0; w < nw; ++w) po.push_back(po.back() + (int32_t)(rng() % 3 == 0 ? rng() % 40 : rng() % 6));
    for (int k = 0; k < po.back(); ++k) {
      const int32_t x0 = (int32_t)(rng() % 500), y0 = (int32_t)(rng() % 100);
      const int32_t b[4] = {x0, y0, x0 + 1 + (int32_t)(rng() % 30), y0 + 1 + (int32_t)(rng() % 30)};
      boxes.insert(boxes.end(), b, b + 4);
    }
    ocr_glyphs_t g{};
    g.n_images = 1;
    g.n_words = nw;
    g.n_glyphs = po.back();
    g.word_offsets = po.data();
    g.boxes = boxes.data();
    ocr::SpanBlock sb;
    ocr::lat_spans(g, M, sb);
    ++tables;
    REQUIRE((int)sb.span_offsets.size() == nw + 1 && sb.span_offsets[0] == 0, "span offsets");
    size_t row = 0;
    for (int w = 0; w < nw; ++w) {
      const int G = po[w + 1] - po[w];
      REQUIRE(sb.span_offsets[w + 1] - sb.span_offsets[w] == ocr::lat_span_count(G, M), "span count of word %d", w);
      for (int e = 1; e <= G; ++e)
        for (int m = 1; m <= std::min(M, e); ++m, ++row) {
          REQUIRE(sb.span_word[row] == w && sb.span_end[row] == e && sb.span_len[row] == m, "order at row %zu", row);
          int32_t u[4] = {INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN};
          for (int k = po[w] + e - m; k < po[w] + e; ++k) {
            u[0] = std::min(u[0], boxes[4 * k]); u[1] = std::min(u[1], boxes[4 * k + 1]);
            u[2] = std::max(u[2], boxes[4 * k + 2]); u[3] = std::max(u[3], boxes[4 * k + 3]);
          }
          REQUIRE(std::equal(u, u + 4, &sb.boxes[4 * row]), "union box at row %zu", row);
        }
    }
    REQUIRE(row == sb.span_word.size() && row * 4 == sb.boxes.size(), "span total");
    if (M == 1) REQUIRE(sb.boxes == boxes && sb.span_offsets == po, "M = 1 is not the piece block");
    {
      const int broke = (int)(rng() % 6);
      std::vector<int32_t> bo = po;
      ocr_glyphs_t b = g;
      int m_arg = M;
      b.word_offsets = bo.data();
      if (broke == 0) bo[0] = 1; else if (broke == 1) b.n_glyphs += 1; else if (broke == 2) m_arg = rng() % 2 ? 0 : 5; else if (broke == 3) b.word_offsets = nullptr;
      else if (broke == 4) b.n_words = -1;
      else if (nw >= 2) { const int k = 1 + (int)(rng() % (nw - 1)); bo[k] = bo[k + 1] + 1; }
      else m_arg = -3;
      try { ocr::lat_spans(b, m_arg, sb); REQUIRE(false, "a broken block (%d) got a span table", broke); }
      catch (const ocr::Error&) { ++refused; }
    }

    // ---- the plan of a decode
    const int top_k = 1 + (int)(rng() % 8);
    std::vector<int32_t> so(1, 0);
    for (int w = 0; w < nw; ++w) so.push_back(so.back() + (int32_t)ocr::lat_span_count(po[w + 1] - po[w], M));
    ocr::LatPlan plan;
    ocr::lat_plan(so.data(), po.data(), nw, so.back(), M, top_k, plan);
    ++plans;
    for (int w = 0; w < nw; ++w) {
      const int G = po[w + 1] - po[w];
      REQUIRE(plan.flags[w] == (G == 0 ? 1 : G > ocr::kLatMaxPieces ? 2 : 0), "flag of word %d", w);
    }
    REQUIRE((int)plan.flags.size() == nw && plan.n_pieces == po.back() && plan.blocks == (nw + ocr::kLatWords - 1) / ocr::kLatWords &&
                plan.link_bytes == (size_t)po.back() * 64 * top_k * 2 && plan.label_count == (size_t)po.back() * top_k, "plan");
    {
      const int broke = (int)(rng() % 9);
      std::vector<int32_t> bs = so, bp = po;
      const int32_t *sp = bs.data(), *pp = bp.data();
      int n_arg = nw, s_arg = so.back(), m_arg = M, k_arg = top_k;
      const int w = nw ? (int)(rng() % nw) : 0;
      if (broke == 0) sp = nullptr; else if (broke == 1) pp = nullptr; else if (broke == 2) bs[0] = 1; else if (broke == 3) bp[0] = 2;
      else if (broke == 4) s_arg += 1 + (int)(rng() % 3); else if (broke == 5) n_arg = -1 - (int)(rng() % 3);
      else if (broke == 6 && nw) { for (int k = w + 1; k <= nw; ++k) bs[k] += 1; s_arg += 1; }            // one span too many in word w
      else if (broke == 7 && nw) { for (int k = w + 1; k <= nw; ++k) bp[k] += 1; }                        // one piece more than the spans say
      else if (broke == 8 && nw >= 2) { const int k = 1 + (int)(rng() % (nw - 1)); bp[k] = bp[k + 1] + 1; }
      else k_arg = 9;
      try { ocr::lat_plan(sp, pp, n_arg, s_arg, m_arg, k_arg, plan); REQUIRE(false, "broken offsets (%d) were planned", broke); }
      catch (const ocr::Error&) { ++refused; }
    }
  }
  printf("%d span tables, %d plans, %d refused\n", tables, plans, refused);
  return 0;
}
