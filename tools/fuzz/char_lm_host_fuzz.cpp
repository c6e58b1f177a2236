// ASan/UBSan run of the host side of the character language model (csrc/char_lm_host.cpp): the model check on random tables, valid and
// broken (a NaN, an infinity, a negative value, a nonzero unused cell: the message must name the first offending cell), the parameter
// check on values in and out of range, and the per-call plan on random offsets, valid and broken.  A plan is checked against its
// source: flags, the count of decoded words, the workgroups and the buffer sizes; every outcome of a broken input must be an ocr::Error.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "char_lm_host.hpp"
int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 3000;
  std::mt19937 rng(8765);
  int accepted = 0, refused = 0, planned = 0;
  try {
    ocr::lm_check_model(nullptr);
    printf("a null model was accepted\n");
    return 1;
  } catch (const ocr::Error&) { ++refused; }
  for (int it = 0; it < iters; ++it) {
    std::vector<float> T(64 * 64, 0.0f);
    for (int p = 0; p < 63; ++p)
      for (int c = 0; c < 63; ++c)
        if (!(p == 62 && c == 62)) T[p * 64 + c] = (rng() % 5 == 0) ? 0.0f : (rng() % 7 == 0 ? 1e30f : (float)(rng() % 1000) / 64.0f);
    const int kind = (int)(rng() % 8);   // 0..2 valid, the rest one or two defects
    int bp = -1, bc = -1;
    auto put = [&](int p, int c, float v) {
      T[p * 64 + c] = v;
      if (bp < 0 || p * 64 + c < bp * 64 + bc) { bp = p; bc = c; }
    };
    const float bads[4] = {NAN, INFINITY, -INFINITY, -0.5f};
    if (kind == 3 || kind == 4) {
      for (int n = 0; n < kind - 2; ++n) {
        int p = (int)(rng() % 63), c = (int)(rng() % 63);
        if (p == 62 && c == 62) c = 0;
        put(p, c, bads[rng() % 4]);
      }
    } else if (kind == 5) put(63, (int)(rng() % 64), 1.0f);
    else if (kind == 6) put((int)(rng() % 64), 63, rng() % 2 ? 2.0f : NAN);
    else if (kind == 7) put(62, 62, 0.25f);
    try {
      ocr::lm_check_model(T.data());
      ++accepted;
      if (kind >= 3) { printf("iteration %d: a broken model was accepted\n", it); return 1; }
    } catch (const ocr::Error& e) {
      ++refused;
      if (kind < 3) { printf("iteration %d: a valid model was refused: %s\n", it, e.what()); return 1; }
      char want[32];
      snprintf(want, sizeof want, "[%d][%d]", bp, bc);
      if (!strstr(e.what(), want)) { printf("iteration %d: the message '%s' does not name %s\n", it, e.what(), want); return 1; }
    }

    ocr_lm_params_t q{1 + (int32_t)(rng() % 8), {0, 0, 0}};
    const int f = (int)(rng() % 10);
    if (f == 0) q.top_k = 0; else if (f == 1) q.top_k = 9; else if (f == 2) q.top_k = -(int32_t)(rng() % 100) - 1; else if (f == 3) q.reserved[rng() % 3] = 1 + (int32_t)(rng() % 9);
    else if (f == 4) q.top_k = 0x7FFFFFFF;
    try { ocr::lm_check_params(q); if (f < 5) { printf("iteration %d: bad parameters accepted\n", it); return 1; } }
    catch (const ocr::Error&) { if (f >= 5) { printf("iteration %d: good parameters refused\n", it); return 1; } ++refused; }

    // the plan on random words, then on broken offsets
    const int nw = (int)(rng() % 40), top_k = 1 + (int)(rng() % 8);
    std::vector<int32_t> wo(1, 0);
    for (int w = 0; w < nw; ++w) wo.push_back(wo.back() + (int32_t)(rng() % 36));
    ocr::LmPlan plan;
    ocr::lm_plan(wo.data(), nw, wo.back(), top_k, plan);
    ++planned;
    int decoded = 0;
    for (int w = 0; w < nw; ++w) {
      const int G = wo[w + 1] - wo[w];
      const int want = G == 0 ? 1 : G > ocr::kLmMaxLen ? 2 : 0;
      decoded += want == 0;
      if (plan.flags[w] != want) { printf("iteration %d: flag of word %d\n", it, w); return 1; }
    }
    if ((int)plan.flags.size() != nw || plan.n_decoded != decoded || plan.blocks != (nw + ocr::kLmWords - 1) / ocr::kLmWords ||
        plan.link_bytes != (size_t)wo.back() * 64 * top_k * 2 || plan.label_count != (size_t)wo.back() * top_k) {
      printf("iteration %d: plan\n", it);
      return 1;
    }
    const int broke = (int)(rng() % 5);
    std::vector<int32_t> bo = wo;
    int n_arg = nw, g_arg = wo.back();
    const int32_t* ptr = bo.data();
    if (broke == 0) bo[0] = 1 + (int32_t)(rng() % 3);
    else if (broke == 1) g_arg += 1 + (int)(rng() % 3);
    else if (broke == 2) n_arg = -1 - (int)(rng() % 3);
    else if (broke == 3) ptr = nullptr;
    else if (nw >= 2) { const int k = 1 + (int)(rng() % (nw - 1)); bo[k] = bo[k + 1] + 1 + (int32_t)(rng() % 3); }
    else g_arg = -1;
    try {
      ocr::lm_plan(ptr, n_arg, g_arg, top_k, plan);
      printf("iteration %d: broken offsets (%d) were planned\n", it, broke);
      return 1;
    } catch (const ocr::Error&) { ++refused; }
  }
  printf("%d models accepted, %d plans, %d refused\n", accepted, planned, refused);
  return 0;
}
