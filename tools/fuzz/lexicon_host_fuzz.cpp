// ASan/UBSan run of the host side of lexicon matching (csrc/lexicon_host.cpp): the packer on random word lists, valid and broken
// (bad bytes, empty and over-long entries, offsets that decrease or start off zero), the parameter check on values in and out of
// range, and the per-word plan on random offsets.  A packed list is checked against its source: every entry is found at one sorted
// position with its length, its caller's index and its class indices; every outcome of a broken input must be an ocr::Error.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>
#include "lexicon_host.hpp"
static const char* kAlphabet = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789";
int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 3000;
  std::mt19937 rng(4321);
  int packed = 0, refused = 0, planned = 0;
  for (int it = 0; it < iters; ++it) {
    const int n = 1 + (int)(rng() % 600);
    std::string bytes;
    std::vector<int32_t> off(1, 0);
    for (int k = 0; k < n; ++k) {
      const int len = 1 + (int)(rng() % ocr::kLexMaxLen);
      for (int j = 0; j < len; ++j) bytes.push_back(kAlphabet[rng() % 62]);
      off.push_back((int32_t)bytes.size());
    }
    bytes.append(64, 'x');               // (the call has no byte count: a moved offset must still point into the caller's buffer)
    const int kind = (int)(rng() % 8);   // 0..2 valid, the rest one defect each
    int n_arg = n;
    if (kind == 3) bytes[rng() % (bytes.size() - 64)] = (char)(rng() % 2 ? ' ' : 0xe9);
    else if (kind == 4 && n > 1) off[1 + rng() % (n - 1)] = off[rng() % n] + (rng() % 2 ? 40 : 0);
    else if (kind == 5) off[0] = 1;
    else if (kind == 6) n_arg = rng() % 2 ? 0 : -3;
    else if (kind == 7 && n > 2) { const int k = 1 + (int)(rng() % (n - 1)); off[k] = off[k - 1]; }
    ocr::LexPacked p;
    try {
      ocr::lex_pack(bytes.data(), off.data(), n_arg, p);
      ++packed;
      if (p.n != n_arg || p.start[ocr::kLexMaxLen + 1] != n_arg) { printf("iteration %d: packed %d of %d\n", it, p.n, n_arg); return 1; }
      std::vector<char> seen(n_arg, 0);
      for (int pos = 0; pos < p.n; ++pos) {
        const int k = p.index[pos], len = p.lens[pos];
        if (k < 0 || k >= n_arg || seen[k] || len != off[k + 1] - off[k] || pos < p.start[len] || pos >= p.start[len + 1] ||
            (pos > 0 && p.lens[pos - 1] == len && p.index[pos - 1] > k)) { printf("iteration %d: position %d is wrong\n", it, pos); return 1; }
        seen[k] = 1;
        for (int j = 0; j < ocr::kLexMaxLen; ++j) {
          const unsigned c = (p.codes[(size_t)(j / 4) * p.n + pos] >> (8 * (j % 4))) & 0xFF;
          if (j < len ? kAlphabet[c] != bytes[off[k] + j] : c != 0) { printf("iteration %d: entry %d character %d\n", it, k, j); return 1; }
        }
      }
      // the plan on random words, then on broken offsets
      const int nw = (int)(rng() % 40);
      std::vector<int32_t> wo(1, 0);
      for (int w = 0; w < nw; ++w) wo.push_back(wo.back() + (int32_t)(rng() % 36));
      ocr::LexPlan plan;
      ocr::lex_plan(p.start, wo.data(), nw, wo.back(), (int)(rng() % 9), plan);
      ++planned;
      for (int w = 0; w < nw; ++w) {
        const ocr::LexWordJob& j = plan.jobs[w];
        if (j.r0 < 0 || j.r1 < j.r0 || j.r1 > p.n || plan.n_candidates[w] != j.r1 - j.r0 || j.r1 - j.r0 > plan.max_range ||
            ((j.G == 0 || j.G > ocr::kLexMaxLen) && j.r1 != j.r0)) { printf("iteration %d: job %d\n", it, w); return 1; }
      }
      if (plan.max_range > 0 && (ocr::lex_span(nw, plan.max_range) < 1)) return 1;
      if (nw > 0) {
        try { wo[rng() % wo.size()] += 1 + (int32_t)(rng() % 3); ocr::lex_plan(p.start, wo.data(), nw, wo.back() + (wo.size() > 1 ? 0 : 1), 2, plan); }
        catch (const ocr::Error&) { ++refused; }
      }
    } catch (const ocr::Error&) {
      ++refused;
      if (kind < 3) { printf("iteration %d: a valid list was refused\n", it); return 1; }
    }
    ocr_lexicon_params_t q{4.0, 4.0, 2, 1, 1, {0, 0, 0}};
    const int f = (int)(rng() % 12);
    if (f == 0) q.ins_cost = -1; else if (f == 1) q.del_cost = NAN; else if (f == 2) q.ins_cost = INFINITY; else if (f == 3) q.max_len_diff = 9;
    else if (f == 4) q.fold_case = 2; else if (f == 5) q.top_k = 0; else if (f == 6) q.top_k = 9; else if (f == 7) q.reserved[2] = 1;
    try { ocr::lex_check_params(q); if (f < 8) { printf("iteration %d: bad parameters accepted\n", it); return 1; } }
    catch (const ocr::Error&) { if (f >= 8) { printf("iteration %d: good parameters refused\n", it); return 1; } ++refused; }
  }
  printf("%d packed, %d planned, %d refused\n", packed, planned, refused);
  return 0;
}
