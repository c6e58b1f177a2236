// The order-critical device code shared by the word-search kernels (lexicon.hip, lexicon_lattice.hip, lexicon_phrase.hip,
// char_lm.hip, lattice.hip): written once, because a slip in any of it changes which of two tied candidates is returned.
//
// The tie rules.  A candidate is a pair (cost, index) and key_less is its total order: the smaller cost first, of equal costs the
// smaller index.  The index is whatever names a candidate uniquely where they meet - the caller's index of a lexicon entry, the class
// of a lane, the lane itself -, so two candidates never compare equal and the winner of any reduction by key_less is the same
// whatever the lanes, waves, chunks or passes the candidates were spread over.  An empty slot is (+inf, kNoIndex): behind every
// candidate.  Every reduction here is by that order: best_insert keeps a lane's K smallest sorted by it, wave_argmin is the plain xor
// butterfly (widths 32 down to 1, every lane ends with the wave's minimum), slots_argmin reads the waves' minima back from LDS in
// slot order, merge_slots takes the smallest key above the previous winner.  list_insert is the one other rule: its candidates arrive
// in the order of their tie-break already, so one is inserted behind its equals (strict < on the value alone).
// Costs are compared and moved, never recomputed: nothing here rounds.
#pragma once
#include <cfloat>
#include <cmath>

#include "lexicon_host.hpp"

namespace ocr {

constexpr int kNoIndex = 0x7FFFFFFF;   // the index of an empty best-k slot: with cost +inf it is behind every entry

template <typename T>
__device__ inline bool key_less(T ca, int ia, T cb, int ib) { return ca < cb || (ca == cb && ia < ib); }

__device__ inline double readlane_f64(double x, int l) {   // l is uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
  return __hiloint2double(hi, lo);
}

// ---- a lane's best K by key_less, sorted in registers (static indices only)
template <int K>
__device__ inline void best_clear(double (&best_c)[K], int (&best_i)[K]) {
#pragma unroll
  for (int t = 0; t < K; ++t) {
    best_c[t] = INFINITY;
    best_i[t] = kNoIndex;
  }
}

template <int K>
__device__ inline void best_insert(double (&best_c)[K], int (&best_i)[K], double nc, int ni) {
#pragma unroll
  for (int t = 0; t < K; ++t) {
    if (key_less(nc, ni, best_c[t], best_i[t])) {
      const double c = best_c[t];
      const int x = best_i[t];
      best_c[t] = nc;
      best_i[t] = ni;
      nc = c;
      ni = x;
    }
  }
}

template <int K>
__device__ inline void best_pop(double (&best_c)[K], int (&best_i)[K]) {
#pragma unroll
  for (int t = 0; t + 1 < K; ++t) {
    best_c[t] = best_c[t + 1];
    best_i[t] = best_i[t + 1];
  }
  best_c[K - 1] = INFINITY;
  best_i[K - 1] = kNoIndex;
}

// a sorted list whose candidates arrive in tie-break order: behind its equals; what it displaces moves down
template <int K>
__device__ inline void list_insert(double (&bv)[K], int (&bc)[K], double nv, int nc) {
  bool ins = false;
#pragma unroll
  for (int t = 0; t < K; ++t) {
    ins = ins || nv < bv[t];
    const double ov = bv[t];
    const int oc = bc[t];
    bv[t] = ins ? nv : ov;
    bc[t] = ins ? nc : oc;
    nv = ins ? ov : nv;
    nc = ins ? oc : nc;
  }
}

// ---- wave butterflies: every lane ends with the result of all 64
__device__ inline float wave_max(float v) {
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) v = fmaxf(v, __shfl_xor(v, k, 64));
  return v;
}

__device__ inline float wave_min(float v) {
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) v = fminf(v, __shfl_xor(v, k, 64));
  return v;
}

// T = double: (cost, index), (value, class), (value, lane); T = float: the (cost, class) of a greedy pass
template <typename T>
__device__ inline void wave_argmin(T& c, int& x) {
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) {
    const T oc = __shfl_xor(c, k, 64);
    const int ox = __shfl_xor(x, k, 64);
    if (key_less(oc, ox, c, x)) {
      c = oc;
      x = ox;
    }
  }
}

// the workgroup's minimum out of the LDS slots its kLexChunk / 64 waves wrote (after the barrier): wave v's slot is at v * stride
__device__ inline void slots_argmin(const double* slot_c, const int32_t* slot_i, int stride, double& c, int& x) {
  c = slot_c[0];
  x = slot_i[0];
#pragma unroll
  for (int v = 1; v < kLexChunk / 64; ++v)
    if (key_less(slot_c[v * stride], slot_i[v * stride], c, x)) {
      c = slot_c[v * stride];
      x = slot_i[v * stride];
    }
}

// ---- cost rows
// the cost rows [first_row, first_row + rows) -> tab, rows of 64 floats (class c in bank c), folded when fold is set
__device__ inline void stage_cost_rows(float (*tab)[64], const float* __restrict__ costs, int first_row, int rows, int fold, int tid,
                                       int threads) {
  for (int t = tid; t < rows * 64; t += threads) {
    const int i = t >> 6, c = t & 63;
    float v = 0.0f;
    if (c < kLexClasses) {
      const float* row = costs + (size_t)(first_row + i) * kLexClasses;
      v = row[c];
      if (fold && c < 52) v = fminf(v, row[c < 26 ? c + 26 : c - 26]);
    }
    tab[i][c] = v;
  }
}

// the minimum of cost row `row` in every lane (f32, which is exact), and the check of its costs
__device__ inline float row_min_checked(const float* __restrict__ costs, size_t row, int lane, bool& bad) {
  float v = INFINITY;
  if (lane < kLexClasses) {
    v = costs[row * kLexClasses + lane];
    bad |= !(v >= 0.0f && v <= FLT_MAX);   // NaN, +-inf or negative
  }
  return wave_min(v);
}

// ---- the body of the two merge kernels (lex_merge_kernel, lexlat_merge_kernel: one wave per word, whose candidates are [r0, r1)):
// top_k rounds over the slots of all the word's chunks, each taking the smallest key above the previous winner.  The key is a total
// order, so neither the chunking nor the layout shows in the result.
__device__ inline void merge_slots(int r0, int r1, int n_chunks, int span, int top_k, const double* __restrict__ part_cost,
                                   const int32_t* __restrict__ part_idx, int32_t* __restrict__ entries, double* __restrict__ out_cost) {
  const int w = blockIdx.x, lane = threadIdx.x;
  const int per = span * kLexChunk;
  const int live = (r1 - r0 + per - 1) / per;   // the chunks of this word that wrote their slots (at most n_chunks)
  const int total = live * top_k;
  const size_t slot = (size_t)w * n_chunks * top_k;
  double prev_c = -1.0;   // below every key: costs are >= 0
  int prev_i = -1;
  for (int r = 0; r < top_k; ++r) {
    double c = INFINITY;
    int x = kNoIndex;
    for (int t = lane; t < total; t += 64) {
      const double pc = part_cost[slot + t];
      const int px = part_idx[slot + t];
      if (px >= 0 && key_less(prev_c, prev_i, pc, px) && key_less(pc, px, c, x)) {
        c = pc;
        x = px;
      }
    }
    wave_argmin(c, x);
    if (lane == 0) {
      entries[(size_t)w * top_k + r] = x == kNoIndex ? -1 : x;
      out_cost[(size_t)w * top_k + r] = c;
    }
    prev_c = c;
    prev_i = x;
  }
}

}  // namespace ocr
