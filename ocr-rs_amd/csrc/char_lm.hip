// Character-bigram language model: the glyphs of a word decoded as the cheapest paths through their classes under glyph cost plus
// transition cost (BUILD-DEFINED; rule in include/ocr_amd.h at ocr_lm_decode, oracle tests/char_lm_oracle.py).  f64, every operation
// separately rounded, adds and mins only: this file is compiled with -ffp-contract=off.
//   lm_decode_kernel<K>  one wave per word, class c in lane c, kLmWords words per workgroup which share the model in LDS as 64 rows of 64
//                        floats (lane c reads T[p][c], bank c: no conflict, and the loop over p is uniform).
//                        First the greedy reading of the word: per glyph a wave argmin by (cost, class), the transition and the glyph
//                        cost added in f64, and the check of every cost (the first bad word is kept by atomicMin; such a word is not
//                        decoded).  Then list Viterbi: every lane keeps the K best (value, p, r) of its class sorted in registers
//                        (static indices only: no scratch).  A step reads the previous lists by v_readlane with the uniform p (no LDS
//                        round trip, no barrier inside a wave) and leaves p's list at the first rank that enters no lane's list:
//                        the lists are sorted in r and a rounded add is monotone, so nothing behind it can enter either.  Candidates
//                        arrive in (p, r) order and are inserted behind their equals, which is the key (value, p, r).  Only ranks
//                        below top_k are read: a list cut at top_k is the prefix of the list cut at K (a candidate of rank r has r
//                        candidates of the same p in front of it), so K = 8 serves every top_k above 1 exactly.  K = 1 has no list
//                        to leave: its loop over p is branch-free, in groups of 8 whose LDS reads are in flight together.
//                        Back-pointers p | r << 6 as uint16 go to a per-call device buffer [glyph][rank][64]: 32 KB of LDS per word at
//                        K = 8 and 32 glyphs would leave one workgroup per CU, the buffer costs one coalesced 128-byte store per rank
//                        and step.  The end: top_k rounds of a wave argmin over (value, c, r) - lane c offers the head of its list,
//                        the winner pops it -, then lane k walks hypothesis k back along the links and stores its labels.
//                        The butterflies, the list insertion and the f64 readlane are word_search.hpp's, shared with lattice.hip.
// LDS: 16 KB per workgroup.  Registers and scratch: DESIGN.md 3.21 and docs/vmcnt_audit.md.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>

#include "api_internal.hpp"
#include "char_lm_host.hpp"
#include "word_search.hpp"

namespace ocr {
namespace {

template <int K>
__global__ __launch_bounds__(kLmWords * 64) void lm_decode_kernel(const float* __restrict__ costs, const int32_t* __restrict__ word_off,
                                                                  int n_words, int n_glyphs, const float* __restrict__ trans, int top_k,
                                                                  uint16_t* __restrict__ links, int32_t* __restrict__ labels,
                                                                  double* __restrict__ out_cost, double* __restrict__ raw,
                                                                  int32_t* __restrict__ bad_word) {
  __shared__ float T[kLmStride][kLmStride];
  for (int t = threadIdx.x; t < kLmStride * kLmStride; t += kLmWords * 64) (&T[0][0])[t] = trans[t];
  __syncthreads();   // the only barrier: whole waves leave behind it
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * kLmWords + (threadIdx.x >> 6);
  if (w >= n_words) return;
  const int g0 = word_off[w], G = word_off[w + 1] - g0;
  const bool cls = lane < kLmClasses;

  // the greedy reading and the check of every cost (a word of any length)
  {
    double acc = 0.0;
    int prev = kLmBegin;
    bool bad = false;
    for (int i = 0; i < G; ++i) {
      float v = INFINITY;
      if (cls) {
        v = costs[(size_t)(g0 + i) * kLmClasses + lane];
        bad |= !(v >= 0.0f && v <= FLT_MAX);   // NaN, +-inf or negative
      }
      int c = lane;
      wave_argmin(v, c);   // the first minimum: by (cost, class)
      acc = acc + (double)T[prev][c];
      acc = acc + (double)v;
      prev = c;
    }
    if (G > 0) acc = acc + (double)T[prev][kLmEnd];
    if (lane == 0) raw[w] = acc;
    if (bad) atomicMin(bad_word, w);
    if (G < 1 || G > kLmMaxLen || __any(bad)) {   // uniform: not decoded (the labels were preset to -1)
      if (lane < top_k) out_cost[(size_t)w * top_k + lane] = INFINITY;
      return;
    }
  }

  double bv[K];   // the list of class `lane`: values ascending, +inf past its length
  int bc[K];      // p | r << 6 of the link
  bv[0] = (double)T[kLmBegin][lane] + (double)(cls ? costs[(size_t)g0 * kLmClasses + lane] : 0.0f);
  bc[0] = 0;
#pragma unroll
  for (int t = 1; t < K; ++t) {
    bv[t] = INFINITY;
    bc[t] = 0;
  }

  for (int i = 1; i < G; ++i) {
    const float gc = cls ? costs[(size_t)(g0 + i) * kLmClasses + lane] : 0.0f;
    double pv[K];
#pragma unroll
    for (int t = 0; t < K; ++t) {
      pv[t] = bv[t];
      bv[t] = INFINITY;
      bc[t] = 0;
    }
    if constexpr (K == 1) {
      // one value per class: no list to leave early, so the loop is branch-free, in groups of 8 whose LDS reads are in flight together
      auto relax = [&](int p) {
        const double nv = readlane_f64(pv[0], p) + (double)T[p][lane];
        const bool ins = nv < bv[0];   // the first minimum: p ascends
        bv[0] = ins ? nv : bv[0];
        bc[0] = ins ? p : bc[0];
      };
#pragma unroll 1
      for (int p0 = 0; p0 < 56; p0 += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) relax(p0 + j);
      }
#pragma unroll
      for (int p = 56; p < kLmClasses; ++p) relax(p);
    }
    for (int p = 0; K > 1 && p < kLmClasses; ++p) {
      const double tr = (double)T[p][lane];
#pragma unroll
      for (int r = 0; r < K; ++r) {
        if (r >= top_k) break;                  // uniform
        const double s = readlane_f64(pv[r], p);
        if (s == INFINITY) break;               // uniform: the end of p's list
        const double nv = s + tr;
        if (!__any(cls && nv < bv[K - 1])) break;   // uniform: enters no list, and neither does a later rank
        list_insert(bv, bc, nv, p | (r << 6));
      }
    }
#pragma unroll
    for (int t = 0; t < K; ++t) {
      bv[t] = bv[t] + (double)gc;
      if (t < top_k) links[((size_t)(g0 + i) * top_k + t) * kLmStride + lane] = (uint16_t)bc[t];
    }
  }

  const double end = (double)T[cls ? lane : 0][kLmEnd];
#pragma unroll
  for (int t = 0; t < K; ++t) bv[t] = cls ? bv[t] + end : INFINITY;
  int popped = 0, my_c = 0, my_r = 0;
  for (int k = 0; k < top_k; ++k) {
    double v = bv[0];
    int c = lane;
    wave_argmin(v, c);   // by (value, class); the rank is the winner's own
    const int r = __shfl(popped, c, 64);
    if (lane == 0) out_cost[(size_t)w * top_k + k] = v;
    if (lane == k) {
      my_c = c;
      my_r = r;
    }
    if (lane == c) {
#pragma unroll
      for (int t = 0; t + 1 < K; ++t) bv[t] = bv[t + 1];
      bv[K - 1] = INFINITY;
      ++popped;
    }
  }
  __threadfence();   // the links of this wave, written by other lanes, before lane k reads them
  if (lane < top_k) {
    int c = my_c, r = my_r;
    for (int i = G - 1; i >= 0; --i) {
      labels[(size_t)lane * n_glyphs + g0 + i] = c;
      if (i > 0) {
        const int code = links[((size_t)(g0 + i) * top_k + r) * kLmStride + c];
        c = code & 63;
        r = code >> 6;
      }
    }
  }
}

}  // namespace
}  // namespace ocr

// ---- the C surface (include/ocr_amd.h)
// (struct ocr_char_lm: api_internal.hpp - lattice.hip decodes under the same model)
namespace {
struct PathsOwned {   // the library-owned storage behind an ocr_lm_paths_t* (released by ocr_lm_paths_free)
  ocr_lm_paths_t view{};
  std::vector<int32_t> labels, word_flags;
  std::vector<double> costs, raw_costs;
  void finish(int n_words, int top_k, int n_glyphs) {
    view.n_words = n_words;
    view.top_k = top_k;
    view.n_glyphs = n_glyphs;
    view.labels = labels.data();
    view.costs = costs.data();
    view.raw_costs = raw_costs.data();
    view.word_flags = word_flags.data();
  }
};
constexpr int32_t kNone = 0x7F7F7F7F;   // what a byte memset of 0x7F leaves: above every word index
}  // namespace

extern "C" {

int ocr_char_lm_create(ocr_rec_t* rec, const float* trans, ocr_char_lm_t** out) {
  return ocr::guard([&] {
    using namespace ocr;
    if (!rec || !out) fail(OCR_ERR_INVALID, "char_lm_create: null argument");
    *out = nullptr;
    lm_check_model(trans);
    std::unique_ptr<ocr_char_lm> lm(new ocr_char_lm());
    lm->device = rec->impl.device();
    OCR_HIP(hipSetDevice(lm->device));
    const size_t bytes = (size_t)kLmStride * kLmStride * 4;
    OCR_HIP(hipMalloc(reinterpret_cast<void**>(&lm->dev), bytes));
    OCR_HIP(hipMemcpy(lm->dev, trans, bytes, hipMemcpyHostToDevice));
    *out = lm.release();
  });
}

void ocr_char_lm_destroy(ocr_char_lm_t* lm) { delete lm; }

void ocr_lm_default_params(ocr_lm_params_t* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->top_k = 1;
}

int ocr_lm_decode(ocr_rec_t* rec, const ocr_char_lm_t* lm, const float* costs, int n_glyphs, int mem_kind, const int32_t* word_offsets,
                  int n_words, const ocr_lm_params_t* params, ocr_lm_paths_t** out) {
  return ocr::guard([&] {
    using namespace ocr;
    if (!rec || !lm || !word_offsets || !out) fail(OCR_ERR_INVALID, "lm_decode: null argument");
    *out = nullptr;
    if (mem_kind != OCR_MEM_HOST && mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "lm_decode: mem_kind %d", mem_kind);
    if (lm->device != rec->impl.device()) fail(OCR_ERR_INVALID, "lm_decode: model on device %d, handle on device %d", lm->device, rec->impl.device());
    ocr_lm_params_t p;
    ocr_lm_default_params(&p);
    if (params) p = *params;
    lm_check_params(p);
    LmPlan plan;
    lm_plan(word_offsets, n_words, n_glyphs, p.top_k, plan);
    if (n_glyphs > 0 && !costs) fail(OCR_ERR_INVALID, "lm_decode: null costs");
    std::unique_ptr<PathsOwned> m(new PathsOwned());
    const int k = p.top_k;
    const size_t nw = (size_t)n_words;
    m->word_flags.swap(plan.flags);
    m->labels.assign(plan.label_count, -1);
    m->costs.assign(nw * k, INFINITY);
    m->raw_costs.assign(nw, 0.0);
    if (n_words == 0) {
      m->finish(0, k, n_glyphs);
      *out = &m.release()->view;
      return;
    }
    OCR_HIP(hipSetDevice(rec->impl.device()));
    hipStream_t s = rec->impl.stream();
    const size_t cost_bytes = (size_t)n_glyphs * kLmClasses * 4;
    Carve c;
    const size_t o_bad = c.take(4), o_cost = c.take(mem_kind == OCR_MEM_HOST ? cost_bytes : 0), o_off = c.take((nw + 1) * 4);
    const size_t o_raw = c.take(nw * 8), o_oc = c.take(nw * k * 8), o_lab = c.take(plan.label_count * 4), o_link = c.take(plan.link_bytes);
    char* ws = lex_workspace(rec, c.end);
    int32_t* bad_dev = at<int32_t>(ws, o_bad);
    OCR_HIP(hipMemsetAsync(bad_dev, 0x7F, 4, s));
    if (plan.label_count) OCR_HIP(hipMemsetAsync(ws + o_lab, 0xFF, plan.label_count * 4, s));   // -1: the rows of words that are not decoded
    const float* cost_dev = costs;
    if (mem_kind == OCR_MEM_HOST && n_glyphs > 0) {
      OCR_HIP(hipMemcpyAsync(ws + o_cost, costs, cost_bytes, hipMemcpyHostToDevice, s));
      cost_dev = at<const float>(ws, o_cost);
    }
    OCR_HIP(hipMemcpyAsync(ws + o_off, word_offsets, (nw + 1) * 4, hipMemcpyHostToDevice, s));
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(plan.blocks), dim3(kLmWords * 64), 0, s, cost_dev, at<const int32_t>(ws, o_off), n_words, n_glyphs,
                         lm->dev, k, at<uint16_t>(ws, o_link), at<int32_t>(ws, o_lab), at<double>(ws, o_oc), at<double>(ws, o_raw), bad_dev);
    };
    if (k == 1) launch(lm_decode_kernel<1>);
    else launch(lm_decode_kernel<8>);
    OCR_HIP(hipGetLastError());
    int32_t bad = kNone;
    OCR_HIP(hipMemcpyAsync(&bad, bad_dev, 4, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(m->raw_costs.data(), ws + o_raw, nw * 8, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(m->costs.data(), ws + o_oc, nw * k * 8, hipMemcpyDeviceToHost, s));
    if (plan.label_count) OCR_HIP(hipMemcpyAsync(m->labels.data(), ws + o_lab, plan.label_count * 4, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipStreamSynchronize(s));
    if (bad != kNone) fail(OCR_ERR_INVALID, "lm_decode: word %d has a cost that is NaN, infinite or negative", bad);
    m->finish(n_words, k, n_glyphs);
    *out = &m.release()->view;
  });
}

void ocr_lm_paths_free(ocr_lm_paths_t* p) {
  if (!p) return;
  delete reinterpret_cast<PathsOwned*>(reinterpret_cast<char*>(p) - offsetof(PathsOwned, view));
}

}  // extern "C"
