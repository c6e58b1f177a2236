// CTC prefix beam search with the top-k hypotheses per crop - an EXTENSION like ctc.hip (the reference has no sequence recogniser).
// The rule is the one include/ocr_amd.h states at ocr_ctc_beam_decode; tests/ctc_beam_oracle.py restates it in f64 numpy.
//   logits [N][T][C] f32 -> labels [N][B][T] int32 (-1 padded), lengths [N][B] (-1: no such hypothesis), scores [N][B] f64 (log P, -inf)
// One 256-thread workgroup per crop; all arithmetic after the f32 load is f64.  Per column t:
//   P1  log-softmax of the column into LDS (block max / sum reductions); the column t + 1 is already loading.  A non-finite logit
//       ends the crop (block-uniform vote) and records the lowest such crop in *bad_crop for the host.
//   P2  rank sort of the column (lp descending, class ascending; one thread per class), and per beam j its parent r (the beam whose
//       prefix is ℓ_j minus its last label: equal length - 1, equal 64-bit hash, then a byte compare): ℓ_r + last_j is merged into the
//       stay of j, so the class last_j is marked in r's 256-bit mask and not offered as an extension of r.  Identity comes from the
//       prefix bytes only, never from slot numbers (a parent may have been pruned and re-created in another slot).
//   P3  one thread per beam r writes its candidates: the stay S(r) (with the merged extension folded in), the extension by its own last
//       label (scored from lb), and the first B unmerged extensions in the sorted column order.  tot_r + lp[c] is non-increasing along
//       that order, so those B are the best of r's extensions, except where rounding makes the B-th score tie later ones: then the
//       tie group is re-taken in class order (the key decides ties).  No extension past these can be among the B survivors.
//   P4  bitonic sort of the <= B (B + 2) candidates (padded to a power of two) on (score desc, key (r, c) asc) in LDS.
//   P5  the first min(B, #candidates) become the beams of the next column; prefixes are double-buffered u8 rows [2][B][T].
// LDS: 7.2 KB fixed (+ 256 B static: __syncthreads_or) + 12 B per candidate slot (pow2 >= B (B + 2): 24 KB at B = 32) + 2 B roundup16(T) prefix bytes
// (64 KB at B = 32, T = 1024) -> 97 KB at the limits (<= 160 KB), 10 KB at B = 8, T = 32.  112 VGPRs, no scratch (4 waves / SIMD
// by registers; one workgroup per CU at the limits by LDS).  The per-step cost is latency-bound (about 15 + 2 log2(B (B + 2)) barriers per column); the kernel is a tail stage.
#include <cstdint>

#include "api_internal.hpp"
#include "common.hpp"

namespace ocr {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxB = 32, kMaxT = 1024, kMaxC = 256;
constexpr unsigned kPadKey = 0xFFFFFFFFu;
constexpr unsigned long long kHashSeed = 0x6a09e667f3bcc909ull;

struct Fixed {
  double lp[kMaxC];                     // the column's log-softmax
  double red[8];                        // reduction scratch: [0, 4) max, [4, 8) sum
  double st_lb[kMaxB], st_lnb[kMaxB];   // stay candidates of this column
  double lb[2][kMaxB], lnb[2][kMaxB];   // beam state, double-buffered
  unsigned long long hash[2][kMaxB], phash[2][kMaxB];   // hash of the prefix and of the prefix minus its last label
  unsigned long long mask[kMaxB][4];    // classes whose extension of beam r is merged into a stay
  int sorted[kMaxC];
  int len[2][kMaxB], last[2][kMaxB];
  int parent[kMaxB];
};
constexpr size_t kFixedBytes = (sizeof(Fixed) + 15) / 16 * 16;

__host__ __device__ inline int pow2_at_least(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}
__host__ __device__ inline int prefix_stride(int t) { return (t + 15) / 16 * 16; }
inline size_t lds_bytes(int t, int b) {
  const int ncap = pow2_at_least(b * (b + 2));
  return kFixedBytes + ((size_t)ncap * 12 + 15) / 16 * 16 + 2ull * b * prefix_stride(t);
}

// a (+) b = M + log1p(exp(m - M)); exactly commutative; -inf (+) x = x
__device__ inline double lse2(double a, double b) {
  const double M = a > b ? a : b, m = a > b ? b : a;
  if (m == -INFINITY) return M;
  return M + log1p(exp(m - M));
}

__device__ inline unsigned long long hash_push(unsigned long long h, int k) { return (h ^ (unsigned long long)(k + 1)) * 0x100000001b3ull + 0x9e3779b97f4a7c15ull; }

__device__ inline bool same_prefix(const unsigned char* a, const unsigned char* b, int n) {   // rows are 16-byte aligned
  const uint32_t* wa = reinterpret_cast<const uint32_t*>(a);
  const uint32_t* wb = reinterpret_cast<const uint32_t*>(b);
  const int nw = n >> 2;
  for (int i = 0; i < nw; ++i)
    if (wa[i] != wb[i]) return false;
  for (int i = nw * 4; i < n; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

__device__ inline double wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ inline double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(kThreads) void ctc_beam_kernel(const float* __restrict__ logits, int t_len, int c, int blank, int B, int stride,
                                                            int32_t* __restrict__ labels, int32_t* __restrict__ lengths, double* __restrict__ scores,
                                                            int* __restrict__ bad_crop) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Fixed& F = *reinterpret_cast<Fixed*>(smem);
  const int ncap_max = pow2_at_least(B * (B + 2));
  double* cs = reinterpret_cast<double*>(smem + kFixedBytes);
  unsigned* ck = reinterpret_cast<unsigned*>(smem + kFixedBytes + (size_t)ncap_max * 8);
  unsigned char* pre = smem + kFixedBytes + ((size_t)ncap_max * 12 + 15) / 16 * 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int crop = blockIdx.x;
  const float* x = logits + (size_t)crop * t_len * c;

  if (tid == 0) {
    F.lb[0][0] = 0.0;
    F.lnb[0][0] = -INFINITY;
    F.hash[0][0] = kHashSeed;
    F.phash[0][0] = 0;
    F.len[0][0] = 0;
    F.last[0][0] = -1;
  }
  int cur = 0, nb = 1;
  float xn = tid < c ? x[tid] : 0.0f;
  for (int t = 0; t < t_len; ++t) {
    // ---- P1: log-softmax of column t (column t + 1 starts loading)
    const float xf = xn;
    if (t + 1 < t_len && tid < c) xn = x[(size_t)(t + 1) * c + tid];
    const int n_cand = pow2_at_least(nb * (B + 2));
    for (int i = tid; i < B * 4; i += kThreads) F.mask[i >> 2][i & 3] = 0;
    for (int i = tid; i < n_cand; i += kThreads) {
      cs[i] = -INFINITY;
      ck[i] = kPadKey;
    }
    if (__syncthreads_or(tid < c && !isfinite(xf))) {
      if (tid == 0) atomicMin(bad_crop, crop);
      return;   // block-uniform
    }
    const double v = tid < c ? (double)xf : -INFINITY;
    double m = wave_max(v);
    if (lane == 0) F.red[wave] = m;
    __syncthreads();
    const double mx = fmax(fmax(F.red[0], F.red[1]), fmax(F.red[2], F.red[3]));
    double e = wave_sum(tid < c ? exp(v - mx) : 0.0);
    if (lane == 0) F.red[4 + wave] = e;
    __syncthreads();
    const double L = log((F.red[4] + F.red[5]) + (F.red[6] + F.red[7]));
    if (tid < c) F.lp[tid] = (v - mx) - L;
    __syncthreads();

    // ---- P2: sort the column; parents and merge masks
    if (tid < c) {
      const double a = F.lp[tid];
      int rank = 0;
      for (int k = 0; k < c; ++k) {
        const double b = F.lp[k];
        rank += (b > a) || (b == a && k < tid);
      }
      F.sorted[rank] = tid;
    }
    const unsigned char* pc = pre + (size_t)cur * B * stride;
    if (tid < nb) {
      int p = -1;
      const int lj = F.len[cur][tid];
      if (lj > 0) {
        const unsigned long long ph = F.phash[cur][tid];
        for (int r = 0; r < nb; ++r)
          if (F.len[cur][r] == lj - 1 && F.hash[cur][r] == ph && same_prefix(pc + (size_t)r * stride, pc + (size_t)tid * stride, lj - 1)) {
            p = r;
            break;
          }
      }
      F.parent[tid] = p;
      if (p >= 0) {
        const int k = F.last[cur][tid];
        atomicOr(&F.mask[p][k >> 6], 1ull << (k & 63));
      }
    }
    __syncthreads();

    // ---- P3: candidates of beam r
    if (tid < nb) {
      const int r = tid;
      const double lb = F.lb[cur][r], lnb = F.lnb[cur][r], tot = lse2(lb, lnb);
      const int er = F.last[cur][r];
      const double slb = tot + F.lp[blank];
      double slnb = er >= 0 ? lnb + F.lp[er] : -INFINITY;
      const int p = F.parent[r];
      if (p >= 0) {
        const double plb = F.lb[cur][p], ptot = lse2(plb, F.lnb[cur][p]);
        slnb = lse2(slnb, (er == F.last[cur][p] ? plb : ptot) + F.lp[er]);
      }
      F.st_lb[r] = slb;
      F.st_lnb[r] = slnb;
      const unsigned kb = (unsigned)r << 9;   // key (r, c) = r * 512 + c + 1; a stay has c = -1
      int w = r * (B + 2);
      cs[w] = lse2(slb, slnb);
      ck[w] = kb;
      ++w;
      const unsigned long long* mr = F.mask[r];
      auto merged = [&](int k) { return (mr[k >> 6] >> (k & 63)) & 1ull; };
      auto excluded = [&](int k) { return k == blank || k == er || merged(k); };
      if (er >= 0 && !merged(er)) {   // ext(r, e_r) = lb_r + lp[e_r]
        cs[w] = lb + F.lp[er];
        ck[w] = kb + (unsigned)er + 1u;
        ++w;
      }
      const int w0 = w;
      int got = 0;
      double cut = 0.0;
      bool overflow = false;
      for (int i = 0; i < c; ++i) {
        const int k = F.sorted[i];
        if (excluded(k)) continue;
        const double s = tot + F.lp[k];
        if (got == B) {
          overflow = s == cut;
          break;
        }
        cs[w] = s;
        ck[w] = kb + (unsigned)k + 1u;
        ++w;
        if (++got == B) cut = s;
      }
      if (overflow) {   // the tie group at the cut runs past the B-th extension: keep what is above it, then the group in class order
        int g = 0;
        while (g < got && cs[w0 + g] > cut) ++g;
        w = w0 + g;
        got = g;
        for (int k = 0; k < c && got < B; ++k) {
          if (excluded(k) || tot + F.lp[k] != cut) continue;
          cs[w] = cut;
          ck[w] = kb + (unsigned)k + 1u;
          ++w;
          ++got;
        }
      }
    }
    __syncthreads();

    // ---- P4: bitonic sort, best first
    for (int k = 2; k <= n_cand; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < (n_cand >> 1); i += kThreads) {
          const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo + j;
          const double s0 = cs[lo], s1 = cs[hi];
          const unsigned k0 = ck[lo], k1 = ck[hi];
          const bool hi_better = s1 > s0 || (s1 == s0 && k1 < k0);
          if (hi_better == ((lo & k) == 0)) {
            cs[lo] = s1;
            cs[hi] = s0;
            ck[lo] = k1;
            ck[hi] = k0;
          }
        }
        __syncthreads();
      }

    // ---- P5: the survivors become the next column's beams
    int kept = 0;
    while (kept < B && kept < n_cand && ck[kept] != kPadKey) ++kept;
    const int nxt = cur ^ 1;
    if (tid < kept) {
      const unsigned key = ck[tid];
      const int r = (int)(key >> 9), k = (int)(key & 511u) - 1;
      if (k < 0) {
        F.lb[nxt][tid] = F.st_lb[r];
        F.lnb[nxt][tid] = F.st_lnb[r];
        F.hash[nxt][tid] = F.hash[cur][r];
        F.phash[nxt][tid] = F.phash[cur][r];
        F.len[nxt][tid] = F.len[cur][r];
        F.last[nxt][tid] = F.last[cur][r];
      } else {
        F.lb[nxt][tid] = -INFINITY;
        F.lnb[nxt][tid] = cs[tid];
        F.hash[nxt][tid] = hash_push(F.hash[cur][r], k);
        F.phash[nxt][tid] = F.hash[cur][r];
        F.len[nxt][tid] = F.len[cur][r] + 1;
        F.last[nxt][tid] = k;
      }
    }
    unsigned char* pn = pre + (size_t)nxt * B * stride;
    for (int q = 0; q < kept; ++q) {
      const unsigned key = ck[q];
      const int r = (int)(key >> 9), k = (int)(key & 511u) - 1;
      const int ls = F.len[cur][r];
      const int nw = (ls + (k >= 0) + 3) >> 2;   // <= roundup4(T) / 4 <= stride / 4
      const uint32_t* src = reinterpret_cast<const uint32_t*>(pc + (size_t)r * stride);
      uint32_t* dst = reinterpret_cast<uint32_t*>(pn + (size_t)q * stride);
      for (int wi = tid; wi < nw; wi += kThreads) {
        uint32_t val = src[wi];
        if (k >= 0 && wi == (ls >> 2)) {
          const int sh = (ls & 3) * 8;
          val = (val & ~(0xFFu << sh)) | ((uint32_t)k << sh);
        }
        dst[wi] = val;
      }
    }
    __syncthreads();
    cur = nxt;
    nb = kept;
  }

  // ---- output: beams in rank order, unused slots -1 / -inf
  if (tid < B) {
    const size_t o = (size_t)crop * B + tid;
    lengths[o] = tid < nb ? F.len[cur][tid] : -1;
    scores[o] = tid < nb ? lse2(F.lb[cur][tid], F.lnb[cur][tid]) : -INFINITY;
  }
  const unsigned char* pf = pre + (size_t)cur * B * stride;
  int32_t* out = labels + (size_t)crop * B * t_len;
  for (int i = tid; i < B * t_len; i += kThreads) {
    const int q = i / t_len, p = i - q * t_len;
    out[i] = (q < nb && p < F.len[cur][q]) ? (int)pf[(size_t)q * stride + p] : -1;
  }
}

}  // namespace

void launch_ctc_beam(const float* logits_dev, int n, int t, int c, int blank, int beam_width, int32_t* labels_dev, int32_t* lengths_dev,
                     double* scores_dev, int32_t* bad_crop_dev, hipStream_t s) {
  if (n <= 0) return;
  if (t < 1 || t > kMaxT || c < 1 || c > kMaxC || blank < 0 || blank >= c || beam_width < 1 || beam_width > kMaxB)
    fail(OCR_ERR_INVALID, "ctc_beam_decode: T=%d C=%d blank=%d B=%d", t, c, blank, beam_width);
  const size_t lds = lds_bytes(t, beam_width);
  // (per launch: the attribute belongs to the device the calling thread has current.  It belongs to the function, not to a handle,
  // so its value is the need of the limits (97 472 B; with the 256 B of static LDS that __syncthreads_or holds, well under 160 KB)
  // whatever this launch's shape: handles that launch side by side then only ever write the same value, and none can lower it
  // between another's set and launch.  The launch itself still requests exactly what its shape needs.)
  static_assert(sizeof(Fixed) == 7360, "tests/test_ctc_beam.py restates lds_bytes() with this size");
  const size_t lds_limit = lds_bytes(kMaxT, kMaxB);
  OCR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_beam_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit));
  hipLaunchKernelGGL(ctc_beam_kernel, dim3((unsigned)n), dim3(kThreads), lds, s, logits_dev, t, c, blank, beam_width, prefix_stride(t), labels_dev,
                     lengths_dev, scores_dev, bad_crop_dev);
  OCR_HIP(hipGetLastError());
}

}  // namespace ocr
