// Line grouping: the words of every page linked into text lines in reading order (BUILD-DEFINED; rule in include/ocr_amd.h at
// ocr_group_lines, oracle tests/line_oracle.py).  f64, every operation separately rounded: this file is compiled with
// -ffp-contract=off, and f64 sqrt and divide are correctly rounded on gfx950 (as unclip.hip relies on).
//   line_feature_kernel  one thread per word: centre, unit axes, side lengths (8 doubles)
//   line_link_kernel     grid (blocks of 64 words, image, role): a workgroup owns 64 words and scans all words of its image, staged
//                        through LDS in tiles of 256 x 8 doubles (16 KB); each of its four waves takes a quarter of every tile for
//                        all 64 owners.  Role 0 owns i and keeps the best right candidate j, role 1 owns j and keeps the best i that
//                        has j as a right candidate, the test evaluated in i's frame either way.  A scan ascends and replaces on a
//                        strict improvement only, and the four partial winners are merged by (a, index): ties go to the smaller
//                        index without atomics and without depending on the execution order.
//   line_chain_kernel    one workgroup per image: mutual links -> next / prev, pointer jumping for head and rank with a carried
//                        minimum index (a cycle is cut on the link into its smallest word), the heads sorted by (Cy, Cx, index) with a
//                        bitonic network over LDS indices, line lengths scanned, order / gaps / line starts written.
// The chain kernel keeps its index arrays as int16 in LDS (an image has at most 4 096 words): 60 KB in all.
#include "common.hpp"

namespace ocr {
namespace {

constexpr int kTile = 256;
constexpr int kScan = 4;                 // parts of a tile, one per wave of the link kernel
constexpr int kOwners = kTile / kScan;   // words a link workgroup owns
constexpr int kChainThreads = 1024;
constexpr int kItems = kLineMaxWords / kChainThreads;   // words per thread of the chain kernel
constexpr int kNone = 0x7FFF;                           // int16 padding of the sort network: after every word
static_assert(kLineMaxWords % kChainThreads == 0 && kLineMaxWords <= kNone, "chain kernel layout");

struct Feat {
  double cx, cy, ux, uy, vx, vy, lu, lv;
};

__device__ inline bool isolated(const Feat& f) { return f.lu == 0 || f.lv == 0; }

// Is j a right candidate of i?  a is the advance of j along i's reading direction, gap = g / hmax.
__device__ inline bool right_candidate(const Feat& fi, const Feat& fj, const LineParams& p, double& a, double& gap) {
  const double dx = fj.cx - fi.cx, dy = fj.cy - fi.cy;
  a = dx * fi.ux + dy * fi.uy;
  const double b = dx * fi.vx + dy * fi.vy;
  const bool lt = fi.lv < fj.lv;
  const double hmin = lt ? fi.lv : fj.lv, hmax = lt ? fj.lv : fi.lv;
  const double g = a - (fi.lu + fj.lu) * 0.5;
  gap = g / hmax;
  return a > 0 && fabs(b) <= p.line_tol * hmin && hmax <= p.height_ratio * hmin && (fi.ux * fj.ux + fi.uy * fj.uy) >= p.min_cos &&
         g <= p.max_gap * hmax;
}

__global__ __launch_bounds__(256) void line_feature_kernel(const double* __restrict__ quads, int n_words, Feat* __restrict__ feat) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_words) return;
  const double* q = quads + 8 * (size_t)k;
  const double ux = q[2] - q[0], uy = q[3] - q[1], vx = q[6] - q[0], vy = q[7] - q[1];
  Feat f;
  f.lu = sqrt(ux * ux + uy * uy);
  f.lv = sqrt(vx * vx + vy * vy);
  f.cx = (q[0] + q[4]) * 0.5;
  f.cy = (q[1] + q[5]) * 0.5;
  f.ux = ux / f.lu;
  f.uy = uy / f.lu;
  f.vx = vx / f.lv;
  f.vy = vy / f.lv;
  feat[k] = f;
}

// link[role][word]: role 0 right[], role 1 left[], image-local indices, -1 for none.  A workgroup owns kOwners words, one per lane,
// and each of its kScan waves scans its own quarter of every tile for all of them; the quarters' winners meet in LDS.
__global__ __launch_bounds__(kTile) void line_link_kernel(const Feat* __restrict__ feat, const int32_t* __restrict__ img_off, int n_words,
                                                          LineParams p, int32_t* __restrict__ link) {
  __shared__ Feat tile[kTile];
  __shared__ double cand_a[kScan][kOwners];
  __shared__ int32_t cand_k[kScan][kOwners];
  const int w0 = img_off[blockIdx.y], P = img_off[blockIdx.y + 1] - w0;
  if ((int)blockIdx.x * kOwners >= P) return;   // the whole workgroup leaves: no barrier is passed by a part of it
  const int role = blockIdx.z, tid = threadIdx.x, lane = tid % kOwners, part = tid / kOwners, me = blockIdx.x * kOwners + lane;
  const bool live = me < P;
  const Feat mine = feat[w0 + (live ? me : 0)];
  const bool scan = live && !isolated(mine);
  int best = -1;
  double best_a = 0;
  for (int t0 = 0; t0 < P; t0 += kTile) {
    const int cnt = min(kTile, P - t0);
    if (tid < cnt) tile[tid] = feat[w0 + t0 + tid];
    __syncthreads();
    if (scan) {
      const int k1 = min(cnt, (part + 1) * (kTile / kScan));
      for (int k = part * (kTile / kScan); k < k1; ++k) {
        const Feat other = tile[k];
        if (t0 + k == me || isolated(other)) continue;
        double a, gap;
        const bool ok = role == 0 ? right_candidate(mine, other, p, a, gap) : right_candidate(other, mine, p, a, gap);
        if (ok && (best < 0 || a < best_a)) {   // ascending scan, strict improvement: the smaller index keeps a tie
          best = t0 + k;
          best_a = a;
        }
      }
    }
    __syncthreads();
  }
  cand_a[part][lane] = best_a;
  cand_k[part][lane] = best;
  __syncthreads();
  if (part != 0 || !live) return;
  for (int s = 1; s < kScan; ++s) {   // the quarters interleave in index: the tie rule is spelled out
    const int k = cand_k[s][lane];
    const double a = cand_a[s][lane];
    if (k >= 0 && (best < 0 || a < best_a || (a == best_a && k < best))) {
      best = k;
      best_a = a;
    }
  }
  link[(size_t)role * n_words + w0 + me] = best;
}

__global__ __launch_bounds__(kChainThreads) void line_chain_kernel(const Feat* __restrict__ feat, const int32_t* __restrict__ img_off,
                                                                   int n_words, LineParams p, const int32_t* __restrict__ link,
                                                                   int32_t* __restrict__ order, int32_t* __restrict__ flags,
                                                                   double* __restrict__ gaps, int32_t* __restrict__ line_start,
                                                                   int32_t* __restrict__ n_lines) {
  __shared__ int16_t nxt[kLineMaxWords], prv[kLineMaxWords], ptr[kLineMaxWords], dist[kLineMaxWords], mn[kLineMaxWords];
  __shared__ int16_t heads[kLineMaxWords], len[kLineMaxWords];
  __shared__ int32_t part[kChainThreads];
  __shared__ int32_t n_heads;
  const int img = blockIdx.x, tid = threadIdx.x;
  const int w0 = img_off[img], P = img_off[img + 1] - w0;
  if (P == 0) {
    if (tid == 0) n_lines[img] = 0;
    return;
  }
  const int32_t* right = link + w0;
  const int32_t* left = link + n_words + w0;
  const Feat* ft = feat + w0;
  int rounds = 0;
  while ((1 << rounds) < P) ++rounds;

  // the link i -> j exists iff right[i] == j && left[j] == i
  for (int i = tid; i < P; i += kChainThreads) {
    const int r = right[i], l = left[i];
    nxt[i] = (int16_t)(r >= 0 && left[r] == i ? r : -1);
    prv[i] = (int16_t)(l >= 0 && right[l] == i ? l : -1);
    flags[w0 + i] = isolated(ft[i]) ? 1 : 0;
  }
  if (tid == 0) n_heads = 0;
  __syncthreads();

  // Pointer jumping towards the head: after `rounds` doublings ptr is the head and dist the rank of every word of an open chain; a
  // word of a cycle never meets a head, and its mn has been carried once around: the cycle's smallest index.  Pass 0 finds and cuts the
  // cycles, pass 1 ranks the chains that the cuts opened.
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = tid; i < P; i += kChainThreads) {
      const int q = prv[i];
      ptr[i] = (int16_t)(q >= 0 ? q : i);
      dist[i] = (int16_t)(q >= 0 ? 1 : 0);
      mn[i] = (int16_t)i;
    }
    __syncthreads();
    for (int r = 0; r < rounds; ++r) {
      int np[kItems], nd[kItems], nm[kItems];
#pragma unroll
      for (int e = 0; e < kItems; ++e) {
        const int i = tid + e * kChainThreads;
        if (i < P) {
          const int q = ptr[i];
          np[e] = ptr[q];
          nd[e] = dist[i] + dist[q];
          nm[e] = min((int)mn[i], (int)mn[q]);
        }
      }
      __syncthreads();
#pragma unroll
      for (int e = 0; e < kItems; ++e) {
        const int i = tid + e * kChainThreads;
        if (i < P) {
          ptr[i] = (int16_t)np[e];
          dist[i] = (int16_t)min(nd[e], kNone);   // (the rank of an open chain is below P; around a cycle the sum is not used)
          mn[i] = (int16_t)nm[e];
        }
      }
      __syncthreads();
    }
    if (pass == 1) break;
    bool cut[kItems];
#pragma unroll
    for (int e = 0; e < kItems; ++e) {
      const int i = tid + e * kChainThreads;
      cut[e] = i < P && prv[ptr[i]] >= 0 && mn[i] == i;   // on a cycle, and its smallest word
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kItems; ++e) {
      const int i = tid + e * kChainThreads;
      if (cut[e]) {   // one word per cycle: nobody else writes these two entries
        nxt[prv[i]] = -1;
        prv[i] = -1;
        flags[w0 + i] = 2;
      }
    }
    __syncthreads();
  }

  // heads, in any order: the sort below is total
  for (int i = tid; i < P; i += kChainThreads)
    if (prv[i] < 0) heads[atomicAdd(&n_heads, 1)] = (int16_t)i;
  __syncthreads();
  const int L = n_heads;
  int N2 = 1;
  while (N2 < L) N2 <<= 1;
  for (int i = L + tid; i < N2; i += kChainThreads) heads[i] = kNone;
  __syncthreads();
  for (int k = 2; k <= N2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < N2; t += kChainThreads) {
        const int x = t ^ j;
        if (x > t) {
          const int a = heads[t], b = heads[x];
          // before(a, b) by (Cy, Cx, index); the padding is behind every word
          bool a_first;
          if (a == kNone || b == kNone)
            a_first = b == kNone;
          else {
            const double ay = ft[a].cy, by = ft[b].cy, ax = ft[a].cx, bx = ft[b].cx;
            a_first = ay < by || (ay == by && (ax < bx || (ax == bx && a < b)));
          }
          const bool asc = (t & k) == 0;
          if (a != b && a_first != asc) {
            heads[t] = (int16_t)b;
            heads[x] = (int16_t)a;
          }
        }
      }
      __syncthreads();
    }
  }

  // line l starts at the head heads[l]; mn is free now and takes the line of every head, len the word count from the tails
  for (int l = tid; l < L; l += kChainThreads) mn[heads[l]] = (int16_t)l;
  __syncthreads();
  for (int i = tid; i < P; i += kChainThreads)
    if (nxt[i] < 0) len[mn[ptr[i]]] = (int16_t)(dist[i] + 1);
  __syncthreads();
  // exclusive scan of len[0..L): kItems consecutive lines per thread, their sums scanned across the workgroup
  int mine[kItems], sum = 0;
#pragma unroll
  for (int e = 0; e < kItems; ++e) {
    const int l = tid * kItems + e;
    mine[e] = l < L ? len[l] : 0;
    sum += mine[e];
  }
  part[tid] = sum;
  __syncthreads();
  for (int off = 1; off < kChainThreads; off <<= 1) {
    const int v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int start = part[tid] - sum;
  __syncthreads();   // len is rewritten as the line starts (int16: below 4 096)
#pragma unroll
  for (int e = 0; e < kItems; ++e) {
    const int l = tid * kItems + e;
    if (l < L) {
      len[l] = (int16_t)start;
      line_start[w0 + l] = w0 + start;
      start += mine[e];
    }
  }
  if (tid == 0) n_lines[img] = L;
  __syncthreads();
  for (int i = tid; i < P; i += kChainThreads) {
    const int pos = w0 + min(len[mn[ptr[i]]] + dist[i], P - 1);   // (line start + rank is below P; the bound keeps a store in its slice)
    order[pos] = w0 + i;
    double a, gap = 0.0;
    const int q = prv[i];
    if (q >= 0) (void)right_candidate(ft[q], ft[i], p, a, gap);
    gaps[pos] = q >= 0 ? gap : 0.0;
  }
}

}  // namespace

static_assert(sizeof(Feat) == kLineFeatBytes, "feature record");

void launch_group_lines(const double* quads_dev, const int32_t* img_off_dev, int n_images, int n_words, int max_words, const LineParams& p,
                        void* feat_dev, int32_t* link_dev, int32_t* order_dev, int32_t* flags_dev, double* gaps_dev,
                        int32_t* line_start_dev, int32_t* n_lines_dev, hipStream_t s) {
  if (n_images <= 0 || n_words <= 0) return;
  Feat* feat = static_cast<Feat*>(feat_dev);
  hipLaunchKernelGGL(line_feature_kernel, dim3((n_words + 255) / 256), dim3(256), 0, s, quads_dev, n_words, feat);
  OCR_HIP(hipGetLastError());
  hipLaunchKernelGGL(line_link_kernel, dim3((max_words + kOwners - 1) / kOwners, n_images, 2), dim3(kTile), 0, s, feat, img_off_dev, n_words, p,
                     link_dev);
  OCR_HIP(hipGetLastError());
  hipLaunchKernelGGL(line_chain_kernel, dim3(n_images), dim3(kChainThreads), 0, s, feat, img_off_dev, n_words, p, link_dev, order_dev,
                     flags_dev, gaps_dev, line_start_dev, n_lines_dev);
  OCR_HIP(hipGetLastError());
}

}  // namespace ocr
