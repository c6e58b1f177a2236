// Glyph segmentation by connected components (ocr_segment_glyphs_cc): kerned letters, whose column ranges overlap without a touching
// pixel, come out as separate glyphs.  BUILD-DEFINED like glyphs.hip: the rule is written down in include/ocr_amd.h and restated in
// tests/glyph_cc_oracle.py; this kernel meets it array for array (integers throughout; the f32 levels are glyph_levels.hpp's, so the
// file is compiled with -ffp-contract=off like glyphs.hip).
//
// segment_cc_kernel, one 256-thread workgroup per word, everything after the two reads of the box in LDS:
//   1. histogram, Otsu, polarity, levels: glyph_levels.hpp, the code segment_kernel runs;
//   2. runs, kRowChunk rows at a time, a wave per row: a ballot per 64 columns, run starts m & ~prev and ends ~m & prev.  First the
//      count of every row, a prefix sum over the chunk, then the same scan writes every run to its slot: run indices are in raster
//      order, so the smallest run index of a component is its anchor and lies in its first row.  A run is (raster index of its first
//      pixel, end column, parent): 12 bytes.  More than kMaxRuns runs: the word is flagged for the column rule and the kernel stops;
//   3. union: every run looks up the runs of the row above that it touches (a binary search over the raster indices) and unites with
//      them: roots are linked larger -> smaller with 32-bit LDS atomicMin, finds halve their path with atomicMin too (a parent only
//      ever decreases, so the root of a finished tree is its smallest run).  Then every run is pointed at its root;
//   4. roots are numbered in index order (a block scan) into at most kMaxComps slots - more: the column rule again - and every run
//      folds its extent and pixel count into its slot with LDS min / max / add: order-free, so scheduling cannot change a bit;
//   5. components of at least min_glyph_pixels pixels are sorted by x0 * 1024 + slot (= by (x0, anchor)) with a bitonic sort in LDS,
//      and lane 0 walks them: merge into the open group or close it (height filter, max_glyphs, truncation).
//   6. segment_cc_labelled_kernel only (the same body, template flag LABELS): every component carries a label - 0xFFFF until the walk
//      closes a kept group over it, then the glyph's index in the word + 1 - and every run paints it over its pixels in the word's
//      uint16 plane, for ocr_extract_glyph_crops_masked.  The label lives in c_cnt, dead once the sort keys are built: no new LDS.
// LDS: 3 x 32 KB runs, 5 x 4 KB components, 4 KB keys, 4 KB row counts, 4 KB histograms: 128 KB of the CU's 160, so one workgroup per
// CU - the words of a batch are few next to CUs x rounds.  48 VGPRs, no scratch, both forms.
#include <type_traits>

#include "common.hpp"
#include "glyph_levels.hpp"

namespace ocr {
namespace {

using glyph_dev::kThreads;
using glyph_dev::kWaves;
using glyph_dev::quantise;

constexpr int kMaxRuns = 8192;
constexpr int kMaxComps = 1024;
constexpr int kRowChunk = 1024;   // rows whose run counts are held in LDS at a time

// parent table reads that race with other lanes' atomicMin: always from LDS, never a cached register copy
__device__ __forceinline__ int peek(const int* p) { return *(const volatile int*)p; }

// the root of x, halving the path on the way (only ever lowers a parent, and only to a member of the same tree)
__device__ __forceinline__ int find_root(int* parent, int x) {
  for (;;) {
    const int p = peek(&parent[x]);
    if (p == x) return x;
    const int g = peek(&parent[p]);
    if (g == p) return p;
    atomicMin(&parent[x], g);
    x = g;
  }
}

__device__ __forceinline__ void unite(int* parent, int a, int b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    if (a < b) { const int s = a; a = b; b = s; }
    const int old = atomicMin(&parent[a], b);   // a was a root when found: link it under the smaller root
    if (old == a) return;
    a = old;                                    // someone linked a first: whatever it hung under still has to meet b
  }
}

// The body of both kernels.  LABELS = false is segment_cc_kernel as it always was; LABELS = true (segment_cc_labelled_kernel) also
// writes the word's label plane (include/ocr_amd.h, ocr_segment_glyphs_cc_labelled): planes + plane_off[word], bh x bw uint16,
// zeroed by the host in front of the launch, so the flat and the two fallback exits - all taken before any label exists - store nothing.
template <bool LABELS>
__device__ __forceinline__ void segment_cc_body(const float* __restrict__ frames, int H, int W, const WordBox* __restrict__ words,
                                                GlyphSegParams prm, GlyphCcParams cc, int32_t* __restrict__ rec,
                                                uint16_t* __restrict__ planes, const long long* __restrict__ plane_off) {
  __shared__ unsigned hist[kWaves][256];
  __shared__ int r_start[kMaxRuns], r_x1[kMaxRuns], parent[kMaxRuns];
  __shared__ int rowcnt[kRowChunk];
  __shared__ int c_x0[kMaxComps], c_x1[kMaxComps], c_y1[kMaxComps], c_cnt[kMaxComps], c_root[kMaxComps];
  __shared__ unsigned keys[kMaxComps];
  __shared__ int s_t, s_pol, s_nruns, s_ncomp, s_nsort, s_wtot[kWaves];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const WordBox wb = words[blockIdx.x];
  const float* img = frames + (size_t)wb.frame * H * W;
  const int bw = wb.x1 - wb.x0, bh = wb.y1 - wb.y0;
  int32_t* out = rec + (size_t)blockIdx.x * glyph_record_ints(prm.max_glyphs);

  glyph_dev::box_histogram(hist, img, W, wb);
  glyph_dev::otsu_levels(hist, wb, prm.polarity, out, &s_t, &s_pol);
  if (tid == 0) s_nruns = 0;
  __syncthreads();
  const int t = s_t, pol = s_pol;
  if (t < 0) {   // flat box: no glyphs
    if (tid == 0) { out[3] = 0; out[6] = 0; }
    return;
  }
  auto fall_back = [&] {   // uniform: the host runs the column kernel over the flagged words
    if (tid == 0) { out[3] = 2; out[6] = 0; }
  };

  // ---- 2. runs.  scan_row: the runs of box row r; WRITE = false counts them, WRITE = true stores them from slot `base` on
  const unsigned long long lt = (1ull << lane) - 1;
  auto scan_row = [&](int r, auto write, int base) -> int {
    constexpr bool WRITE = decltype(write)::value;
    const float* rowp = img + (size_t)(wb.y0 + r) * W + wb.x0;
    int ns = 0, ne = 0;
    unsigned long long carry = 0;
    for (int b0 = 0; b0 < bw; b0 += 64) {
      const int x = b0 + lane;
      bool inkp = false;
      if (x < bw) {
        const int q = quantise(rowp[x]);
        inkp = pol == 1 ? q <= t : q > t;
      }
      const unsigned long long m = __ballot(inkp);
      const unsigned long long prev = (m << 1) | carry;
      const unsigned long long starts = m & ~prev, ends = ~m & prev;   // a lane past the box is no ink: it ends a run at column bw
      if (WRITE) {
        if ((starts >> lane) & 1) {
          const int k = base + ns + __popcll(starts & lt);
          if (k < kMaxRuns) r_start[k] = r * bw + x;
        }
        if ((ends >> lane) & 1) {
          const int k = base + ne + __popcll(ends & lt);
          if (k < kMaxRuns) r_x1[k] = x;
        }
        ne += __popcll(ends);
      }
      ns += __popcll(starts);
      carry = m >> 63;
    }
    if (WRITE && carry && lane == 0 && base + ne < kMaxRuns) r_x1[base + ne] = bw;   // the row's last run reaches column 64 k = bw
    return ns;
  };

  for (int r0 = 0; r0 < bh; r0 += kRowChunk) {
    const int rc = min(kRowChunk, bh - r0);
    for (int r = wv; r < rc; r += kWaves) {
      const int n = scan_row(r0 + r, std::false_type{}, 0);
      if (lane == 0) rowcnt[r] = n;
    }
    __syncthreads();
    // exclusive prefix over the chunk's rows (4 per thread + a wave scan + the wave totals), offset by the runs so far
    {
      int c[4], sum = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        c[k] = 4 * tid + k < rc ? rowcnt[4 * tid + k] : 0;
        sum += c[k];
      }
      int inc = sum;
      for (int o = 1; o < 64; o <<= 1) {
        const int p = __shfl_up(inc, o);
        if (lane >= o) inc += p;
      }
      if (lane == 63) s_wtot[wv] = inc;
      __syncthreads();
      int off = s_nruns + inc - sum;
      for (int k = 0; k < wv; ++k) off += s_wtot[k];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (4 * tid + k < rc) rowcnt[4 * tid + k] = off;
        off += c[k];
      }
      __syncthreads();
      if (tid == kThreads - 1) s_nruns = off;
      __syncthreads();
    }
    if (s_nruns > kMaxRuns) { fall_back(); return; }
    for (int r = wv; r < rc; r += kWaves) scan_row(r0 + r, std::true_type{}, rowcnt[r]);
    __syncthreads();
  }
  const int nruns = s_nruns;

  // ---- 3. union with the touching runs of the row above: [a0, a1) and [b0, b1) touch when a0 <= b1 && b0 <= a1 (8-connectivity)
  for (int i = tid; i < nruns; i += kThreads) parent[i] = i;
  for (int i = tid; i < kMaxComps; i += kThreads) { c_x0[i] = 0x7fffffff; c_x1[i] = 0; c_y1[i] = 0; c_cnt[i] = 0; }
  __syncthreads();
  for (int i = tid; i < nruns; i += kThreads) {
    const int st = r_start[i], y = st / bw;
    if (y == 0) continue;
    const int a0 = st - y * bw, a1 = r_x1[i];
    const int up = (y - 1) * bw;   // raster index of the row above
    // the first run (of any row) that starts at or after column a0 of the row above; the one before it may still reach a0
    int lo = 0, hi = i;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (r_start[mid] < up + a0) lo = mid + 1; else hi = mid;
    }
    if (lo > 0 && r_start[lo - 1] >= up && r_x1[lo - 1] >= a0) unite(parent, i, lo - 1);
    const int last = up + min(a1, bw - 1);   // b0 <= a1, and still in the row above
    for (int k = lo; k < i && r_start[k] <= last; ++k) unite(parent, i, k);
  }
  __syncthreads();
  for (int i = tid; i < nruns; i += kThreads) parent[i] = find_root(parent, i);   // a lowered parent stays inside its tree
  __syncthreads();

  // ---- 4. number the roots in index order; a root's parent entry becomes ~slot
  {
    const int per = (nruns + kThreads - 1) / kThreads, i0 = min(tid * per, nruns), i1 = min(i0 + per, nruns);
    int n = 0;
    for (int i = i0; i < i1; ++i) n += parent[i] == i;
    int inc = n;
    for (int o = 1; o < 64; o <<= 1) {
      const int p = __shfl_up(inc, o);
      if (lane >= o) inc += p;
    }
    if (lane == 63) s_wtot[wv] = inc;
    __syncthreads();
    int slot = inc - n;
    for (int k = 0; k < wv; ++k) slot += s_wtot[k];
    if (tid == kThreads - 1) s_ncomp = slot + n;
    __syncthreads();
    if (s_ncomp > kMaxComps) { fall_back(); return; }
    for (int i = i0; i < i1; ++i)
      if (parent[i] == i) {
        c_root[slot] = i;
        parent[i] = ~slot;
        ++slot;
      }
  }
  if (tid == 0) s_nsort = 0;
  __syncthreads();
  const int ncomp = s_ncomp;
  for (int i = tid; i < nruns; i += kThreads) {
    const int p = parent[i], slot = p < 0 ? ~p : ~parent[p];
    const int st = r_start[i], y = st / bw, a0 = st - y * bw, a1 = r_x1[i];
    atomicMin(&c_x0[slot], a0);
    atomicMax(&c_x1[slot], a1);
    atomicMax(&c_y1[slot], y + 1);
    atomicAdd(&c_cnt[slot], a1 - a0);
  }
  __syncthreads();

  // ---- 5. sort the components that are large enough by (x0, anchor); x0 < 2^22 and slot < 1024, so the key fits 32 bits.  A dropped
  // component's key is the largest value: it sorts behind (or ties with) every kept one, and only the first s_nsort keys are read
  int npow = 64;
  while (npow < ncomp) npow <<= 1;
  for (int i = tid; i < npow; i += kThreads) {
    unsigned key = 0xffffffffu;
    if (i < ncomp && c_cnt[i] >= prm.min_glyph_pixels) {
      key = (unsigned)c_x0[i] * 1024u + (unsigned)i;
      atomicAdd(&s_nsort, 1);
    }
    keys[i] = key;
    // the count has had its last reader (this thread, this entry): c_cnt becomes the component's label, "ink of no glyph" until the
    // walk says otherwise - dropped here, by the height filter, behind max_glyphs or never reached by the truncated walk
    if (LABELS && i < ncomp) c_cnt[i] = 0xFFFF;
  }
  __syncthreads();
  for (int k = 2; k <= npow; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < npow; i += kThreads) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned a = keys[i], b = keys[l];
          if (((i & k) == 0) == (a > b)) { keys[i] = b; keys[l] = a; }
        }
      }
      __syncthreads();
    }

  if (tid == 0) {
    const int nsort = s_nsort, pct = cc.merge_overlap_pct, min_h = cc.min_height_pct * bh;
    int nkept = 0, trunc = 0;
    int gx0 = 0, gy0 = 0, gx1 = 0, gy1 = 0;
    int gfirst = 0;   // LABELS: the open group is keys[gfirst, gend) - a group is a contiguous range of the sorted order
    bool open = false;
    auto close_group = [&](int gend) {
      if ((gy1 - gy0) * 100 < min_h) return;
      if (nkept < prm.max_glyphs) {
        int32_t* b = out + 8 + 4 * nkept;
        b[0] = wb.x0 + gx0; b[1] = wb.y0 + gy0; b[2] = wb.x0 + gx1; b[3] = wb.y0 + gy1;
        ++nkept;
        if (LABELS)
          for (int k = gfirst; k < gend; ++k) c_cnt[keys[k] & 1023u] = nkept;   // glyph g of the word is label g + 1
      } else {
        trunc = 1;
      }
    };
    for (int n = 0; n < nsort && !trunc; ++n) {
      const int slot = (int)(keys[n] & 1023u);
      const int x0 = c_x0[slot], x1 = c_x1[slot], y0 = r_start[c_root[slot]] / bw, y1 = c_y1[slot];
      if (open) {
        const int ov = min(gx1, x1) - max(gx0, x0), nar = min(gx1 - gx0, x1 - x0);
        if (pct > 0 && ov > 0 && ov * 100 >= nar * pct) {
          gx0 = min(gx0, x0); gy0 = min(gy0, y0); gx1 = max(gx1, x1); gy1 = max(gy1, y1);
          continue;
        }
        close_group(n);
      }
      gx0 = x0; gy0 = y0; gx1 = x1; gy1 = y1;
      gfirst = n;
      open = true;
    }
    if (open && !trunc) close_group(nsort);
    out[3] = trunc;
    out[6] = nkept;
  }

  // ---- 6. (LABELS) every run paints its component's label over its pixels: a wave per run, lanes over columns, so the 2-byte stores
  // of one instruction are contiguous.  Runs partition the ink, so every ink pixel is written once and no other pixel at all
  if constexpr (LABELS) {
    __syncthreads();
    uint16_t* plane = planes + plane_off[blockIdx.x];
    for (int i = wv; i < nruns; i += kWaves) {
      const int p = parent[i], slot = p < 0 ? ~p : ~parent[p];
      const int st = r_start[i], a1 = r_x1[i], y = st / bw;
      const uint16_t lab = (uint16_t)c_cnt[slot];
      for (int k = st + lane, e = y * bw + a1; k < e; k += 64) plane[k] = lab;
    }
  }
}

__global__ __launch_bounds__(kThreads) void segment_cc_kernel(const float* __restrict__ frames, int H, int W, const WordBox* __restrict__ words,
                                                              GlyphSegParams prm, GlyphCcParams cc, int32_t* __restrict__ rec) {
  segment_cc_body<false>(frames, H, W, words, prm, cc, rec, nullptr, nullptr);
}

__global__ __launch_bounds__(kThreads) void segment_cc_labelled_kernel(const float* __restrict__ frames, int H, int W,
                                                                       const WordBox* __restrict__ words, GlyphSegParams prm, GlyphCcParams cc,
                                                                       int32_t* __restrict__ rec, uint16_t* __restrict__ planes,
                                                                       const long long* __restrict__ plane_off) {
  segment_cc_body<true>(frames, H, W, words, prm, cc, rec, planes, plane_off);
}

}  // namespace

void launch_segment_cc(const float* frames_dev, int H, int W, const WordBox* words_dev, int n_words, const GlyphSegParams& p,
                       const GlyphCcParams& cc, int32_t* records_dev, hipStream_t s) {
  if (n_words <= 0) return;
  hipLaunchKernelGGL(segment_cc_kernel, dim3(n_words), dim3(kThreads), 0, s, frames_dev, H, W, words_dev, p, cc, records_dev);
  OCR_HIP(hipGetLastError());
}

void launch_segment_cc_labelled(const float* frames_dev, int H, int W, const WordBox* words_dev, int n_words, const GlyphSegParams& p,
                                const GlyphCcParams& cc, int32_t* records_dev, uint16_t* planes_dev, const long long* plane_off_dev,
                                hipStream_t s) {
  if (n_words <= 0) return;
  hipLaunchKernelGGL(segment_cc_labelled_kernel, dim3(n_words), dim3(kThreads), 0, s, frames_dev, H, W, words_dev, p, cc, records_dev, planes_dev,
                     plane_off_dev);
  OCR_HIP(hipGetLastError());
}

}  // namespace ocr
