// Column-aware reading order: the words of every page as blocks (columns, paragraphs) in reading order, every block its lines top to
// bottom, every line its words left to right (BUILD-DEFINED; rule in include/ocr_amd.h at ocr_group_columns, oracle
// tests/column_oracle.py).  f64, every operation separately rounded: this file is compiled with -ffp-contract=off; min and max are
// selects in the oracle's operand order.
//   stage A              launch_group_lines (lines.hip, unchanged) with row_gap as max_gap: rows with their cycle cut, in position order
//   column_gap_kernel    one workgroup per image: every word's left neighbour in its row and the gap element of that link
//   pair_link_kernel<R>  grid (blocks of 64 records, image, role), the shape of line_link_kernel: a workgroup owns 64 records and scans
//                        all records of its image, staged through LDS in tiles of 256; role 0 owns p and keeps its nearest below
//                        candidate q, role 1 owns q and keeps the nearest p that has q as a candidate, the test in p's frame either
//                        way.  Ascending scans, strict improvement, partial winners merged by (a, index): no atomics.  R = Gap for
//                        the stacked gaps of stage B, R = Line for the stacked lines of stage D.
//   column_line_kernel   one workgroup per image: gap chains ranked by pointer jumping (a cycle is opened to count it), the cuts, and
//                        the lines that remain: a row is contiguous in stage A's order, so a line is a run of positions between two
//                        starts and its first thread walks it (tail, largest lv)
//   column_block_kernel  one workgroup per image: line chains with their cycle cut -> blocks, one thread per block walks its lines for
//                        the box, the "precedes" relation of all pairs once into a bit matrix (the X side tiled through LDS), the level
//                        rounds over its bits (to a fixed point or max_levels - 1 rounds), blocks sorted by
//                        (level, TLy, TLx, index) with a bitonic network, two scans (lines of blocks, words of lines), the output
// Records live at the index of the word that names them (a gap by its right word, a line by its head word, a block by the head
// word of its head line); the other slots are dead and skipped.  Index arrays are int16 in LDS (at most 4 096 words an image).
#include "common.hpp"

namespace ocr {
namespace {

constexpr int kTile = 256;
constexpr int kScan = 4;
constexpr int kOwners = kTile / kScan;
constexpr int kThreads = 1024;
constexpr int kItems = kLineMaxWords / kThreads;
constexpr int kNone = 0x7FFF;
constexpr int kPredBatch = 8;   // words of a block's "precedes" row loaded together in a level round
static_assert(kLineMaxWords % kThreads == 0 && kLineMaxWords <= kNone, "per-image kernels' layout");

struct Feat {   // the record of line_feature_kernel (lines.hip)
  double cx, cy, ux, uy, vx, vy, lu, lv;
};
__device__ inline bool isolated(const Feat& f) { return f.lu == 0 || f.lv == 0; }

struct Gap {
  double gx, gy, ux, uy, vx, vy, w, h;
  int32_t live, pad;   // live: eligible
  // is q a below candidate of p?  a is the advance of q down p's column direction
  __device__ static bool cand(const Gap& p, const Gap& q, const ColumnParams& c, double& a) {
    const double dx = q.gx - p.gx, dy = q.gy - p.gy;
    a = dx * p.vx + dy * p.vy;
    const double b = dx * p.ux + dy * p.uy;
    const double hm = q.h > p.h ? q.h : p.h;
    return a > 0 && fabs(b) < p.w + q.w && a <= c.gutter_reach * hm && (p.ux * q.ux + p.uy * q.uy) >= c.min_cos;
  }
};

struct Line {
  double sx, sy, ex, ey, mx, my, ux, uy, vx, vy, len, h;
  int32_t live, pad;   // live: the line of a word that is not isolated
  __device__ static bool cand(const Line& s, const Line& t, const ColumnParams& c, double& a) {
    const double x0 = (t.sx - s.sx) * s.ux + (t.sy - s.sy) * s.uy, x1 = (t.ex - s.sx) * s.ux + (t.ey - s.sy) * s.uy;
    const double lo = x1 < x0 ? x1 : x0, hi = x1 > x0 ? x1 : x0;
    const double ov = (s.len < hi ? s.len : hi) - (0.0 > lo ? 0.0 : lo);
    a = (t.mx - s.mx) * s.vx + (t.my - s.my) * s.vy;
    const double hmax = t.h > s.h ? t.h : s.h, hmin = t.h < s.h ? t.h : s.h;
    const double span = hi - lo, m = span < s.len ? span : s.len;
    return a > 0 && ov > 0 && ov >= c.min_overlap * m && a <= c.block_reach * hmax && hmax <= c.height_ratio * hmin &&
           (s.ux * t.ux + s.uy * t.uy) >= c.min_cos;
  }
};

struct Block {   // frame of a block's box from its TL corner
  double tx, ty, ux, uy, vx, vy, w, h;
};

// does the block X precede the block whose quad is y?
__device__ inline bool precedes(const Block& X, const double* y) {
  double ax0 = 0, ax1 = 0, ay0 = 0, ay1 = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double dx = y[2 * c] - X.tx, dy = y[2 * c + 1] - X.ty;
    const double px = dx * X.ux + dy * X.uy, py = dx * X.vx + dy * X.vy;
    if (c == 0) {
      ax0 = ax1 = px;
      ay0 = ay1 = py;
    } else {
      ax0 = px < ax0 ? px : ax0;
      ax1 = px > ax1 ? px : ax1;
      ay0 = py < ay0 ? py : ay0;
      ay1 = py > ay1 ? py : ay1;
    }
  }
  const bool left = ax0 >= X.w && ((X.h < ay1 ? X.h : ay1) - (0.0 > ay0 ? 0.0 : ay0)) > 0;
  const bool above = ay0 >= X.h && ((X.w < ax1 ? X.w : ax1) - (0.0 > ax0 ? 0.0 : ax0)) > 0;
  return left || above;
}

__device__ inline int clampi(int v, int hi) { return min(max(v, 0), hi); }

__global__ __launch_bounds__(kThreads) void column_gap_kernel(const Feat* __restrict__ feat, const int32_t* __restrict__ img_off,
                                                              ColumnParams p, const int32_t* __restrict__ row_order,
                                                              const int32_t* __restrict__ row_start, const int32_t* __restrict__ n_rows,
                                                              int32_t* __restrict__ row_prev, int32_t* __restrict__ row_pos,
                                                              Gap* __restrict__ gap_rec, int32_t* __restrict__ gap_state,
                                                              double* __restrict__ gap_by_word) {
  __shared__ uint8_t head[kLineMaxWords];
  const int img = blockIdx.x, tid = threadIdx.x;
  const int w0 = img_off[img], P = img_off[img + 1] - w0;
  if (P == 0) return;
  for (int i = tid; i < P; i += kThreads) head[i] = 0;
  __syncthreads();
  const int R = min(n_rows[img], P);
  for (int l = tid; l < R; l += kThreads) head[clampi(row_start[w0 + l] - w0, P - 1)] = 1;
  __syncthreads();
  for (int pos = tid; pos < P; pos += kThreads) {
    const int j = clampi(row_order[w0 + pos] - w0, P - 1);
    const int i = head[pos] ? -1 : clampi(row_order[w0 + pos - 1] - w0, P - 1);   // (position 0 is a head)
    Gap e = {};
    int state = 0;
    double gap = 0.0;
    if (i >= 0) {
      const Feat fi = feat[w0 + i], fj = feat[w0 + j];
      const double dx = fj.cx - fi.cx, dy = fj.cy - fi.cy;
      const double a = dx * fi.ux + dy * fi.uy;
      const double g = a - (fi.lu + fj.lu) * 0.5;
      const double hmax = fi.lv < fj.lv ? fj.lv : fi.lv;
      const double hi = fi.lu * 0.5, hj = fj.lu * 0.5;
      const double rx = fi.cx + fi.ux * hi, ry = fi.cy + fi.uy * hi, lx = fj.cx - fj.ux * hj, ly = fj.cy - fj.uy * hj;
      e.gx = (rx + lx) * 0.5;
      e.gy = (ry + ly) * 0.5;
      e.ux = fi.ux;
      e.uy = fi.uy;
      e.vx = fi.vx;
      e.vy = fi.vy;
      e.w = g * 0.5;
      e.h = hmax;
      gap = g / hmax;
      state = 1 | (g >= p.min_gutter * hmax ? 2 : 0) | (g > p.max_gap * hmax ? 4 : 0);
      e.live = (state & 2) != 0;
    }
    row_prev[w0 + j] = i;
    row_pos[w0 + j] = pos;
    gap_rec[w0 + j] = e;
    gap_state[w0 + j] = state;
    gap_by_word[w0 + j] = gap;
  }
}

// link[role][record]: role 0 the nearest below candidate, role 1 the nearest record that has this one as a candidate; image-local
// indices, -1 for none.  A workgroup owns kOwners records, one per lane; each of its kScan waves scans a quarter of every tile.
template <class R>
__global__ __launch_bounds__(kTile) void pair_link_kernel(const R* __restrict__ rec, const int32_t* __restrict__ img_off, int n_words,
                                                          ColumnParams p, int32_t* __restrict__ link) {
  __shared__ R tile[kTile];
  __shared__ double cand_a[kScan][kOwners];
  __shared__ int32_t cand_k[kScan][kOwners];
  const int w0 = img_off[blockIdx.y], P = img_off[blockIdx.y + 1] - w0;
  if ((int)blockIdx.x * kOwners >= P) return;   // the whole workgroup leaves
  const int role = blockIdx.z, tid = threadIdx.x, lane = tid % kOwners, part = tid / kOwners, me = blockIdx.x * kOwners + lane;
  const bool live = me < P;
  const R mine = rec[w0 + (live ? me : 0)];
  const bool scan = live && mine.live;
  int best = -1;
  double best_a = 0;
  for (int t0 = 0; t0 < P; t0 += kTile) {
    const int cnt = min(kTile, P - t0);
    if (tid < cnt) tile[tid] = rec[w0 + t0 + tid];
    __syncthreads();
    if (scan) {
      const int k1 = min(cnt, (part + 1) * (kTile / kScan));
      for (int k = part * (kTile / kScan); k < k1; ++k) {
        const R other = tile[k];
        if (t0 + k == me || !other.live) continue;
        double a;
        const bool ok = role == 0 ? R::cand(mine, other, p, a) : R::cand(other, mine, p, a);
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

// Mutual links of an image into nxt / prv, then pointer jumping towards the head as in line_chain_kernel: after the doublings ptr is
// the head and dist the rank of every record of an open chain; a record of a cycle never meets a head, and its mn has been carried
// around: the cycle's smallest index.  Pass 0 finds the cycles and cuts each on the link into that record (cut_flag[record] = 1 when
// given), pass 1 ranks the chains that the cuts opened.  All arrays are LDS; ends with a barrier.
__device__ void chain_rank(const int32_t* __restrict__ down, const int32_t* __restrict__ up, int P, int16_t* nxt, int16_t* prv,
                           int16_t* ptr, int16_t* dist, int16_t* mn, int32_t* cut_flag) {
  const int tid = threadIdx.x;
  int rounds = 0;
  while ((1 << rounds) < P) ++rounds;
  for (int i = tid; i < P; i += kThreads) {
    const int d = down[i], u = up[i];
    nxt[i] = (int16_t)(d >= 0 && d < P && up[d] == i ? d : -1);
    prv[i] = (int16_t)(u >= 0 && u < P && down[u] == i ? u : -1);
  }
  __syncthreads();
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = tid; i < P; i += kThreads) {
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
        const int i = tid + e * kThreads;
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
        const int i = tid + e * kThreads;
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
      const int i = tid + e * kThreads;
      cut[e] = i < P && prv[ptr[i]] >= 0 && mn[i] == i;   // on a cycle, and its smallest record
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kItems; ++e) {
      const int i = tid + e * kThreads;
      if (cut[e]) {   // one record per cycle: nobody else writes these two entries
        nxt[prv[i]] = -1;
        prv[i] = -1;
        if (cut_flag) cut_flag[i] = 1;
      }
    }
    __syncthreads();
  }
}

// Exclusive scan of v[0..n) in place (n <= kLineMaxWords, sums below 32 768): kItems consecutive entries per thread, their sums
// scanned across the workgroup.  Ends with a barrier; returns the total.
__device__ int scan_exclusive(int16_t* v, int n, int32_t* part) {
  const int tid = threadIdx.x;
  int mine[kItems], sum = 0;
#pragma unroll
  for (int e = 0; e < kItems; ++e) {
    const int l = tid * kItems + e;
    mine[e] = l < n ? v[l] : 0;
    sum += mine[e];
  }
  part[tid] = sum;
  __syncthreads();
  for (int off = 1; off < kThreads; off <<= 1) {
    const int t = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += t;
    __syncthreads();
  }
  int start = part[tid] - sum;
  const int total = part[kThreads - 1];
#pragma unroll
  for (int e = 0; e < kItems; ++e) {
    const int l = tid * kItems + e;
    if (l < n) {
      v[l] = (int16_t)min(start, kNone);
      start += mine[e];
    }
  }
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(kThreads) void column_line_kernel(const Feat* __restrict__ feat, const int32_t* __restrict__ img_off,
                                                               int n_words, ColumnParams p, const int32_t* __restrict__ link,
                                                               const int32_t* __restrict__ row_order, const int32_t* __restrict__ row_prev,
                                                               const int32_t* __restrict__ row_pos, const int32_t* __restrict__ gap_state,
                                                               int32_t* __restrict__ flags, Line* __restrict__ line_rec,
                                                               int32_t* __restrict__ line_state, int32_t* __restrict__ line_head,
                                                               int32_t* __restrict__ line_len, int32_t* __restrict__ line_cut) {
  __shared__ int16_t nxt[kLineMaxWords], prv[kLineMaxWords], ptr[kLineMaxWords], dist[kLineMaxWords], mn[kLineMaxWords];
  __shared__ uint8_t start[kLineMaxWords];
  const int img = blockIdx.x, tid = threadIdx.x;
  const int w0 = img_off[img], P = img_off[img + 1] - w0;
  if (P == 0) return;
  const Feat* ft = feat + w0;
  chain_rank(link + w0, link + n_words + w0, P, nxt, prv, ptr, dist, mn, nullptr);
  // the size of a chain, left at its head by its tail (mn is free now)
  for (int i = tid; i < P; i += kThreads)
    if (nxt[i] < 0) mn[ptr[i]] = (int16_t)(dist[i] + 1);
  __syncthreads();
  for (int j = tid; j < P; j += kThreads) {
    const int st = gap_state[w0 + j];
    const bool gutter = (st & 2) && mn[ptr[j]] >= p.min_rows;
    if (gutter) flags[w0 + j] |= 4;
    const bool first = row_prev[w0 + j] < 0 || (st & 4) || gutter;
    start[clampi(row_pos[w0 + j], P - 1)] = first;
    line_cut[w0 + j] = 0;
    if (!first) {
      line_rec[w0 + j].live = 0;
      line_state[w0 + j] = 0;
      line_len[w0 + j] = 0;
    }
  }
  __syncthreads();
  for (int pos = tid; pos < P; pos += kThreads) {
    if (!start[pos]) continue;
    const int h = clampi(row_order[w0 + pos] - w0, P - 1);
    const Feat fh = ft[h];
    int tail = h, k = pos + 1;
    double hmax = fh.lv;
    line_head[w0 + h] = h;
    for (; k < P && !start[k]; ++k) {
      tail = clampi(row_order[w0 + k] - w0, P - 1);
      const double lv = ft[tail].lv;
      hmax = lv > hmax ? lv : hmax;
      line_head[w0 + tail] = h;
    }
    const Feat fe = ft[tail];
    const double hh = fh.lu * 0.5, he = fe.lu * 0.5;
    Line l;
    l.sx = fh.cx - fh.ux * hh;
    l.sy = fh.cy - fh.uy * hh;
    l.ex = fe.cx + fe.ux * he;
    l.ey = fe.cy + fe.uy * he;
    l.mx = (l.sx + l.ex) * 0.5;
    l.my = (l.sy + l.ey) * 0.5;
    l.ux = fh.ux;
    l.uy = fh.uy;
    l.vx = fh.vx;
    l.vy = fh.vy;
    l.len = (l.ex - l.sx) * fh.ux + (l.ey - l.sy) * fh.uy;
    l.h = hmax;
    l.live = !isolated(fh);
    l.pad = 0;
    line_rec[w0 + h] = l;
    line_state[w0 + h] = isolated(fh) ? 2 : 1;
    line_len[w0 + h] = k - pos;
  }
}

__global__ __launch_bounds__(kThreads) void column_block_kernel(
    const double* __restrict__ quads, const int32_t* __restrict__ img_off, int n_words, ColumnParams p, const int32_t* __restrict__ link,
    const Line* __restrict__ line_rec, const int32_t* __restrict__ line_state, const int32_t* __restrict__ line_head,
    const int32_t* __restrict__ line_len, int32_t* line_cut, const int32_t* __restrict__ row_pos, const double* __restrict__ gap_by_word,
    Block* block_rec, double* quad_by_slot, uint32_t* pred_bits, int pred_stride, int32_t* __restrict__ order, double* __restrict__ gaps, int32_t* __restrict__ line_start,
    int32_t* __restrict__ line_flags, int32_t* __restrict__ block_start, int32_t* __restrict__ block_levels,
    double* __restrict__ block_quads, int32_t* __restrict__ counts) {
  __shared__ int16_t nxt[kLineMaxWords], prv[kLineMaxWords], ptr[kLineMaxWords], dist[kLineMaxWords], mn[kLineMaxWords];
  __shared__ int16_t slot_of[kLineMaxWords];      // head line -> slot of its block
  __shared__ int16_t bhead[kLineMaxWords];        // slot -> head line
  __shared__ int16_t blines[kLineMaxWords];       // slot -> lines of the block, later its first line
  __shared__ int16_t level[2][kLineMaxWords];     // by slot
  __shared__ int16_t sorted[kLineMaxWords];       // rank -> slot
  __shared__ int16_t by_rank[kLineMaxWords];      // rank -> lines of the block, scanned: its first line
  __shared__ int16_t by_line[kLineMaxWords];      // line -> words, scanned: its first position
  __shared__ int16_t line_of[kLineMaxWords];      // head word -> line
  __shared__ int32_t part[kThreads];
  __shared__ Block xt[kTile];
  __shared__ int32_t n_blocks, changed;
  const int img = blockIdx.x, tid = threadIdx.x;
  const int w0 = img_off[img], P = img_off[img + 1] - w0;
  if (P == 0) {
    if (tid == 0) counts[2 * img] = counts[2 * img + 1] = 0;
    return;
  }
  const Line* lr = line_rec + w0;
  const int32_t* ls = line_state + w0;
  Block* br = block_rec + w0;
  double* qs = quad_by_slot + 8 * (size_t)w0;
  if (tid == 0) n_blocks = 0;
  chain_rank(link + w0, link + n_words + w0, P, nxt, prv, ptr, dist, mn, line_cut + w0);

  // blocks: a slot for every head line, in any order (the sort below is total); the tail leaves the number of lines
  for (int i = tid; i < P; i += kThreads)
    if (ls[i] && prv[i] < 0) {
      const int s = atomicAdd(&n_blocks, 1);
      bhead[s] = (int16_t)i;
      slot_of[i] = (int16_t)s;
    }
  __syncthreads();
  const int B = n_blocks;
  for (int i = tid; i < P; i += kThreads)
    if (ls[i] && nxt[i] < 0) blines[slot_of[ptr[i]]] = (int16_t)(dist[i] + 1);
  // the box of every block: one thread walks its lines, head to tail
  for (int s = tid; s < B; s += kThreads) {
    const int h = bhead[s];
    Block b;
    double q[8];
    if (ls[h] == 2) {   // an isolated word: its axis-aligned bounding box
      const double* w = quads + 8 * (size_t)(w0 + h);
      double x0 = w[0], x1 = w[0], y0 = w[1], y1 = w[1];
      for (int c = 1; c < 4; ++c) {
        x0 = w[2 * c] < x0 ? w[2 * c] : x0;
        x1 = w[2 * c] > x1 ? w[2 * c] : x1;
        y0 = w[2 * c + 1] < y0 ? w[2 * c + 1] : y0;
        y1 = w[2 * c + 1] > y1 ? w[2 * c + 1] : y1;
      }
      q[0] = x0, q[1] = y0, q[2] = x1, q[3] = y0, q[4] = x1, q[5] = y1, q[6] = x0, q[7] = y1;
      b.ux = 1.0, b.uy = 0.0, b.vx = 0.0, b.vy = 1.0;
      b.w = x1 - x0;
      b.h = y1 - y0;
    } else {
      const Line hl = lr[h];
      double X0 = 0, X1 = 0, Y0 = 0, Y1 = 0;
      int t = h;
      for (int n = 0; t >= 0 && n < P; ++n, t = nxt[t]) {
        const Line l = lr[t];
        const double xs = (l.sx - hl.sx) * hl.ux + (l.sy - hl.sy) * hl.uy, xe = (l.ex - hl.sx) * hl.ux + (l.ey - hl.sy) * hl.uy;
        const double mid = (l.mx - hl.sx) * hl.vx + (l.my - hl.sy) * hl.vy;
        const double ya = mid - l.h * 0.5, yb = mid + l.h * 0.5;
        if (n == 0) {
          X0 = X1 = xs;
          Y0 = ya;
          Y1 = yb;
        }
        X0 = xs < X0 ? xs : X0;
        X1 = xs > X1 ? xs : X1;
        X0 = xe < X0 ? xe : X0;
        X1 = xe > X1 ? xe : X1;
        Y0 = ya < Y0 ? ya : Y0;
        Y1 = yb > Y1 ? yb : Y1;
      }
      const double cx[4] = {X0, X1, X1, X0}, cy[4] = {Y0, Y0, Y1, Y1};
      for (int c = 0; c < 4; ++c) {
        q[2 * c] = (hl.sx + hl.ux * cx[c]) + hl.vx * cy[c];
        q[2 * c + 1] = (hl.sy + hl.uy * cx[c]) + hl.vy * cy[c];
      }
      b.ux = hl.ux, b.uy = hl.uy, b.vx = hl.vx, b.vy = hl.vy;
      b.w = X1 - X0;
      b.h = Y1 - Y0;
    }
    b.tx = q[0];
    b.ty = q[1];
    br[s] = b;
    for (int c = 0; c < 8; ++c) qs[8 * s + c] = q[c];
    level[0][s] = 0;
  }
  __syncthreads();

  // the relation, once: bit b of pred[xw * P + y] says that block 32 xw + b precedes block y.  The X side passes through LDS in tiles;
  // an item is one word of one y, and a wave's items share their word, so the tile reads are broadcasts
  uint32_t* pred = pred_bits + (size_t)w0 * pred_stride;
  for (int t0 = 0; t0 < B; t0 += kTile) {
    const int cnt = min(kTile, B - t0), words = (cnt + 31) / 32;
    if (tid < cnt) xt[tid] = br[t0 + tid];
    __syncthreads();
    for (int item = tid; item < B * words; item += kThreads) {
      const int y = item % B, wl = item / B, k1 = min(cnt, 32 * wl + 32);
      double yq[8];
      for (int c = 0; c < 8; ++c) yq[c] = qs[8 * y + c];
      uint32_t bits = 0;
      for (int k = 32 * wl; k < k1; ++k)
        if (t0 + k != y && precedes(xt[k], yq)) bits |= 1u << (k - 32 * wl);
      pred[(size_t)(t0 / 32 + wl) * P + y] = bits;
    }
    __syncthreads();
  }

  // levels: a round reads all old values and writes all new ones; a round that changes nothing ends them
  const int cap = p.max_levels - 1, XW = (B + 31) / 32;
  int cur = 0;
  for (int round = 0; round < cap; ++round) {
    if (tid == 0) changed = 0;
    __syncthreads();
    for (int y = tid; y < B; y += kThreads) {
      int m = -1;
      for (int xw0 = 0; xw0 < XW; xw0 += kPredBatch) {   // (the round is bound by the latency of these loads: a batch is in flight at once)
        uint32_t w[kPredBatch];
#pragma unroll
        for (int u = 0; u < kPredBatch; ++u) w[u] = xw0 + u < XW ? pred[(size_t)(xw0 + u) * P + y] : 0u;
#pragma unroll
        for (int u = 0; u < kPredBatch; ++u)
          while (w[u]) {
            m = max(m, (int)level[cur][32 * (xw0 + u) + __ffs(w[u]) - 1]);
            w[u] &= w[u] - 1;
          }
      }
      const int lv = min(cap, m + 1);
      level[cur ^ 1][y] = (int16_t)lv;
      if (lv != level[cur][y]) changed = 1;
    }
    __syncthreads();
    cur ^= 1;
    if (!changed) break;
    __syncthreads();   // (changed is reset at the top of the next round)
  }
  const int16_t* lvl = level[cur];

  // blocks by (level, TLy, TLx, index of the head line)
  int N2 = 1;
  while (N2 < B) N2 <<= 1;
  for (int i = tid; i < N2; i += kThreads) sorted[i] = (int16_t)(i < B ? i : kNone);
  __syncthreads();
  for (int k = 2; k <= N2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < N2; t += kThreads) {
        const int x = t ^ j;
        if (x > t) {
          const int a = sorted[t], b = sorted[x];
          bool a_first;
          if (a == kNone || b == kNone)
            a_first = b == kNone;
          else if (lvl[a] != lvl[b])
            a_first = lvl[a] < lvl[b];
          else {
            const double ay = br[a].ty, by = br[b].ty, ax = br[a].tx, bx = br[b].tx;
            a_first = ay < by || (ay == by && (ax < bx || (ax == bx && bhead[a] < bhead[b])));
          }
          const bool asc = (t & k) == 0;
          if (a != b && a_first != asc) {
            sorted[t] = (int16_t)b;
            sorted[x] = (int16_t)a;
          }
        }
      }
      __syncthreads();
    }
  }

  // lines of blocks: block r of the output is slot sorted[r]
  for (int r = tid; r < B; r += kThreads) by_rank[r] = blines[sorted[r]];
  __syncthreads();
  const int L = min(scan_exclusive(by_rank, B, part), P);
  for (int r = tid; r < B; r += kThreads) {
    const int s = sorted[r];
    blines[s] = by_rank[r];
    block_start[w0 + r] = by_rank[r];
    block_levels[w0 + r] = lvl[s];
    for (int c = 0; c < 8; ++c) block_quads[8 * (size_t)(w0 + r) + c] = qs[8 * s + c];
  }
  __syncthreads();
  // words of lines: line ptr's block start + rank
  for (int i = tid; i < P; i += kThreads)
    if (ls[i]) {
      const int l = clampi(blines[slot_of[ptr[i]]] + dist[i], P - 1);
      line_of[i] = (int16_t)l;
      by_line[l] = (int16_t)line_len[w0 + i];
      line_flags[w0 + l] = line_cut[w0 + i];
    }
  __syncthreads();
  (void)scan_exclusive(by_line, L, part);
  for (int l = tid; l < L; l += kThreads) line_start[w0 + l] = w0 + by_line[l];
  if (tid == 0) {
    counts[2 * img] = L;
    counts[2 * img + 1] = B;
  }
  for (int j = tid; j < P; j += kThreads) {
    const int h = clampi(line_head[w0 + j], P - 1);
    const int pos = clampi(by_line[line_of[h]] + (row_pos[w0 + j] - row_pos[w0 + h]), P - 1);   // (a line is a run of its row)
    order[w0 + pos] = w0 + j;
    gaps[w0 + pos] = j == h ? 0.0 : gap_by_word[w0 + j];
  }
}

}  // namespace

static_assert(sizeof(Feat) == kLineFeatBytes && sizeof(Gap) == kColumnGapBytes && sizeof(Line) == kColumnLineBytes &&
                  sizeof(Block) == kColumnBlockBytes, "records");

void launch_group_columns(const double* quads_dev, const int32_t* img_off_dev, int n_images, int n_words, int max_words,
                          const LineParams& row_params, const ColumnParams& p, const ColumnBuffers& b, hipStream_t s) {
  if (n_images <= 0 || n_words <= 0) return;
  launch_group_lines(quads_dev, img_off_dev, n_images, n_words, max_words, row_params, b.feat, b.link, b.row_order, b.flags, b.row_gaps,
                     b.row_start, b.n_rows, s);
  const Feat* feat = static_cast<const Feat*>(b.feat);
  Gap* gap_rec = static_cast<Gap*>(b.gap_rec);
  Line* line_rec = static_cast<Line*>(b.line_rec);
  const dim3 pairs((max_words + kOwners - 1) / kOwners, n_images, 2);
  hipLaunchKernelGGL(column_gap_kernel, dim3(n_images), dim3(kThreads), 0, s, feat, img_off_dev, p, b.row_order, b.row_start, b.n_rows,
                     b.row_prev, b.row_pos, gap_rec, b.gap_state, b.gap_by_word);
  OCR_HIP(hipGetLastError());
  hipLaunchKernelGGL(pair_link_kernel<Gap>, pairs, dim3(kTile), 0, s, gap_rec, img_off_dev, n_words, p, b.link);
  OCR_HIP(hipGetLastError());
  hipLaunchKernelGGL(column_line_kernel, dim3(n_images), dim3(kThreads), 0, s, feat, img_off_dev, n_words, p, b.link, b.row_order,
                     b.row_prev, b.row_pos, b.gap_state, b.flags, line_rec, b.line_state, b.line_head, b.line_len, b.line_cut);
  OCR_HIP(hipGetLastError());
  hipLaunchKernelGGL(pair_link_kernel<Line>, pairs, dim3(kTile), 0, s, line_rec, img_off_dev, n_words, p, b.link);
  OCR_HIP(hipGetLastError());
  hipLaunchKernelGGL(column_block_kernel, dim3(n_images), dim3(kThreads), 0, s, quads_dev, img_off_dev, n_words, p, b.link, line_rec,
                     b.line_state, b.line_head, b.line_len, b.line_cut, b.row_pos, b.gap_by_word, static_cast<Block*>(b.block_rec),
                     b.block_quads_by_slot, b.pred_bits, (max_words + 31) / 32, b.order, b.gaps, b.line_start, b.line_flags, b.block_start, b.block_levels, b.block_quads,
                     b.counts);
  OCR_HIP(hipGetLastError());
}

}  // namespace ocr
