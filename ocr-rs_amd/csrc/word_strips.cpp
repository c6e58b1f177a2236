// Word strips, host geometry (ocr_plan_word_strips): polygon -> exact convex hull -> minimum-area rectangle -> reading direction ->
// strip size and per-word f32 sampling map; and of ocr_plan_curved_strips: the same rectangle -> centreline of the polygon's ring ->
// 33 knots with normals.  BUILD-DEFINED; the rules are written out in include/ocr_amd.h and restated in tests/strip_oracle.py and
// tests/curved_strip_oracle.py.  Plain C++ compiled with -ffp-contract=off: every f64 operation is separately rounded, as numpy's are.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "hypot_glibc.hpp"
#include "word_strips.hpp"

namespace ocr {
namespace {

struct IPt {
  int64_t x, y;
};
struct DPt {
  double x, y;
};

int64_t cross(const IPt& o, const IPt& a, const IPt& b) { return (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x); }

// Andrew's monotone chain: counter-clockwise (x right, y up), collinear points dropped, starting at the smallest (x, y)
std::vector<IPt> convex_hull(std::vector<IPt> pts) {
  std::sort(pts.begin(), pts.end(), [](const IPt& a, const IPt& b) { return a.x < b.x || (a.x == b.x && a.y < b.y); });
  pts.erase(std::unique(pts.begin(), pts.end(), [](const IPt& a, const IPt& b) { return a.x == b.x && a.y == b.y; }), pts.end());
  if (pts.size() < 2) return pts;
  std::vector<IPt> h;
  for (const IPt& p : pts) {   // lower chain
    while (h.size() >= 2 && cross(h[h.size() - 2], h.back(), p) <= 0) h.pop_back();
    h.push_back(p);
  }
  const size_t lower = h.size();
  for (size_t k = pts.size() - 1; k-- > 0;) {   // upper chain
    const IPt& p = pts[k];
    while (h.size() > lower && cross(h[h.size() - 2], h.back(), p) <= 0) h.pop_back();
    h.push_back(p);
  }
  h.pop_back();   // the first point again
  return h;
}

void widen(DPt* c, int lo0, int lo1, int hi0, int hi1, double len, double ux, double uy) {
  const double h = (1.0 - len) * 0.5, s = std::sqrt(ux * ux + uy * uy);
  const double dx = h * (ux / s), dy = h * (uy / s);
  c[lo0].x -= dx; c[lo0].y -= dy;
  c[lo1].x -= dx; c[lo1].y -= dy;
  c[hi0].x += dx; c[hi0].y += dy;
  c[hi1].x += dx; c[hi1].y += dy;
}

// steps 1-4 of the straight rule, shared by both planners: the hull's vertex count and the widened rectangle with its sides
struct Rect {
  int m;
  DPt C[4];   // TL, TR, BR, BL
  double Ux, Uy, Vx, Vy, lu, lv;
};

Rect word_rectangle(const std::vector<IPt>& pts, double ax, double ay) {
  Rect r;
  const std::vector<IPt> hull = convex_hull(pts);
  const int m = r.m = (int)hull.size();
  std::vector<DPt> P(m);
  for (int i = 0; i < m; ++i) P[i] = {(double)hull[i].x * ax, (double)hull[i].y * ay};
  // 2. minimum-area rectangle over the hull edges
  const int edges = m >= 3 ? m : 1;
  int best = -1;
  double best_area = 0, ba0 = 0, ba1 = 0, bb0 = 0, bb1 = 0, bex = 1, bey = 0;
  for (int i = 0; i < edges; ++i) {
    double ex = 1.0, ey = 0.0;
    if (m >= 2) {
      const DPt& q = P[(i + 1) % m];
      ex = q.x - P[i].x;
      ey = q.y - P[i].y;
    }
    const double ee = ex * ex + ey * ey;
    double a0 = 0, a1 = 0, b0 = 0, b1 = 0;
    for (int j = 0; j < m; ++j) {
      const double dx = P[j].x - P[i].x, dy = P[j].y - P[i].y;
      const double a = dx * ex + dy * ey, bb = dy * ex - dx * ey;
      if (j == 0 || a < a0) a0 = a;
      if (j == 0 || a > a1) a1 = a;
      if (j == 0 || bb < b0) b0 = bb;
      if (j == 0 || bb > b1) b1 = bb;
    }
    const double area = ((a1 - a0) * (b1 - b0)) / ee;
    if (best < 0 || area < best_area) {
      best = i; best_area = area;
      ba0 = a0; ba1 = a1; bb0 = b0; bb1 = b1; bex = ex; bey = ey;
    }
  }
  const DPt& Pi = P[best];
  const double ee = bex * bex + bey * bey;
  auto corner = [&](double a, double bb) { return DPt{Pi.x + (a * bex - bb * bey) / ee, Pi.y + (a * bey + bb * bex) / ee}; };
  const DPt R[4] = {corner(ba0, bb0), corner(ba1, bb0), corner(ba1, bb1), corner(ba0, bb1)};
  // 3. reading direction: +e, +e', -e, -e' (in the order of the cyclic shift of R they select)
  const double cand[4][2] = {{bex, bey}, {-bey, bex}, {-bex, -bey}, {bey, -bex}};
  int d = 0;
  for (int c = 1; c < 4; ++c)
    if (cand[c][0] > cand[d][0] || (cand[c][0] == cand[d][0] && cand[c][1] < cand[d][1])) d = c;
  const double ux = cand[d][0], uy = cand[d][1], vx = -uy, vy = ux;
  DPt* C = r.C;
  for (int c = 0; c < 4; ++c) C[c] = R[(c + d) % 4];
  // 4. side lengths; a side under one pixel is widened about the centre
  auto sides = [&] {
    r.Ux = C[1].x - C[0].x; r.Uy = C[1].y - C[0].y; r.Vx = C[3].x - C[0].x; r.Vy = C[3].y - C[0].y;
    r.lu = std::sqrt(r.Ux * r.Ux + r.Uy * r.Uy); r.lv = std::sqrt(r.Vx * r.Vx + r.Vy * r.Vy);
  };
  sides();
  if (r.lu < 1.0) {
    widen(C, 0, 3, 1, 2, r.lu, ux, uy);
    sides();
  }
  if (r.lv < 1.0) {
    widen(C, 0, 1, 3, 2, r.lv, vx, vy);
    sides();
  }
  return r;
}

// the polygon block and adjust values checked; f(image, polygon, its integer vertices in order, adj_x, adj_y) for every polygon
template <typename F>
void for_each_polygon(const char* who, const ocr_polygons_t& polys, const double* adj_xy, int n, F f) {
  if (polys.n_images != n) fail(OCR_ERR_INVALID, "%s: polygon block holds %d images, frames %d", who, polys.n_images, n);
  if (polys.n_polygons < 0 || (n > 0 && (!polys.img_offsets || (polys.n_polygons > 0 && (!polys.poly_offsets || !polys.xy || !polys.scores)))))
    fail(OCR_ERR_INVALID, "%s: null array in the polygon block", who);
  if (n > 0 && (polys.img_offsets[0] != 0 || polys.img_offsets[n] != polys.n_polygons))
    fail(OCR_ERR_INVALID, "%s: image offsets do not span the %d polygons", who, polys.n_polygons);
  std::vector<IPt> pts;
  for (int b = 0; b < n; ++b) {
    const double ax = adj_xy[2 * b], ay = adj_xy[2 * b + 1];
    if (!(std::isfinite(ax) && ax > 0 && std::isfinite(ay) && ay > 0))
      fail(OCR_ERR_INVALID, "%s: adjust values (%g, %g) of image %d (finite and > 0)", who, ax, ay, b);
    const int k0 = polys.img_offsets[b], k1 = polys.img_offsets[b + 1];
    if (k1 < k0 || k0 < 0 || k1 > polys.n_polygons) fail(OCR_ERR_INVALID, "%s: image %d polygon range [%d, %d)", who, b, k0, k1);
    for (int k = k0; k < k1; ++k) {
      const int v0 = polys.poly_offsets[k], v1 = polys.poly_offsets[k + 1];
      if (v1 <= v0 || v0 < 0 || v1 > polys.n_vertices) fail(OCR_ERR_INVALID, "%s: polygon %d vertex range [%d, %d)", who, k, v0, v1);
      pts.clear();
      for (int v = v0; v < v1; ++v) {
        const uint32_t x = polys.xy[2 * (size_t)v], y = polys.xy[2 * (size_t)v + 1];
        if (x >= (1u << 24) || y >= (1u << 24)) fail(OCR_ERR_INVALID, "%s: polygon %d vertex (%u, %u) (limit 2^24)", who, k, x, y);
        pts.push_back({(int64_t)x, (int64_t)y});
      }
      f(b, k, pts, ax, ay);
    }
  }
}

// 5. of the straight rule: floor(wd + 0.5) already taken; clamped to [1, max_width], above it the word is squeezed
int clamp_width(double wd, int max_width, int* flags) {
  if (wd > (double)max_width) {
    *flags |= 1;
    return max_width;
  }
  return wd < 1.0 ? 1 : (int)wd;
}

}  // namespace

void plan_word_strips(const ocr_polygons_t& polys, const double* adj_xy, int n, const ocr_strip_params_t& p, WordStripsOwned& out) {
  const int Hs = p.strip_height;
  out.height = Hs;
  out.col_offsets.assign(1, 0);
  out.total_width = 0;
  for_each_polygon("plan_word_strips", polys, adj_xy, n, [&](int b, int k, const std::vector<IPt>& pts, double ax, double ay) {
    const Rect r = word_rectangle(pts, ax, ay);
    const DPt* C = r.C;
    // 5. strip width
    int flags = r.m < 3 ? 2 : 0;
    const int Ws = clamp_width(std::floor(((double)Hs * r.lu) / r.lv + 0.5), p.max_width, &flags);
    // 6. the map
    out.word_info.push_back(b);
    out.word_info.push_back(flags);
    for (int c = 0; c < 4; ++c) {
      out.quads.push_back(C[c].x);
      out.quads.push_back(C[c].y);
    }
    const float mp[6] = {(float)C[0].x, (float)C[0].y, (float)(r.Ux / Ws), (float)(r.Uy / Ws), (float)(r.Vx / Hs), (float)(r.Vy / Hs)};
    out.maps.insert(out.maps.end(), mp, mp + 6);
    out.scores.push_back(polys.scores[k]);
    out.total_width += Ws;
    if (out.total_width * Hs > kStripMaxAtlas)
      fail(OCR_ERR_INVALID, "plan_word_strips: atlas of more than 2^31 elements (%d rows, %lld columns after word %d)", Hs,
           (long long)out.total_width, k);
    out.col_offsets.push_back((int32_t)out.total_width);
  });
  out.img_offsets.assign(polys.img_offsets, polys.img_offsets + n + 1);
}

// Curved strips (rule: include/ocr_amd.h ocr_plan_curved_strips, oracle tests/curved_strip_oracle.py): the centreline of the polygon's
// own ring between 32 scan lines across the rectangle, resampled to 33 knots at equal arc length with their normals.
void plan_curved_strips(const ocr_polygons_t& polys, const double* adj_xy, int n, const ocr_curve_params_t& p, CurvedStripsOwned& out) {
  constexpr int S = OCR_CURVE_SCANLINES, K = OCR_CURVE_KNOTS;
  const int Hs = p.strip_height;
  const double fHs = (double)Hs;
  out.height = Hs;
  out.col_offsets.assign(1, 0);
  out.total_width = 0;
  std::vector<double> ra, rb;
  for_each_polygon("plan_curved_strips", polys, adj_xy, n, [&](int b, int k, const std::vector<IPt>& pts, double ax, double ay) {
    const Rect r = word_rectangle(pts, ax, ay);
    const double tlx = r.C[0].x, tly = r.C[0].y;
    int flags = 0;
    double kn[K][4], h = 0, L = 0, wd = 0;
    // 9. the straight fallback
    auto straight = [&] {
      flags |= 16;
      for (int q = 0; q < K; ++q) {
        const double f = q / 32.0;
        kn[q][0] = (tlx + r.Ux * f) + r.Vx * 0.5;
        kn[q][1] = (tly + r.Uy * f) + r.Vy * 0.5;
        kn[q][2] = r.Vx / fHs;
        kn[q][3] = r.Vy / fHs;
      }
      h = r.lv / 2;
      L = r.lu;
      wd = std::floor((fHs * r.lu) / r.lv + 0.5);
    };
    auto curved = [&]() -> bool {
      const double eux = r.Ux / r.lu, euy = r.Uy / r.lu, evx = r.Vx / r.lv, evy = r.Vy / r.lv;
      // 2. the ring in rectangle coordinates
      const int nv = (int)pts.size();
      ra.resize(nv);
      rb.resize(nv);
      for (int i = 0; i < nv; ++i) {
        const double dx = (double)pts[i].x * ax - tlx, dy = (double)pts[i].y * ay - tly;
        ra[i] = dx * eux + dy * euy;
        rb[i] = dx * evx + dy * evy;
      }
      // 3. scan lines
      double as[S], ms[S], ts[S];
      for (int s = 0; s < S; ++s) {
        const double a = (r.lu * (s + 0.5)) / 32;
        double top = 0, bot = 0;
        int cnt = 0;
        for (int i = 0; i < nv; ++i) {
          const int j = i + 1 < nv ? i + 1 : 0;
          if ((ra[i] <= a) != (ra[j] <= a)) {
            const double bb = rb[i] + ((a - ra[i]) * (rb[j] - rb[i])) / (ra[j] - ra[i]);
            if (cnt == 0 || bb < top) top = bb;
            if (cnt == 0 || bb > bot) bot = bb;
            ++cnt;
          }
        }
        if (cnt > 2) flags |= 4;
        as[s] = a;
        ms[s] = (top + bot) * 0.5;
        ts[s] = bot - top;
      }
      // 4. valid span
      double sorted[S];
      std::copy(ts, ts + S, sorted);
      std::sort(sorted, sorted + S);
      const double tm = sorted[16];
      if (!(tm > 0)) return false;
      int lo = -1, hi = -1;
      for (int s = 0; s < S; ++s)
        if (ts[s] * 100 >= (double)p.valid_pct * tm) {
          if (lo < 0) lo = s;
          hi = s;
        }
      if (lo < 0 || hi - lo < 1) return false;
      // 5. centreline
      const double s0 = (ms[lo + 1] - ms[lo]) / (as[lo + 1] - as[lo]), s1 = (ms[hi] - ms[hi - 1]) / (as[hi] - as[hi - 1]);
      double Qa[S + 2], Qb[S + 2], len[S + 1], start[S + 2];
      int nq = 0;
      Qa[nq] = 0.0; Qb[nq++] = ms[lo] - s0 * as[lo];
      for (int s = lo; s <= hi; ++s) { Qa[nq] = as[s]; Qb[nq++] = ms[s]; }
      Qa[nq] = r.lu; Qb[nq++] = ms[hi] + s1 * (r.lu - as[hi]);
      const int nseg = nq - 1;
      start[0] = 0.0;
      for (int i = 0; i < nseg; ++i) {
        const double da = Qa[i + 1] - Qa[i], db = Qb[i + 1] - Qb[i];
        if (std::fabs(db) * 10 > std::fabs(da) * 7) flags |= 8;
        len[i] = hypot_glibc(da, db);
        start[i + 1] = start[i] + len[i];
      }
      L = start[nseg];
      // 6. half height
      double hh[S];
      const int cnt = hi - lo + 1;
      for (int s = lo; s <= hi; ++s) {
        const int i = s - lo + 1;
        const double da = Qa[i + 1] - Qa[i - 1], db = Qb[i + 1] - Qb[i - 1];
        const double c = da / hypot_glibc(da, db);
        hh[s - lo] = (ts[s] * c) * 0.5;
      }
      std::sort(hh, hh + cnt);
      h = hh[cnt / 2];
      if (h < 0.5) h = 0.5;
      // 7. width
      wd = std::floor((fHs * L) / (2 * h) + 0.5);
      // 8. knots
      double Pa[K], Pb[K];
      for (int q = 0; q < K - 1; ++q) {
        const double l = (L * q) / 32;
        int i = 0;
        while (i + 1 < nseg && start[i + 1] <= l) ++i;
        const double d = l - start[i];
        Pa[q] = Qa[i] + (d * (Qa[i + 1] - Qa[i])) / len[i];
        Pb[q] = Qb[i] + (d * (Qb[i + 1] - Qb[i])) / len[i];
      }
      Pa[K - 1] = Qa[nq - 1];
      Pb[K - 1] = Qb[nq - 1];
      const double kk = (2 * h) / fHs;
      for (int q = 0; q < K; ++q) {
        const int q1 = q + 1 < K ? q + 1 : K - 1, q0 = q > 0 ? q - 1 : 0;
        const double da = Pa[q1] - Pa[q0], db = Pb[q1] - Pb[q0];
        const double hy = hypot_glibc(da, db);
        const double ta = da / hy, tb = db / hy;
        const double na = (-tb) * kk, nb = ta * kk;
        kn[q][0] = (tlx + Pa[q] * eux) + Pb[q] * evx;
        kn[q][1] = (tly + Pa[q] * euy) + Pb[q] * evy;
        kn[q][2] = na * eux + nb * evx;
        kn[q][3] = na * euy + nb * evy;
      }
      return true;
    };
    if (r.m < 3) {
      flags |= 2;
      straight();
    } else if (!curved()) {
      straight();
    }
    const int Ws = clamp_width(wd, p.max_width, &flags);
    out.word_info.push_back(b);
    out.word_info.push_back(flags);
    for (int q = 0; q < K; ++q)
      for (int c = 0; c < 4; ++c) out.knots.push_back((float)kn[q][c]);
    out.tscale.push_back((float)(32.0 / Ws));
    out.half_heights.push_back(h);
    out.lengths.push_back(L);
    out.scores.push_back(polys.scores[k]);
    out.total_width += Ws;
    if (out.total_width * Hs > kStripMaxAtlas)
      fail(OCR_ERR_INVALID, "plan_curved_strips: atlas of more than 2^31 elements (%d rows, %lld columns after word %d)", Hs,
           (long long)out.total_width, k);
    out.col_offsets.push_back((int32_t)out.total_width);
  });
  out.img_offsets.assign(polys.img_offsets, polys.img_offsets + n + 1);
}

}  // namespace ocr
