// Word strips, host geometry (ocr_plan_word_strips): polygon -> exact convex hull -> minimum-area rectangle -> reading direction ->
// strip size and per-word f32 sampling map.  BUILD-DEFINED; the rule is written out in include/ocr_amd.h and restated in
// tests/strip_oracle.py.  Plain C++ compiled with -ffp-contract=off: every f64 operation is separately rounded, as numpy's are.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
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

}  // namespace

void plan_word_strips(const ocr_polygons_t& polys, const double* adj_xy, int n, const ocr_strip_params_t& p, WordStripsOwned& out) {
  if (polys.n_images != n) fail(OCR_ERR_INVALID, "plan_word_strips: polygon block holds %d images, frames %d", polys.n_images, n);
  if (polys.n_polygons < 0 || (n > 0 && (!polys.img_offsets || (polys.n_polygons > 0 && (!polys.poly_offsets || !polys.xy || !polys.scores)))))
    fail(OCR_ERR_INVALID, "plan_word_strips: null array in the polygon block");
  if (n > 0 && (polys.img_offsets[0] != 0 || polys.img_offsets[n] != polys.n_polygons))
    fail(OCR_ERR_INVALID, "plan_word_strips: image offsets do not span the %d polygons", polys.n_polygons);
  const int Hs = p.strip_height;
  out.height = Hs;
  out.img_offsets.assign(polys.img_offsets, polys.img_offsets + n + 1);
  out.col_offsets.assign(1, 0);
  out.total_width = 0;
  std::vector<IPt> pts;
  for (int b = 0; b < n; ++b) {
    const double ax = adj_xy[2 * b], ay = adj_xy[2 * b + 1];
    if (!(std::isfinite(ax) && ax > 0 && std::isfinite(ay) && ay > 0))
      fail(OCR_ERR_INVALID, "plan_word_strips: adjust values (%g, %g) of image %d (finite and > 0)", ax, ay, b);
    const int k0 = polys.img_offsets[b], k1 = polys.img_offsets[b + 1];
    if (k1 < k0 || k0 < 0 || k1 > polys.n_polygons) fail(OCR_ERR_INVALID, "plan_word_strips: image %d polygon range [%d, %d)", b, k0, k1);
    for (int k = k0; k < k1; ++k) {
      const int v0 = polys.poly_offsets[k], v1 = polys.poly_offsets[k + 1];
      if (v1 <= v0 || v0 < 0 || v1 > polys.n_vertices) fail(OCR_ERR_INVALID, "plan_word_strips: polygon %d vertex range [%d, %d)", k, v0, v1);
      pts.clear();
      for (int v = v0; v < v1; ++v) {
        const uint32_t x = polys.xy[2 * (size_t)v], y = polys.xy[2 * (size_t)v + 1];
        if (x >= (1u << 24) || y >= (1u << 24)) fail(OCR_ERR_INVALID, "plan_word_strips: polygon %d vertex (%u, %u) (limit 2^24)", k, x, y);
        pts.push_back({(int64_t)x, (int64_t)y});
      }
      const std::vector<IPt> hull = convex_hull(pts);
      const int m = (int)hull.size();
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
      DPt C[4];   // TL, TR, BR, BL
      for (int c = 0; c < 4; ++c) C[c] = R[(c + d) % 4];
      // 4. side lengths; a side under one pixel is widened about the centre
      double Ux = C[1].x - C[0].x, Uy = C[1].y - C[0].y, Vx = C[3].x - C[0].x, Vy = C[3].y - C[0].y;
      double lu = std::sqrt(Ux * Ux + Uy * Uy), lv = std::sqrt(Vx * Vx + Vy * Vy);
      if (lu < 1.0) {
        widen(C, 0, 3, 1, 2, lu, ux, uy);
        Ux = C[1].x - C[0].x; Uy = C[1].y - C[0].y; Vx = C[3].x - C[0].x; Vy = C[3].y - C[0].y;
        lu = std::sqrt(Ux * Ux + Uy * Uy); lv = std::sqrt(Vx * Vx + Vy * Vy);
      }
      if (lv < 1.0) {
        widen(C, 0, 1, 3, 2, lv, vx, vy);
        Ux = C[1].x - C[0].x; Uy = C[1].y - C[0].y; Vx = C[3].x - C[0].x; Vy = C[3].y - C[0].y;
        lu = std::sqrt(Ux * Ux + Uy * Uy); lv = std::sqrt(Vx * Vx + Vy * Vy);
      }
      // 5. strip width
      const double wd = std::floor(((double)Hs * lu) / lv + 0.5);
      int flags = m < 3 ? 2 : 0;
      int Ws;
      if (wd > (double)p.max_width) {
        Ws = p.max_width;
        flags |= 1;
      } else {
        Ws = wd < 1.0 ? 1 : (int)wd;
      }
      // 6. the map
      out.word_info.push_back(b);
      out.word_info.push_back(flags);
      for (int c = 0; c < 4; ++c) {
        out.quads.push_back(C[c].x);
        out.quads.push_back(C[c].y);
      }
      const float mp[6] = {(float)C[0].x, (float)C[0].y, (float)(Ux / Ws), (float)(Uy / Ws), (float)(Vx / Hs), (float)(Vy / Hs)};
      out.maps.insert(out.maps.end(), mp, mp + 6);
      out.scores.push_back(polys.scores[k]);
      out.total_width += Ws;
      if (out.total_width * Hs > kStripMaxAtlas)
        fail(OCR_ERR_INVALID, "plan_word_strips: atlas of more than 2^31 elements (%d rows, %lld columns after word %d)", Hs,
             (long long)out.total_width, k);
      out.col_offsets.push_back((int32_t)out.total_width);
    }
  }
}

}  // namespace ocr
