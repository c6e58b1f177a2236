// Test and tuning hooks (libocr_amd_test.so): NOT part of the drop-in surface and not in libocr_amd.so.  They reach
// into the product library's internals (it exports its C++ symbols) so that kernels and host geometry can be pinned
// one piece at a time: the host-geometry hooks need no GPU and pin the C++ geometry against the reference KATs.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <limits>

#include "api_internal.hpp"
#include "test_kernels.hpp"

using ocr::guard;
namespace ocr { void winograd43_set_debug(int d); }
#ifdef W43_STAMPS
namespace ocr { void winograd43_read_stamps(long long* out); }
#endif
#ifdef STEM_STAMPS
namespace ocr { void stem_read_stamps(long long* out); }
extern "C" int ocr_test_stem_stamps(long long* out) { ocr::stem_read_stamps(out); return 0; }
#endif
#ifdef WS_STAMPS
#endif

// the conv hooks' launch: the 256 x 128 persistent split-bf16 form (conv_x3w.hip, in this library only) where it is asked for and takes
// the launch, conv_igemm otherwise
static void launch_conv(const ocr::ConvDesc& d, bool wide, int cus, hipStream_t s) {
  if (wide && ocr::conv_x3_wide_applicable(d)) ocr::launch_conv_x3_wide(d, cus, s);
  else ocr::launch_conv_igemm(d, s);
}

extern "C" {

int ocr_test_contour_candidates(const uint8_t* bitmap01, int h, int w, int32_t* xy_out, int32_t* counts_out,
                                int max_pts, int max_polys, int* n_polys) {
  return guard([&] {
    std::vector<std::vector<ocr::geom::Pt>> cands;
    ocr::geom::contour_candidates(bitmap01, h, w, cands);
    int np = 0, used = 0;
    for (const auto& c : cands) {
      if (np >= max_polys || used + (int)c.size() > max_pts) ocr::fail(OCR_ERR_INVALID, "test buffer too small");
      counts_out[np++] = (int)c.size();
      for (const auto& p : c) {
        xy_out[2 * used] = p.x;
        xy_out[2 * used + 1] = p.y;
        ++used;
      }
    }
    *n_polys = np;
  });
}
// the form launch_contour_trace runs for an h x w map (contour_trace_form: 0 does not fit, 1 one wave, else the parallel form's LDS words)
int ocr_test_contour_trace_form(int h, int w, int sequential, int have_spec, int* form) {
  return guard([&] { *form = ocr::contour_trace_form(h, w, sequential != 0, have_spec != 0); });
}
// the device tracer (contours.hip) on one 0/1 bitmap: raw contours (not the Douglas-Peucker candidates); status = the kernel's
// (0 ok, 1 buffers too small, 2 iteration guard, 3 parallel form only: a start outside its list).  max_pts / max_polys double as the kernel's capacities.
// form = the form that ran (contour_trace_form), starts_k = the parallel form's count of plausible starts (header word 3; 0 for the one-wave form)
int ocr_test_device_contours(const uint8_t* bitmap01, int h, int w, int32_t* xy_out, int32_t* counts_out, int max_pts, int max_polys,
                             int* n_polys, int* status, int sequential, int* form, int* starts_k) {
  return guard([&] {
    *form = ocr::contour_trace_form(h, w, sequential != 0, true);
    if (!*form) ocr::fail(OCR_ERR_INVALID, "device contours: %dx%d does not fit", h, w);
    const size_t npx = (size_t)h * w, wpi = ocr::binarize_pack_words(npx);
    std::vector<uint32_t> bits(wpi, 0u);
    for (size_t i = 0; i < npx; ++i)
      if (bitmap01[i]) bits[i >> 5] |= 1u << (i & 31);
    uint32_t *d_bits = nullptr, *d_pts = nullptr, *d_pk = nullptr;
    int *d_st = nullptr, *d_hdr = nullptr, *d_ln = nullptr;
    OCR_HIP(hipMalloc(reinterpret_cast<void**>(&d_bits), wpi * 4));
    OCR_HIP(hipMalloc(reinterpret_cast<void**>(&d_pts), (size_t)max_pts * 4));
    OCR_HIP(hipMalloc(reinterpret_cast<void**>(&d_pk), (size_t)max_pts * 4));
    OCR_HIP(hipMalloc(reinterpret_cast<void**>(&d_st), ((size_t)max_polys + 1) * 4));
    OCR_HIP(hipMalloc(reinterpret_cast<void**>(&d_ln), (size_t)max_polys * 4));
    OCR_HIP(hipMalloc(reinterpret_cast<void**>(&d_hdr), 16));
    void* d_spec = nullptr;
    OCR_HIP(hipMalloc(&d_spec, ocr::contour_spec_bytes(1)));
    OCR_HIP(hipMemcpy(d_bits, bits.data(), wpi * 4, hipMemcpyHostToDevice));
    ocr::launch_contour_trace(d_bits, wpi, 1, h, w, d_pts, max_pts, d_st, max_polys, d_hdr, d_pk, d_ln, d_spec, sequential, nullptr);
    int hdr[4];
    OCR_HIP(hipMemcpy(hdr, d_hdr, 16, hipMemcpyDeviceToHost));
    *status = hdr[2];
    *starts_k = hdr[3];
    *n_polys = 0;
    if (hdr[2] == 0) {
      std::vector<uint32_t> pts((size_t)hdr[1]);
      std::vector<int32_t> lens((size_t)hdr[0]);
      if (hdr[1]) OCR_HIP(hipMemcpy(pts.data(), d_pk, pts.size() * 4, hipMemcpyDeviceToHost));
      if (hdr[0]) OCR_HIP(hipMemcpy(lens.data(), d_ln, lens.size() * 4, hipMemcpyDeviceToHost));
      for (int k = 0; k < hdr[0]; ++k) counts_out[k] = lens[k];
      for (int i = 0; i < hdr[1]; ++i) {
        xy_out[2 * i] = (int32_t)(pts[i] & 0xffffu);
        xy_out[2 * i + 1] = (int32_t)(pts[i] >> 16);
      }
      *n_polys = hdr[0];
    }
    for (void* q : {(void*)d_bits, (void*)d_pts, (void*)d_pk, (void*)d_st, (void*)d_ln, (void*)d_hdr, d_spec}) (void)hipFree(q);
  });
}
// candidates.hip alone (arc length, Douglas-Peucker, the >= 4 points filter, job list with the clamped boxes) on contours GIVEN by the
// caller - any map size, e.g. the oracle's contours of the reference's 800 x 800 fixtures - laid out as the device tracer would have
// left them for one image.  Out: the candidate polygons in list order and per candidate its job box (min_x, min_y, bw, bh).
int ocr_test_device_candidates(const int32_t* xy, const int32_t* lens, int nc, int h, int w, int32_t* xy_out, int32_t* counts_out, int32_t* box_out,
                               int max_pts, int max_polys, int* n_polys) {
  return guard([&] {
    if (nc < 0 || nc > 65535 || h <= 0 || w <= 0 || h > 65535 || w > 65535) ocr::fail(OCR_ERR_INVALID, "device candidates: bad shape");
    size_t total = 0;
    for (int c = 0; c < nc; ++c) total += (size_t)lens[c];
    const int cap = (int)std::max<size_t>(total, 64), maxc = std::max(nc, 1);
    std::vector<uint32_t> pts((size_t)cap, 0u);
    std::vector<int> starts((size_t)maxc + 1, 0);
    size_t at = 0;
    for (int c = 0; c < nc; ++c) {
      starts[c] = (int)at;
      for (int i = 0; i < lens[c]; ++i, ++at) pts[at] = ((uint32_t)xy[2 * at + 1] << 16) | ((uint32_t)xy[2 * at] & 0xffffu);
    }
    for (int c = nc; c <= maxc; ++c) starts[c] = (int)at;
    const int hdr[4] = {nc, (int)total, 0, 0};
    const size_t sb = ocr::candidates_scratch_bytes(1, cap, maxc);
    char* d = nullptr;
    auto al = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t o_pts = al(16), o_st = o_pts + al((size_t)cap * 4), o_sc = o_st + al(((size_t)maxc + 1) * 4), o_jobs = o_sc + al(sb),
                 o_xy = o_jobs + al((size_t)max_polys * sizeof(ocr::BoxScoreJob)), o_tot = o_xy + al((size_t)max_pts * 8), o_hd = o_tot + 256, end = o_hd + 256;
    OCR_HIP(hipMalloc(reinterpret_cast<void**>(&d), end));
    OCR_HIP(hipMemset(d, 0, end));
    OCR_HIP(hipMemcpy(d, hdr, 16, hipMemcpyHostToDevice));
    OCR_HIP(hipMemcpy(d + o_pts, pts.data(), (size_t)cap * 4, hipMemcpyHostToDevice));
    OCR_HIP(hipMemcpy(d + o_st, starts.data(), ((size_t)maxc + 1) * 4, hipMemcpyHostToDevice));
    ocr::launch_candidates(reinterpret_cast<const int*>(d), reinterpret_cast<const uint32_t*>(d + o_pts), cap, reinterpret_cast<const int*>(d + o_st), maxc, 1, h, w,
                           d + o_sc, reinterpret_cast<ocr::BoxScoreJob*>(d + o_jobs), max_polys, reinterpret_cast<int32_t*>(d + o_xy), max_pts,
                           reinterpret_cast<int*>(d + o_tot), reinterpret_cast<int*>(d + o_hd), nullptr);
    int totals[4] = {0, 0, 0, 0};
    OCR_HIP(hipMemcpy(totals, d + o_hd, 12, hipMemcpyDeviceToHost));
    if (totals[2] != 0) {
      (void)hipFree(d);
      ocr::fail(OCR_ERR_INVALID, "test buffer too small");
    }
    std::vector<ocr::BoxScoreJob> jobs((size_t)totals[0]);
    std::vector<int32_t> oxy(2 * (size_t)totals[1]);
    if (totals[0]) OCR_HIP(hipMemcpy(jobs.data(), d + o_jobs, jobs.size() * sizeof(ocr::BoxScoreJob), hipMemcpyDeviceToHost));
    if (totals[1]) OCR_HIP(hipMemcpy(oxy.data(), d + o_xy, oxy.size() * 4, hipMemcpyDeviceToHost));
    (void)hipFree(d);
    size_t used = 0;
    for (int j = 0; j < totals[0]; ++j) {
      const auto& jb = jobs[j];
      counts_out[j] = jb.n_pts;
      box_out[4 * j] = jb.min_x;
      box_out[4 * j + 1] = jb.min_y;
      box_out[4 * j + 2] = jb.bw;
      box_out[4 * j + 3] = jb.bh;
      for (int i = 0; i < jb.n_pts; ++i, ++used) {
        xy_out[2 * used] = oxy[2 * ((size_t)jb.pt_offset + i)];
        xy_out[2 * used + 1] = oxy[2 * ((size_t)jb.pt_offset + i) + 1];
      }
    }
    *n_polys = totals[0];
  });
}
// candidates.hip on a BATCH laid out as the device tracer leaves it, with nothing interpreted: per image the tracer status (header
// word 2) and its contour count, flat contour lengths and flat (x, y); image i's points at i * cap, its starts row maxc + 1 long with
// entries 0 .. nc written (the tracer writes no more).  max_jobs / max_pts are the caller's, too small ones included.  Before the one
// launch the whole candidates scratch is filled with the byte scratch_fill and the job list, the point list, `guard` further jobs and
// points behind each, tot and totals with the word `poison`.  Out, raw: tot [n][2], totals [3], (max_jobs + guard) jobs of 7 ints,
// (max_pts + guard) points of 2 ints.
int ocr_test_candidates_batch(int n, int h, int w, const int32_t* status, const int32_t* ncs, const int32_t* lens, const int32_t* xy, int cap, int maxc,
                              int max_jobs, int max_pts, int scratch_fill, int guard_n, uint32_t poison, int32_t* tot_out, int32_t* totals_out,
                              int32_t* jobs_out, int32_t* pts_out) {
  return guard([&] {
    static_assert(sizeof(ocr::BoxScoreJob) == 28, "the hook returns a job as 7 ints");
    if (n <= 0 || n > 65535 || h <= 0 || w <= 0 || h > 65535 || w > 65535 || cap < 64 || maxc < 1 || max_jobs < 0 || max_pts < 0 || guard_n < 0 ||
        scratch_fill < 0 || scratch_fill > 255 || max_jobs > (1 << 24) || max_pts > (1 << 26) || guard_n > (1 << 20))
      ocr::fail(OCR_ERR_INVALID, "candidates batch: bad shape");
    std::vector<uint32_t> pts((size_t)n * cap, 0u);
    std::vector<int> starts((size_t)n * (maxc + 1), 0), hdr((size_t)n * 4, 0);
    size_t c_at = 0, p_at = 0;
    for (int b = 0; b < n; ++b) {
      const int nc = ncs[b];
      if (nc < 0 || nc > maxc) ocr::fail(OCR_ERR_INVALID, "candidates batch: image %d has %d contours, maxc %d", b, nc, maxc);
      size_t at = 0;
      for (int c = 0; c < nc; ++c, ++c_at) {
        const int len = lens[c_at];
        if (len < 0 || at + (size_t)len > (size_t)cap) ocr::fail(OCR_ERR_INVALID, "candidates batch: image %d holds more than cap = %d points", b, cap);
        starts[(size_t)b * (maxc + 1) + c] = (int)at;
        for (int i = 0; i < len; ++i, ++at, ++p_at) {
          const int32_t x = xy[2 * p_at], y = xy[2 * p_at + 1];
          if (x < 0 || x > 65535 || y < 0 || y > 65535) ocr::fail(OCR_ERR_INVALID, "candidates batch: coordinate outside 0..65535");
          pts[(size_t)b * cap + at] = ((uint32_t)y << 16) | (uint32_t)x;
        }
      }
      starts[(size_t)b * (maxc + 1) + nc] = (int)at;
      hdr[4 * (size_t)b] = nc;
      hdr[4 * (size_t)b + 1] = (int)at;
      hdr[4 * (size_t)b + 2] = status[b];
    }
    const size_t sb = ocr::candidates_scratch_bytes(n, cap, maxc);
    const size_t n_jobs = (size_t)max_jobs + guard_n, n_pts = (size_t)max_pts + guard_n;
    auto al = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t o_pts = al(hdr.size() * 4), o_st = o_pts + al(pts.size() * 4), o_sc = o_st + al(starts.size() * 4), o_jobs = o_sc + al(sb),
                 o_xy = o_jobs + al(n_jobs * sizeof(ocr::BoxScoreJob) + 4), o_tot = o_xy + al(n_pts * 8 + 4), o_hd = o_tot + al((size_t)n * 8), end = o_hd + 256;
    char* d = nullptr;
    OCR_HIP(hipMalloc(reinterpret_cast<void**>(&d), end));
    try {
      OCR_HIP(hipMemcpy(d, hdr.data(), hdr.size() * 4, hipMemcpyHostToDevice));
      OCR_HIP(hipMemcpy(d + o_pts, pts.data(), pts.size() * 4, hipMemcpyHostToDevice));
      OCR_HIP(hipMemcpy(d + o_st, starts.data(), starts.size() * 4, hipMemcpyHostToDevice));
      OCR_HIP(hipMemset(d + o_sc, scratch_fill, al(sb)));
      OCR_HIP(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(d + o_jobs), (int)poison, (end - o_jobs) / 4));   // jobs, points, guards, tot, totals
      ocr::launch_candidates(reinterpret_cast<const int*>(d), reinterpret_cast<const uint32_t*>(d + o_pts), cap, reinterpret_cast<const int*>(d + o_st), maxc, n, h, w,
                             d + o_sc, reinterpret_cast<ocr::BoxScoreJob*>(d + o_jobs), max_jobs, reinterpret_cast<int32_t*>(d + o_xy), max_pts,
                             reinterpret_cast<int*>(d + o_tot), reinterpret_cast<int*>(d + o_hd), nullptr);
      OCR_HIP(hipDeviceSynchronize());
      OCR_HIP(hipMemcpy(tot_out, d + o_tot, (size_t)n * 8, hipMemcpyDeviceToHost));
      OCR_HIP(hipMemcpy(totals_out, d + o_hd, 12, hipMemcpyDeviceToHost));
      if (n_jobs) OCR_HIP(hipMemcpy(jobs_out, d + o_jobs, n_jobs * sizeof(ocr::BoxScoreJob), hipMemcpyDeviceToHost));
      if (n_pts) OCR_HIP(hipMemcpy(pts_out, d + o_xy, n_pts * 8, hipMemcpyDeviceToHost));
    } catch (...) {
      (void)hipFree(d);
      throw;
    }
    (void)hipFree(d);
  });
}
// the host tracer's raw contours, for the same comparison
int ocr_test_host_contours(const uint8_t* bitmap01, int h, int w, int32_t* xy_out, int32_t* counts_out, int max_pts, int max_polys, int* n_polys) {
  return guard([&] {
    std::vector<std::vector<ocr::geom::Pt>> cs;
    ocr::geom::find_contours(bitmap01, h, w, cs);
    int np = 0, used = 0;
    for (const auto& c : cs) {
      if (np >= max_polys || used + (int)c.size() > max_pts) ocr::fail(OCR_ERR_INVALID, "test buffer too small");
      counts_out[np++] = (int)c.size();
      for (const auto& q : c) {
        xy_out[2 * used] = q.x;
        xy_out[2 * used + 1] = q.y;
        ++used;
      }
    }
    *n_polys = np;
  });
}
int ocr_test_expand_polygon(const int32_t* xy, int n, double factor, int32_t* xy_out, int max_out, int* n_out,
                            double* sside_out) {
  return guard([&] {
    std::vector<ocr::geom::Pt> in(n), out;
    for (int i = 0; i < n; ++i) in[i] = {xy[2 * i], xy[2 * i + 1]};
    if (!ocr::geom::expand_polygon(in, factor, out)) {
      *n_out = 0;
      return;
    }
    if ((int)out.size() > max_out) ocr::fail(OCR_ERR_INVALID, "test buffer too small");
    for (size_t i = 0; i < out.size(); ++i) {
      xy_out[2 * i] = out[i].x;
      xy_out[2 * i + 1] = out[i].y;
    }
    *n_out = (int)out.size();
    ocr::geom::Pt box[4];
    if (sside_out) *sside_out = ocr::geom::min_area_bounding_box(out, box);
  });
}
int ocr_test_det_stage(ocr_det_t* det, int id, float* out_host, size_t capacity, size_t* elems) {
  return guard([&] {
    if (!det || !elems) ocr::fail(OCR_ERR_INVALID, "null argument");
    const float* p = det->impl.stage(id, elems);
    if (out_host) {
      if (*elems > capacity) ocr::fail(OCR_ERR_INVALID, "stage %d needs %zu floats", id, *elems);
      det->impl.synchronize();
      OCR_HIP(hipMemcpy(out_host, p, *elems * sizeof(float), hipMemcpyDeviceToHost));
    }
  });
}
// raw GPU box scores of given polygons over a host map (sum and pixel count per polygon)
int ocr_test_box_scores(ocr_det_t* det, const float* prob_host, int h, int w, const int32_t* xy, const int32_t* counts,
                        int n_polys, double* sums_out, double* counts_out) {
  return guard([&] {
    using namespace ocr;
    if (!det) fail(OCR_ERR_INVALID, "null handle");
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    std::vector<BoxScoreJob> jobs;
    int pos = 0;
    for (int k = 0; k < n_polys; ++k) {
      int mnx = INT32_MAX, mxx = 0, mny = INT32_MAX, mxy = 0;
      for (int i = 0; i < counts[k]; ++i) {
        mnx = std::min(mnx, xy[2 * (pos + i)]);
        mxx = std::max(mxx, xy[2 * (pos + i)]);
        mny = std::min(mny, xy[2 * (pos + i) + 1]);
        mxy = std::max(mxy, xy[2 * (pos + i) + 1]);
      }
      mnx = std::clamp(mnx, 0, h - 1);
      mxx = std::clamp(mxx, 0, h - 1);
      mny = std::clamp(mny, 0, w - 1);
      mxy = std::clamp(mxy, 0, w - 1);
      if (mxx >= w || mxy >= h || counts[k] > kBoxScoreMaxPts) fail(OCR_ERR_INVALID, "bad test polygon");
      jobs.push_back({0, pos, counts[k], mnx, mny, mxx - mnx + 1, mxy - mny + 1});
      pos += counts[k];
    }
    Carve c;   // the map first
    c.take((size_t)h * w * 4);
    const size_t o_jobs = c.take(jobs.size() * sizeof(BoxScoreJob)), o_pts = c.take((size_t)pos * 8), o_sum = c.take((size_t)n_polys * 8),
                 o_cnt = c.take((size_t)n_polys * 8);
    char* sc = static_cast<char*>(det->impl.scratch(0, c.end));
    OCR_HIP(hipMemcpyAsync(sc, prob_host, (size_t)h * w * 4, hipMemcpyHostToDevice, s));
    OCR_HIP(hipMemcpyAsync(sc + o_jobs, jobs.data(), jobs.size() * sizeof(BoxScoreJob), hipMemcpyHostToDevice, s));
    OCR_HIP(hipMemcpyAsync(sc + o_pts, xy, (size_t)pos * 8, hipMemcpyHostToDevice, s));
    launch_box_scores(at<const float>(sc, 0), h, w, at<const BoxScoreJob>(sc, o_jobs), at<const int32_t>(sc, o_pts), n_polys, at<double>(sc, o_sum),
                      at<double>(sc, o_cnt), s);
    OCR_HIP(hipMemcpyAsync(sums_out, sc + o_sum, (size_t)n_polys * 8, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(counts_out, sc + o_cnt, (size_t)n_polys * 8, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipStreamSynchronize(s));
  });
}
// the whole box-score kernel on caller data: n maps of h x w, polygons with an image index each, through either launch.  grid == 0:
// launch_box_scores; grid > 0: launch_box_scores_counted with `grid` workgroups and the job count in device memory (dev_count, 0 ..
// n_polys - what candidates.hip's totals[0] would hold).  Behind the n_polys jobs lie `slack` more, copies of job 0, which no launch may
// touch.  EVERY result slot (n_polys + slack sums and counts) holds `sentinel` before the launch and comes back as it is afterwards.
// Boxes as build_jobs (postprocess.hip) makes them - x clamped by H, y by W - and returned as (min_x, min_y, bw, bh) per polygon.
int ocr_test_box_scores_batch(ocr_det_t* det, const float* prob_host, int n, int h, int w, const int32_t* xy, const int32_t* counts,
                              const int32_t* images, int n_polys, int grid, int dev_count, int slack, double sentinel, double* sums_out,
                              double* counts_out, int32_t* box_out) {
  return guard([&] {
    using namespace ocr;
    if (!det || !prob_host || !sums_out || !counts_out || !box_out) fail(OCR_ERR_INVALID, "null argument");
    if (n <= 0 || h <= 0 || w <= 0 || n_polys < 0 || slack < 0 || grid < 0 || grid > 65535 || dev_count < 0 || dev_count > n_polys ||
        (slack > 0 && n_polys == 0))
      fail(OCR_ERR_INVALID, "box scores: bad shape");
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    std::vector<BoxScoreJob> jobs;
    int pos = 0;
    for (int k = 0; k < n_polys; ++k) {
      if (counts[k] < 1 || counts[k] > kBoxScoreMaxPts) fail(OCR_ERR_INVALID, "polygon with %d vertices (1 .. %d)", counts[k], kBoxScoreMaxPts);
      if (images[k] < 0 || images[k] >= n) fail(OCR_ERR_INVALID, "polygon %d: image %d of %d", k, images[k], n);
      int mnx = INT32_MAX, mxx = 0, mny = INT32_MAX, mxy = 0;
      for (int i = 0; i < counts[k]; ++i) {
        const int x = xy[2 * (pos + i)], y = xy[2 * (pos + i) + 1];
        if (x < -65535 || x > 65535 || y < -65535 || y > 65535) fail(OCR_ERR_INVALID, "polygon %d: coordinate out of range", k);
        mnx = std::min(mnx, x), mxx = std::max(mxx, x);
        mny = std::min(mny, y), mxy = std::max(mxy, y);
      }
      // the reference clamps x by size[-2] (=H) and y by size[-1] (=W): metrics.rs:151-166
      mnx = std::clamp(mnx, 0, h - 1), mxx = std::clamp(mxx, 0, h - 1);
      mny = std::clamp(mny, 0, w - 1), mxy = std::clamp(mxy, 0, w - 1);
      if (mxx >= w || mxy >= h) fail(OCR_ERR_INVALID, "non-square map: box (%d,%d) leaves the %dx%d map (the reference would fail in narrow())", mxx, mxy, w, h);
      jobs.push_back(BoxScoreJob{images[k], pos, counts[k], mnx, mny, mxx - mnx + 1, mxy - mny + 1});
      box_out[4 * k] = mnx, box_out[4 * k + 1] = mny, box_out[4 * k + 2] = mxx - mnx + 1, box_out[4 * k + 3] = mxy - mny + 1;
      pos += counts[k];
    }
    for (int k = 0; k < slack; ++k) jobs.push_back(jobs[0]);
    const size_t slots = (size_t)n_polys + slack, map_bytes = (size_t)n * h * w * 4;
    for (size_t k = 0; k < slots; ++k) sums_out[k] = counts_out[k] = sentinel;
    if (slots == 0) return;
    Carve c;   // the maps first
    c.take(map_bytes);
    const size_t o_jobs = c.take(slots * sizeof(BoxScoreJob)), o_pts = c.take((size_t)pos * 8), o_sum = c.take(slots * 8), o_cnt = c.take(slots * 8),
                 o_n = c.take(4);
    char* sc = static_cast<char*>(det->impl.scratch(0, c.end));
    OCR_HIP(hipMemcpyAsync(sc, prob_host, map_bytes, hipMemcpyHostToDevice, s));
    OCR_HIP(hipMemcpyAsync(sc + o_jobs, jobs.data(), slots * sizeof(BoxScoreJob), hipMemcpyHostToDevice, s));
    OCR_HIP(hipMemcpyAsync(sc + o_pts, xy, (size_t)pos * 8, hipMemcpyHostToDevice, s));
    OCR_HIP(hipMemcpyAsync(sc + o_sum, sums_out, slots * 8, hipMemcpyHostToDevice, s));
    OCR_HIP(hipMemcpyAsync(sc + o_cnt, counts_out, slots * 8, hipMemcpyHostToDevice, s));
    OCR_HIP(hipMemcpyAsync(sc + o_n, &dev_count, 4, hipMemcpyHostToDevice, s));
    if (grid == 0)
      launch_box_scores(at<const float>(sc, 0), h, w, at<const BoxScoreJob>(sc, o_jobs), at<const int32_t>(sc, o_pts), n_polys, at<double>(sc, o_sum),
                        at<double>(sc, o_cnt), s);
    else
      launch_box_scores_counted(at<const float>(sc, 0), h, w, at<const BoxScoreJob>(sc, o_jobs), at<const int32_t>(sc, o_pts), at<const int>(sc, o_n), grid,
                                at<double>(sc, o_sum), at<double>(sc, o_cnt), s);
    OCR_HIP(hipMemcpyAsync(sums_out, sc + o_sum, slots * 8, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(counts_out, sc + o_cnt, slots * 8, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipStreamSynchronize(s));
  });
}
// one conv_igemm launch on caller data (kernel-level parity hook).  All host arrays are f32; with in_bf16 /
// out_bf16 they are rounded to bf16 (nearest even) on the way in and widened on the way out, so the caller
// compares against a reference computed from the SAME rounded operands.  in: NHWC; cat4: the four pyramid
// levels p5 (h/8), p4 (h/4), p3 (h/2), p2 (h) back to back, 64 channels each.  wgt: [cout][ks*ks][cin].
int ocr_test_conv_run(ocr_det_t* det, int in_bf16, int out_bf16, const float* in, int n, int h, int w, int cin,
                      const float* wgt, int cout, int ks, int stride, const float* scale, const float* bias,
                      const float* residual, const float* up_residual, int relu, int cat4, int variant, float* out, float* out2) {
  return guard([&] {
    using namespace ocr;
    if (!det || !in || !wgt) fail(OCR_ERR_INVALID, "null argument");
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    const int pad = (ks - 1) / 2;
    const int ho = (h + 2 * pad - ks) / stride + 1, wo = (w + 2 * pad - ks) / stride + 1;
    size_t lvl[4] = {0, 0, 0, 0};
    size_t in_e = (size_t)n * h * w * cin;
    if (cat4) {
      if (cin != 256 || (h % 8) || (w % 8)) fail(OCR_ERR_INVALID, "cat4 needs cin 256 and h, w multiples of 8");
      in_e = 0;
      for (int l = 0; l < 4; ++l) {
        lvl[l] = in_e;
        in_e += (size_t)n * (h >> (3 - l)) * (w >> (3 - l)) * 64;
      }
    }
    // variant: low byte = kernel form (0 conv_igemm, 1 conv3x3_bf16_c64, 2 split-bf16 128-wide tiles, 3 split-bf16 256 x 128 persistent form);
    // variant >> 8 = B > 1: a batched GEMM of B problems (1x1 s1; in [B][n h w][cin], wgt [B][cout][cin], out [B][n h w][cout])
    const int nbatch = variant >> 8 > 1 ? variant >> 8 : 1;
    variant &= 0xff;
    if (nbatch > 1 && (ks != 1 || stride != 1 || cat4 || residual || up_residual || out2)) fail(OCR_ERR_INVALID, "batched test GEMM: 1x1 s1, no residuals");
    in_e *= (size_t)nbatch;
    const size_t w_e = (size_t)nbatch * cout * ks * ks * cin, out_e = (size_t)nbatch * n * ho * wo * cout;
    const size_t up_e = (size_t)n * (ho / 2) * (wo / 2) * cout;
    auto bf16_bits = [](float f) {
      uint32_t u;
      std::memcpy(&u, &f, 4);
      if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
      return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    };
    std::vector<void*> allocs;
    auto up = [&](const float* src, size_t elems, bool bf) -> void* {
      if (!src) return nullptr;
      void* d = nullptr;
      OCR_HIP(hipMalloc(&d, elems * (bf ? 2 : 4)));
      allocs.push_back(d);
      if (bf) {
        std::vector<uint16_t> t(elems);
        for (size_t i = 0; i < elems; ++i) t[i] = bf16_bits(src[i]);
        OCR_HIP(hipMemcpy(d, t.data(), elems * 2, hipMemcpyHostToDevice));
      } else {
        OCR_HIP(hipMemcpy(d, src, elems * 4, hipMemcpyHostToDevice));
      }
      return d;
    };
    auto down = [&](float* dst, const void* dev, size_t elems, bool bf) {
      if (!dst) return;
      if (bf) {
        std::vector<uint16_t> t(elems);
        OCR_HIP(hipMemcpy(t.data(), dev, elems * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < elems; ++i) {
          const uint32_t u = (uint32_t)t[i] << 16;
          std::memcpy(&dst[i], &u, 4);
        }
      } else {
        OCR_HIP(hipMemcpy(dst, dev, elems * 4, hipMemcpyDeviceToHost));
      }
    };
    const size_t ies = in_bf16 ? 2 : 4, oes = out_bf16 ? 2 : 4;
    char* d_in = static_cast<char*>(up(in, in_e, in_bf16));
    ConvDesc d{};
    d.in_bf16 = in_bf16 ? 1 : 0;
    d.out_bf16 = out_bf16 ? 1 : 0;
    d.src_mode = cat4 ? SRC_CAT4 : SRC_PLAIN;
    d.src[0] = d_in;
    if (cat4) {
      for (int l = 0; l < 4; ++l) d.src[l] = d_in + lvl[l] * ies;
      d.src_base = d_in;
    }
    d.src_bytes = in_e * ies;
    d.wgt = up(wgt, w_e, in_bf16);
    d.wgt_bytes = w_e * ies;
    d.N = n; d.Hin = h; d.Win = w; d.Cin = cin; d.Ho = ho; d.Wo = wo; d.Cout = cout;
    d.ks = ks; d.stride = stride; d.pad = pad;
    d.scale = static_cast<const float*>(up(scale, cout, false));
    d.bias = static_cast<const float*>(up(bias, cout, false));
    d.residual = up(residual, out_e, out_bf16);
    d.up_residual = up(up_residual, up_e, out_bf16);
    d.relu = relu; d.store_mode = STORE_NHWC; d.name = "test_conv";
    d.batch = nbatch;
    void* d_out = nullptr;
    void* d_out2 = nullptr;
    if (out) { OCR_HIP(hipMalloc(&d_out, out_e * oes)); allocs.push_back(d_out); }
    if (out2) { OCR_HIP(hipMalloc(&d_out2, out_e * oes)); allocs.push_back(d_out2); }
    d.out = d_out;
    d.out2 = d_out2;
    struct Free { std::vector<void*>& v; ~Free() { for (void* p : v) (void)hipFree(p); } } free_all{allocs};
    if (variant == 1) {  // conv3x3_bf16_c64.hip instead of conv_igemm
      if (!in_bf16 || !out_bf16 || ks != 3 || stride != 1 || cin != 64 || cout != 64 || cat4 || out2 || !out)
        fail(OCR_ERR_INVALID, "variant 1 is the bf16 3x3 s1 64 -> 64 kernel");
      const std::vector<uint16_t> fr = conv3x3_bf16_c64_fragments(wgt);
      void* d_fr = nullptr;
      OCR_HIP(hipMalloc(&d_fr, fr.size() * 2));
      allocs.push_back(d_fr);
      OCR_HIP(hipMemcpy(d_fr, fr.data(), fr.size() * 2, hipMemcpyHostToDevice));
      launch_conv3x3_bf16_c64(d_in, d_fr, d.scale, d.bias, d.residual, relu, d_out, n, h, w, 256, s);
      OCR_HIP(hipStreamSynchronize(s));
      down(out, d_out, out_e, true);
      return;
    }
    if (variant == 2 || variant == 3) {  // the split-bf16 form of the f32 conv: weights as three bf16 planes; 3: the 256 x 128 persistent kernel
      if (variant == 3 && !conv_x3_wide_applicable([&] { ConvDesc t = d; t.x3 = 1; return t; }())) fail(OCR_ERR_INVALID, "variant 3: the wide split-bf16 form does not take this launch");
      if (in_bf16 || out_bf16 || cat4) fail(OCR_ERR_INVALID, "variant 2 (split bf16) takes f32 tensors");
      const std::vector<uint16_t> planes = split3_weights_tiled(wgt, w_e, ks * ks * cin);
      void* d_pl = nullptr;
      OCR_HIP(hipMalloc(&d_pl, planes.size() * 2));
      allocs.push_back(d_pl);
      OCR_HIP(hipMemcpy(d_pl, planes.data(), planes.size() * 2, hipMemcpyHostToDevice));
      d.x3 = 1;
      d.wgt = d_pl;
      d.wgt_bytes = planes.size() * 2;
    }
    launch_conv(d, variant == 3, det->impl.num_cus(), s);
    OCR_HIP(hipStreamSynchronize(s));
    down(out, d_out, out_e, out_bf16);
    down(out2, d_out2, out_e, out_bf16);
  });
}
// one BasicBlock 64 -> 64 of the bf16 precision on caller data (f32 arrays, rounded to bf16 on the way in, widened on the way out):
// fused != 0: basic_block_bf16_c64.hip, one launch (num_cus sizes its persistent grid, 0 = 256); fused == 0: the same block as two
// conv3x3_bf16_c64 launches.  x: NHWC, w1 / w2: [64][9][64]; iters > 1 repeats the block and returns the average time in ms
int ocr_test_bf16_basic_block(ocr_det_t* det, const float* x, int n, int h, int w, const float* w1, const float* scale1, const float* bias1,
                              const float* w2, const float* scale2, const float* bias2, int fused, int num_cus, int iters, float* out, float* ms_out) {
  return guard([&] {
    using namespace ocr;
    if (!det || !x || !w1 || !w2 || !out) fail(OCR_ERR_INVALID, "null argument");
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    const size_t e = (size_t)n * h * w * 64;
    auto bf16_bits = [](float f) {
      uint32_t u;
      std::memcpy(&u, &f, 4);
      if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
      return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    };
    std::vector<void*> allocs;
    struct Free { std::vector<void*>& v; ~Free() { for (void* p : v) (void)hipFree(p); } } free_all{allocs};
    auto dev = [&](const void* src, size_t bytes) -> void* {
      void* d = nullptr;
      OCR_HIP(hipMalloc(&d, bytes));
      allocs.push_back(d);
      if (src) OCR_HIP(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
      return d;
    };
    std::vector<uint16_t> xb(e);
    for (size_t i = 0; i < e; ++i) xb[i] = bf16_bits(x[i]);
    void* d_x = dev(xb.data(), e * 2);
    void* d_t = dev(nullptr, e * 2);
    void* d_y = dev(nullptr, e * 2);
    const std::vector<uint16_t> f1 = conv3x3_bf16_c64_fragments(w1), f2 = conv3x3_bf16_c64_fragments(w2);
    void* d_f1 = dev(f1.data(), f1.size() * 2);
    void* d_f2 = dev(f2.data(), f2.size() * 2);
    const float* d_s1 = scale1 ? static_cast<const float*>(dev(scale1, 256)) : nullptr;
    const float* d_b1 = bias1 ? static_cast<const float*>(dev(bias1, 256)) : nullptr;
    const float* d_s2 = scale2 ? static_cast<const float*>(dev(scale2, 256)) : nullptr;
    const float* d_b2 = bias2 ? static_cast<const float*>(dev(bias2, 256)) : nullptr;
    const int cus = num_cus > 0 ? num_cus : 256;
    auto run = [&] {
      if (fused) {
        launch_basic_block_bf16_c64(d_x, d_f1, d_s1, d_b1, d_f2, d_s2, d_b2, d_y, n, h, w, cus, s);
      } else {
        launch_conv3x3_bf16_c64(d_x, d_f1, d_s1, d_b1, nullptr, 1, d_t, n, h, w, cus, s);
        launch_conv3x3_bf16_c64(d_t, d_f2, d_s2, d_b2, d_x, 1, d_y, n, h, w, cus, s);
      }
    };
    run();
    OCR_HIP(hipStreamSynchronize(s));
    if (iters > 1) {
      hipEvent_t e0, e1;
      OCR_HIP(hipEventCreate(&e0));
      OCR_HIP(hipEventCreate(&e1));
      OCR_HIP(hipEventRecord(e0, s));
      for (int i = 0; i < iters; ++i) run();
      OCR_HIP(hipEventRecord(e1, s));
      OCR_HIP(hipEventSynchronize(e1));
      float ms = 0.f;
      OCR_HIP(hipEventElapsedTime(&ms, e0, e1));
      (void)hipEventDestroy(e0);
      (void)hipEventDestroy(e1);
      if (ms_out) *ms_out = ms / iters;
    }
    std::vector<uint16_t> yb(e);
    OCR_HIP(hipMemcpy(yb.data(), d_y, e * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < e; ++i) {
      const uint32_t u = (uint32_t)yb[i] << 16;
      std::memcpy(&out[i], &u, 4);
    }
  });
}
}  // extern "C"

// what the stem / head / recogniser hooks below share: host f32 -> bf16 bits (nearest even) and back, device buffers freed on every way out
namespace {
uint16_t hook_bf16_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
struct HookBuffers {
  std::vector<void*> allocs;
  ~HookBuffers() { for (void* p : allocs) (void)hipFree(p); }
  void* raw(const void* src, size_t bytes) {   // src == nullptr: zeroed
    void* d = nullptr;
    OCR_HIP(hipMalloc(&d, std::max<size_t>(bytes, 16)));
    allocs.push_back(d);
    if (src) OCR_HIP(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
    else OCR_HIP(hipMemset(d, 0, std::max<size_t>(bytes, 16)));
    return d;
  }
  // `bytes` of src inside one allocation with at least `lead` bytes (rounded up to whole 256) in front of them and behind them, every
  // 4-byte word of both leads = fill: what a kernel reads outside the source it was given is then in mapped memory and of a known value
  void* framed(const void* src, size_t bytes, size_t lead, uint32_t fill) {
    lead = (lead + 255) / 256 * 256;
    const size_t total = (lead + bytes + lead + 3) / 4 * 4;
    std::vector<uint8_t> t(total);
    for (size_t i = 0; i < total; i += 4) std::memcpy(&t[i], &fill, 4);
    std::memcpy(&t[lead], src, bytes);
    return static_cast<uint8_t*>(raw(t.data(), total)) + lead;
  }
  float* f32(const float* src, size_t elems) { return static_cast<float*>(raw(src, elems * 4)); }
  void* u16(const std::vector<uint16_t>& v) { return raw(v.data(), v.size() * 2); }
  void* as_bf16(const float* src, size_t elems) {
    std::vector<uint16_t> t(elems);
    for (size_t i = 0; i < elems; ++i) t[i] = hook_bf16_bits(src[i]);
    return u16(t);
  }
};
}  // namespace

extern "C" {

// The hooks below share two habits.  SOURCES sit inside one allocation between two leads (HookBuffers::framed) of zeros, or with
// poison = 1 of quiet NaN (u8 data: 255), or with poison = 2 of +inf (u8: 255): the sizes handed to the launcher state the real data only,
// so a read outside them - multiplied by a zero weight or not - shows as a changed bit.  OUTPUTS are *_io arrays with guard rows behind the
// result: uploaded before the launch and downloaded whole after it, so what the caller put into the guard comes back only if the kernel
// wrote nothing there.
static uint32_t hook_lead_fill(int poison, int elem_bytes) {
  if (!poison) return 0u;
  if (elem_bytes == 1) return 0xffffffffu;
  if (elem_bytes == 2) return poison == 2 ? 0x7f807f80u : 0x7fc07fc0u;
  return poison == 2 ? 0x7f800000u : 0x7fc00000u;
}
static void hook_check_poison(int poison, int guard) {
  if (poison < 0 || poison > 2 || guard < 0) ocr::fail(OCR_ERR_INVALID, "hook: poison is 0, 1 or 2 and the guard not negative");
}

// the stem alone (stem_tail.hip) on caller data: conv 7x7 s2 p3 (1 -> 64) * scale + bias, ReLU, max pool 3x3 s2 p1.  form 0 = launch_stem
// (exact f32), 1 = launch_stem_bf16 (bf16 precision; the output is widened to f32), 2 = launch_stem_x3 (split bf16).  x: n x h x w frames, f32
// or (x_is_u8) u8, framed by at least eight frame rows; w64x49: conv1.weight [64][7][7]; out_io: [n * h / 4 * w / 4 + guard_rows][64] f32 -
// form 1's output is bf16 on the device, guard included (out_io is rounded on the way up and widened on the way back)
int ocr_test_stem_run(ocr_det_t* det, int form, const void* x, int x_is_u8, int n, int h, int w, const float* w64x49, const float* scale64,
                      const float* bias64, int poison, float* out_io, int guard_rows) {
  return guard([&] {
    using namespace ocr;
    if (!det || !x || !w64x49 || !scale64 || !bias64 || !out_io) fail(OCR_ERR_INVALID, "null argument");
    if (form < 0 || form > 2 || n <= 0 || h <= 0 || w <= 0) fail(OCR_ERR_INVALID, "stem hook: bad form or shape");
    hook_check_poison(poison, guard_rows);
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    HookBuffers b;
    const size_t eb = x_is_u8 ? 1 : 4;
    const size_t in_e = (size_t)n * h * w, out_e = ((size_t)n * (h / 4) * (w / 4) + guard_rows) * 64;
    void* d_x = b.framed(x, in_e * eb, (size_t)8 * w * eb, hook_lead_fill(poison, (int)eb));
    const float* d_sc = b.f32(scale64, 64);
    const float* d_bi = b.f32(bias64, 64);
    void* d_out = form == 1 ? b.as_bf16(out_io, out_e) : b.f32(out_io, out_e);
    if (form == 0) {   // [64][49] -> [49][64], as the engine uploads it
      std::vector<float> t(49 * 64);
      for (int c = 0; c < 64; ++c)
        for (int k = 0; k < 49; ++k) t[k * 64 + c] = w64x49[c * 49 + k];
      launch_stem(d_x, x_is_u8, b.f32(t.data(), t.size()), d_sc, d_bi, d_out, 0, n, h, w, s);
    } else if (form == 1) {
      launch_stem_bf16(d_x, x_is_u8, b.u16(stem_bf16_fragments(w64x49)), d_sc, d_bi, d_out, n, h, w, s);
    } else {
      launch_stem_x3(d_x, x_is_u8, b.u16(stem_x3_fragments(w64x49)), d_sc, d_bi, static_cast<float*>(d_out), n, h, w, s);
    }
    OCR_HIP(hipStreamSynchronize(s));
    if (form == 1) {
      std::vector<uint16_t> t(out_e);
      OCR_HIP(hipMemcpy(t.data(), d_out, out_e * 2, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < out_e; ++i) {
        const uint32_t u = (uint32_t)t[i] << 16;
        std::memcpy(&out_io[i], &u, 4);
      }
    } else {
      OCR_HIP(hipMemcpy(out_io, d_out, out_e * 4, hipMemcpyDeviceToHost));
    }
  });
}
// the fused head alone (tail_fused.hip) on caller data: form = launch_tail_fused's `bf16` (0 f32 MFMA, 1 bf16 operands - y and wt1 are
// rounded on the way in -, 2 split bf16: wt1 as split3_weights planes).  y: [n][h4][w4][64], framed by at least 128 pixel rows (one
// workgroup's worth); wt1: [4 taps][64 co][64 ci]; s4 / b4: [256] (tap * 64 + co); w2t: [64 co][4]; prob_io: [n * 4 h4 + guard_rows][4 w4]
// f32, bitmap_io (optional) the same shape in u8
int ocr_test_head_run(ocr_det_t* det, int form, const float* y_nhwc, int n, int h4, int w4, const float* wt1, const float* s4, const float* b4,
                      const float* w2t, float bias2, float thresh, int poison, float* prob_io, uint8_t* bitmap_io_or_null, int guard_rows) {
  return guard([&] {
    using namespace ocr;
    if (!det || !y_nhwc || !wt1 || !s4 || !b4 || !w2t || !prob_io) fail(OCR_ERR_INVALID, "null argument");
    if (form < 0 || form > 2 || n <= 0 || h4 <= 0 || w4 <= 0) fail(OCR_ERR_INVALID, "head hook: bad form or shape");
    hook_check_poison(poison, guard_rows);
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    HookBuffers b;
    const size_t m = (size_t)n * h4 * w4, y_e = m * 64, w_e = (size_t)4 * 64 * 64, px = ((size_t)n * 4 * h4 + guard_rows) * 4 * w4;
    const void* d_y;
    if (form == 1) {
      std::vector<uint16_t> t(y_e);
      for (size_t i = 0; i < y_e; ++i) t[i] = hook_bf16_bits(y_nhwc[i]);
      d_y = b.framed(t.data(), y_e * 2, (size_t)128 * 64 * 2, hook_lead_fill(poison, 2));
    } else {
      d_y = b.framed(y_nhwc, y_e * 4, (size_t)128 * 64 * 4, hook_lead_fill(poison, 4));
    }
    const void* d_w = form == 1 ? b.as_bf16(wt1, w_e) : form == 2 ? b.u16(split3_weights(wt1, w_e)) : b.f32(wt1, w_e);
    float* d_prob = b.f32(prob_io, px);
    uint8_t* d_bm = bitmap_io_or_null ? static_cast<uint8_t*>(b.raw(bitmap_io_or_null, px)) : nullptr;
    launch_tail_fused(d_y, d_w, form, b.f32(s4, 256), b.f32(b4, 256), b.f32(w2t, 256), bias2, d_prob, d_bm, thresh, n, h4, w4, s);
    OCR_HIP(hipStreamSynchronize(s));
    OCR_HIP(hipMemcpy(prob_io, d_prob, px * 4, hipMemcpyDeviceToHost));
    if (d_bm) OCR_HIP(hipMemcpy(bitmap_io_or_null, d_bm, px, hipMemcpyDeviceToHost));
  });
}
// the two-kernel head's second half (stem_tail.hip's convt2_sigmoid_kernel) on caller data: convT 2x2 s2 (64 -> 1) + bias + sigmoid
// (+ binarize).  in: [n][H2][W2][64] f32, framed by at least 128 pixels; w4x64: [4 taps a * 2 + b][64]; prob_io: [n * 2 H2 + guard_rows][2 W2]
// f32, bitmap_io (optional) the same shape in u8
int ocr_test_convt2_sigmoid(ocr_det_t* det, const float* in, int n, int H2, int W2, const float* w4x64, float bias, float thresh, int poison,
                            float* prob_io, uint8_t* bitmap_io_or_null, int guard_rows) {
  return guard([&] {
    using namespace ocr;
    if (!det || !in || !w4x64 || !prob_io) fail(OCR_ERR_INVALID, "null argument");
    if (n <= 0 || H2 <= 0 || W2 <= 0) fail(OCR_ERR_INVALID, "convt2 hook: bad shape");
    hook_check_poison(poison, guard_rows);
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    HookBuffers b;
    const size_t in_e = (size_t)n * H2 * W2 * 64, px = ((size_t)n * 2 * H2 + guard_rows) * 2 * W2;
    const float* d_in = static_cast<const float*>(b.framed(in, in_e * 4, (size_t)128 * 64 * 4, hook_lead_fill(poison, 4)));
    float* d_prob = b.f32(prob_io, px);
    uint8_t* d_bm = bitmap_io_or_null ? static_cast<uint8_t*>(b.raw(bitmap_io_or_null, px)) : nullptr;
    launch_convt2_sigmoid(d_in, b.f32(w4x64, 256), bias, d_prob, d_bm, thresh, n, H2, W2, s);
    OCR_HIP(hipStreamSynchronize(s));
    OCR_HIP(hipMemcpy(prob_io, d_prob, px * 4, hipMemcpyDeviceToHost));
    if (d_bm) OCR_HIP(hipMemcpy(bitmap_io_or_null, d_bm, px, hipMemcpyDeviceToHost));
  });
}
// launch_binarize on caller data: prob [n] f32, framed by at least 4096 floats; bitmap_io: [n + guard_elems] u8
int ocr_test_binarize(ocr_det_t* det, const float* prob, size_t n, float thresh, int poison, uint8_t* bitmap_io, int guard_elems) {
  return guard([&] {
    using namespace ocr;
    if (!det || !prob || !bitmap_io) fail(OCR_ERR_INVALID, "null argument");
    if (n == 0) fail(OCR_ERR_INVALID, "binarize hook: no pixels");
    hook_check_poison(poison, guard_elems);
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    HookBuffers b;
    const float* d_prob = static_cast<const float*>(b.framed(prob, n * 4, (size_t)4096 * 4, hook_lead_fill(poison, 4)));
    uint8_t* d_bm = static_cast<uint8_t*>(b.raw(bitmap_io, n + guard_elems));
    launch_binarize(d_prob, d_bm, thresh, n, s);
    OCR_HIP(hipStreamSynchronize(s));
    OCR_HIP(hipMemcpy(bitmap_io, d_bm, n + guard_elems, hipMemcpyDeviceToHost));
  });
}
// launch_binarize_pack on caller data: prob [n_images][px_per_image] f32, framed by at least 4096 floats; words_io: [n_images *
// binarize_pack_words(px_per_image) + guard_words] 32-bit words
int ocr_test_binarize_pack(ocr_det_t* det, const float* prob, int n_images, size_t px_per_image, float thresh, int poison, uint32_t* words_io,
                           int guard_words) {
  return guard([&] {
    using namespace ocr;
    if (!det || !prob || !words_io) fail(OCR_ERR_INVALID, "null argument");
    if (n_images <= 0 || px_per_image == 0) fail(OCR_ERR_INVALID, "binarize_pack hook: no pixels");
    hook_check_poison(poison, guard_words);
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    HookBuffers b;
    const size_t words = (size_t)n_images * binarize_pack_words(px_per_image) + guard_words;
    const float* d_prob =
        static_cast<const float*>(b.framed(prob, (size_t)n_images * px_per_image * 4, (size_t)4096 * 4, hook_lead_fill(poison, 4)));
    uint32_t* d_w = static_cast<uint32_t*>(b.raw(words_io, words * 4));
    launch_binarize_pack(d_prob, d_w, thresh, n_images, px_per_image, s);
    OCR_HIP(hipStreamSynchronize(s));
    OCR_HIP(hipMemcpy(words_io, d_w, words * 4, hipMemcpyDeviceToHost));
  });
}
// conv1 + pool + conv2 + pool of the recogniser (rec_net.hip) on caller weights: form 0 = launch_rec_conv (exact f32; crops_per_block 0 =
// chosen by n as shipped, 1 / 2 / 4 = that instantiation of rec_conv_kernel), 1 = launch_rec_small stage 0 (split-bf16 conv2;
// crops_per_block must be 0).  crops: [n][784], framed by at least four crops; w1: [32][25]; w2: [64][32][25].  feat_io: rows of 1024 as
// k = co * 16 + p in both forms.  Form 0: n + guard_rows rows.  Form 1: 16 (ceil(n / 16) + max(1, ceil(guard_rows / 16))) rows - the kernel
// writes the operand order of the fc1 kernel, whole 16-crop tiles: the hook permutes every row on the way up and back, so the pad rows
// of the last tile and the tiles behind it reach the caller as well
int ocr_test_rec_features(ocr_rec_t* rec, int form, int crops_per_block, const float* crops, int n, const float* w1, const float* b1,
                          const float* w2, const float* b2, int poison, float* feat_io, int guard_rows) {
  return guard([&] {
    using namespace ocr;
    if (!rec || !crops || !w1 || !b1 || !w2 || !b2 || !feat_io) fail(OCR_ERR_INVALID, "null argument");
    if (form < 0 || form > 1 || n <= 0) fail(OCR_ERR_INVALID, "rec hook: bad form or batch");
    if (form == 1 && crops_per_block != 0) fail(OCR_ERR_INVALID, "rec hook: crops_per_block belongs to form 0");
    hook_check_poison(poison, guard_rows);
    OCR_HIP(hipSetDevice(rec->impl.device()));
    hipStream_t s = rec->impl.stream();
    HookBuffers b;
    RecWeights rw{};
    rw.c1f = b.f32(rec_conv1_fragments(w1).data(), 13 * 64);
    rw.c1b = b.f32(b1, 32);
    rw.c2b = b.f32(b2, 64);
    const float* d_crops = static_cast<const float*>(b.framed(crops, (size_t)n * 784 * 4, (size_t)4 * 784 * 4, hook_lead_fill(poison, 4)));
    if (form == 0) {
      const size_t e = ((size_t)n + guard_rows) * 1024;
      float* d_feat = b.f32(feat_io, e);
      const std::vector<float> f2 = rec_conv2_fragments(w2);
      rw.c2f = b.f32(f2.data(), f2.size());
      launch_rec_conv(rw, d_crops, n, d_feat, s, crops_per_block);
      OCR_HIP(hipStreamSynchronize(s));
      OCR_HIP(hipMemcpy(feat_io, d_feat, e * 4, hipMemcpyDeviceToHost));
      return;
    }
    // operand order [tile of 16 crops][g: sixteen k][q][r: crop of the tile][e] holds k = 16 g + 4 q + e of crop 16 tile + r
    const size_t tiles = ((size_t)n + 15) / 16 + std::max<size_t>(1, ((size_t)guard_rows + 15) / 16);
    std::vector<float> t(tiles * 16 * 1024);
    auto permute = [&](bool up) {
      for (size_t tile = 0; tile < tiles; ++tile)
        for (int g = 0; g < 64; ++g)
          for (int q = 0; q < 4; ++q)
            for (int r = 0; r < 16; ++r)
              for (int e = 0; e < 4; ++e) {
                float& dev = t[((((tile * 64 + g) * 4 + q) * 16 + r) * 4) + e];
                float& host = feat_io[(tile * 16 + r) * 1024 + 16 * g + 4 * q + e];
                if (up) dev = host;
                else host = dev;
              }
    };
    permute(true);
    float* d_feat = b.f32(t.data(), t.size());
    rw.c2x = b.u16(rec_conv2_small_x3_fragments(w2));
    launch_rec_small(rw, d_crops, n, d_feat, nullptr, nullptr, nullptr, nullptr, s, 0);
    OCR_HIP(hipStreamSynchronize(s));
    OCR_HIP(hipMemcpy(t.data(), d_feat, t.size() * 4, hipMemcpyDeviceToHost));
    permute(false);
  });
}

// fc1 + bias + ReLU of the recogniser on caller weights: form 0 = launch_rec_fc1 (the large-batch conv_igemm GEMM, w uploaded as is), 1 =
// launch_rec_small stage 1 (rec_fc1_ksplit_kernel: w through rec_fc1_small_weights, feat permuted into the operand order [tile][g][q][r][e]).
// feat: [n][1024]; w: [512][1024]; bias: [512].  Rows the kernel may read but must not use - form 1: the rows n .. 16 ceil(n / 16) - 1 of the last
// tile; form 0: 16 rows behind the n real ones in the same allocation, past the src_bytes = n * 4096 the launcher states - are zero, or with
// poison != 0 quiet NaN.  hid_io: [n + guard_rows][512], uploaded before the launch and downloaded whole after it: what the caller put into
// rows n .. n + guard_rows - 1 comes back only if the kernel wrote nothing there
int ocr_test_rec_fc1(ocr_rec_t* rec, int form, const float* feat, int n, const float* w, const float* bias, int poison, float* hid_io, int guard_rows) {
  return guard([&] {
    using namespace ocr;
    if (!rec || !feat || !w || !bias || !hid_io) fail(OCR_ERR_INVALID, "null argument");
    if (form < 0 || form > 1 || n <= 0 || guard_rows < 0) fail(OCR_ERR_INVALID, "rec fc1 hook: bad form, batch or guard");
    OCR_HIP(hipSetDevice(rec->impl.device()));
    hipStream_t s = rec->impl.stream();
    HookBuffers b;
    RecWeights rw{};
    rw.f1b = b.f32(bias, 512);
    const float pad = poison ? std::numeric_limits<float>::quiet_NaN() : 0.f;
    const size_t hid_e = ((size_t)n + guard_rows) * 512;
    float* d_hid = b.f32(hid_io, hid_e);
    if (form == 0) {
      std::vector<float> t(((size_t)n + 16) * 1024, pad);
      std::copy(feat, feat + (size_t)n * 1024, t.begin());
      rw.f1w = b.f32(w, (size_t)512 * 1024);
      launch_rec_fc1(rw, b.f32(t.data(), t.size()), n, d_hid, s);
    } else {
      const size_t tiles = ((size_t)n + 15) / 16;
      std::vector<float> t(tiles * 16 * 1024);
      for (size_t tile = 0; tile < tiles; ++tile)
        for (int g = 0; g < 64; ++g)
          for (int q = 0; q < 4; ++q)
            for (int r = 0; r < 16; ++r)
              for (int e = 0; e < 4; ++e) {
                const size_t crop = tile * 16 + r;
                t[((((tile * 64 + g) * 4 + q) * 16 + r) * 4) + e] = crop < (size_t)n ? feat[crop * 1024 + 16 * g + 4 * q + e] : pad;
              }
      const std::vector<float> ws = rec_fc1_small_weights(w);
      rw.f1s = b.f32(ws.data(), ws.size());
      launch_rec_small(rw, nullptr, n, b.f32(t.data(), t.size()), d_hid, nullptr, nullptr, nullptr, s, 1);
    }
    OCR_HIP(hipStreamSynchronize(s));
    OCR_HIP(hipMemcpy(hid_io, d_hid, hid_e * 4, hipMemcpyDeviceToHost));
  });
}
// fc2 + bias + softmax(f64) + top-1 of the recogniser on caller weights: form 0 = launch_rec_fc2_softmax (w through rec_fc2_fragments), 1 =
// launch_rec_small stage 2 (rec_fc2_small_kernel, w through rec_fc2_small_fragments).  hid: [n][512]; w: [62][512]; bias: [62], padded to 64
// with zeros as the Recognizer does.  logits_io [n + guard_rows][62] f32, labels_io [n + guard_rows] i32, probs_io [n + guard_rows] f64: each
// optional (null goes to the launcher as null), uploaded before the launch and downloaded whole after it
int ocr_test_rec_fc2(ocr_rec_t* rec, int form, const float* hid, int n, const float* w, const float* bias, float* logits_io, int32_t* labels_io,
                     double* probs_io, int guard_rows) {
  return guard([&] {
    using namespace ocr;
    if (!rec || !hid || !w || !bias) fail(OCR_ERR_INVALID, "null argument");
    if (form < 0 || form > 1 || n <= 0 || guard_rows < 0) fail(OCR_ERR_INVALID, "rec fc2 hook: bad form, batch or guard");
    OCR_HIP(hipSetDevice(rec->impl.device()));
    hipStream_t s = rec->impl.stream();
    HookBuffers b;
    RecWeights rw{};
    std::vector<float> b2(bias, bias + 62);
    b2.resize(64, 0.f);
    rw.f2b = b.f32(b2.data(), 64);
    const float* d_hid = b.f32(hid, (size_t)n * 512);
    const size_t rows = (size_t)n + guard_rows;
    float* d_lg = logits_io ? b.f32(logits_io, rows * 62) : nullptr;
    int32_t* d_lab = labels_io ? static_cast<int32_t*>(b.raw(labels_io, rows * 4)) : nullptr;
    double* d_pr = probs_io ? static_cast<double*>(b.raw(probs_io, rows * 8)) : nullptr;
    if (form == 0) {
      const std::vector<float> f = rec_fc2_fragments(w);
      rw.f2f = b.f32(f.data(), f.size());
      launch_rec_fc2_softmax(rw, d_hid, n, d_lg, d_lab, d_pr, s);
    } else {
      const std::vector<float> f = rec_fc2_small_fragments(w);
      rw.f2s = b.f32(f.data(), f.size());
      launch_rec_small(rw, nullptr, n, nullptr, const_cast<float*>(d_hid), d_lg, d_lab, d_pr, s, 2);
    }
    OCR_HIP(hipStreamSynchronize(s));
    if (d_lg) OCR_HIP(hipMemcpy(logits_io, d_lg, rows * 62 * 4, hipMemcpyDeviceToHost));
    if (d_lab) OCR_HIP(hipMemcpy(labels_io, d_lab, rows * 4, hipMemcpyDeviceToHost));
    if (d_pr) OCR_HIP(hipMemcpy(probs_io, d_pr, rows * 8, hipMemcpyDeviceToHost));
  });
}

// one 3x3 s1 p1 conv (+ scale / bias / residual / ReLU) through the Winograd F(2x2,3x3) path on caller data:
// weight transform, input transform, batched 16-problem GEMM, output transform.  x: NHWC, wgt: [cout][9][cin].
int ocr_test_winograd_conv(ocr_det_t* det, const float* x, int n, int h, int w, int cin, const float* wgt, int cout,
                           const float* scale, const float* bias, const float* residual, int relu, int unfused_and_cus, float* out) {
  return guard([&] {
    int unfused = unfused_and_cus;
    using namespace ocr;
    if (!det || !x || !wgt || !out) fail(OCR_ERR_INVALID, "null argument");
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    const int num_cus = unfused >> 8;   // optional, for the fused kernel's grid
    unfused &= 0xff;
    const size_t wm = unfused >= 3 ? 4 : 2, wa = (wm + 2) * (wm + 2);   // unfused: 1 = F(2x2,3x3), 3 = F(4x4,3x3), both unfused; 4 = the fused F(4x4,3x3) kernel
    const size_t th = (h + wm - 1) / wm, tw = (w + wm - 1) / wm, T = (size_t)n * th * tw;
    const size_t in_e = (size_t)n * h * w * cin, out_e = (size_t)n * h * w * cout;
    const std::vector<float> u = winograd_weights(wgt, cout, cin, (int)wm);
    std::vector<void*> allocs;
    struct Free { std::vector<void*>& v; ~Free() { for (void* p : v) (void)hipFree(p); } } free_all{allocs};
    auto dev = [&](const float* src, size_t elems) -> float* {
      void* d = nullptr;
      OCR_HIP(hipMalloc(&d, elems * 4));
      allocs.push_back(d);
      if (src) OCR_HIP(hipMemcpy(d, src, elems * 4, hipMemcpyHostToDevice));
      return static_cast<float*>(d);
    };
    float* d_x = dev(x, in_e);
    float* d_u = dev(u.data(), u.size());
    float* d_v = dev(nullptr, wa * T * cin);
    float* d_m = dev(nullptr, wa * T * cout);
    float* d_y = dev(nullptr, out_e);
    const float* d_sc = scale ? dev(scale, cout) : nullptr;
    const float* d_bi = bias ? dev(bias, cout) : nullptr;
    const float* d_res = residual ? dev(residual, out_e) : nullptr;
    if (unfused == 5) {  // fused F(4x4,3x3) on the bf16 matrix cores (split-bf16); one workgroup per CU
      const std::vector<uint16_t> uf = winograd43_x3_fragments(u, cout, cin);
      void* d_uf = nullptr;
      OCR_HIP(hipMalloc(&d_uf, uf.size() * 2));
      allocs.push_back(d_uf);
      OCR_HIP(hipMemcpy(d_uf, uf.data(), uf.size() * 2, hipMemcpyHostToDevice));
      launch_winograd43_x3(d_x, d_uf, d_sc, d_bi, d_res, relu, d_y, n, h, w, cin, cout, num_cus > 0 ? num_cus : 256, s);
      OCR_HIP(hipStreamSynchronize(s));
      OCR_HIP(hipMemcpy(out, d_y, out_e * 4, hipMemcpyDeviceToHost));
      return;
    }
    if (unfused == 4) {  // fused F(4x4,3x3); num_cus sizes its persistent grid (two workgroups per CU)
      float* d_uf = dev(winograd43_fragments(u, cout, cin).data(), u.size());
      launch_winograd43_fused(d_x, d_uf, d_sc, d_bi, d_res, relu, d_y, n, h, w, cin, cout, num_cus > 0 ? num_cus : 256, s);
      OCR_HIP(hipStreamSynchronize(s));
      OCR_HIP(hipMemcpy(out, d_y, out_e * 4, hipMemcpyDeviceToHost));
      return;
    }
    launch_winograd_input(d_x, d_v, n, h, w, cin, (int)wm, s);
    ConvDesc d{};
    d.src[0] = d_v;
    d.src_mode = SRC_PLAIN;
    d.src_bytes = wa * T * cin * 4;
    d.wgt = d_u;
    d.wgt_bytes = u.size() * 4;
    d.batch = (int)wa;
    d.N = 1; d.Hin = d.Ho = 1; d.Win = d.Wo = (int)T; d.Cin = cin; d.Cout = cout;
    d.ks = 1; d.stride = 1; d.pad = 0; d.store_mode = STORE_NHWC; d.out = d_m; d.name = "test_winograd";
    launch_conv_igemm(d, s);
    launch_winograd_output(d_m, d_sc, d_bi, d_res, relu, d_y, n, h, w, cout, (int)wm, s);
    OCR_HIP(hipStreamSynchronize(s));
    OCR_HIP(hipMemcpy(out, d_y, out_e * 4, hipMemcpyDeviceToHost));
  });
}

// Two kernels of complementary families on two streams (tuning aid): A = the fused F(4x4,3x3) kernel (f32 MFMA)
// on n x 160 x 160 x 64 with its persistent grid sized for `w43_cus` CUs (two workgroups each; 128 -> one workgroup per CU), B = one
// split-bf16 conv_igemm launch (which_b: 0 = 3x3 s2 64 -> 128 from 160 x 160, 1 = 3x3 s2 128 -> 256 from 80 x 80, 2 = the 36 batched
// Winograd GEMMs of layer3, 3 = 3x3 s2 256 -> 512 from 40 x 40).  ms_out: [0] A alone (per launch), [1] B alone (per launch), [2] wall
// time of reps_a launches of A on one stream beside reps_b launches of B on another, [3] the same 2 queues on ONE stream.
int ocr_test_dual_stream_bench(ocr_det_t* det, int n, int which_b, int w43_cus, int reps_a, int reps_b, float* ms_out) {
  return guard([&] {
    using namespace ocr;
    if (!det || !ms_out) fail(OCR_ERR_INVALID, "null argument");
    OCR_HIP(hipSetDevice(det->impl.device()));
    std::vector<void*> allocs;
    struct Free { std::vector<void*>& v; ~Free() { for (void* p : v) (void)hipFree(p); } } free_all{allocs};
    uint32_t st = 4242u;
    auto rnd = [&] { st = st * 1664525u + 1013904223u; return ((st >> 8) & 0xffff) / 32768.0f - 1.0f; };
    auto dev_rand = [&](size_t elems, float amp) -> float* {
      std::vector<float> hbuf(elems);
      for (auto& v : hbuf) v = amp * rnd();
      void* d = nullptr;
      OCR_HIP(hipMalloc(&d, elems * 4));
      allocs.push_back(d);
      OCR_HIP(hipMemcpy(d, hbuf.data(), elems * 4, hipMemcpyHostToDevice));
      return static_cast<float*>(d);
    };
    auto dev_bytes = [&](const void* src, size_t bytes) -> void* {
      void* d = nullptr;
      OCR_HIP(hipMalloc(&d, bytes));
      allocs.push_back(d);
      if (src) OCR_HIP(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
      return d;
    };
    // A
    const int ha = 160, wa = 160, ca = 64;
    float* ax = dev_rand((size_t)n * ha * wa * ca, 1.0f);
    float* ay = static_cast<float*>(dev_bytes(nullptr, (size_t)n * ha * wa * ca * 4));
    std::vector<float> wg((size_t)ca * 9 * ca);
    for (auto& v : wg) v = 0.05f * rnd();
    const std::vector<float> ufr = winograd43_fragments(winograd_weights(wg.data(), ca, ca, 4), ca, ca);
    float* auf = static_cast<float*>(dev_bytes(ufr.data(), ufr.size() * 4));
    // B
    ConvDesc d{};
    d.x3 = 1;
    d.src_mode = SRC_PLAIN;
    d.store_mode = STORE_NHWC;
    d.relu = 1;
    d.name = "dual";
    size_t in_e, w_e, out_e;
    if (which_b == 2) {
      const size_t T = (size_t)n * 10 * 10;
      in_e = 36 * T * 256; w_e = (size_t)36 * 256 * 256; out_e = 36 * T * 256;
      d.batch = 36; d.N = 1; d.Hin = d.Ho = 1; d.Win = d.Wo = (int)T; d.Cin = 256; d.Cout = 256; d.ks = 1; d.stride = 1; d.pad = 0;
    } else {
      const int hb = which_b == 0 ? 160 : which_b == 1 ? 80 : 40, cb = which_b == 0 ? 64 : which_b == 1 ? 128 : 256;
      in_e = (size_t)n * hb * hb * cb; w_e = (size_t)2 * cb * 9 * cb; out_e = (size_t)n * (hb / 2) * (hb / 2) * 2 * cb;
      d.N = n; d.Hin = d.Win = hb; d.Ho = d.Wo = hb / 2; d.Cin = cb; d.Cout = 2 * cb; d.ks = 3; d.stride = 2; d.pad = 1;
    }
    d.src[0] = dev_rand(in_e, 1.0f);
    d.src_bytes = in_e * 4;
    std::vector<float> hw(w_e);
    for (auto& v : hw) v = 0.05f * rnd();
    const std::vector<uint16_t> planes = split3_weights_tiled(hw.data(), w_e, d.ks * d.ks * d.Cin);
    d.wgt = dev_bytes(planes.data(), planes.size() * 2);
    d.wgt_bytes = w_e * 6;
    d.out = dev_bytes(nullptr, out_e * 4);
    hipStream_t sa, sb;
    OCR_HIP(hipStreamCreateWithFlags(&sa, hipStreamNonBlocking));
    OCR_HIP(hipStreamCreateWithFlags(&sb, hipStreamNonBlocking));
    hipEvent_t e0, e1, e2;
    OCR_HIP(hipEventCreate(&e0));
    OCR_HIP(hipEventCreate(&e1));
    OCR_HIP(hipEventCreate(&e2));
    auto run_a = [&](hipStream_t s) { launch_winograd43_fused(ax, auf, nullptr, nullptr, nullptr, 1, ay, n, ha, wa, ca, ca, w43_cus, s); };
    auto run_b = [&](hipStream_t s) { launch_conv_igemm(d, s); };
    float ms = 0.f;
    for (int i = 0; i < 3; ++i) { run_a(sa); run_b(sa); }
    OCR_HIP(hipEventRecord(e0, sa));
    for (int i = 0; i < reps_a; ++i) run_a(sa);
    OCR_HIP(hipEventRecord(e1, sa));
    for (int i = 0; i < reps_b; ++i) run_b(sa);
    OCR_HIP(hipEventRecord(e2, sa));
    OCR_HIP(hipStreamSynchronize(sa));
    OCR_HIP(hipEventElapsedTime(&ms, e0, e1));
    ms_out[0] = ms / reps_a;
    OCR_HIP(hipEventElapsedTime(&ms, e1, e2));
    ms_out[1] = ms / reps_b;
    OCR_HIP(hipEventElapsedTime(&ms, e0, e2));
    ms_out[3] = ms;
    // together: both streams start behind e0, the end is when both have drained
    OCR_HIP(hipEventRecord(e0, sa));
    OCR_HIP(hipStreamWaitEvent(sb, e0, 0));
    for (int i = 0; i < std::max(reps_a, reps_b); ++i) {   // interleaved submission
      if (i < reps_a) run_a(sa);
      if (i < reps_b) run_b(sb);
    }
    OCR_HIP(hipEventRecord(e1, sb));
    OCR_HIP(hipStreamWaitEvent(sa, e1, 0));
    OCR_HIP(hipEventRecord(e2, sa));
    OCR_HIP(hipStreamSynchronize(sa));
    OCR_HIP(hipEventElapsedTime(&ms, e0, e2));
    ms_out[2] = ms;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(e2);
    (void)hipStreamDestroy(sa); (void)hipStreamDestroy(sb);
  });
}

// unclip.hip against postproc_geom.cpp::finish_polygon on caller polygons (one image, given scores): every polygon the device settles
// (UNCLIP_KEEP / UNCLIP_DROP) must be what the host does with it; counts how many it hands back (UNCLIP_HOST).  stats: keep, host, drop, mismatches.
int ocr_test_unclip_compare(ocr_det_t* det, const int32_t* xy, const int32_t* counts, int n_polys, const double* scores, double adj_x,
                            double adj_y, double box_thresh, double unclip_ratio, double min_size, int32_t* stats, int32_t* status_out,
                            int32_t* len_out, uint32_t* xy_out) {   // the three optional: per polygon status, length, and 3 x its input points of (x, y) room
  return guard([&] {
    using namespace ocr;
    if (!det || !xy || !counts || !scores || !stats || n_polys <= 0) fail(OCR_ERR_INVALID, "bad argument");
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    std::vector<BoxScoreJob> jobs(n_polys);
    std::vector<double> sums(scores, scores + n_polys), cnts(n_polys, 1.0);
    size_t npts = 0;
    for (int k = 0; k < n_polys; ++k) {
      jobs[k] = BoxScoreJob{0, (int)npts, counts[k], 0, 0, 1, 1};
      npts += (size_t)counts[k];
    }
    std::vector<void*> allocs;
    struct Free { std::vector<void*>& v; ~Free() { for (void* p : v) (void)hipFree(p); } } free_all{allocs};
    auto dev = [&](const void* src, size_t bytes) -> void* {
      void* d = nullptr;
      OCR_HIP(hipMalloc(&d, std::max<size_t>(bytes, 16)));
      allocs.push_back(d);
      if (src) OCR_HIP(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
      return d;
    };
    const double adj[2] = {adj_x, adj_y};
    auto* d_jobs = static_cast<BoxScoreJob*>(dev(jobs.data(), jobs.size() * sizeof(BoxScoreJob)));
    auto* d_pts = static_cast<int32_t*>(dev(xy, npts * 8));
    auto* d_sum = static_cast<double*>(dev(sums.data(), sums.size() * 8));
    auto* d_cnt = static_cast<double*>(dev(cnts.data(), cnts.size() * 8));
    auto* d_adj = static_cast<double*>(dev(adj, 16));
    void* d_work = dev(nullptr, unclip_work_bytes(npts, n_polys));
    auto* d_oxy = static_cast<uint32_t*>(dev(nullptr, 3 * npts * 8));
    auto* d_len = static_cast<int32_t*>(dev(nullptr, (size_t)n_polys * 4));
    auto* d_st = static_cast<int32_t*>(dev(nullptr, (size_t)n_polys * 4));
    const UnclipParams up{box_thresh, unclip_ratio, min_size};
    launch_unclip(d_jobs, d_pts, nullptr, n_polys, npts, d_sum, d_cnt, d_adj, up, d_work, d_oxy, d_len, d_st, s);
    OCR_HIP(hipStreamSynchronize(s));
    std::vector<int32_t> st(n_polys), len(n_polys);
    std::vector<uint32_t> oxy(3 * npts * 2);
    OCR_HIP(hipMemcpy(st.data(), d_st, st.size() * 4, hipMemcpyDeviceToHost));
    OCR_HIP(hipMemcpy(len.data(), d_len, len.size() * 4, hipMemcpyDeviceToHost));
    OCR_HIP(hipMemcpy(oxy.data(), d_oxy, oxy.size() * 4, hipMemcpyDeviceToHost));
    ocr_postproc_params_t prm{};
    ocr_postproc_default_params(&prm);
    prm.box_thresh = box_thresh;
    prm.unclip_ratio = unclip_ratio;
    prm.min_size = min_size;
    prm.skip_degenerate = 1;
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (status_out) std::copy(st.begin(), st.end(), status_out);
    if (len_out) std::copy(len.begin(), len.end(), len_out);
    if (xy_out) std::copy(oxy.begin(), oxy.end(), xy_out);
    for (int k = 0; k < n_polys; ++k) {
      std::vector<geom::Pt> c((size_t)counts[k]);
      for (int i = 0; i < counts[k]; ++i) c[i] = {xy[2 * (jobs[k].pt_offset + i)], xy[2 * (jobs[k].pt_offset + i) + 1]};
      std::vector<uint32_t> hxy;
      const bool kept = geom::finish_polygon(c, scores[k], adj_x, adj_y, prm, hxy);
      if (st[k] == UNCLIP_KEEP) {
        ++stats[0];
        const uint32_t* o = oxy.data() + 6 * (size_t)jobs[k].pt_offset;
        if (!kept || hxy.size() != 2 * (size_t)len[k] || !std::equal(hxy.begin(), hxy.end(), o)) ++stats[3];
      } else if (st[k] == UNCLIP_HOST) {
        ++stats[1];
      } else {
        ++stats[2];
        if (kept || !(box_thresh > scores[k])) ++stats[3];
      }
    }
  });
}
// no GPU: the device code's restatement of glibc's hypot against std::hypot on all integer pairs up to `limit`
long long ocr_test_hypot_port_mismatches(int limit) { return ocr::geom::hypot_port_mismatches(limit); }
int ocr_test_set_conv_debug(int d) {
  ocr::set_conv_debug(d);
  return OCR_OK;
}
int ocr_test_set_conv_tile(int t) {
  ocr::set_conv_tile_override(t);
  return OCR_OK;
}
// micro-benchmark of one conv_igemm launch shape on constant data (kernel tuning aid)
int ocr_test_conv_bench(ocr_det_t* det, int n, int h, int w, int cin, int cout, int ks, int stride, int src_mode,
                        int iters, float* ms_out) {
  return guard([&] {
    using namespace ocr;
    if (!det) fail(OCR_ERR_INVALID, "null handle");
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    const int pad = (ks - 1) / 2;
    const int ho = (h + 2 * pad - ks) / stride + 1, wo = (w + 2 * pad - ks) / stride + 1;
    const size_t in_e = (size_t)n * h * w * cin, w_e = (size_t)cout * ks * ks * cin, out_e = (size_t)n * ho * wo * cout;
    float *in = nullptr, *wt = nullptr, *out = nullptr;
    OCR_HIP(hipMalloc(reinterpret_cast<void**>(&in), in_e * 4));
    OCR_HIP(hipMalloc(reinterpret_cast<void**>(&wt), w_e * 4));
    OCR_HIP(hipMalloc(reinterpret_cast<void**>(&out), out_e * 4));
    OCR_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(in), 0x3f8ccccd, in_e, s));   // 1.1f
    OCR_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(wt), 0x3c23d70a, w_e, s));    // 0.01f
    if (src_mode & 32) {  // random operands: MFMA power (and with it the clock) depends on the data
      src_mode &= ~32;
      std::vector<float> h(std::max(in_e, w_e));
      uint32_t st = 12345u;
      auto rnd = [&] { st = st * 1664525u + 1013904223u; return ((st >> 8) & 0xffff) / 32768.0f - 1.0f; };
      for (size_t i = 0; i < in_e; ++i) h[i] = rnd();
      OCR_HIP(hipMemcpy(in, h.data(), in_e * 4, hipMemcpyHostToDevice));
      for (size_t i = 0; i < w_e; ++i) h[i] = 0.05f * rnd();
      OCR_HIP(hipMemcpy(wt, h.data(), w_e * 4, hipMemcpyHostToDevice));
    }
    const int x3 = (src_mode & 64) ? 1 : 0;  // split-bf16 form: the weight buffer is reinterpreted as three bf16 planes
    src_mode &= ~64;
    const int wide = (src_mode & 128) ? 1 : 0;  // ... on the 256 x 128 persistent form (conv_x3w.hip) where it takes the launch
    src_mode &= ~128;
    if (x3) {
      (void)hipFree(wt);
      OCR_HIP(hipMalloc(reinterpret_cast<void**>(&wt), w_e * 6));
      std::vector<float> hw(w_e);
      uint32_t st = 777u;
      for (size_t i = 0; i < w_e; ++i) { st = st * 1664525u + 1013904223u; hw[i] = 0.05f * (((st >> 8) & 0xffff) / 32768.0f - 1.0f); }
      const std::vector<uint16_t> planes = split3_weights_tiled(hw.data(), w_e, ks * ks * cin);
      OCR_HIP(hipMemcpy(wt, planes.data(), planes.size() * 2, hipMemcpyHostToDevice));
    }
    ConvDesc d{};
    d.x3 = x3;
    d.src[0] = in;
    d.src_mode = SRC_PLAIN;
    const int bf = src_mode == 16 ? 1 : 0;  // src_mode 16: bf16 operands and output (the buffers are just reinterpreted)
    d.in_bf16 = d.out_bf16 = bf;
    d.src_bytes = in_e * (bf ? 2 : 4);
    d.wgt_bytes = w_e * (x3 ? 6 : bf ? 2 : 4); d.N = n; d.Hin = h; d.Win = w; d.Cin = cin; d.Ho = ho; d.Wo = wo; d.Cout = cout;
    d.ks = ks; d.stride = stride; d.pad = pad; d.wgt = wt; d.relu = 1; d.store_mode = STORE_NHWC; d.out = out;
    d.name = "bench";
    hipEvent_t e0, e1;
    OCR_HIP(hipEventCreate(&e0));
    OCR_HIP(hipEventCreate(&e1));
    launch_conv(d, wide, det->impl.num_cus(), s);
    OCR_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) launch_conv(d, wide, det->impl.num_cus(), s);
    OCR_HIP(hipEventRecord(e1, s));
    OCR_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    OCR_HIP(hipEventElapsedTime(&ms, e0, e1));
    *ms_out = ms / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(in);
    (void)hipFree(wt);
    (void)hipFree(out);
  });
}
int ocr_test_min_area_box(const int32_t* xy, int n, int32_t* box_xy, double* sside) {
  return guard([&] {
    std::vector<ocr::geom::Pt> in(n);
    for (int i = 0; i < n; ++i) in[i] = {xy[2 * i], xy[2 * i + 1]};
    ocr::geom::Pt box[4];
    *sside = ocr::geom::min_area_bounding_box(in, box);
    for (int i = 0; i < 4; ++i) {
      box_xy[2 * i] = box[i].x;
      box_xy[2 * i + 1] = box[i].y;
    }
  });
}

// the result all-gather without RCCL: packs every shard as its rank would and assembles them as the receiver does
int ocr_test_comm_assemble(const ocr_polygons_t* const* shards, int world, ocr_polygons_t** all) {
  return guard([&] {
    if (!shards || !all || world < 1) ocr::fail(OCR_ERR_INVALID, "null argument");
    std::vector<std::vector<uint8_t>> packed;
    std::vector<const uint8_t*> ptr;
    std::vector<size_t> len;
    for (int r = 0; r < world; ++r) {
      packed.push_back(ocr::pack_shard(*shards[r]));
      ptr.push_back(packed.back().data());
      len.push_back(packed.back().size());
    }
    auto res = std::make_unique<ocr::PolygonsOwned>();
    ocr::assemble_shards(ptr.data(), len.data(), world, *res);
    *all = &res.release()->view;
  });
}

#ifdef W43_STAMPS
int ocr_test_w43_stamps(long long* out) { ocr::winograd43_read_stamps(out); return 0; }
int ocr_test_w43x_stamps(long long* out) { ocr::winograd43_x3_read_stamps(out); return 0; }
#endif
int ocr_test_w43_debug(int d) { ocr::winograd43_set_debug(d); return 0; }
#ifdef WS_STAMPS
#endif

}  // extern "C"

// ---- the phase and pyramid convs of the composed FPN (conv_igemm.hip STORE_PHASE / SRC_PYR4) and their weight builders (engine.hip) ----
namespace {
// host f32 -> device buffer of the form's element type, n_pre / n_post elements of `pad` around it inside the allocation
struct Padded {
  char* base;      // start of the allocation
  char* data;      // the tensor
  size_t bytes;    // the whole allocation
};
void fill_elems(std::vector<uint8_t>& buf, size_t at_bytes, const float* src, size_t elems, bool bf, float pad) {   // src == nullptr: `pad`
  if (bf) {
    uint16_t* d = reinterpret_cast<uint16_t*>(buf.data() + at_bytes);
    for (size_t i = 0; i < elems; ++i) d[i] = hook_bf16_bits(src ? src[i] : pad);
  } else {
    float* d = reinterpret_cast<float*>(buf.data() + at_bytes);
    for (size_t i = 0; i < elems; ++i) d[i] = src ? src[i] : pad;
  }
}
// out_io [elems] f32 <-> a device buffer of f32 or bf16
void* upload_io(HookBuffers& b, const float* io, size_t elems, bool bf) { return bf ? b.as_bf16(io, elems) : static_cast<void*>(b.f32(io, elems)); }
void download_io(float* io, const void* dev, size_t elems, bool bf) {
  if (!bf) {
    OCR_HIP(hipMemcpy(io, dev, elems * 4, hipMemcpyDeviceToHost));
    return;
  }
  std::vector<uint16_t> t(elems);
  OCR_HIP(hipMemcpy(t.data(), dev, elems * 2, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < elems; ++i) {
    const uint32_t u = (uint32_t)t[i] << 16;
    std::memcpy(&io[i], &u, 4);
  }
}
// the weights of a form: 0 f32 as built, 1 split3_weights_tiled (rows of `wrow`), 2 bf16
const void* upload_form_weights(HookBuffers& b, int form, const float* w, size_t count, int wrow, size_t* bytes) {
  if (form == 1) {
    *bytes = count * 6;
    return b.u16(ocr::split3_weights_tiled(w, count, wrow));
  }
  *bytes = count * (form == 2 ? 2 : 4);
  return form == 2 ? b.as_bf16(w, count) : static_cast<const void*>(b.f32(w, count));
}
}  // namespace

extern "C" {

// host only: engine.hip's compose_taps.  out_ohwi [cout][9][mid], in_oi [mid][cin] -> taps_out [cout][9][cin] f64
int ocr_test_compose_taps(const float* out_ohwi, int cout, int mid, const float* in_oi, int cin, double* taps_out) {
  return guard([&] {
    if (!out_ohwi || !in_oi || !taps_out || cout <= 0 || mid <= 0 || cin <= 0) ocr::fail(OCR_ERR_INVALID, "compose_taps hook: bad argument");
    const std::vector<double> t = ocr::compose_taps(out_ohwi, cout, mid, in_oi, cin);
    std::copy(t.begin(), t.end(), taps_out);
  });
}
// host only: engine.hip's phase_weights.  taps [cout][9][cin] f64 -> w_out [up*up][cout][2x2][cin] f32
int ocr_test_phase_weights(const double* taps, int cout, int cin, int up, float* w_out) {
  return guard([&] {
    if (!taps || !w_out || cout <= 0 || cin <= 0 || (up != 2 && up != 4 && up != 8)) ocr::fail(OCR_ERR_INVALID, "phase_weights hook: bad argument");
    const std::vector<float> w = ocr::phase_weights(std::vector<double>(taps, taps + (size_t)cout * 9 * cin), cout, cin, up);
    std::copy(w.begin(), w.end(), w_out);
  });
}
// host only: engine.hip's pyr4_weights.  bin1_ohwi [64][9][256], scale64 [64] -> w_out [64 phases][64][21 slots][64] f32
int ocr_test_pyr4_weights(const float* bin1_ohwi, const float* scale64, float* w_out) {
  return guard([&] {
    if (!bin1_ohwi || !scale64 || !w_out) ocr::fail(OCR_ERR_INVALID, "null argument");
    const std::vector<float> w = ocr::pyr4_weights(bin1_ohwi, scale64);
    std::copy(w.begin(), w.end(), w_out);
  });
}

// one launch_conv_igemm with STORE_PHASE / SRC_PLAIN on caller data.  form: 0 exact f32, 1 split bf16 (weights through split3_weights_tiled
// with rows of 4 * cin, as Detector::add_split_weights), 2 bf16 operands (x and the weights rounded on the way in); out_bf16: bf16 results.
// x: [n][h][w][cin]; wphase: [up*up][cout][2x2][cin] (phase_weights); bias [cout] or null.  out_io: [n][up h][up w][cout] and, behind it,
// guard_rows rows of cout elements, f32 on the host (rounded to bf16 on the way in and widened on the way out with out_bf16): uploaded
// before the launch and downloaded whole after it.  residual_in_place: the launch's residual IS that buffer, as the engine runs it.  The
// source sits between two guard regions of its allocation that src_bytes does not cover: zeros, or with poison != 0 quiet NaN.  Which
// combinations exist is conv_igemm.hip's check(): its refusals come back as errors
int ocr_test_phase_conv_run(ocr_det_t* det, int form, int out_bf16, const float* x, int n, int h, int w, int cin, const float* wphase, int cout, int up,
                            int win, const float* bias, int relu, int residual_in_place, int poison, float* out_io, int guard_rows) {
  return guard([&] {
    using namespace ocr;
    if (!det || !x || !wphase || !out_io) fail(OCR_ERR_INVALID, "null argument");
    if (form < 0 || form > 2 || n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || up <= 0 || up > 8 || guard_rows < 0)
      fail(OCR_ERR_INVALID, "phase conv hook: bad form or shape");
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    HookBuffers b;
    const bool in_bf = form == 2, out_bf = out_bf16 != 0;
    const size_t ies = in_bf ? 2 : 4;
    const size_t x_e = (size_t)n * h * w * cin, w_e = (size_t)up * up * cout * 4 * cin;
    const size_t out_e = ((size_t)n * up * h * up * w + guard_rows) * cout;
    const float pad = poison ? std::numeric_limits<float>::quiet_NaN() : 0.f;
    const size_t gap = (((size_t)2 * (w + 2) * cin * ies + 4095) / 4096) * 4096;   // more than two low-res rows on either side
    std::vector<uint8_t> img(gap + x_e * ies + gap);
    fill_elems(img, 0, nullptr, gap / ies, in_bf, pad);
    fill_elems(img, gap, x, x_e, in_bf, 0.f);
    fill_elems(img, gap + x_e * ies, nullptr, gap / ies, in_bf, pad);
    char* d_x = static_cast<char*>(b.raw(img.data(), img.size()));
    ConvDesc d{};
    d.in_bf16 = in_bf ? 1 : 0;
    d.out_bf16 = out_bf ? 1 : 0;
    d.x3 = form == 1 ? 1 : 0;
    d.src_mode = SRC_PLAIN;
    d.src[0] = d_x + gap;
    d.src_bytes = x_e * ies;
    d.wgt = upload_form_weights(b, form, wphase, w_e, 4 * cin, &d.wgt_bytes);
    d.N = n; d.Hin = h; d.Win = w; d.Cin = cin; d.Ho = h; d.Wo = w; d.Cout = cout;
    d.ks = 2; d.stride = 1; d.pad = 1; d.up = up; d.win = win;
    d.bias = bias ? b.f32(bias, cout) : nullptr;
    d.relu = relu ? 1 : 0;
    d.store_mode = STORE_PHASE;
    d.name = "test_phase_conv";
    void* d_out = upload_io(b, out_io, out_e, out_bf);
    d.out = d_out;
    d.residual = residual_in_place ? d_out : nullptr;
    launch_conv_igemm(d, s);
    OCR_HIP(hipStreamSynchronize(s));
    download_io(out_io, d_out, out_e, out_bf);
  });
}

// the same for SRC_PYR4: bin_conv1 over [up8(p5), up4(p4), up2(p3), p2] on the p5 grid.  p5 [n][h][w][64], p4 [n][2h][2w][64], p3 [n][4h][4w][64],
// p2 [n][8h][8w][64] (p2 may be null with nsrc 3: its place then holds the gaps' fill); the hook puts them into ONE allocation, a gap in front
// of, between and behind them, src_bytes covering all of it - zeros, or with poison != 0 quiet NaN: a correct kernel uses no byte of a gap.
// wpyr: [64 phases][64][21 slots][64] (pyr4_weights); nsrc 3 or 4; residual: [n][8h][8w][64] of the results' type, or null.  launches: 0 = one
// launch with pyr_group 0, 1 = pyr_group 1 only, 2 = pyr_group 2 only, 3 = 1 then 2 as the engine runs them.  out_io as above
int ocr_test_pyr4_conv_run(ocr_det_t* det, int form, int out_bf16, const float* p5, const float* p4, const float* p3, const float* p2, int n, int h, int w,
                           const float* wpyr, int nsrc, const float* bias, int relu, const float* residual, int launches, int poison, float* out_io,
                           int guard_rows) {
  return guard([&] {
    using namespace ocr;
    if (!det || !p5 || !p4 || !p3 || !wpyr || !out_io) fail(OCR_ERR_INVALID, "null argument");
    if (form < 0 || form > 2 || n <= 0 || h <= 0 || w <= 0 || guard_rows < 0 || launches < 0 || launches > 3 || (nsrc != 3 && nsrc != 4) || (nsrc == 4 && !p2))
      fail(OCR_ERR_INVALID, "pyramid conv hook: bad form, shape, sources or launches");
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    HookBuffers b;
    const bool in_bf = form == 2, out_bf = out_bf16 != 0;
    const size_t ies = in_bf ? 2 : 4;
    const size_t w_e = (size_t)64 * 64 * 21 * 64, px = (size_t)n * 8 * h * 8 * w, out_e = (px + guard_rows) * 64;
    const float pad = poison ? std::numeric_limits<float>::quiet_NaN() : 0.f;
    const float* lv[4] = {p5, p4, p3, p2};
    size_t lv_e[4], lv_at[4], at = 0;
    for (int i = 0; i < 4; ++i) {
      lv_e[i] = (size_t)n * (h << i) * (w << i) * 64;
      const size_t gap = (((size_t)2 * ((w << i) + 2) * 64 * ies + 4095) / 4096) * 4096;   // more than two rows of the level behind it
      at += gap;
      lv_at[i] = at;
      at += lv_e[i] * ies;
    }
    const size_t total = at + 8192 + (((size_t)2 * (8 * w + 2) * 64 * ies + 4095) / 4096) * 4096;
    std::vector<uint8_t> img(total);
    fill_elems(img, 0, nullptr, total / ies, in_bf, pad);
    for (int i = 0; i < 4; ++i)
      if (lv[i]) fill_elems(img, lv_at[i], lv[i], lv_e[i], in_bf, 0.f);
    char* d_src = static_cast<char*>(b.raw(img.data(), img.size()));
    ConvDesc d{};
    d.in_bf16 = in_bf ? 1 : 0;
    d.out_bf16 = out_bf ? 1 : 0;
    d.x3 = form == 1 ? 1 : 0;
    d.src_mode = SRC_PYR4;
    for (int i = 0; i < 4; ++i) d.src[i] = d_src + lv_at[i];
    d.src_base = d_src;
    d.src_bytes = total;
    d.wgt = upload_form_weights(b, form, wpyr, w_e, 21 * 64, &d.wgt_bytes);
    d.N = n; d.Hin = h; d.Win = w; d.Cin = 64; d.Ho = h; d.Wo = w; d.Cout = 64;
    d.ks = 3; d.stride = 1; d.pad = 0; d.up = 8;
    d.pyr_nsrc = nsrc;
    d.bias = bias ? b.f32(bias, 64) : nullptr;
    d.relu = relu ? 1 : 0;
    d.store_mode = STORE_PHASE;
    d.name = "test_pyr4_conv";
    d.residual = residual ? upload_io(b, residual, px * 64, out_bf) : nullptr;
    void* d_out = upload_io(b, out_io, out_e, out_bf);
    d.out = d_out;
    for (int g = 1; g <= 2; ++g) {
      if (launches != 0 && !(launches & g)) continue;
      d.pyr_group = launches == 0 ? 0 : g;
      launch_conv_igemm(d, s);
      if (launches == 0) break;
    }
    OCR_HIP(hipStreamSynchronize(s));
    download_io(out_io, d_out, out_e, out_bf);
  });
}

}  // extern "C"

// ---- the Winograd F(4x4,3x3) convs of the trunk: the fused kernel (winograd43_fused.hip), the three-launch form (winograd.hip around
// launch_winograd_gemm) and their host-side weight transforms ----
extern "C" {

// host only: engine.hip's winograd_weights.  ohwi [cout][9][cin] -> u_out [(m+2)^2][cout][cin] f32, m = 2 or 4
int ocr_test_winograd_weights(const float* ohwi, int cout, int cin, int m, float* u_out) {
  return guard([&] {
    if (!ohwi || !u_out || cout <= 0 || cin <= 0) ocr::fail(OCR_ERR_INVALID, "winograd_weights hook: bad argument");
    const std::vector<float> u = ocr::winograd_weights(ohwi, cout, cin, m);
    std::copy(u.begin(), u.end(), u_out);
  });
}
// host only: winograd43_fused.hip's winograd43_fragments.  u [36][cout][cin] -> f_out, the same count, in the MFMA B-fragment order
int ocr_test_winograd43_fragments(const float* u, int cout, int cin, float* f_out) {
  return guard([&] {
    if (!u || !f_out || cout <= 0 || cin <= 0) ocr::fail(OCR_ERR_INVALID, "winograd43_fragments hook: bad argument");
    const std::vector<float> f = ocr::winograd43_fragments(std::vector<float>(u, u + (size_t)36 * cout * cin), cout, cin);
    std::copy(f.begin(), f.end(), f_out);
  });
}

// one 3x3 s1 p1 conv (+ scale / bias / residual / ReLU) through a Winograd form on caller data.  form: 0 = launch_winograd43_fused (one
// launch; num_cus sizes its persistent grid, 0 = 256); 1 = launch_winograd_input, launch_winograd_gemm over split3_weights_tiled(u) (the 36
// split-bf16 GEMMs, as Detector::forward runs layer3 / layer4 / out4 / out5), launch_winograd_output; 2 = the same three launches with the
// exact-f32 GEMM; 3 = the three launches of F(2x2,3x3), exact f32.  x: [n][h][w][cin]; wgt: [cout][9][cin]; scale / bias [cout] or null.
// out_io: [n h w + guard_rows][cout], uploaded before the launch and downloaded whole after it: what the caller put into the guard rows comes
// back only if no launch wrote there.  inplace != 0: the residual IS the output buffer (residual == y, as fpn.lateral runs), i.e. what
// out_io holds on the way in; otherwise `residual` is a separate buffer, or null.  The source sits inside one allocation with `lead` >=
// (w + 1) cin floats in front of it and as many behind it - zeros, or with poison != 0 quiet NaN: winograd43_input_kernel's descriptor
// starts (w + 1) cin floats before the tensor, so the front region is what a failed mask of it would read
int ocr_test_winograd_run(ocr_det_t* det, int form, const float* x, int n, int h, int w, int cin, const float* wgt, int cout, const float* scale,
                          const float* bias, const float* residual, int relu, int inplace, int num_cus, int poison, float* out_io, int guard_rows) {
  return guard([&] {
    using namespace ocr;
    if (!det || !x || !wgt || !out_io) fail(OCR_ERR_INVALID, "null argument");
    if (form < 0 || form > 3 || n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || guard_rows < 0 || num_cus < 0 || (inplace && residual))
      fail(OCR_ERR_INVALID, "winograd hook: bad form, shape or residual");
    if (form == 1 && (cin % 32 || cout % 16)) fail(OCR_ERR_INVALID, "winograd hook: the split-bf16 GEMMs need Cin a multiple of 32 and Cout of 16");
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    HookBuffers b;
    const int wm = form == 3 ? 2 : 4, comps = (wm + 2) * (wm + 2);
    const size_t T = (size_t)n * ((h + wm - 1) / wm) * ((w + wm - 1) / wm);
    const size_t px = (size_t)n * h * w, in_e = px * cin, out_e = (px + guard_rows) * cout;
    const size_t lead = (((size_t)(w + 1) * cin + 1023) / 1024) * 1024;
    std::vector<float> img(lead + in_e + lead, poison ? std::numeric_limits<float>::quiet_NaN() : 0.f);
    std::copy(x, x + in_e, img.begin() + lead);
    const float* d_x = b.f32(img.data(), img.size()) + lead;
    const float* d_sc = scale ? b.f32(scale, cout) : nullptr;
    const float* d_bi = bias ? b.f32(bias, cout) : nullptr;
    float* d_y = b.f32(out_io, out_e);
    const float* d_res = inplace ? d_y : residual ? b.f32(residual, px * cout) : nullptr;
    const std::vector<float> u = winograd_weights(wgt, cout, cin, wm);
    if (form == 0) {
      const std::vector<float> uf = winograd43_fragments(u, cout, cin);
      launch_winograd43_fused(d_x, b.f32(uf.data(), uf.size()), d_sc, d_bi, d_res, relu ? 1 : 0, d_y, n, h, w, cin, cout, num_cus > 0 ? num_cus : 256, s);
    } else {
      float* d_v = b.f32(nullptr, (size_t)comps * T * cin);
      float* d_m = b.f32(nullptr, (size_t)comps * T * cout);
      const void* d_u = form == 1 ? b.u16(split3_weights_tiled(u.data(), u.size(), cin)) : static_cast<const void*>(b.f32(u.data(), u.size()));
      launch_winograd_input(d_x, d_v, n, h, w, cin, wm, s);
      launch_winograd_gemm(d_v, d_u, form == 1, comps, T, cin, cout, d_m, "test_winograd_gemm", s);
      launch_winograd_output(d_m, d_sc, d_bi, d_res, relu ? 1 : 0, d_y, n, h, w, cout, wm, s);
    }
    OCR_HIP(hipStreamSynchronize(s));
    OCR_HIP(hipMemcpy(out_io, d_y, out_e * 4, hipMemcpyDeviceToHost));
  });
}

// the F(4x4) input transform alone, as the engine launches it for out4.  low != null: launch_winograd_input_up2 over x [n][h][w][c] and low
// [n][h / 2][w / 2][c] (top_side: the top-down sum formed on load); low == null: launch_winograd_input over x.  x and low sit inside one
// allocation each with (w + 1) c floats or more in front and behind - quiet NaN: both descriptors start one row and one pixel before their
// tensor, so the front region is what a failed mask would read.  v_io: [36 T c + guard_elems], T = n ceil(h / 4) ceil(w / 4), uploaded before
// the launch and downloaded whole after it
int ocr_test_winograd_topdown(ocr_det_t* det, const float* x, const float* low, int n, int h, int w, int c, float* v_io, int guard_elems) {
  return guard([&] {
    using namespace ocr;
    if (!det || !x || !v_io) fail(OCR_ERR_INVALID, "null argument");
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0 || guard_elems < 0 || (low && ((h | w) & 1))) fail(OCR_ERR_INVALID, "winograd top-down hook: bad shape");
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    HookBuffers b;
    const size_t T = (size_t)n * ((h + 3) / 4) * ((w + 3) / 4), v_e = 36 * T * c + guard_elems;
    auto between_nan = [&](const float* src, int hh, int ww) {
      const size_t e = (size_t)n * hh * ww * c, lead = (((size_t)(ww + 1) * c + 1023) / 1024) * 1024;
      std::vector<float> img(lead + e + lead, std::numeric_limits<float>::quiet_NaN());
      std::copy(src, src + e, img.begin() + lead);
      return b.f32(img.data(), img.size()) + lead;
    };
    const float* d_x = between_nan(x, h, w);
    const float* d_low = low ? between_nan(low, h / 2, w / 2) : nullptr;
    float* d_v = b.f32(v_io, v_e);
    if (d_low) launch_winograd_input_up2(d_x, d_low, d_v, n, h, w, c, s);
    else launch_winograd_input(d_x, d_v, n, h, w, c, 4, s);
    OCR_HIP(hipStreamSynchronize(s));
    OCR_HIP(hipMemcpy(v_io, d_v, v_e * 4, hipMemcpyDeviceToHost));
  });
}

}  // extern "C"

// ---- the trunk convs of the bf16 precision: conv3x3_bf16_c64.hip, basic_block_bf16_c64.hip and conv_igemm with bf16 operands ----
extern "C" {

// one launch of the bf16 trunk on caller data.  form: 0 = launch_conv3x3_bf16_c64 (3x3 s1 64 -> 64; grid 2 x num_cus, 0 = 256 CUs);
// 1 = launch_basic_block_bf16_c64 (conv (wgt, scale, bias) + ReLU, conv (wgt2, scale2, bias2), + x, ReLU as one launch; grid num_cus);
// 2 = launch_conv_igemm with in_bf16 = out_bf16 = 1, the descriptor ocr_test_conv_run builds (ks 1 | 3, stride 1 | 2, residual,
// up_residual [n][ho / 2][wo / 2][cout] with out2 = the lateral's top-down sum; out_io == null stores the sum only).  All host arrays are f32,
// rounded to bf16 (nearest even) on the way in and widened on the way out.  x: [n][h][w][cin]; wgt: [cout][ks ks][cin].
// out_io / out2_io: [n ho wo + guard_rows][cout], uploaded before the launch and downloaded whole after it: what the caller put into the guard
// rows comes back only if no launch wrote there.  The source sits inside one allocation with `lead` >= (w + 1) cin elements in front of it and
// as many behind it - zeros, or with poison != 0 bf16 quiet NaN: the kernels take their zero padding from buffer offsets outside
// [0, tensor bytes), so these regions are what a failed mask or a wrapped offset would read.  residual and up_residual are buffers of their own.
// A tensor of 2^31 bytes or more is handed to the launcher before anything is read or allocated, without operands: it must refuse by its shape
int ocr_test_bf16_trunk_run(ocr_det_t* det, int form, const float* x, int n, int h, int w, int cin, const float* wgt, int cout, int ks, int stride,
                            const float* scale, const float* bias, const float* residual, const float* up_residual, int relu, const float* wgt2,
                            const float* scale2, const float* bias2, int num_cus, int poison, float* out_io, float* out2_io, int guard_rows) {
  return guard([&] {
    using namespace ocr;
    if (!det || !x || !wgt) fail(OCR_ERR_INVALID, "null argument");
    if (form < 0 || form > 2 || n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || guard_rows < 0 || num_cus < 0 || (ks != 1 && ks != 3) ||
        (stride != 1 && stride != 2))
      fail(OCR_ERR_INVALID, "bf16 trunk hook: bad form, shape, kernel size or stride");
    if (form != 2 && (cin != 64 || cout != 64 || ks != 3 || stride != 1 || up_residual || out2_io || !out_io))
      fail(OCR_ERR_INVALID, "bf16 trunk hook: forms 0 and 1 are the 3x3 s1 64 -> 64 kernels with one output");
    if (form == 1 && (!wgt2 || residual || !relu)) fail(OCR_ERR_INVALID, "bf16 trunk hook: the block takes two convs, adds x itself and always ends in ReLU");
    if (form != 1 && (wgt2 || scale2 || bias2)) fail(OCR_ERR_INVALID, "bf16 trunk hook: a second conv exists in form 1 only");
    if (!out_io && !out2_io) fail(OCR_ERR_INVALID, "bf16 trunk hook: no output");
    if (out2_io && !up_residual) fail(OCR_ERR_INVALID, "bf16 trunk hook: out2 is the sum with up_residual");
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    const int pad = (ks - 1) / 2, cus = num_cus > 0 ? num_cus : 256;
    const int ho = (h + 2 * pad - ks) / stride + 1, wo = (w + 2 * pad - ks) / stride + 1;
    ConvDesc d{};
    d.in_bf16 = d.out_bf16 = 1;
    d.src_mode = SRC_PLAIN;
    d.N = n; d.Hin = h; d.Win = w; d.Cin = cin; d.Ho = ho; d.Wo = wo; d.Cout = cout;
    d.ks = ks; d.stride = stride; d.pad = pad;
    d.relu = relu ? 1 : 0; d.store_mode = STORE_NHWC; d.name = "test_bf16_trunk";
    const unsigned long long in_bytes = 2ull * (unsigned long long)n * h * w * cin;
    if (in_bytes >= (1ull << 31)) {
      if (form == 0) launch_conv3x3_bf16_c64(nullptr, nullptr, nullptr, nullptr, nullptr, d.relu, nullptr, n, h, w, cus, s);
      else if (form == 1) launch_basic_block_bf16_c64(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n, h, w, cus, s);
      else {
        d.src_bytes = in_bytes;
        launch_conv_igemm(d, s);
      }
      fail(OCR_ERR_INTERNAL, "bf16 trunk hook: the launcher took a tensor of %llu bytes", in_bytes);
    }
    HookBuffers b;
    const size_t px_out = (size_t)n * ho * wo, in_e = (size_t)n * h * w * cin, out_e = (px_out + guard_rows) * cout;
    const size_t lead = (((size_t)(w + 1) * cin + 1023) / 1024) * 1024;
    std::vector<uint16_t> img(lead + in_e + lead, poison ? (uint16_t)0x7fc0 : (uint16_t)0);
    for (size_t i = 0; i < in_e; ++i) img[lead + i] = hook_bf16_bits(x[i]);
    const char* d_x = static_cast<const char*>(b.u16(img)) + lead * 2;
    const float* d_sc = scale ? b.f32(scale, cout) : nullptr;
    const float* d_bi = bias ? b.f32(bias, cout) : nullptr;
    void* d_y = out_io ? b.as_bf16(out_io, out_e) : nullptr;
    void* d_y2 = out2_io ? b.as_bf16(out2_io, out_e) : nullptr;
    const void* d_res = residual ? b.as_bf16(residual, px_out * cout) : nullptr;
    if (form == 0) {
      launch_conv3x3_bf16_c64(d_x, b.u16(conv3x3_bf16_c64_fragments(wgt)), d_sc, d_bi, d_res, d.relu, d_y, n, h, w, cus, s);
    } else if (form == 1) {
      const float* d_sc2 = scale2 ? b.f32(scale2, cout) : nullptr;
      const float* d_bi2 = bias2 ? b.f32(bias2, cout) : nullptr;
      launch_basic_block_bf16_c64(d_x, b.u16(conv3x3_bf16_c64_fragments(wgt)), d_sc, d_bi, b.u16(conv3x3_bf16_c64_fragments(wgt2)), d_sc2, d_bi2, d_y,
                                  n, h, w, cus, s);
    } else {
      const size_t w_e = (size_t)cout * ks * ks * cin;
      d.src[0] = d_x;
      d.src_bytes = in_e * 2;
      d.wgt = b.as_bf16(wgt, w_e);
      d.wgt_bytes = w_e * 2;
      d.scale = d_sc;
      d.bias = d_bi;
      d.residual = d_res;
      d.up_residual = up_residual ? b.as_bf16(up_residual, (size_t)n * (ho / 2) * (wo / 2) * cout) : nullptr;
      d.out = d_y;
      d.out2 = d_y2;
      launch_conv_igemm(d, s);
    }
    OCR_HIP(hipStreamSynchronize(s));
    auto down = [&](float* dst, const void* dev) {
      if (!dst) return;
      std::vector<uint16_t> t(out_e);
      OCR_HIP(hipMemcpy(t.data(), dev, out_e * 2, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < out_e; ++i) {
        const uint32_t u = (uint32_t)t[i] << 16;
        std::memcpy(&dst[i], &u, 4);
      }
    };
    down(out_io, d_y);
    down(out2_io, d_y2);
  });
}

}  // extern "C"

// ---- conv_igemm's plain, concat and shuffle forms: SRC_PLAIN / SRC_CAT4 sources with STORE_NHWC / STORE_SHUFFLE2 stores ----
namespace {
// the tile override for one launch: put back on every way out
struct TileOverride {
  int before;
  explicit TileOverride(int t) : before(ocr::set_conv_tile_override(t)) {}
  ~TileOverride() { ocr::set_conv_tile_override(before); }
};
}  // namespace

extern "C" {

// one launch_conv_igemm on caller data with the descriptor the engine builds.  form: 0 exact f32, 1 split bf16 (weights through
// split3_weights_tiled with rows of ks ks cin), 2 bf16 operands (x and the weights rounded on the way in); out_bf16: bf16 results, residual and
// up_residual.  src_mode SRC_PLAIN: x [batch][n][h][w][cin]; SRC_CAT4: the levels p5 (h / 8), p4 (h / 4), p3 (h / 2), p2 (h) one after the other,
// 64 channels each.  wgt [batch][cout][ks ks][cin]; store_mode STORE_NHWC: results [batch][n ho wo][cout]; STORE_SHUFFLE2: [n][2 ho][2 wo][64].
// out_io / out2_io (either may be null): the result and, behind it, guard_rows rows of its row length, f32 on the host: uploaded before the
// launch and downloaded whole after it.  residual [n ho wo][cout], up_residual [n][ho / 2][wo / 2][cout] are buffers of their own.  tile: 0 =
// pick_tile's choice, 1 = 128 x 128, 2 = 128 x 64, 3 = 64 x 64, for this launch only.  The source sits inside one allocation with a lead of at
// least (w + 1) cin elements in front of it and behind it which src_bytes does not cover; the four levels of CAT4 sit in one allocation with
// such a region in front of, between and behind them, all of it inside src_bytes - zeros, or with poison != 0 quiet NaN.  Which combinations
// exist is conv_igemm.hip's check(): its refusals come back as errors.  A source or a result of 2^31 bytes or more is handed to the launcher
// before anything is read or allocated, without operands: it must refuse by the shape
int ocr_test_igemm_run(ocr_det_t* det, int form, int out_bf16, const float* x, int n, int h, int w, int cin, const float* wgt, int cout, int ks, int stride,
                       int src_mode, int store_mode, int batch, const float* scale, const float* bias, const float* residual, const float* up_residual,
                       int relu, int tile, int poison, float* out_io, float* out2_io, int guard_rows) {
  return guard([&] {
    using namespace ocr;
    if (!det || !x || !wgt) fail(OCR_ERR_INVALID, "null argument");
    if (form < 0 || form > 2 || n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || guard_rows < 0 || batch < 1 || tile < 0 || tile > 3 ||
        (ks != 1 && ks != 3) || (stride != 1 && stride != 2) || (src_mode != SRC_PLAIN && src_mode != SRC_CAT4) ||
        (store_mode != STORE_NHWC && store_mode != STORE_SHUFFLE2))
      fail(OCR_ERR_INVALID, "igemm hook: bad form, shape, kernel size, stride, mode, batch or tile");
    if (!out_io && !out2_io) fail(OCR_ERR_INVALID, "igemm hook: no output");
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    const bool in_bf = form == 2, out_bf = out_bf16 != 0, cat4 = src_mode == SRC_CAT4, shuffle = store_mode == STORE_SHUFFLE2;
    const size_t ies = in_bf ? 2 : 4, oes = out_bf ? 2 : 4;
    const int pad = (ks - 1) / 2;
    const int ho = (h + 2 * pad - ks) / stride + 1, wo = (w + 2 * pad - ks) / stride + 1;
    ConvDesc d{};
    d.in_bf16 = in_bf ? 1 : 0;
    d.out_bf16 = out_bf ? 1 : 0;
    d.x3 = form == 1 ? 1 : 0;
    d.src_mode = src_mode;
    d.store_mode = store_mode;
    d.N = n; d.Hin = h; d.Win = w; d.Cin = cin; d.Ho = ho; d.Wo = wo; d.Cout = cout;
    d.ks = ks; d.stride = stride; d.pad = pad;
    d.batch = batch;
    d.relu = relu ? 1 : 0;
    d.name = "test_igemm";
    TileOverride tile_for_this_launch(tile);
    const size_t w_e = (size_t)batch * cout * ks * ks * cin;
    const unsigned long long in_bytes = (unsigned long long)batch * n * h * w * cin * ies, res_bytes = (unsigned long long)batch * n * ho * wo * cout * oes;
    if (in_bytes >= (1ull << 31) || res_bytes >= (1ull << 31)) {
      d.src_bytes = in_bytes;
      d.wgt_bytes = w_e * (form == 1 ? 6 : ies);
      launch_conv_igemm(d, s);
      fail(OCR_ERR_INTERNAL, "igemm hook: the launcher took a source of %llu and a result of %llu bytes", in_bytes, res_bytes);
    }
    HookBuffers b;
    const float fill = poison ? std::numeric_limits<float>::quiet_NaN() : 0.f;
    if (cat4) {
      size_t lv_e[4], lv_at[4], at = 0;
      auto gap = [&](int lw) { return (((size_t)2 * (lw + 2) * 64 * ies + 4095) / 4096) * 4096; };   // more than two rows of the level behind it
      for (int l = 0; l < 4; ++l) {
        lv_e[l] = (size_t)n * (h >> (3 - l)) * (w >> (3 - l)) * 64;
        at += gap(w >> (3 - l));
        lv_at[l] = at;
        at += lv_e[l] * ies;
      }
      const size_t total = at + gap(w);
      std::vector<uint8_t> img(total);
      fill_elems(img, 0, nullptr, total / ies, in_bf, fill);
      const float* lv = x;
      for (int l = 0; l < 4; ++l) {
        fill_elems(img, lv_at[l], lv, lv_e[l], in_bf, 0.f);
        lv += lv_e[l];
      }
      char* d_src = static_cast<char*>(b.raw(img.data(), img.size()));
      for (int l = 0; l < 4; ++l) d.src[l] = d_src + lv_at[l];
      d.src_base = d_src;
      d.src_bytes = total;
    } else {
      const size_t in_e = (size_t)batch * n * h * w * cin;
      const size_t lead = ((((size_t)(w + 1) * cin * ies) + 4095) / 4096) * 4096;
      std::vector<uint8_t> img(lead + in_e * ies + lead);
      fill_elems(img, 0, nullptr, lead / ies, in_bf, fill);
      fill_elems(img, lead, x, in_e, in_bf, 0.f);
      fill_elems(img, lead + in_e * ies, nullptr, lead / ies, in_bf, fill);
      d.src[0] = static_cast<char*>(b.raw(img.data(), img.size())) + lead;
      d.src_bytes = in_e * ies;
    }
    d.wgt = upload_form_weights(b, form, wgt, w_e, ks * ks * cin, &d.wgt_bytes);
    d.scale = scale ? b.f32(scale, cout) : nullptr;
    d.bias = bias ? b.f32(bias, cout) : nullptr;
    const size_t px = (size_t)batch * n * ho * wo;
    d.residual = residual ? upload_io(b, residual, px * cout, out_bf) : nullptr;
    d.up_residual = up_residual ? upload_io(b, up_residual, (size_t)n * (ho / 2) * (wo / 2) * cout, out_bf) : nullptr;
    const size_t rows = shuffle ? 4 * px : px, row_e = shuffle ? 64 : cout, out_e = (rows + guard_rows) * row_e;
    void* d_out = out_io ? upload_io(b, out_io, out_e, out_bf) : nullptr;
    void* d_out2 = out2_io ? upload_io(b, out2_io, out_e, out_bf) : nullptr;
    d.out = d_out;
    d.out2 = d_out2;
    launch_conv_igemm(d, s);
    OCR_HIP(hipStreamSynchronize(s));
    if (out_io) download_io(out_io, d_out, out_e, out_bf);
    if (out2_io) download_io(out2_io, d_out2, out_e, out_bf);
  });
}

}  // extern "C"
