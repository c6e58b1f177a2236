// Post-processing behind the C ABI: get_boxes_and_box_scores (metrics.rs:37-56) over a whole batch, and the pipelined detect
// calls that run it beside the next batch's forward.  postprocess() picks one of three strategies for the candidates of every image -
// the whole polygon chain on the device, device contours with Douglas-Peucker on the host pool, or the host tracer - and sends what
// is left through the shared tail: box scores (and unclip) on the GPU, finish_polygon on the pool, one CSR block out.
// Scratch slots: 0 map copy + bit images, 1 jobs / results of a call, 2 device contours, 3 / 4 contours / chain of the pending batch.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <optional>

#include "api_internal.hpp"
#include "thread_pool.hpp"

namespace {
using namespace ocr;

// device contours (contours.hip): where the pieces live inside one scratch slot, and the launches that fill them
struct ContourBuffers {
  static constexpr int CAP = 1 << 15, MAXC = 4096;   // points / contours per image (a dense page: 12 k / 60)
  char* base = nullptr;
  size_t o_bits, o_pts, o_st, o_hdr, o_pk, o_ln, o_sp, total, wpi;
  ContourBuffers(int n, size_t hw) {
    wpi = binarize_pack_words(hw);
    Carve c;
    o_bits = c.take((size_t)n * wpi * 4);
    o_pts = c.take((size_t)n * CAP * 4);
    o_st = c.take((size_t)n * (MAXC + 1) * 4);
    o_hdr = c.take((size_t)n * 16);
    o_pk = c.take((size_t)n * CAP * 4);
    o_ln = c.take((size_t)n * MAXC * 4);
    o_sp = c.take(contour_spec_bytes(n));
    total = c.end;
  }
  ContourBuffers(Detector& det, int slot, int n, size_t hw) : ContourBuffers(n, hw) { base = static_cast<char*>(det.scratch(slot, total)); }
  uint32_t* bits() const { return at<uint32_t>(base, o_bits); }
  uint32_t* pts() const { return at<uint32_t>(base, o_pts); }
  int* starts() const { return at<int>(base, o_st); }
  int* hdr() const { return at<int>(base, o_hdr); }
};
// binarize + pack + trace of a batch whose map is (or will be, stream order) on the device: everything on `s`, nothing waits
ContourBuffers enqueue_contours(Detector& det, int slot, const float* prob_dev, int n, int h, int w, float thresh, hipStream_t s) {
  const ContourBuffers cb(det, slot, n, (size_t)h * w);
  launch_binarize_pack(prob_dev, cb.bits(), thresh, n, (size_t)h * w, s);
  launch_contour_trace(cb.bits(), cb.wpi, n, h, w, cb.pts(), ContourBuffers::CAP, cb.starts(), ContourBuffers::MAXC, cb.hdr(), at<uint32_t>(cb.base, cb.o_pk),
                       at<int>(cb.base, cb.o_ln), cb.base + cb.o_sp, det.device_contours() == 2, s);
  return cb;
}

// the polygon chain behind the device tracer (candidates.hip, box_score.hip, unclip.hip): where its pieces live inside one scratch slot
struct ChainBuffers {
  char* sc = nullptr;
  int max_jobs = 0, max_pts = 0;
  size_t o_jobs, o_pts, o_sum, o_cnt, o_adj, o_st, o_len, o_oxy, o_work, o_tot, o_hd, o_cs, total;
  explicit ChainBuffers(int n) {
    max_jobs = n * 1024;   // a dense page: 60 - 130 candidates of 4 - 16 points; a batch that needs more takes the host path
    max_pts = n * 8192;
    Carve c;
    o_jobs = c.take((size_t)max_jobs * sizeof(BoxScoreJob));
    o_pts = c.take((size_t)max_pts * 8);
    o_sum = c.take((size_t)max_jobs * 8);
    o_cnt = c.take((size_t)max_jobs * 8);
    o_adj = c.take((size_t)n * 16);
    o_st = c.take((size_t)max_jobs * 4);
    o_len = c.take((size_t)max_jobs * 4);
    o_oxy = c.take(3 * (size_t)max_pts * 8);
    o_work = c.take(unclip_work_bytes((size_t)max_pts, max_jobs));
    o_tot = c.take((size_t)n * 8);
    o_hd = c.take(256);   // the batch totals: one aligned piece whatever the batch
    o_cs = c.take(candidates_scratch_bytes(n, ContourBuffers::CAP, ContourBuffers::MAXC));   // (a multiple of 256 by construction)
    total = c.end;
  }
  ChainBuffers(Detector& det, int slot, int n) : ChainBuffers(n) { sc = static_cast<char*>(det.scratch(slot, total)); }
  BoxScoreJob* jobs() const { return at<BoxScoreJob>(sc, o_jobs); }
  int32_t* pts() const { return at<int32_t>(sc, o_pts); }
  double* sums() const { return at<double>(sc, o_sum); }
  double* counts() const { return at<double>(sc, o_cnt); }
  double* adj() const { return at<double>(sc, o_adj); }
  int* tot() const { return at<int>(sc, o_tot); }
  int* totals() const { return at<int>(sc, o_hd); }
};
// Douglas-Peucker + job list, box scores, unclip of a batch whose contours are (or will be, stream order) in `cb`: everything on `s`.
// The adjust values are (or will be, stream order) at ch.adj(): the caller uploads them.
void enqueue_chain(const ChainBuffers& ch, const ContourBuffers& cb, const float* prob_dev, int n, int h, int w, const ocr_postproc_params_t& prm,
                   hipStream_t s) {
  const UnclipParams up{prm.box_thresh, prm.unclip_ratio, prm.min_size};
  launch_candidates(cb.hdr(), cb.pts(), ContourBuffers::CAP, cb.starts(), ContourBuffers::MAXC, n, h, w, ch.sc + ch.o_cs, ch.jobs(), ch.max_jobs, ch.pts(),
                    ch.max_pts, ch.tot(), ch.totals(), s);
  launch_box_scores_counted(prob_dev, h, w, ch.jobs(), ch.pts(), ch.totals(), std::min(ch.max_jobs, 4096), ch.sums(), ch.counts(), s);
  launch_unclip(ch.jobs(), ch.pts(), ch.totals(), ch.max_jobs, (size_t)ch.max_pts, ch.sums(), ch.counts(), ch.adj(), up, ch.sc + ch.o_work,
                at<uint32_t>(ch.sc, ch.o_oxy), at<int32_t>(ch.sc, ch.o_len), at<int32_t>(ch.sc, ch.o_st), s);
}

// device_contours in the pipelined calls: the contours of the batch that was just queued are requested right away - behind its
// forward, on a stream of their own - so that the call which brings its polygons back finds them done instead of waiting
void pretrace_pending(Detector& d) {
  if (!d.has_pending() || !d.device_contours()) return;
  Detector::Pending& p = d.pending();
  if (!contour_trace_fits(p.h, p.w)) return;
  hipStream_t ts = d.trace_stream();   // not the post-processing stream: crops of the batch that just came back must not queue behind this forward
  const bool chain = d.device_polygons() && d.device_unclip() && p.h == p.w;
  std::optional<ChainBuffers> ch;
  if (chain) {
    // The adjust values do not depend on the forward: they go up FIRST, while the trace stream is idle (the batch that used scratch
    // slot 4 before has been collected), from a pinned block.  Queued behind the wait for the forward from pageable memory the copy is
    // staged and awaited on the host - this call would not return before forward k and its trace had finished, and the caller could
    // not queue forward k + 1 behind forward k.
    ch.emplace(d, 4, p.n);
    double* pin = static_cast<double*>(d.host_adj((size_t)p.n * 16));
    std::memcpy(pin, p.adj.data(), (size_t)p.n * 16);
    OCR_HIP(hipMemcpyAsync(ch->adj(), pin, (size_t)p.n * 16, hipMemcpyHostToDevice, ts));
  }
  OCR_HIP(hipStreamWaitEvent(ts, p.event, 0));
  const ContourBuffers cb = enqueue_contours(d, 3, p.prob, p.n, p.h, p.w, (float)p.params.thresh, ts);
  if (chain) {   // ... and the rest of the chain behind them: the call that comes back only collects
    enqueue_chain(*ch, cb, p.prob, p.n, p.h, p.w, p.params, ts);
    p.prechained = true;
  }
  OCR_HIP(hipEventRecord(d.trace_done_event(), ts));
  p.pretraced = true;
}

// ---- one post-processing call: what every stage reads, and what the stages hand to each other
struct PerImage {   // the finished polygons of one image
  std::vector<uint32_t> xy;
  std::vector<int32_t> lens;
  std::vector<double> scores;
};
struct Post {
  Detector& det;
  const float* prob_dev;   // the map on the device
  int n, h, w;
  const double* adj;
  const ocr_postproc_params_t& prm;
  hipStream_t s;
  bool pretraced, prechained;   // contours (slot 3) / the chain behind them (slot 4) were queued when the batch was (pretrace_pending)
  size_t wpi;                   // 32-bit words per packed bit image
  uint32_t* bits_dev;           // the bit images on the device, once a stage has made them
  std::vector<uint32_t> bits;   // ... and the ones the host tracer needs
  std::vector<PerImage> per;
  std::vector<std::vector<std::vector<geom::Pt>>> cands;   // per image: the candidates the host has
  std::vector<int> todo;        // images whose candidates the host has (or must make): box scores + unclip in the tail

  // contour tracing + Douglas-Peucker of image b on the host, from its bit image (metrics.rs:78-98)
  void trace_on_host(int b) { geom::contour_candidates_bits(bits.data() + (size_t)b * wpi, h, w, cands[b]); }
  // the bit images of `imgs` on their way to the host: queued on `s`, the caller waits
  void queue_bits_home(const std::vector<int>& imgs) {
    bits.resize((size_t)n * wpi);
    for (int b : imgs) OCR_HIP(hipMemcpyAsync(bits.data() + (size_t)b * wpi, bits_dev + (size_t)b * wpi, wpi * 4, hipMemcpyDeviceToHost, s));
  }
  // a device-settled or host-finished candidate into its image's lists
  void take(int b, int st, const uint32_t* o, int olen, const std::vector<geom::Pt>& c, double score) {
    PerImage& r = per[b];
    const size_t before = r.xy.size();
    if (st == UNCLIP_KEEP) r.xy.insert(r.xy.end(), o, o + 2 * (size_t)olen);
    else if (st != UNCLIP_HOST || !geom::finish_polygon(c, score, adj[2 * b], adj[2 * b + 1], prm, r.xy)) return;
    r.lens.push_back((int32_t)((r.xy.size() - before) / 2));
    r.scores.push_back(score);
  }
};

// the batch's contours (and its bit images): requested when the batch was queued (slot 3: `s` waits for them), or requested now (slot 2)
ContourBuffers contours_of(Post& p) {
  const ContourBuffers cb = p.pretraced ? ContourBuffers(p.det, 3, p.n, (size_t)p.h * p.w)
                                        : enqueue_contours(p.det, 2, p.prob_dev, p.n, p.h, p.w, (float)p.prm.thresh, p.s);
  if (p.pretraced) OCR_HIP(hipStreamWaitEvent(p.s, p.det.trace_done_event(), 0));
  p.bits_dev = cb.bits();
  return cb;
}

// ---- host trace: binarize + pack, bit images home (metrics.rs:41,129); then the host tracer for every image
void host_trace_fetch(Post& p) {
  launch_binarize_pack(p.prob_dev, p.bits_dev, (float)p.prm.thresh, p.n, (size_t)p.h * p.w, p.s);
  p.bits.resize((size_t)p.n * p.wpi);
  OCR_HIP(hipMemcpyAsync(p.bits.data(), p.bits_dev, p.bits.size() * 4, hipMemcpyDeviceToHost, p.s));
  OCR_HIP(hipStreamSynchronize(p.s));
}
void host_trace(Post& p) {
  p.det.pool().parallel_for(p.n, [&](int b) { p.trace_on_host(b); });
  for (int b = 0; b < p.n; ++b) p.todo.push_back(b);
  p.det.post_stats[1] += p.n;
}

// ---- device trace: contour tracing on the device (contours.hip), Douglas-Peucker on the pool.  An image the device gives up on
// (buffers too small - noise: thousands of contours - or a start outside the parallel form's list) takes the host tracer.
struct DeviceContours {
  std::vector<int32_t> hdr;   // [n][4] = {contours, points, status, -}
  std::vector<size_t> p_at, c_at;
  std::vector<uint32_t> cpts;
  std::vector<int32_t> clens;
  std::vector<int> gave_up;
};
// headers, then the packed points and lengths (and the bit images of the images the device gave up) home
DeviceContours device_trace_fetch(Post& p) {
  const int n = p.n;
  const ContourBuffers cb = contours_of(p);
  DeviceContours dc;
  dc.hdr.resize((size_t)n * 4);
  OCR_HIP(hipMemcpyAsync(dc.hdr.data(), cb.hdr(), dc.hdr.size() * 4, hipMemcpyDeviceToHost, p.s));
  OCR_HIP(hipStreamSynchronize(p.s));
  dc.p_at.assign(n + 1, 0), dc.c_at.assign(n + 1, 0);
  for (int b = 0; b < n; ++b) {
    const bool ok = dc.hdr[4 * b + 2] == 0;
    if (!ok) dc.gave_up.push_back(b);
    dc.c_at[b + 1] = dc.c_at[b] + (ok ? (size_t)dc.hdr[4 * b] : 0);
    dc.p_at[b + 1] = dc.p_at[b] + (ok ? (size_t)dc.hdr[4 * b + 1] : 0);
  }
  dc.cpts.resize(dc.p_at[n]), dc.clens.resize(dc.c_at[n]);
  if (!dc.cpts.empty()) OCR_HIP(hipMemcpyAsync(dc.cpts.data(), cb.base + cb.o_pk, dc.cpts.size() * 4, hipMemcpyDeviceToHost, p.s));
  if (!dc.clens.empty()) OCR_HIP(hipMemcpyAsync(dc.clens.data(), cb.base + cb.o_ln, dc.clens.size() * 4, hipMemcpyDeviceToHost, p.s));
  if (!dc.gave_up.empty()) p.queue_bits_home(dc.gave_up);
  OCR_HIP(hipStreamSynchronize(p.s));
  return dc;
}
void device_trace_candidates(Post& p, const DeviceContours& dc) {
  p.det.pool().parallel_for(p.n, [&](int b) {
    if (dc.hdr[4 * b + 2] == 0) geom::contour_candidates_packed(dc.cpts.data() + dc.p_at[b], dc.clens.data() + dc.c_at[b], dc.hdr[4 * b], p.cands[b]);
    else p.trace_on_host(b);
  });
  p.det.post_stats[0] += p.n - (int)dc.gave_up.size();
  p.det.post_stats[1] += (int)dc.gave_up.size();
  for (int b = 0; b < p.n; ++b) p.todo.push_back(b);
}

// ---- device chain: everything on the device (contours.hip, candidates.hip, box_score.hip, unclip.hip); ONE round trip of small
// headers, one of results.  Both land in the handle's pinned buffer: the copies are queued back to back and really asynchronous (into
// pageable memory each of them is a blocking staged copy)
struct DeviceChain {
  ChainBuffers ch;
  std::vector<int32_t> tot;   // [n][2]: candidates of the image (< 0: the tracer gave it up), -
  int32_t totals[4] = {0, 0, 0, 0};   // jobs, points, overflow
};
// contours and chain from slots 3 / 4 or enqueued into 2 / 1; the first round trip
DeviceChain device_chain_fetch(Post& p) {
  const int n = p.n;
  const ContourBuffers cb = contours_of(p);
  DeviceChain dc{ChainBuffers(p.det, p.prechained ? 4 : 1, n), {}};   // slot 4: queued with the contours (pretrace_pending)
  if (!p.prechained) {
    OCR_HIP(hipMemcpyAsync(dc.ch.adj(), p.adj, (size_t)n * 16, hipMemcpyHostToDevice, p.s));
    enqueue_chain(dc.ch, cb, p.prob_dev, n, p.h, p.w, p.prm, p.s);
  }
  Carve hc;
  const size_t h_tot = hc.take((size_t)n * 8), h_totals = hc.take(256);
  char* hb = static_cast<char*>(p.det.host_scratch(hc.end));
  OCR_HIP(hipMemcpyAsync(hb + h_tot, dc.ch.tot(), (size_t)n * 8, hipMemcpyDeviceToHost, p.s));
  OCR_HIP(hipMemcpyAsync(hb + h_totals, dc.ch.totals(), 12, hipMemcpyDeviceToHost, p.s));
  OCR_HIP(hipStreamSynchronize(p.s));
  dc.tot.assign(at<const int32_t>(hb, h_tot), at<const int32_t>(hb, h_tot) + 2 * (size_t)n);
  std::memcpy(dc.totals, hb + h_totals, 12);
  return dc;
}
// the second round trip, the device-settled polygons taken per image; p.todo = the images handed back to the host
void device_chain_collect(Post& p, const DeviceChain& dc) {
  const int n = p.n;
  if (dc.totals[2] != 0) {
    for (int b = 0; b < n; ++b) p.todo.push_back(b);   // the lists overflowed: the host path takes the batch
    return;
  }
  const ChainBuffers& ch = dc.ch;
  const std::vector<int32_t>& tot = dc.tot;
  const int tj = dc.totals[0];
  const size_t tp = (size_t)dc.totals[1];
  Carve hc;
  const size_t h_jobs = hc.take((size_t)tj * sizeof(BoxScoreJob)), h_sum = hc.take((size_t)tj * 8), h_cnt = hc.take((size_t)tj * 8),
               h_st = hc.take((size_t)tj * 4), h_len = hc.take((size_t)tj * 4), h_pts = hc.take(tp * 8), h_oxy = hc.take(3 * tp * 8);
  char* hb = static_cast<char*>(p.det.host_scratch(hc.end + 256));
  const BoxScoreJob* jobs = at<const BoxScoreJob>(hb, h_jobs);
  const double *sums = at<const double>(hb, h_sum), *counts = at<const double>(hb, h_cnt);
  const int32_t *ustatus = at<const int32_t>(hb, h_st), *ulen = at<const int32_t>(hb, h_len), *pts = at<const int32_t>(hb, h_pts);
  const uint32_t* uxy = at<const uint32_t>(hb, h_oxy);
  if (tj > 0) {
    OCR_HIP(hipMemcpyAsync(hb + h_jobs, ch.jobs(), (size_t)tj * sizeof(BoxScoreJob), hipMemcpyDeviceToHost, p.s));
    OCR_HIP(hipMemcpyAsync(hb + h_sum, ch.sums(), (size_t)tj * 8, hipMemcpyDeviceToHost, p.s));
    OCR_HIP(hipMemcpyAsync(hb + h_cnt, ch.counts(), (size_t)tj * 8, hipMemcpyDeviceToHost, p.s));
    OCR_HIP(hipMemcpyAsync(hb + h_st, ch.sc + ch.o_st, (size_t)tj * 4, hipMemcpyDeviceToHost, p.s));
    OCR_HIP(hipMemcpyAsync(hb + h_len, ch.sc + ch.o_len, (size_t)tj * 4, hipMemcpyDeviceToHost, p.s));
    OCR_HIP(hipMemcpyAsync(hb + h_pts, ch.pts(), tp * 8, hipMemcpyDeviceToHost, p.s));
    OCR_HIP(hipMemcpyAsync(hb + h_oxy, ch.sc + ch.o_oxy, 3 * tp * 8, hipMemcpyDeviceToHost, p.s));
    OCR_HIP(hipStreamSynchronize(p.s));
  }
  std::vector<int> first_job(n + 1, 0);
  int at_job = 0;
  for (int b = 0; b < n; ++b) {
    first_job[b] = at_job;
    if (tot[2 * b] > 0) at_job += tot[2 * b];
    if (tot[2 * b] < 0) p.todo.push_back(b);
  }
  first_job[n] = at_job;
  if (at_job != tj) fail(OCR_ERR_INTERNAL, "postprocess: device job list holds %d jobs, its image table %d", tj, at_job);
  for (int b = 0; b < n; ++b)
    if (tot[2 * b] >= 0) {
      ++p.det.post_stats[0];
      ++p.det.post_stats[4];   // counted although the unclip kernel may still hand candidates of this image to the host (UNCLIP_HOST)
    }
  for (int j = 0; j < tj; ++j) ++p.det.post_stats[ustatus[j] == UNCLIP_HOST ? 3 : 2];
  p.det.pool().parallel_for(n, [&](int b) {
    std::vector<geom::Pt> c;
    for (int j = first_job[b]; j < first_job[b + 1]; ++j) {
      const BoxScoreJob& jb = jobs[j];
      const double score = sums[j] / counts[j];
      if (ustatus[j] == UNCLIP_HOST) {
        c.resize((size_t)jb.n_pts);
        for (int i = 0; i < jb.n_pts; ++i) c[i] = {pts[2 * ((size_t)jb.pt_offset + i)], pts[2 * ((size_t)jb.pt_offset + i) + 1]};
      }
      p.take(b, ustatus[j], uxy + 6 * (size_t)jb.pt_offset, ulen[j], c, score);
    }
  });
}
// the images the device gave up: bit image to the host, host tracer + Douglas-Peucker
void device_chain_leftovers(Post& p) {
  if (p.todo.empty()) return;
  p.queue_bits_home(p.todo);
  OCR_HIP(hipStreamSynchronize(p.s));
  p.det.pool().parallel_for((int)p.todo.size(), [&](int k) { p.trace_on_host(p.todo[k]); });
  p.det.post_stats[1] += (long long)p.todo.size();
}

// ---- score and finish on the host, for the images whose candidates are on the host (p.todo): box scores on the GPU
// (metrics.rs:99 -> :150-184), unclip behind them, what the device did not settle on the pool
struct HostJobs {
  std::vector<BoxScoreJob> jobs;
  std::vector<int32_t> pts;
  std::vector<int> first_job;   // per entry of p.todo
  bool dev_unclip = false;
  const double *sums = nullptr, *counts = nullptr;   // results, in the handle's pinned buffer
  const int32_t *ustatus = nullptr, *ulen = nullptr;
  const uint32_t* uxy = nullptr;
};
HostJobs build_jobs(const Post& p) {
  const int h = p.h, w = p.w;
  HostJobs hj;
  hj.first_job.assign(p.todo.size() + 1, 0);
  for (size_t k = 0; k < p.todo.size(); ++k) {
    const int b = p.todo[k];
    hj.first_job[k] = (int)hj.jobs.size();
    for (const auto& c : p.cands[b]) {
      if ((int)c.size() > kBoxScoreMaxPts) fail(OCR_ERR_INVALID, "polygon with %zu vertices exceeds %d", c.size(), kBoxScoreMaxPts);
      int mnx = INT32_MAX, mxx = 0, mny = INT32_MAX, mxy = 0;
      for (const auto& q : c) {
        mnx = std::min(mnx, q.x), mxx = std::max(mxx, q.x);
        mny = std::min(mny, q.y), mxy = std::max(mxy, q.y);
      }
      // the reference clamps x by size[-2] (=H) and y by size[-1] (=W): metrics.rs:151-166
      mnx = std::clamp(mnx, 0, h - 1), mxx = std::clamp(mxx, 0, h - 1);
      mny = std::clamp(mny, 0, w - 1), mxy = std::clamp(mxy, 0, w - 1);
      if (mxx >= w || mxy >= h) fail(OCR_ERR_INVALID, "non-square map: box (%d,%d) leaves the %dx%d map (the reference would fail in narrow())", mxx, mxy, w, h);
      hj.jobs.push_back(BoxScoreJob{b, (int)(hj.pts.size() / 2), (int)c.size(), mnx, mny, mxx - mnx + 1, mxy - mny + 1});
      for (const auto& q : c) hj.pts.insert(hj.pts.end(), {q.x, q.y});
    }
  }
  hj.first_job[p.todo.size()] = (int)hj.jobs.size();
  // The unclip kernel is lane-serial: about 0.2 ms however few polygons it gets, against 6 us per polygon and pool thread on the host -
  // it takes the list when there are more than 40 polygons per thread (32 text maps of three polygons with 16 threads: host; with one: device)
  hj.dev_unclip = p.det.device_unclip() && (p.det.device_unclip_always() || (int)hj.jobs.size() > 40 * p.det.post_threads());
  return hj;
}
// box scores, and unclip on the device behind them (unclip.hip): per candidate a status, and for the ones it settles the adjusted
// polygon.  Job list up and results down through the handle's pinned buffer (asynchronous copies, one wait)
void score_jobs(Post& p, HostJobs& hj) {
  const int nj = (int)hj.jobs.size();
  if (nj == 0) return;
  const size_t npts = hj.pts.size() / 2;
  Carve c;
  const size_t o_jobs = c.take(hj.jobs.size() * sizeof(BoxScoreJob)), o_pts = c.take(hj.pts.size() * 4), o_adj = c.take((size_t)p.n * 16);
  const size_t o_sum = c.take((size_t)nj * 8);   // from here on: results (one block on either side)
  const size_t o_cnt = c.take((size_t)nj * 8), o_st = c.take((size_t)nj * 4), o_len = c.take((size_t)nj * 4);
  const size_t o_oxy = c.take(hj.dev_unclip ? 3 * npts * 8 : 0), o_work = c.take(hj.dev_unclip ? unclip_work_bytes(npts, nj) : 0);
  char* sc = static_cast<char*>(p.det.scratch(1, c.end));  // slot 0 (map copy) stays valid
  char* hb = static_cast<char*>(p.det.host_scratch(o_work));
  std::memcpy(hb + o_jobs, hj.jobs.data(), hj.jobs.size() * sizeof(BoxScoreJob));
  std::memcpy(hb + o_pts, hj.pts.data(), hj.pts.size() * 4);
  std::memcpy(hb + o_adj, p.adj, (size_t)p.n * 16);
  OCR_HIP(hipMemcpyAsync(sc + o_jobs, hb + o_jobs, o_sum - o_jobs, hipMemcpyHostToDevice, p.s));   // jobs, points, adjust values: one copy
  launch_box_scores(p.prob_dev, p.h, p.w, at<const BoxScoreJob>(sc, o_jobs), at<const int32_t>(sc, o_pts), nj, at<double>(sc, o_sum), at<double>(sc, o_cnt), p.s);
  if (hj.dev_unclip) {
    const UnclipParams up{p.prm.box_thresh, p.prm.unclip_ratio, p.prm.min_size};
    launch_unclip(at<const BoxScoreJob>(sc, o_jobs), at<const int32_t>(sc, o_pts), nullptr, nj, npts, at<const double>(sc, o_sum), at<const double>(sc, o_cnt),
                  at<const double>(sc, o_adj), up, sc + o_work, at<uint32_t>(sc, o_oxy), at<int32_t>(sc, o_len), at<int32_t>(sc, o_st), p.s);
  }
  OCR_HIP(hipMemcpyAsync(hb + o_sum, sc + o_sum, (hj.dev_unclip ? o_work : o_st) - o_sum, hipMemcpyDeviceToHost, p.s));   // sums, counts [, status, lengths, polygons]
  OCR_HIP(hipStreamSynchronize(p.s));
  hj.sums = at<const double>(hb, o_sum), hj.counts = at<const double>(hb, o_cnt);
  hj.ustatus = at<const int32_t>(hb, o_st), hj.ulen = at<const int32_t>(hb, o_len), hj.uxy = at<const uint32_t>(hb, o_oxy);
}
// what the device did not settle - filters + unclip + coordinate adjustment (metrics.rs:100-123) - per image on the pool
void finish_on_host(Post& p, const HostJobs& hj) {
  const int nj = (int)hj.jobs.size();
  ++p.det.post_stats[5];
  for (int j = 0; j < nj; ++j) ++p.det.post_stats[(hj.dev_unclip && hj.ustatus[j] != UNCLIP_HOST) ? 2 : 3];
  p.det.pool().parallel_for((int)p.todo.size(), [&](int k) {
    const int b = p.todo[k];
    int j = hj.first_job[k];
    for (const auto& c : p.cands[b]) {
      const double score = hj.sums[j] / hj.counts[j];
      if (hj.dev_unclip) p.take(b, hj.ustatus[j], hj.uxy + 6 * (size_t)hj.jobs[j].pt_offset, hj.ulen[j], c, score);
      else p.take(b, UNCLIP_HOST, nullptr, 0, c, score);
      ++j;
    }
  });
}

// ---- the CSR block in image order
ocr_polygons_t* csr_block(const std::vector<PerImage>& per) {
  auto res = std::make_unique<PolygonsOwned>();
  res->img_offsets.push_back(0);
  res->poly_offsets.push_back(0);
  for (const PerImage& r : per) {
    res->xy.insert(res->xy.end(), r.xy.begin(), r.xy.end());
    for (int32_t L : r.lens) res->poly_offsets.push_back(res->poly_offsets.back() + L);
    res->scores.insert(res->scores.end(), r.scores.begin(), r.scores.end());
    res->img_offsets.push_back((int32_t)res->scores.size());
  }
  res->finish();
  return &res.release()->view;
}

// get_boxes_and_box_scores (metrics.rs:37-56) over the whole batch.  Dense, regular work on the GPU (binarisation into
// a packed bit image, box scores, unclip), irregular work on the detector's host thread pool, one image per task.
// With device contours AND device polygons (options device_contours, device_polygons) a square map's whole chain runs on the
// device - trace, Douglas-Peucker, job list, box scores, unclip - and the host only collects results; it still finishes the polygons
// the unclip kernel hands back (UNCLIP_HOST) and takes, from the bit image on, the images the tracer gave up.
// pretraced: the batch's contours were requested on the trace stream earlier (pretrace_pending, scratch slot 3): only read them
void postprocess(Detector& det, const float* prob, int n, int h, int w, int mem_kind, const double* adj, const ocr_postproc_params_t& prm,
                 ocr_polygons_t** out, hipStream_t s, bool pretraced = false, bool prechained = false) {
  // make EXTRA=-DPOSTPROC_TIMING: one line per call, the time between the marks below
#ifdef POSTPROC_TIMING
  double T[5];
  int marks = 0;
  auto mark = [&] { T[marks++] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
#else
  auto mark = [] {};
#endif
  mark();
  if (!prob || !adj || !out) fail(OCR_ERR_INVALID, "det_postprocess: null argument");
  if (n <= 0 || h <= 0 || w <= 0) fail(OCR_ERR_INVALID, "det_postprocess: bad shape");
  OCR_HIP(hipSetDevice(det.device()));
  const size_t px = (size_t)n * h * w, wpi = binarize_pack_words((size_t)h * w);
  const bool dev_trace = pretraced || (det.device_contours() && contour_trace_fits(h, w));
  const bool dev_chain = prechained || (dev_trace && det.device_polygons() && det.device_unclip() && h == w);
  // scratch slot 0: [map copy if the map is the host's] [packed bit images]
  Carve c0;
  if (mem_kind == OCR_MEM_HOST) c0.take(px * 4);
  const size_t o_bits = c0.take((size_t)n * wpi * 4);
  char* sc0 = static_cast<char*>(det.scratch(0, c0.end));
  if (mem_kind == OCR_MEM_HOST) {
    if (pretraced) fail(OCR_ERR_INTERNAL, "postprocess: a pretraced batch lives on the device");
    OCR_HIP(hipMemcpyAsync(sc0, prob, px * 4, hipMemcpyHostToDevice, s));
    prob = at<const float>(sc0, 0);
  }
  Post p{det, prob, n, h, w, adj, prm, s, pretraced, prechained, wpi, at<uint32_t>(sc0, o_bits), {}, std::vector<PerImage>(n),
         std::vector<std::vector<std::vector<geom::Pt>>>(n), {}};

  // the candidates of every image, by one of three strategies; the second mark: candidates are on the host (or settled on the device)
  if (dev_chain) {
    const DeviceChain dc = device_chain_fetch(p);
    mark();
    mark();
    device_chain_collect(p, dc);
    device_chain_leftovers(p);
  } else if (dev_trace) {
    const DeviceContours dc = device_trace_fetch(p);
    mark();
    device_trace_candidates(p, dc);
    mark();
  } else {
    host_trace_fetch(p);
    mark();
    host_trace(p);
    mark();
  }
  // the host tail for the images in p.todo
  HostJobs hj = build_jobs(p);
  score_jobs(p, hj);
  mark();
  finish_on_host(p, hj);
  *out = csr_block(p.per);
#ifdef POSTPROC_TIMING
  mark();
  fprintf(stderr, "postprocess n=%d: binarize+copy %.3f ms, contours %.3f ms, box scores (%d) %.3f ms, finish %.3f ms\n", n, T[1] - T[0], T[2] - T[1],
          (int)hj.jobs.size(), T[3] - T[2], T[4] - T[3]);
#endif
}

// the batch a pipelined call leaves pending
Detector::Pending make_pending(const float* prob, float* prob_host, int n, int h, int w, const double* adj_xy, const ocr_postproc_params_t* params,
                               hipEvent_t forward_done) {
  Detector::Pending next;
  next.prob = prob, next.prob_host = prob_host;
  next.n = n, next.h = h, next.w = w;
  next.adj.assign(adj_xy, adj_xy + 2 * (size_t)n);
  ocr_postproc_default_params(&next.params);
  if (params) next.params = *params;
  next.event = forward_done;
  next.valid = true;
  return next;
}
// finishing a batch: wait for its forward, send the map home if it was asked for, polygons out
void finish_pending(Detector& d, Detector::Pending& prev, ocr_polygons_t** out) {
  hipStream_t ps = d.post_stream();
  OCR_HIP(hipStreamWaitEvent(ps, prev.event, 0));   // the forward that produced prev.prob
  if (prev.prob_host)   // the caller asked for the map too: it leaves on the same stream, ahead of the bit image
    OCR_HIP(hipMemcpyAsync(prev.prob_host, prev.prob, (size_t)prev.n * prev.h * prev.w * 4, hipMemcpyDeviceToHost, ps));
  postprocess(d, prev.prob, prev.n, prev.h, prev.w, OCR_MEM_DEVICE, prev.adj.data(), prev.params, out, ps, prev.pretraced, prev.prechained);
}
}  // namespace

extern "C" {

void ocr_postproc_default_params(ocr_postproc_params_t* p) {
  if (!p) return;
  p->thresh = 0.6;        // metrics.rs:38
  p->box_thresh = 0.7;    // metrics.rs:64
  p->min_size = 5.0;      // metrics.rs:66
  p->unclip_ratio = 2.0;  // metrics.rs:103
  p->skip_degenerate = 0; // faithful: the reference aborts on such a candidate
  p->reserved = 0;
}

int ocr_det_postprocess(ocr_det_t* det, const float* prob, int n, int h, int w, int mem_kind, const double* adj,
                        const ocr_postproc_params_t* params, ocr_polygons_t** out) {
  return guard([&] {
    if (!det) fail(OCR_ERR_INVALID, "det_postprocess needs a detector handle (GPU + stream)");
    if (mem_kind != OCR_MEM_HOST && mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "mem_kind %d", mem_kind);
    ocr_postproc_params_t prm;
    ocr_postproc_default_params(&prm);
    if (params) prm = *params;
    if (out) *out = nullptr;
    postprocess(det->impl, prob, n, h, w, mem_kind, adj, prm, out, det->impl.stream());
  });
}

int ocr_det_post_stats(ocr_det_t* det, int64_t out[6]) {
  return guard([&] {
    if (!det || !out) fail(OCR_ERR_INVALID, "det_post_stats: null argument");
    for (int i = 0; i < 6; ++i) out[i] = (int64_t)det->impl.post_stats[i];
  });
}

int ocr_det_detect_pipelined(ocr_det_t* det, const float* x_dev, int n, int h, int w, float* prob_dev, const double* adj_xy,
                             const ocr_postproc_params_t* params, ocr_polygons_t** prev_out) {
  return guard([&] {
    if (!det || !prev_out) fail(OCR_ERR_INVALID, "detect_pipelined: null argument");
    *prev_out = nullptr;
    Detector& d = det->impl;
    OCR_HIP(hipSetDevice(d.device()));
    Detector::Pending next;
    if (x_dev) {
      if (!prob_dev || !adj_xy) fail(OCR_ERR_INVALID, "detect_pipelined: null tensor");
      d.mark_before_forward();
      d.forward(x_dev, n, h, w, prob_dev, nullptr, 0.f, nullptr);   // enqueue: runs while the previous batch is post-processed
      next = make_pending(prob_dev, nullptr, n, h, w, adj_xy, params, d.pipeline_event());
      OCR_HIP(hipEventRecord(next.event, d.stream()));
    }
    Detector::Pending prev = d.swap_pending(next);
    if (prev.valid) finish_pending(d, prev, prev_out);
    pretrace_pending(d);
  });
}

int ocr_det_detect_pipelined_host(ocr_det_t* det, const void* x_host, int x_elem, int n, int h, int w, float* prob_host,
                                  const double* adj_xy, const ocr_postproc_params_t* params, ocr_polygons_t** prev_out) {
  return guard([&] {
    if (!det || !prev_out) fail(OCR_ERR_INVALID, "detect_pipelined_host: null argument");
    *prev_out = nullptr;
    Detector& d = det->impl;
    OCR_HIP(hipSetDevice(d.device()));
    Detector::Pending next;
    if (x_host) {
      if (!adj_xy) fail(OCR_ERR_INVALID, "detect_pipelined_host: null adjust values");
      if (x_elem != OCR_ELEM_F32 && x_elem != OCR_ELEM_U8) fail(OCR_ERR_INVALID, "detect_pipelined_host: element kind %d", x_elem);
      if (n <= 0 || h <= 0 || w <= 0 || h % 32 || w % 32) fail(OCR_ERR_INVALID, "detect_pipelined_host: N=%d H=%d W=%d (H and W must be positive multiples of 32)", n, h, w);
      const size_t es = x_elem == OCR_ELEM_U8 ? 1 : 4, px = (size_t)n * h * w;
      constexpr int SET = Detector::STAGE_PIPELINED;
      // a batch that needs larger staging slots than the pending one (more frames, or f32 after u8) frees the slot the pending
      // batch's map lives in: that batch is finished FIRST (this one call loses its overlap), then the slots grow
      if (d.staging_would_grow(SET, px * es, px) && d.has_pending()) {
        Detector::Pending none;
        Detector::Pending prev = d.swap_pending(none);
        finish_pending(d, prev, prev_out);
      }
      d.ensure_staging(SET, px * es, px);
      // this batch's frames into the free input slot (the slot's previous forward was awaited when ITS polygons came back),
      // the forward behind the copy; the map stays on the device
      const int slot = d.next_stage_slot(SET);
      hipEvent_t arrived;
      const void* xd = d.stage_input(SET, slot, x_host, px * es, &arrived);
      d.mark_before_forward();
      d.forward(xd, n, h, w, d.stage_prob(SET, slot), nullptr, 0.f, nullptr, x_elem == OCR_ELEM_U8 ? 1 : 0, arrived);
      OCR_HIP(hipEventRecord(d.forward_done_event(SET, slot), d.stream()));
      d.stage_used(SET);
      next = make_pending(d.stage_prob(SET, slot), prob_host, n, h, w, adj_xy, params, d.forward_done_event(SET, slot));
    }
    Detector::Pending prev = d.swap_pending(next);
    if (prev.valid) finish_pending(d, prev, prev_out);
    pretrace_pending(d);
  });
}

void ocr_polygons_free(ocr_polygons_t* p) {
  if (!p) return;
  delete reinterpret_cast<PolygonsOwned*>(reinterpret_cast<char*>(p) - offsetof(PolygonsOwned, view));
}

}  // extern "C"
