// extern "C" boundary (include/ocr_amd.h), except post-processing and the pipelined detect calls (postprocess.hip).  Nothing throws across it.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "api_internal.hpp"
#include "word_strips.hpp"

namespace ocr {
thread_local std::string g_last_error;
}

namespace {
using ocr::guard;
using ocr::PolygonsOwned;
using ocr::Carve;
using ocr::at;

// Frames for a kernel that writes `out_bytes` of output.  Device frames are read where they are and the kernel writes straight into
// the caller's buffer; host frames go up into scratch slot 0 with the output beside them, and home() brings the output back.
// Either way home() waits for the stream.  (Job lists live in slot 1 in both cases.)
struct StagedFrames {
  const float* frames;
  float* out;
  StagedFrames(ocr::Detector& d, const float* frames_in, size_t fr_bytes, float* out_in, size_t out_bytes, int mem_kind, hipStream_t s)
      : frames(frames_in), out(out_in) {
    if (mem_kind == OCR_MEM_DEVICE) return;
    Carve c;
    const size_t o_fr = c.take(fr_bytes), o_out = c.take(out_bytes);
    void* sc = d.scratch(0, c.end);
    OCR_HIP(hipMemcpyAsync(at<char>(sc, o_fr), frames_in, fr_bytes, hipMemcpyHostToDevice, s));
    frames = at<const float>(sc, o_fr);
    out = at<float>(sc, o_out);
  }
  void home(float* out_host, size_t out_bytes, hipStream_t s) const {
    if (out != out_host) OCR_HIP(hipMemcpyAsync(out_host, out, out_bytes, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipStreamSynchronize(s));
  }
};

// The CTC decoders on host memory: one device block per call (freed when the call returns), carved into the logits and the outputs
struct CtcBlock {
  char* d = nullptr;
  size_t off[4], bytes[4];
  explicit CtcBlock(std::initializer_list<size_t> pieces) {
    Carve c;
    std::copy(pieces.begin(), pieces.end(), bytes);
    for (size_t i = 0; i < pieces.size(); ++i) off[i] = c.take(bytes[i]);
    OCR_HIP(hipMalloc(reinterpret_cast<void**>(&d), c.end));
  }
  ~CtcBlock() { (void)hipFree(d); }
  CtcBlock(const CtcBlock&) = delete;
  template <typename T>
  T* piece(int i) const { return at<T>(d, off[i]); }
  void up(int i, const void* src, hipStream_t s) const { OCR_HIP(hipMemcpyAsync(d + off[i], src, bytes[i], hipMemcpyHostToDevice, s)); }
  void home(int i, void* dst, hipStream_t s) const { OCR_HIP(hipMemcpyAsync(dst, d + off[i], bytes[i], hipMemcpyDeviceToHost, s)); }
};
}  // namespace

extern "C" {

const char* ocr_last_error(void) { return ocr::g_last_error.c_str(); }
const char* ocr_version(void) { return "ocr_amd 0.1 gfx950"; }
int ocr_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

int ocr_det_create(const void* weights, size_t bytes, int device, ocr_det_t** out) {
  return ocr_det_create_with_options(weights, bytes, device, nullptr, out);
}
int ocr_det_create_with_options(const void* weights, size_t bytes, int device, const char* options, ocr_det_t** out) {
  return guard([&] {
    if (!out) ocr::fail(OCR_ERR_INVALID, "ocr_det_create: out is null");
    *out = nullptr;
    *out = new ocr_det(weights, bytes, device, options);
  });
}
int ocr_det_create_from_varstore(const char* path, int device, ocr_det_t** out) {
  return guard([&] {
    if (!out) ocr::fail(OCR_ERR_INVALID, "ocr_det_create_from_varstore: out is null");
    *out = nullptr;
    const std::vector<uint8_t> blob = ocr::varstore_to_blob(path, 1);
    *out = new ocr_det(blob.data(), blob.size(), device);
  });
}
void ocr_det_destroy(ocr_det_t* det) { delete det; }

int ocr_varstore_to_blob(const char* path, int kind, void** blob, size_t* blob_bytes) {
  return guard([&] {
    if (!blob || !blob_bytes) ocr::fail(OCR_ERR_INVALID, "ocr_varstore_to_blob: null output");
    *blob = nullptr;
    *blob_bytes = 0;
    if (kind < 0 || kind > 2) ocr::fail(OCR_ERR_INVALID, "ocr_varstore_to_blob: kind %d", kind);
    const std::vector<uint8_t> b = ocr::varstore_to_blob(path, kind);
    void* p = std::malloc(b.size() ? b.size() : 1);
    if (!p) ocr::fail(OCR_ERR_INTERNAL, "out of memory");
    std::memcpy(p, b.data(), b.size());
    *blob = p;
    *blob_bytes = b.size();
  });
}
void ocr_blob_free(void* blob) { std::free(blob); }

int ocr_det_set_stream(ocr_det_t* det, void* s) {
  return guard([&] {
    if (!det) ocr::fail(OCR_ERR_INVALID, "null handle");
    det->impl.set_stream(static_cast<hipStream_t>(s));
  });
}

int ocr_det_set_precision(ocr_det_t* det, int precision) {
  return guard([&] {
    if (!det) ocr::fail(OCR_ERR_INVALID, "null handle");
    det->impl.set_precision(precision);
  });
}

int ocr_det_forward(ocr_det_t* det, const float* x, int n, int h, int w, float* prob, int mem_kind) {
  return guard([&] {
    if (!det) ocr::fail(OCR_ERR_INVALID, "null handle");
    if (mem_kind == OCR_MEM_HOST) {
      if (!x || !prob) ocr::fail(OCR_ERR_INVALID, "det_forward: null tensor");
      if (n <= 0 || h <= 0 || w <= 0 || h % 32 || w % 32) ocr::fail(OCR_ERR_INVALID, "det_forward: N=%d H=%d W=%d (H and W must be positive multiples of 32)", n, h, w);
      det->impl.forward_host(x, 0, n, h, w, prob);
    } else if (mem_kind == OCR_MEM_DEVICE) {
      det->impl.forward(x, n, h, w, prob, nullptr, 0.f, nullptr);
      det->impl.synchronize();
    } else {
      ocr::fail(OCR_ERR_INVALID, "mem_kind %d", mem_kind);
    }
  });
}

int ocr_det_forward_u8(ocr_det_t* det, const uint8_t* x, int n, int h, int w, float* prob, int mem_kind) {
  return guard([&] {
    if (!det) ocr::fail(OCR_ERR_INVALID, "null handle");
    if (!x || !prob) ocr::fail(OCR_ERR_INVALID, "det_forward_u8: null tensor");
    if (n <= 0 || h <= 0 || w <= 0 || h % 32 || w % 32) ocr::fail(OCR_ERR_INVALID, "det_forward_u8: N=%d H=%d W=%d (H and W must be positive multiples of 32)", n, h, w);
    if (mem_kind == OCR_MEM_HOST) {
      det->impl.forward_host(x, 1, n, h, w, prob);
    } else if (mem_kind == OCR_MEM_DEVICE) {
      det->impl.forward(x, n, h, w, prob, nullptr, 0.f, nullptr, 1);
      det->impl.synchronize();
    } else {
      ocr::fail(OCR_ERR_INVALID, "mem_kind %d", mem_kind);
    }
  });
}

int ocr_host_alloc(size_t bytes, void** out) {
  return guard([&] {
    if (!out) ocr::fail(OCR_ERR_INVALID, "ocr_host_alloc: out is null");
    *out = nullptr;
    OCR_HIP(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
  });
}
void ocr_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int ocr_det_forward_async(ocr_det_t* det, const float* x, int n, int h, int w, float* prob, uint8_t* bitmap, float thresh) {
  return guard([&] {
    if (!det) ocr::fail(OCR_ERR_INVALID, "null handle");
    det->impl.forward(x, n, h, w, prob, bitmap, thresh, nullptr);
  });
}

int ocr_det_last_front_split(ocr_det_t* det, int32_t* k) {
  return guard([&] {
    if (!det || !k) ocr::fail(OCR_ERR_INVALID, "det_last_front_split: null argument");
    *k = det->impl.last_front_split();
  });
}

int ocr_det_last_top_side(ocr_det_t* det, int32_t* moves) {
  return guard([&] {
    if (!det || !moves) ocr::fail(OCR_ERR_INVALID, "det_last_top_side: null argument");
    *moves = det->impl.last_top_side();
  });
}

int ocr_det_synchronize(ocr_det_t* det) {
  return guard([&] {
    if (!det) ocr::fail(OCR_ERR_INVALID, "null handle");
    det->impl.synchronize();
  });
}

int ocr_det_forward_profile(ocr_det_t* det, const float* x, int n, int h, int w, float* prob, int max_entries,
                            const char** names, float* ms, double* flops, double* bytes, int* n_entries) {
  return guard([&] {
    if (!det || !n_entries) ocr::fail(OCR_ERR_INVALID, "null argument");
    std::vector<ocr::ProfileEntry> prof;
    det->impl.forward(x, n, h, w, prob, nullptr, 0.f, &prof);
    const int k = std::min<int>(max_entries, (int)prof.size());
    for (int i = 0; i < k; ++i) {
      if (names) names[i] = prof[i].name;
      if (ms) ms[i] = prof[i].ms;
      if (flops) flops[i] = prof[i].flops;
      if (bytes) bytes[i] = prof[i].bytes;
    }
    *n_entries = k;
  });
}

int ocr_preprocess_image(ocr_det_t* det, const uint8_t* rgba, int w, int h, int target_w, int target_h, uint8_t* gray,
                         float* gray_f32, double* adj_xy, int mem_kind) {
  return guard([&] {
    using namespace ocr;
    if (!det || !rgba || (!gray && !gray_f32)) fail(OCR_ERR_INVALID, "preprocess_image: null argument");
    if (w < 1 || h < 1 || target_w < 1 || target_h < 1) fail(OCR_ERR_INVALID, "preprocess_image: bad dimensions");
    if (mem_kind != OCR_MEM_HOST && mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "mem_kind %d", mem_kind);
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    const size_t px_in = (size_t)w * h * 4, px_out = (size_t)target_w * target_h;
    const size_t need = preprocess_scratch_bytes(w, h, target_w, target_h);
    if (mem_kind == OCR_MEM_DEVICE) {
      // gray may be null when only the f32 frame is wanted: stage it in scratch
      Carve c;
      c.take(need);
      const size_t o_g = c.take(px_out);
      char* sc = static_cast<char*>(det->impl.scratch(1, c.end));
      launch_preprocess(rgba, w, h, target_w, target_h, gray ? gray : at<uint8_t>(sc, o_g), gray_f32, sc, need, adj_xy, s);
      OCR_HIP(hipStreamSynchronize(s));
    } else {
      Carve c;
      c.take(need);
      const size_t o_in = c.take(px_in), o_g = c.take(px_out), o_f = c.take(px_out * 4);
      char* sc = static_cast<char*>(det->impl.scratch(1, c.end));
      OCR_HIP(hipMemcpyAsync(sc + o_in, rgba, px_in, hipMemcpyHostToDevice, s));
      launch_preprocess(at<const unsigned char>(sc, o_in), w, h, target_w, target_h, at<unsigned char>(sc, o_g), gray_f32 ? at<float>(sc, o_f) : nullptr, sc,
                        need, adj_xy, s);
      if (gray) OCR_HIP(hipMemcpyAsync(gray, sc + o_g, px_out, hipMemcpyDeviceToHost, s));
      if (gray_f32) OCR_HIP(hipMemcpyAsync(gray_f32, sc + o_f, px_out * 4, hipMemcpyDeviceToHost, s));
      OCR_HIP(hipStreamSynchronize(s));
    }
  });
}

// ---- batched pre-processing (preprocess.hip: preprocess_batch_kernel; rule in include/ocr_amd.h)
namespace {
// everything both entry points refuse, before anything is queued; fills the effective strides
void check_preprocess_batch(const char* who, ocr_det_t* det, const ocr_image_t* images, int n, int src_mem_kind, int target_w, int target_h,
                            const uint8_t* gray, const float* gray_f32, int dst_mem_kind, const double* adj_xy, std::vector<int64_t>& strides) {
  using ocr::fail;
  if (!det || !images || !adj_xy) fail(OCR_ERR_INVALID, "%s: null argument", who);
  if (!gray && !gray_f32) fail(OCR_ERR_INVALID, "%s: both outputs are null", who);
  if (n < 0) fail(OCR_ERR_INVALID, "%s: n = %d", who, n);
  if (target_w < 1 || target_h < 1) fail(OCR_ERR_INVALID, "%s: target size %d x %d", who, target_w, target_h);
  if (src_mem_kind != OCR_MEM_HOST && src_mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "%s: src_mem_kind %d", who, src_mem_kind);
  if (dst_mem_kind != OCR_MEM_HOST && dst_mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "%s: dst_mem_kind %d", who, dst_mem_kind);
  strides.resize(n);
  for (int i = 0; i < n; ++i) {
    const ocr_image_t& im = images[i];
    if (!im.rgba) fail(OCR_ERR_INVALID, "%s: image %d: null pixels", who, i);
    if (im.w < 1 || im.w > 16384 || im.h < 1 || im.h > 16384) fail(OCR_ERR_INVALID, "%s: image %d: %d x %d (1 .. 16384 each)", who, i, im.w, im.h);
    const int64_t st = im.stride_bytes == 0 ? (int64_t)4 * im.w : im.stride_bytes;
    if (st < (int64_t)4 * im.w || st % 4 != 0)
      fail(OCR_ERR_INVALID, "%s: image %d: stride of %lld bytes (0, or at least 4 * w = %d and a multiple of 4)", who, i, (long long)im.stride_bytes, 4 * im.w);
    if (src_mem_kind == OCR_MEM_DEVICE && reinterpret_cast<uintptr_t>(im.rgba) % 4 != 0)
      fail(OCR_ERR_INVALID, "%s: image %d: device pixels are not 4-byte aligned", who, i);
    strides[i] = st;
  }
}

void preprocess_adjust(const ocr_image_t* images, int n, int target_w, int target_h, double* adj_xy) {
  for (int i = 0; i < n; ++i) {
    int nw, nh;
    ocr::resize_dimensions(images[i].w, images[i].h, target_w, target_h, &nw, &nh);
    adj_xy[2 * i] = (double)nw / (double)images[i].w;  // image_ops.rs:200-202
    adj_xy[2 * i + 1] = (double)nh / (double)images[i].h;
  }
}

// one launch: the plan of `cnt` device-resident images into the next plan slot, up in one copy, the kernel behind it.  Nothing waits.
void preprocess_launch(ocr::Detector& d, ocr::PrePlanner& pl, const ocr::PreSource* src, int cnt, int first_frame, uint8_t* gray_dev,
                       float* gray_f32_dev, std::vector<uint32_t>& blob, hipStream_t s) {
  const long long tiles = pl.plan(src, cnt, first_frame, blob);
  const size_t bytes = blob.size() * 4;
  ocr::Detector::PrePlanSlot& slot = d.pre_plan_slot(bytes);
  std::memcpy(slot.host, blob.data(), bytes);
  struct Mark {   // the slot is busy from its upload on, whatever happens to the launch
    ocr::Detector::PrePlanSlot& p;
    hipStream_t s;
    ~Mark() {
      if (hipEventRecord(p.done, s) == hipSuccess) p.in_flight = true;
    }
  } mark{slot, s};
  OCR_HIP(hipMemcpyAsync(slot.dev, slot.host, bytes, hipMemcpyHostToDevice, s));
  ocr::launch_preprocess_batch(slot.dev, cnt, tiles, pl.W, pl.H, gray_dev, gray_f32_dev, s);
}
}  // namespace

int ocr_preprocess_batch_async(ocr_det_t* det, const ocr_image_t* images, int n, int target_w, int target_h, uint8_t* gray_dev,
                               float* gray_f32_dev, double* adj_xy) {
  return guard([&] {
    using namespace ocr;
    std::vector<int64_t> strides;
    check_preprocess_batch("preprocess_batch_async", det, images, n, OCR_MEM_DEVICE, target_w, target_h, gray_dev, gray_f32_dev, OCR_MEM_DEVICE,
                           adj_xy, strides);
    if (n == 0) return;
    preprocess_adjust(images, n, target_w, target_h, adj_xy);
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    PrePlanner pl{target_w, target_h, {}};
    std::vector<PreSource> src(n);
    for (int i = 0; i < n; ++i) src[i] = {images[i].rgba, strides[i], images[i].w, images[i].h};
    std::vector<uint32_t> blob;
    const int step = pl.max_images();
    for (int b = 0; b < n; b += step)
      preprocess_launch(det->impl, pl, src.data() + b, std::min(step, n - b), b, gray_dev, gray_f32_dev, blob, s);
  });
}

int ocr_preprocess_batch(ocr_det_t* det, const ocr_image_t* images, int n, int src_mem_kind, int target_w, int target_h, uint8_t* gray,
                         float* gray_f32, int dst_mem_kind, double* adj_xy) {
  return guard([&] {
    using namespace ocr;
    std::vector<int64_t> strides;
    check_preprocess_batch("preprocess_batch", det, images, n, src_mem_kind, target_w, target_h, gray, gray_f32, dst_mem_kind, adj_xy, strides);
    if (n == 0) return;
    preprocess_adjust(images, n, target_w, target_h, adj_xy);
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    const bool src_host = src_mem_kind == OCR_MEM_HOST, dst_host = dst_mem_kind == OCR_MEM_HOST;
    const size_t px = (size_t)target_w * target_h;
    PrePlanner pl{target_w, target_h, {}};
    // chunks: what a chunk stages (host sources packed to 4 * w bytes a row, frames on their way to the host) stays within the
    // budget, except that an image alone may exceed it; a chunk's tiles fit one launch
    const size_t budget = det->impl.pre_stage_budget();
    auto staged = [&](int i) {
      return (src_host ? align256((size_t)4 * images[i].w * images[i].h) : 0) +
             (dst_host ? (gray ? px : 0) + (gray_f32 ? 4 * px : 0) : 0);
    };
    const size_t slack = 512;   // the two output blocks start on 256-byte boundaries
    std::vector<int> begin{0};
    size_t used = 0, stage_bytes = 0;
    for (int i = 0; i < n; ++i) {
      const int cnt = i - begin.back();
      if (cnt > 0 && (cnt >= pl.max_images() || used + staged(i) + slack > budget)) {
        begin.push_back(i);
        used = 0;
      }
      used += staged(i);
      stage_bytes = std::max(stage_bytes, used + slack);
    }
    begin.push_back(n);
    char* stage = (src_host || dst_host) ? static_cast<char*>(det->impl.pre_stage(stage_bytes)) : nullptr;
    std::vector<PreSource> src;
    std::vector<uint32_t> blob;
    for (size_t c = 0; c + 1 < begin.size(); ++c) {
      const int b = begin[c], cnt = begin[c + 1] - b;
      Carve cv;
      src.resize(cnt);
      for (int k = 0; k < cnt; ++k) {
        const ocr_image_t& im = images[b + k];
        src[k] = {im.rgba, strides[b + k], im.w, im.h};
        if (!src_host) continue;
        const size_t row = (size_t)4 * im.w;
        unsigned char* dst = at<unsigned char>(stage, cv.take(row * im.h));
        if ((size_t)strides[b + k] == row) OCR_HIP(hipMemcpyAsync(dst, im.rgba, row * im.h, hipMemcpyHostToDevice, s));
        else OCR_HIP(hipMemcpy2DAsync(dst, row, im.rgba, (size_t)strides[b + k], row, im.h, hipMemcpyHostToDevice, s));
        src[k].dev = dst;
        src[k].stride = (int64_t)row;
      }
      uint8_t* g = gray;
      float* f = gray_f32;
      if (dst_host) {
        if (gray) g = at<uint8_t>(stage, cv.take(cnt * px));
        if (gray_f32) f = at<float>(stage, cv.take(cnt * px * 4));
      }
      if (cv.end > stage_bytes && stage) fail(OCR_ERR_INTERNAL, "preprocess_batch: chunk of %zu bytes, %zu staged", cv.end, stage_bytes);
      preprocess_launch(det->impl, pl, src.data(), cnt, dst_host ? 0 : b, g, f, blob, s);
      if (dst_host) {
        if (gray) OCR_HIP(hipMemcpyAsync(gray + (size_t)b * px, g, cnt * px, hipMemcpyDeviceToHost, s));
        if (gray_f32) OCR_HIP(hipMemcpyAsync(gray_f32 + (size_t)b * px, f, cnt * px * 4, hipMemcpyDeviceToHost, s));
      }
    }
    OCR_HIP(hipStreamSynchronize(s));
  });
}

// the box of every polygon in frame coordinates (oracle/crop_oracle.py crop_boxes), shared by the crop and glyph entry points.
// h, w >= 1 (the callers check).  Non-finite adjust values cannot move a box off the frame: std::min / std::max keep their first
// argument against a NaN, so a NaN product never enters an extreme and an axis whose products are all NaN keeps the +-1e300
// sentinels, which clamp to the last pixel [w - 1, w] / [h - 1, h]; +-inf clamps like any other value.
static std::vector<ocr::CropBox> crop_boxes(const ocr_polygons_t* polys, const double* adj_xy, int n, int h, int w) {
  std::vector<ocr::CropBox> boxes;
  boxes.reserve(polys->n_polygons);
  for (int b = 0; b < n; ++b) {
    const double ax = adj_xy[2 * b], ay = adj_xy[2 * b + 1];
    for (int k = polys->img_offsets[b]; k < polys->img_offsets[b + 1]; ++k) {
      double mnx = 1e300, mxx = -1e300, mny = 1e300, mxy = -1e300;
      for (int v = polys->poly_offsets[k]; v < polys->poly_offsets[k + 1]; ++v) {
        const double x = polys->xy[2 * v] * ax, y = polys->xy[2 * v + 1] * ay;  // back to frame coordinates
        mnx = std::min(mnx, x); mxx = std::max(mxx, x);
        mny = std::min(mny, y); mxy = std::max(mxy, y);
      }
      const double x0 = std::min(std::max(mnx, 0.0), w - 1.0), x1 = std::min(std::max(mxx + 1.0, x0 + 1.0), (double)w);
      const double y0 = std::min(std::max(mny, 0.0), h - 1.0), y1 = std::min(std::max(mxy + 1.0, y0 + 1.0), (double)h);
      boxes.push_back({b, (float)x0, (float)y0, (float)x1, (float)y1});
    }
  }
  return boxes;
}

int ocr_extract_crops(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_polygons_t* polys,
                      const double* adj_xy, float* crops) {
  return guard([&] {
    using namespace ocr;
    if (!det || !frames || !polys || !adj_xy || (!crops && polys->n_polygons > 0)) fail(OCR_ERR_INVALID, "extract_crops: null argument");
    if (mem_kind != OCR_MEM_HOST && mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "extract_crops: mem_kind %d", mem_kind);
    // H, W <= 2^24: the kernel clamps a sample position to (float)(H - 1), which is H - 1 itself only up to there
    if (n < 0 || h < 1 || w < 1 || h > (1 << 24) || w > (1 << 24))
      fail(OCR_ERR_INVALID, "extract_crops: N=%d H=%d W=%d (limits: N >= 0, H and W 1..2^24)", n, h, w);
    if (polys->n_images != n) fail(OCR_ERR_INVALID, "extract_crops: polygon block holds %d images, frames %d", polys->n_images, n);
    const int np = polys->n_polygons;
    if (np == 0) return;
    const std::vector<CropBox> boxes = crop_boxes(polys, adj_xy, n, h, w);
    OCR_HIP(hipSetDevice(det->impl.device()));
    // while a pipelined forward is in flight on the handle's stream the crops of the batch that just came back are cut on
    // the post-processing stream, beside it: ordered behind everything that was queued on the handle's stream BEFORE that
    // forward (whatever produced these frames), not behind the forward itself
    hipStream_t s = det->impl.stream();
    if (det->impl.has_pending()) {
      s = det->impl.post_stream();
      if (det->impl.before_forward_event()) OCR_HIP(hipStreamWaitEvent(s, det->impl.before_forward_event(), 0));
    }
    const size_t fr_bytes = (size_t)n * h * w * 4, bx_bytes = boxes.size() * sizeof(CropBox), cr_bytes = (size_t)np * 784 * 4;
    CropBox* d_boxes = static_cast<CropBox*>(det->impl.scratch(1, ocr::align256(bx_bytes)));
    OCR_HIP(hipMemcpyAsync(d_boxes, boxes.data(), bx_bytes, hipMemcpyHostToDevice, s));
    const StagedFrames st(det->impl, frames, fr_bytes, crops, cr_bytes, mem_kind, s);
    launch_crops(st.frames, h, w, d_boxes, np, st.out, s);
    st.home(crops, cr_bytes, s);
  });
}

// ---- glyph segmentation (glyphs.hip; rule in include/ocr_amd.h, oracle tests/glyph_oracle.py)
using ocr::GlyphsOwned;   // api_internal.hpp: glyph_split.hip and lattice.hip return glyph blocks too

static ocr_segment_params_t segment_params(const ocr_segment_params_t* params, const char* who) {
  ocr_segment_params_t p;
  ocr_segment_default_params(&p);
  if (params) p = *params;
  if (p.polarity < 0 || p.polarity > 2 || p.min_col_ink < 1 || p.min_glyph_pixels < 0 || p.max_glyphs < 1 || p.max_glyphs > 256 ||
      p.glyph_box < 1 || p.glyph_box > 28 || (p.ink_high != 0 && p.ink_high != 1))
    ocr::fail(OCR_ERR_INVALID,
              "%s: params polarity=%d min_col_ink=%d min_glyph_pixels=%d max_glyphs=%d glyph_box=%d ink_high=%d (limits: polarity 0..2, "
              "min_col_ink >= 1, min_glyph_pixels >= 0, max_glyphs 1..256, glyph_box 1..28, ink_high 0..1)",
              who, p.polarity, p.min_col_ink, p.min_glyph_pixels, p.max_glyphs, p.glyph_box, p.ink_high);
  return p;
}

void ocr_segment_default_params(ocr_segment_params_t* p) {
  if (!p) return;
  p->polarity = 0;
  p->min_col_ink = 1;
  p->min_glyph_pixels = 4;
  p->max_glyphs = 32;
  p->glyph_box = 20;
  p->ink_high = 1;
}

struct LabelsOwned {   // the library-owned storage behind an ocr_glyph_labels_t* (released by ocr_glyph_labels_free)
  ocr_glyph_labels_t view{};
  std::vector<int32_t> word_boxes;
  std::vector<int64_t> plane_offsets;
  uint16_t* d_planes = nullptr;
  ~LabelsOwned() {
    if (d_planes) (void)hipFree(d_planes);
  }
  void finish(int device) {
    view.n_words = (int32_t)plane_offsets.size() - 1;
    view.device = device;
    view.word_boxes = word_boxes.data();
    view.plane_offsets = plane_offsets.data();
    view.planes = d_planes;
  }
};

// the three segmentation entry points: cc == nullptr is the column rule (ocr_segment_glyphs), else the connected-component rule;
// labels != nullptr (with cc) also keeps the label planes of the words on the device
static int segment_glyphs(const char* who, ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_polygons_t* polys,
                          const double* adj_xy, const ocr_segment_params_t* params, const ocr_cc_params_t* cc, ocr_glyphs_t** out,
                          ocr_glyph_labels_t** labels = nullptr, bool want_labels = false) {
  return guard([&] {
    using namespace ocr;
    if (labels) *labels = nullptr;
    if (!det || !frames || !polys || !adj_xy || !out || (want_labels && !labels)) fail(OCR_ERR_INVALID, "%s: null argument", who);
    *out = nullptr;
    if (mem_kind != OCR_MEM_HOST && mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "%s: mem_kind %d", who, mem_kind);
    if (n < 0 || h < 1 || w < 1) fail(OCR_ERR_INVALID, "%s: N=%d H=%d W=%d", who, n, h, w);
    if (polys->n_images != n) fail(OCR_ERR_INVALID, "%s: polygon block holds %d images, frames %d", who, polys->n_images, n);
    const ocr_segment_params_t p = segment_params(params, who);
    if (cc && (cc->merge_overlap_pct < 0 || cc->merge_overlap_pct > 100 || cc->min_height_pct < 0 || cc->min_height_pct > 100 ||
               cc->reserved[0] != 0 || cc->reserved[1] != 0))
      fail(OCR_ERR_INVALID, "%s: cc merge_overlap_pct=%d min_height_pct=%d reserved=%d, %d (limits: 0..100, 0..100, reserved 0)", who,
           cc->merge_overlap_pct, cc->min_height_pct, cc->reserved[0], cc->reserved[1]);
    std::vector<WordBox> words;
    words.reserve(polys->n_polygons);
    for (const CropBox& c : crop_boxes(polys, adj_xy, n, h, w)) {
      const int x0 = std::min(std::max((int)std::floor(c.x0), 0), w), x1 = std::min(std::max((int)std::ceil(c.x1), 0), w);
      const int y0 = std::min(std::max((int)std::floor(c.y0), 0), h), y1 = std::min(std::max((int)std::ceil(c.y1), 0), h);
      if ((int64_t)(x1 - x0) * (y1 - y0) > (int64_t(1) << 22))
        fail(OCR_ERR_INVALID, "%s: word %zu box of %lld pixels (limit 2^22)", who, words.size(), (long long)(x1 - x0) * (y1 - y0));
      words.push_back({c.frame, x0, y0, x1, y1});
    }
    std::unique_ptr<GlyphsOwned> g(new GlyphsOwned());
    g->img_offsets.assign(polys->img_offsets, polys->img_offsets + n + 1);
    g->word_offsets.push_back(0);
    const int nw = (int)words.size();
    std::unique_ptr<LabelsOwned> lb;
    if (want_labels) {
      lb.reset(new LabelsOwned());
      lb->plane_offsets.push_back(0);
      for (const WordBox& wb : words) {
        lb->word_boxes.insert(lb->word_boxes.end(), {wb.x0, wb.y0, wb.x1, wb.y1});
        lb->plane_offsets.push_back(lb->plane_offsets.back() + (int64_t)(wb.x1 - wb.x0) * (wb.y1 - wb.y0));
      }
      if (lb->plane_offsets.back() > INT32_MAX)
        fail(OCR_ERR_INVALID, "%s: %lld label plane elements (limit 2^31 - 1)", who, (long long)lb->plane_offsets.back());
    }
    if (nw > 0) {
      const int R = glyph_record_ints(p.max_glyphs);
      std::vector<int32_t> rec((size_t)nw * R);
      OCR_HIP(hipSetDevice(det->impl.device()));
      hipStream_t s = det->impl.stream();
      const size_t wd_bytes = words.size() * sizeof(WordBox), rec_bytes = rec.size() * 4, fr_bytes = (size_t)n * h * w * 4;
      const size_t po_bytes = lb ? lb->plane_offsets.size() * 8 : 0, pl_bytes = lb ? (size_t)lb->plane_offsets.back() * 2 : 0;
      if (pl_bytes) OCR_HIP(hipMalloc(reinterpret_cast<void**>(&lb->d_planes), pl_bytes));
      Carve c;
      const size_t o_wd = c.take(wd_bytes), o_rec = c.take(rec_bytes), o_po = c.take(po_bytes);
      char* sc = static_cast<char*>(det->impl.scratch(1, c.end));
      const WordBox* d_words = at<const WordBox>(sc, o_wd);
      int32_t* d_rec = at<int32_t>(sc, o_rec);
      const float* d_fr = frames;
      if (mem_kind == OCR_MEM_HOST) {
        float* f = static_cast<float*>(det->impl.scratch(0, fr_bytes));
        OCR_HIP(hipMemcpyAsync(f, frames, fr_bytes, hipMemcpyHostToDevice, s));
        d_fr = f;
      }
      OCR_HIP(hipMemcpyAsync(sc + o_wd, words.data(), wd_bytes, hipMemcpyHostToDevice, s));
      const GlyphSegParams gp{p.polarity, p.min_col_ink, p.min_glyph_pixels, p.max_glyphs};
      if (lb) {
        // flat words and both fallback exits store nothing: the planes are zero before the kernel starts, on its stream
        static_assert(sizeof(long long) == sizeof(int64_t), "plane offsets");
        OCR_HIP(hipMemcpyAsync(sc + o_po, lb->plane_offsets.data(), po_bytes, hipMemcpyHostToDevice, s));
        if (pl_bytes) OCR_HIP(hipMemsetAsync(lb->d_planes, 0, pl_bytes, s));
        launch_segment_cc_labelled(d_fr, h, w, d_words, nw, gp, GlyphCcParams{cc->merge_overlap_pct, cc->min_height_pct}, d_rec, lb->d_planes,
                                   at<const long long>(sc, o_po), s);
      } else if (cc)
        launch_segment_cc(d_fr, h, w, d_words, nw, gp, GlyphCcParams{cc->merge_overlap_pct, cc->min_height_pct}, d_rec, s);
      else
        launch_segment(d_fr, h, w, d_words, nw, gp, d_rec, s);
      OCR_HIP(hipMemcpyAsync(rec.data(), d_rec, rec_bytes, hipMemcpyDeviceToHost, s));
      OCR_HIP(hipStreamSynchronize(s));
      if (cc) {
        // words over a limit of the component rule (flag 2): the column kernel over just those, their records patched in
        std::vector<int> over;
        for (int i = 0; i < nw; ++i)
          if (rec[(size_t)i * R + 3] & 2) over.push_back(i);
        if (!over.empty()) {
          std::vector<WordBox> ow;
          for (int i : over) ow.push_back(words[i]);
          std::vector<int32_t> orec(over.size() * (size_t)R);
          // the word list and the records of the first launch have been read back: their scratch is reused
          OCR_HIP(hipMemcpyAsync(sc + o_wd, ow.data(), ow.size() * sizeof(WordBox), hipMemcpyHostToDevice, s));
          launch_segment(d_fr, h, w, d_words, (int)over.size(), gp, d_rec, s);
          OCR_HIP(hipMemcpyAsync(orec.data(), d_rec, orec.size() * 4, hipMemcpyDeviceToHost, s));
          OCR_HIP(hipStreamSynchronize(s));
          for (size_t k = 0; k < over.size(); ++k) {
            int32_t* r = &rec[(size_t)over[k] * R];
            std::copy(&orec[k * R], &orec[k * R] + R, r);
            r[3] |= 2;
          }
        }
      }
      g->word_info.resize((size_t)4 * nw);
      g->word_levels.resize((size_t)2 * nw);
      for (int i = 0; i < nw; ++i) {   // the per-word records -> CSR
        const int32_t* r = &rec[(size_t)i * R];
        std::copy(r, r + 4, &g->word_info[(size_t)4 * i]);
        std::memcpy(&g->word_levels[(size_t)2 * i], r + 4, 8);
        if (r[6] < 0 || r[6] > p.max_glyphs) fail(OCR_ERR_INTERNAL, "%s: word %d reports %d glyphs", who, i, r[6]);
        g->boxes.insert(g->boxes.end(), r + 8, r + 8 + 4 * r[6]);
        g->word_offsets.push_back((int32_t)(g->boxes.size() / 4));
      }
    }
    g->finish();
    if (lb) {
      lb->finish(det->impl.device());
      *labels = &lb.release()->view;
    }
    *out = &g.release()->view;
  });
}

int ocr_segment_glyphs(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_polygons_t* polys,
                       const double* adj_xy, const ocr_segment_params_t* params, ocr_glyphs_t** out) {
  return segment_glyphs("segment_glyphs", det, frames, n, h, w, mem_kind, polys, adj_xy, params, nullptr, out);
}

void ocr_cc_default_params(ocr_cc_params_t* p) {
  if (!p) return;
  p->merge_overlap_pct = 50;
  p->min_height_pct = 25;
  p->reserved[0] = p->reserved[1] = 0;
}

int ocr_segment_glyphs_cc(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_polygons_t* polys,
                          const double* adj_xy, const ocr_segment_params_t* params, const ocr_cc_params_t* cc, ocr_glyphs_t** out) {
  ocr_cc_params_t c;
  ocr_cc_default_params(&c);
  if (cc) c = *cc;
  return segment_glyphs("segment_glyphs_cc", det, frames, n, h, w, mem_kind, polys, adj_xy, params, &c, out);
}

int ocr_segment_glyphs_cc_labelled(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_polygons_t* polys,
                                   const double* adj_xy, const ocr_segment_params_t* params, const ocr_cc_params_t* cc, ocr_glyphs_t** out,
                                   ocr_glyph_labels_t** labels) {
  ocr_cc_params_t c;
  ocr_cc_default_params(&c);
  if (cc) c = *cc;
  return segment_glyphs("segment_glyphs_cc_labelled", det, frames, n, h, w, mem_kind, polys, adj_xy, params, &c, out, labels, true);
}

void ocr_mask_default_params(ocr_mask_params_t* p) {
  if (!p) return;
  p->halo = 1;
  p->reserved[0] = p->reserved[1] = p->reserved[2] = 0;
}

int ocr_glyph_labels_read(ocr_det_t* det, const ocr_glyph_labels_t* labels, uint16_t* planes_host) {
  return guard([&] {
    using namespace ocr;
    if (!det || !labels) fail(OCR_ERR_INVALID, "glyph_labels_read: null argument");
    if (labels->n_words < 0 || !labels->plane_offsets) fail(OCR_ERR_INVALID, "glyph_labels_read: %d words, or no plane offsets", labels->n_words);
    if (labels->device != det->impl.device())
      fail(OCR_ERR_INVALID, "glyph_labels_read: planes on device %d, handle on device %d", labels->device, det->impl.device());
    const int64_t total = labels->plane_offsets[labels->n_words];
    if (total < 0 || total > INT32_MAX) fail(OCR_ERR_INVALID, "glyph_labels_read: %lld plane elements", (long long)total);
    if (total == 0) return;
    if (!labels->planes || !planes_host) fail(OCR_ERR_INVALID, "glyph_labels_read: null planes");
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    OCR_HIP(hipMemcpyAsync(planes_host, labels->planes, (size_t)total * 2, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipStreamSynchronize(s));
  });
}

void ocr_glyph_labels_free(ocr_glyph_labels_t* l) {
  if (!l) return;
  delete reinterpret_cast<LabelsOwned*>(reinterpret_cast<char*>(l) - offsetof(LabelsOwned, view));
}

// both crop entry points: labels == nullptr cuts the crops from the boxes alone (ocr_extract_glyph_crops), else through the label planes
static int extract_glyph_crops(const char* who, ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_glyphs_t* glyphs,
                               const ocr_glyph_labels_t* labels, bool masked, const ocr_segment_params_t* params,
                               const ocr_mask_params_t* mask, float* crops) {
  return guard([&] {
    using namespace ocr;
    if (!det || !frames || !glyphs || (masked && !labels) || (!crops && glyphs->n_glyphs > 0)) fail(OCR_ERR_INVALID, "%s: null argument", who);
    if (mem_kind != OCR_MEM_HOST && mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "%s: mem_kind %d", who, mem_kind);
    if (n < 0 || h < 1 || w < 1) fail(OCR_ERR_INVALID, "%s: N=%d H=%d W=%d", who, n, h, w);
    if (glyphs->n_images != n) fail(OCR_ERR_INVALID, "%s: glyph block holds %d images, frames %d", who, glyphs->n_images, n);
    const ocr_segment_params_t p = segment_params(params, who);
    const int nw = glyphs->n_words, ng = glyphs->n_glyphs;
    if (nw < 0 || ng < 0) fail(OCR_ERR_INVALID, "%s: %d words, %d glyphs", who, nw, ng);
    ocr_mask_params_t mp;
    ocr_mask_default_params(&mp);
    if (masked) {
      if (mask) mp = *mask;
      if (mp.halo < 0 || mp.halo > 1 || mp.reserved[0] != 0 || mp.reserved[1] != 0 || mp.reserved[2] != 0)
        fail(OCR_ERR_INVALID, "%s: mask halo=%d reserved=%d, %d, %d (limits: halo 0..1, reserved 0)", who, mp.halo, mp.reserved[0],
             mp.reserved[1], mp.reserved[2]);
      if (labels->n_words != nw) fail(OCR_ERR_INVALID, "%s: label block holds %d words, glyph block %d", who, labels->n_words, nw);
      if (labels->device != det->impl.device())
        fail(OCR_ERR_INVALID, "%s: label planes on device %d, handle on device %d", who, labels->device, det->impl.device());
    }
    if (ng == 0) return;
    if (!glyphs->word_offsets || !glyphs->word_info || !glyphs->word_levels || !glyphs->boxes)
      fail(OCR_ERR_INVALID, "%s: null array in the glyph block", who);
    if (glyphs->word_offsets[0] != 0 || glyphs->word_offsets[nw] != ng) fail(OCR_ERR_INVALID, "%s: word offsets do not span the glyphs", who);
    if (masked) {   // the kernel reads a plane inside its word box only: the offsets must be the boxes' sizes, end to end
      if (!labels->word_boxes || !labels->plane_offsets || labels->plane_offsets[0] != 0) fail(OCR_ERR_INVALID, "%s: null array in the label block", who);
      for (int i = 0; i < nw; ++i) {
        const int32_t* wbx = labels->word_boxes + 4 * (size_t)i;
        const int64_t bw = (int64_t)wbx[2] - wbx[0], bh = (int64_t)wbx[3] - wbx[1];
        if (bw < 0 || bh < 0 || bw * bh > (int64_t(1) << 22) || labels->plane_offsets[i + 1] - labels->plane_offsets[i] != bw * bh)
          fail(OCR_ERR_INVALID, "%s: word %d box (%d, %d, %d, %d) does not fit its plane of %lld elements", who, i, wbx[0], wbx[1], wbx[2], wbx[3],
               (long long)(labels->plane_offsets[i + 1] - labels->plane_offsets[i]));
      }
      if (labels->plane_offsets[nw] > INT32_MAX) fail(OCR_ERR_INVALID, "%s: %lld label plane elements", who, (long long)labels->plane_offsets[nw]);
      if (labels->plane_offsets[nw] > 0 && !labels->planes) fail(OCR_ERR_INVALID, "%s: null planes", who);
    }
    std::vector<GlyphJob> jobs;
    std::vector<GlyphMaskJob> mjobs;
    if (masked) mjobs.reserve(ng); else jobs.reserve(ng);
    for (int i = 0; i < nw; ++i) {   // every box is checked against the frames: the kernel reads inside them only
      const int fr = glyphs->word_info[4 * i];
      const int k0 = glyphs->word_offsets[i], k1 = glyphs->word_offsets[i + 1];
      if (k1 < k0 || k1 > ng) fail(OCR_ERR_INVALID, "%s: word %d glyph range [%d, %d)", who, i, k0, k1);
      if (k1 > k0 && (fr < 0 || fr >= n)) fail(OCR_ERR_INVALID, "%s: word %d on frame %d of %d", who, i, fr, n);
      if (masked && k1 - k0 > 65534) fail(OCR_ERR_INVALID, "%s: word %d holds %d glyphs (limit 65534: labels are 16 bits)", who, i, k1 - k0);
      for (int k = k0; k < k1; ++k) {
        const int32_t* b = glyphs->boxes + 4 * (size_t)k;
        if (b[0] < 0 || b[1] < 0 || b[2] > w || b[3] > h || b[0] >= b[2] || b[1] >= b[3])
          fail(OCR_ERR_INVALID, "%s: glyph %d box (%d, %d, %d, %d) outside the %d x %d frame", who, k, b[0], b[1], b[2], b[3], w, h);
        const GlyphJob job{fr, b[0], b[1], b[2], b[3], glyphs->word_levels[2 * i], glyphs->word_levels[2 * i + 1]};
        if (!masked) {
          jobs.push_back(job);
          continue;
        }
        const int32_t* wbx = labels->word_boxes + 4 * (size_t)i;
        if (b[0] < wbx[0] || b[1] < wbx[1] || b[2] > wbx[2] || b[3] > wbx[3])
          fail(OCR_ERR_INVALID, "%s: glyph %d box (%d, %d, %d, %d) not inside its word's box (%d, %d, %d, %d)", who, k, b[0], b[1], b[2], b[3],
               wbx[0], wbx[1], wbx[2], wbx[3]);
        mjobs.push_back({job, wbx[0], wbx[1], wbx[2], wbx[3], k - k0 + 1, labels->planes + labels->plane_offsets[i]});
      }
    }
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    const size_t jb_bytes = masked ? mjobs.size() * sizeof(GlyphMaskJob) : jobs.size() * sizeof(GlyphJob);
    const size_t fr_bytes = (size_t)n * h * w * 4, cr_bytes = (size_t)ng * 784 * 4;
    void* d_jobs = det->impl.scratch(1, ocr::align256(jb_bytes));
    OCR_HIP(hipMemcpyAsync(d_jobs, masked ? static_cast<const void*>(mjobs.data()) : jobs.data(), jb_bytes, hipMemcpyHostToDevice, s));
    const StagedFrames st(det->impl, frames, fr_bytes, crops, cr_bytes, mem_kind, s);
    if (masked)
      launch_glyph_crops_masked(st.frames, h, w, static_cast<const GlyphMaskJob*>(d_jobs), ng, p.glyph_box, p.ink_high, mp.halo, st.out, s);
    else
      launch_glyph_crops(st.frames, h, w, static_cast<const GlyphJob*>(d_jobs), ng, p.glyph_box, p.ink_high, st.out, s);
    st.home(crops, cr_bytes, s);
  });
}

int ocr_extract_glyph_crops(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_glyphs_t* glyphs,
                            const ocr_segment_params_t* params, float* crops) {
  return extract_glyph_crops("extract_glyph_crops", det, frames, n, h, w, mem_kind, glyphs, nullptr, false, params, nullptr, crops);
}

int ocr_extract_glyph_crops_masked(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_glyphs_t* glyphs,
                                   const ocr_glyph_labels_t* labels, const ocr_segment_params_t* params, const ocr_mask_params_t* mask,
                                   float* crops) {
  return extract_glyph_crops("extract_glyph_crops_masked", det, frames, n, h, w, mem_kind, glyphs, labels, true, params, mask, crops);
}

void ocr_glyphs_free(ocr_glyphs_t* g) {
  if (!g) return;
  delete reinterpret_cast<GlyphsOwned*>(reinterpret_cast<char*>(g) - offsetof(GlyphsOwned, view));
}

// ---- word strips (word_strips.cpp geometry, strips.hip sampling; rule in include/ocr_amd.h, oracle tests/strip_oracle.py)
void ocr_strip_default_params(ocr_strip_params_t* p) {
  if (!p) return;
  p->strip_height = 32;
  p->max_width = 1024;
  p->reserved[0] = p->reserved[1] = 0;
}

int ocr_plan_word_strips(const ocr_polygons_t* polys, const double* adj_xy, int n, int h, int w, const ocr_strip_params_t* params,
                         ocr_word_strips_t** out) {
  return guard([&] {
    using namespace ocr;
    if (!polys || !adj_xy || !out) fail(OCR_ERR_INVALID, "plan_word_strips: null argument");
    *out = nullptr;
    if (n < 0 || h < 1 || w < 1) fail(OCR_ERR_INVALID, "plan_word_strips: N=%d H=%d W=%d", n, h, w);
    ocr_strip_params_t p;
    ocr_strip_default_params(&p);
    if (params) p = *params;
    if (p.strip_height < 8 || p.strip_height > 128 || p.max_width < 1 || p.max_width > 8192 || p.reserved[0] || p.reserved[1])
      fail(OCR_ERR_INVALID, "plan_word_strips: params strip_height=%d max_width=%d reserved=(%d, %d) (limits: strip_height 8..128, "
           "max_width 1..8192, reserved 0)", p.strip_height, p.max_width, p.reserved[0], p.reserved[1]);
    std::unique_ptr<WordStripsOwned> s(new WordStripsOwned());
    plan_word_strips(*polys, adj_xy, n, p, *s);
    s->finish();
    *out = &s.release()->view;
  });
}

// a strips block from the caller: offsets, frames and size checked before anything reads through it
static void check_strips(const ocr_word_strips_t* s, int n, const char* who) {
  using ocr::fail;
  if (s->n_images != n) fail(OCR_ERR_INVALID, "%s: strips block holds %d images, frames %d", who, s->n_images, n);
  const int nw = s->n_words;
  if (nw < 0 || s->total_width < 0 || s->height < 8 || s->height > 128)
    fail(OCR_ERR_INVALID, "%s: %d words, height %d, total width %d", who, nw, s->height, s->total_width);
  if ((int64_t)s->height * s->total_width > ocr::kStripMaxAtlas)
    fail(OCR_ERR_INVALID, "%s: atlas of %d x %d is more than 2^31 elements", who, s->height, s->total_width);
  if (!s->col_offsets || (nw > 0 && (!s->word_info || !s->maps || !s->quads || !s->scores)))
    fail(OCR_ERR_INVALID, "%s: null array in the strips block", who);
  if (s->col_offsets[0] != 0 || s->col_offsets[nw] != s->total_width)
    fail(OCR_ERR_INVALID, "%s: column offsets do not span the %d atlas columns", who, s->total_width);
  for (int k = 0; k < nw; ++k) {
    if (s->col_offsets[k + 1] <= s->col_offsets[k]) fail(OCR_ERR_INVALID, "%s: word %d columns [%d, %d)", who, k, s->col_offsets[k], s->col_offsets[k + 1]);
    if (s->word_info[2 * k] < 0 || s->word_info[2 * k] >= n) fail(OCR_ERR_INVALID, "%s: word %d on frame %d of %d", who, k, s->word_info[2 * k], n);
  }
}

int ocr_extract_word_strips(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_word_strips_t* strips,
                            float* atlas) {
  return guard([&] {
    using namespace ocr;
    if (!det || !frames || !strips) fail(OCR_ERR_INVALID, "extract_word_strips: null argument");
    if (mem_kind != OCR_MEM_HOST && mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "extract_word_strips: mem_kind %d", mem_kind);
    if (n < 0 || h < 1 || w < 1) fail(OCR_ERR_INVALID, "extract_word_strips: N=%d H=%d W=%d", n, h, w);
    check_strips(strips, n, "extract_word_strips");
    const int nw = strips->n_words, Hs = strips->height, tw = strips->total_width;
    if (tw == 0) return;
    if (!atlas) fail(OCR_ERR_INVALID, "extract_word_strips: null atlas");
    std::vector<StripWord> words(nw);
    std::vector<int32_t> col_word(tw);
    for (int k = 0; k < nw; ++k) {
      const float* m = strips->maps + 6 * (size_t)k;
      const int c0 = strips->col_offsets[k];
      words[k] = {m[0], m[1], m[2], m[3], m[4], m[5], strips->word_info[2 * k], c0};
      std::fill(col_word.begin() + c0, col_word.begin() + strips->col_offsets[k + 1], k);
    }
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    const size_t wd_bytes = words.size() * sizeof(StripWord), cw_bytes = col_word.size() * 4;
    const size_t fr_bytes = (size_t)n * h * w * 4, at_bytes = (size_t)Hs * tw * 4;
    Carve c;
    const size_t o_wd = c.take(wd_bytes), o_cw = c.take(cw_bytes);
    char* sc = static_cast<char*>(det->impl.scratch(1, c.end));
    OCR_HIP(hipMemcpyAsync(sc + o_wd, words.data(), wd_bytes, hipMemcpyHostToDevice, s));
    OCR_HIP(hipMemcpyAsync(sc + o_cw, col_word.data(), cw_bytes, hipMemcpyHostToDevice, s));
    const StagedFrames st(det->impl, frames, fr_bytes, atlas, at_bytes, mem_kind, s);
    launch_word_strips(st.frames, h, w, at<const StripWord>(sc, o_wd), at<const int32_t>(sc, o_cw), Hs, tw, st.out, s);
    st.home(atlas, at_bytes, s);
  });
}

int ocr_word_strip_polygons(const ocr_word_strips_t* strips, ocr_polygons_t** out) {
  return guard([&] {
    using namespace ocr;
    if (!strips || !out) fail(OCR_ERR_INVALID, "word_strip_polygons: null argument");
    *out = nullptr;
    check_strips(strips, strips->n_images, "word_strip_polygons");
    const int nw = strips->n_words;
    const uint32_t y1 = (uint32_t)strips->height - 1;
    std::unique_ptr<PolygonsOwned> p(new PolygonsOwned());
    p->img_offsets = {0, nw};
    p->poly_offsets.push_back(0);
    for (int k = 0; k < nw; ++k) {
      const uint32_t c0 = (uint32_t)strips->col_offsets[k], c1 = (uint32_t)strips->col_offsets[k + 1] - 1;
      const uint32_t v[8] = {c0, 0, c1, 0, c1, y1, c0, y1};
      p->xy.insert(p->xy.end(), v, v + 8);
      p->poly_offsets.push_back(4 * (k + 1));
      p->scores.push_back(strips->scores[k]);
    }
    p->finish();
    *out = &p.release()->view;
  });
}

void ocr_word_strips_free(ocr_word_strips_t* s) {
  if (!s) return;
  delete reinterpret_cast<ocr::WordStripsOwned*>(reinterpret_cast<char*>(s) - offsetof(ocr::WordStripsOwned, view));
}

// ---- curved strips (word_strips.cpp geometry, curved_strips.hip sampling; rule in include/ocr_amd.h, oracle tests/curved_strip_oracle.py)
void ocr_curve_default_params(ocr_curve_params_t* p) {
  if (!p) return;
  p->strip_height = 32;
  p->max_width = 1024;
  p->valid_pct = 80;
  p->reserved = 0;
}

int ocr_plan_curved_strips(const ocr_polygons_t* polys, const double* adj_xy, int n, int h, int w, const ocr_curve_params_t* params,
                           ocr_curved_strips_t** out) {
  return guard([&] {
    using namespace ocr;
    if (!polys || !adj_xy || !out) fail(OCR_ERR_INVALID, "plan_curved_strips: null argument");
    *out = nullptr;
    if (n < 0 || h < 1 || w < 1) fail(OCR_ERR_INVALID, "plan_curved_strips: N=%d H=%d W=%d", n, h, w);
    ocr_curve_params_t p;
    ocr_curve_default_params(&p);
    if (params) p = *params;
    if (p.strip_height < 8 || p.strip_height > 128 || p.max_width < 1 || p.max_width > 8192 || p.valid_pct < 1 || p.valid_pct > 100 ||
        p.reserved)
      fail(OCR_ERR_INVALID, "plan_curved_strips: params strip_height=%d max_width=%d valid_pct=%d reserved=%d (limits: strip_height "
           "8..128, max_width 1..8192, valid_pct 1..100, reserved 0)", p.strip_height, p.max_width, p.valid_pct, p.reserved);
    std::unique_ptr<CurvedStripsOwned> s(new CurvedStripsOwned());
    plan_curved_strips(*polys, adj_xy, n, p, *s);
    s->finish();
    *out = &s.release()->view;
  });
}

// a curved strips block from the caller: offsets, frames, knot intervals and size checked before anything reads through it
static void check_curved_strips(const ocr_curved_strips_t* s, int n, const char* who) {
  using ocr::fail;
  if (s->n_images != n) fail(OCR_ERR_INVALID, "%s: strips block holds %d images, frames %d", who, s->n_images, n);
  const int nw = s->n_words;
  if (nw < 0 || s->total_width < 0 || s->height < 8 || s->height > 128)
    fail(OCR_ERR_INVALID, "%s: %d words, height %d, total width %d", who, nw, s->height, s->total_width);
  if ((int64_t)s->height * s->total_width > ocr::kStripMaxAtlas)
    fail(OCR_ERR_INVALID, "%s: atlas of %d x %d is more than 2^31 elements", who, s->height, s->total_width);
  if (!s->col_offsets || (nw > 0 && (!s->word_info || !s->knots || !s->tscale || !s->scores)))
    fail(OCR_ERR_INVALID, "%s: null array in the strips block", who);
  if (s->col_offsets[0] != 0 || s->col_offsets[nw] != s->total_width)
    fail(OCR_ERR_INVALID, "%s: column offsets do not span the %d atlas columns", who, s->total_width);
  for (int k = 0; k < nw; ++k) {
    if (s->col_offsets[k + 1] <= s->col_offsets[k]) fail(OCR_ERR_INVALID, "%s: word %d columns [%d, %d)", who, k, s->col_offsets[k], s->col_offsets[k + 1]);
    if (s->word_info[2 * k] < 0 || s->word_info[2 * k] >= n) fail(OCR_ERR_INVALID, "%s: word %d on frame %d of %d", who, k, s->word_info[2 * k], n);
    if (!(std::isfinite(s->tscale[k]) && s->tscale[k] > 0)) fail(OCR_ERR_INVALID, "%s: word %d tscale %g (finite and > 0)", who, k, (double)s->tscale[k]);
  }
}

int ocr_extract_curved_strips(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_curved_strips_t* strips,
                              float* atlas) {
  return guard([&] {
    using namespace ocr;
    if (!det || !frames || !strips) fail(OCR_ERR_INVALID, "extract_curved_strips: null argument");
    if (mem_kind != OCR_MEM_HOST && mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "extract_curved_strips: mem_kind %d", mem_kind);
    if (n < 0 || h < 1 || w < 1) fail(OCR_ERR_INVALID, "extract_curved_strips: N=%d H=%d W=%d", n, h, w);
    check_curved_strips(strips, n, "extract_curved_strips");
    const int nw = strips->n_words, Hs = strips->height, tw = strips->total_width;
    if (tw == 0) return;
    if (!atlas) fail(OCR_ERR_INVALID, "extract_curved_strips: null atlas");
    std::vector<CurveWord> words(nw);
    std::vector<int32_t> col_word(tw);
    for (int k = 0; k < nw; ++k) {
      const int c0 = strips->col_offsets[k];
      words[k] = {strips->word_info[2 * k], c0, strips->tscale[k], 0};
      std::fill(col_word.begin() + c0, col_word.begin() + strips->col_offsets[k + 1], k);
    }
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    const size_t wd_bytes = words.size() * sizeof(CurveWord), kn_bytes = (size_t)nw * OCR_CURVE_KNOTS * 16, cw_bytes = col_word.size() * 4;
    const size_t fr_bytes = (size_t)n * h * w * 4, at_bytes = (size_t)Hs * tw * 4;
    Carve c;
    const size_t o_wd = c.take(wd_bytes), o_kn = c.take(kn_bytes), o_cw = c.take(cw_bytes);
    char* sc = static_cast<char*>(det->impl.scratch(1, c.end));
    OCR_HIP(hipMemcpyAsync(sc + o_wd, words.data(), wd_bytes, hipMemcpyHostToDevice, s));
    OCR_HIP(hipMemcpyAsync(sc + o_kn, strips->knots, kn_bytes, hipMemcpyHostToDevice, s));
    OCR_HIP(hipMemcpyAsync(sc + o_cw, col_word.data(), cw_bytes, hipMemcpyHostToDevice, s));
    const StagedFrames st(det->impl, frames, fr_bytes, atlas, at_bytes, mem_kind, s);
    launch_curved_strips(st.frames, h, w, at<const CurveWord>(sc, o_wd), at<const float>(sc, o_kn), at<const int32_t>(sc, o_cw), Hs, tw,
                         st.out, s);
    st.home(atlas, at_bytes, s);
  });
}

int ocr_curved_strip_polygons(const ocr_curved_strips_t* strips, ocr_polygons_t** out) {
  return guard([&] {
    using namespace ocr;
    if (!strips || !out) fail(OCR_ERR_INVALID, "curved_strip_polygons: null argument");
    *out = nullptr;
    check_curved_strips(strips, strips->n_images, "curved_strip_polygons");
    const int nw = strips->n_words;
    const uint32_t y1 = (uint32_t)strips->height - 1;
    std::unique_ptr<PolygonsOwned> p(new PolygonsOwned());
    p->img_offsets = {0, nw};
    p->poly_offsets.push_back(0);
    for (int k = 0; k < nw; ++k) {
      const uint32_t c0 = (uint32_t)strips->col_offsets[k], c1 = (uint32_t)strips->col_offsets[k + 1] - 1;
      const uint32_t v[8] = {c0, 0, c1, 0, c1, y1, c0, y1};
      p->xy.insert(p->xy.end(), v, v + 8);
      p->poly_offsets.push_back(4 * (k + 1));
      p->scores.push_back(strips->scores[k]);
    }
    p->finish();
    *out = &p.release()->view;
  });
}

void ocr_curved_strips_free(ocr_curved_strips_t* s) {
  if (!s) return;
  delete reinterpret_cast<ocr::CurvedStripsOwned*>(reinterpret_cast<char*>(s) - offsetof(ocr::CurvedStripsOwned, view));
}

// ---- line grouping (lines.hip; rule in include/ocr_amd.h, oracle tests/line_oracle.py)
void ocr_line_default_params(ocr_line_params_t* p) {
  if (!p) return;
  p->line_tol = 0.5;
  p->height_ratio = 2.0;
  p->min_cos = 0.866;
  p->max_gap = 3.0;
  p->reserved[0] = p->reserved[1] = 0;
}

int ocr_group_lines(ocr_det_t* det, const double* quads, const int32_t* word_img_offsets, int n_images, const ocr_line_params_t* params,
                    ocr_lines_t** out) {
  return guard([&] {
    using namespace ocr;
    if (!det || !word_img_offsets || !out) fail(OCR_ERR_INVALID, "group_lines: null argument");
    *out = nullptr;
    if (n_images < 1) fail(OCR_ERR_INVALID, "group_lines: %d images", n_images);
    ocr_line_params_t p;
    ocr_line_default_params(&p);
    if (params) p = *params;
    // (written so that a NaN is out of range)
    if (!(p.line_tol > 0 && p.line_tol <= 4) || !(p.height_ratio >= 1 && p.height_ratio <= 16) || !(p.min_cos >= 0 && p.min_cos <= 1) ||
        !(p.max_gap >= 0 && p.max_gap <= 64) || p.reserved[0] || p.reserved[1])
      fail(OCR_ERR_INVALID, "group_lines: params line_tol=%g height_ratio=%g min_cos=%g max_gap=%g reserved=(%d, %d) (limits: line_tol "
           "(0, 4], height_ratio [1, 16], min_cos [0, 1], max_gap [0, 64], reserved 0)", p.line_tol, p.height_ratio, p.min_cos, p.max_gap,
           p.reserved[0], p.reserved[1]);
    if (word_img_offsets[0] != 0) fail(OCR_ERR_INVALID, "group_lines: word offsets start at %d", word_img_offsets[0]);
    int max_words = 0;
    for (int b = 0; b < n_images; ++b) {
      const int64_t cnt = (int64_t)word_img_offsets[b + 1] - word_img_offsets[b];
      if (cnt < 0) fail(OCR_ERR_INVALID, "group_lines: word offsets decrease at image %d", b);
      if (cnt > OCR_LINE_MAX_WORDS) fail(OCR_ERR_INVALID, "group_lines: image %d has %lld words (limit %d)", b, (long long)cnt, OCR_LINE_MAX_WORDS);
      max_words = std::max(max_words, (int)cnt);
    }
    const int nw = word_img_offsets[n_images];
    if (nw > 0 && !quads) fail(OCR_ERR_INVALID, "group_lines: null quads");
    for (size_t e = 0; e < (size_t)nw * 8; ++e)
      if (!std::isfinite(quads[e])) fail(OCR_ERR_INVALID, "group_lines: word %zu has a non-finite coordinate", e / 8);
    std::unique_ptr<LinesOwned> l(new LinesOwned());
    l->img_offsets.assign(1, 0);
    l->line_offsets.assign(1, 0);
    if (nw == 0) {
      l->img_offsets.assign((size_t)n_images + 1, 0);
      l->finish();
      *out = &l.release()->view;
      return;
    }
    static_assert(OCR_LINE_MAX_WORDS == kLineMaxWords, "line grouping limit");
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    const size_t q_bytes = (size_t)nw * 64, off_bytes = ((size_t)n_images + 1) * 4, w4 = (size_t)nw * 4;
    Carve c;
    const size_t o_q = c.take(q_bytes), o_off = c.take(off_bytes), o_feat = c.take((size_t)nw * kLineFeatBytes), o_link = c.take(2 * w4);
    const size_t o_ord = c.take(w4), o_fl = c.take(w4), o_gap = c.take((size_t)nw * 8), o_ls = c.take(w4), o_nl = c.take((size_t)n_images * 4);
    char* sc = static_cast<char*>(det->impl.scratch(1, c.end));
    OCR_HIP(hipMemcpyAsync(sc + o_q, quads, q_bytes, hipMemcpyHostToDevice, s));
    OCR_HIP(hipMemcpyAsync(sc + o_off, word_img_offsets, off_bytes, hipMemcpyHostToDevice, s));
    launch_group_lines(at<const double>(sc, o_q), at<const int32_t>(sc, o_off), n_images, nw, max_words,
                       LineParams{p.line_tol, p.height_ratio, p.min_cos, p.max_gap}, sc + o_feat, at<int32_t>(sc, o_link),
                       at<int32_t>(sc, o_ord), at<int32_t>(sc, o_fl), at<double>(sc, o_gap), at<int32_t>(sc, o_ls), at<int32_t>(sc, o_nl), s);
    std::vector<int32_t> line_start(nw), n_lines(n_images);
    l->order.resize(nw);
    l->word_flags.resize(nw);
    l->gaps.resize(nw);
    OCR_HIP(hipMemcpyAsync(l->order.data(), sc + o_ord, w4, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(l->word_flags.data(), sc + o_fl, w4, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(l->gaps.data(), sc + o_gap, (size_t)nw * 8, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(line_start.data(), sc + o_ls, w4, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(n_lines.data(), sc + o_nl, (size_t)n_images * 4, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipStreamSynchronize(s));
    // the kernel leaves the line starts of image b in its own word slice; the CSR over the batch is their concatenation
    l->line_offsets.clear();
    for (int b = 0; b < n_images; ++b) {
      const int w0 = word_img_offsets[b], cnt = word_img_offsets[b + 1] - w0;
      if (n_lines[b] < 0 || n_lines[b] > cnt || (cnt > 0 && n_lines[b] == 0)) fail(OCR_ERR_INTERNAL, "group_lines: image %d reports %d lines of %d words", b, n_lines[b], cnt);
      l->line_offsets.insert(l->line_offsets.end(), line_start.begin() + w0, line_start.begin() + w0 + n_lines[b]);
      l->img_offsets.push_back((int32_t)l->line_offsets.size());
    }
    l->line_offsets.push_back(nw);
    l->finish();
    *out = &l.release()->view;
  });
}

void ocr_lines_free(ocr_lines_t* l) {
  if (!l) return;
  delete reinterpret_cast<ocr::LinesOwned*>(reinterpret_cast<char*>(l) - offsetof(ocr::LinesOwned, view));
}

// ---- column-aware reading order (columns.hip; rule in include/ocr_amd.h, oracle tests/column_oracle.py)
void ocr_column_default_params(ocr_column_params_t* p) {
  if (!p) return;
  ocr_line_default_params(&p->line);
  p->row_gap = 16.0;
  p->min_gutter = 1.5;
  p->gutter_reach = 2.5;
  p->min_overlap = 0.25;
  p->block_reach = 2.5;
  p->min_rows = 3;
  p->max_levels = 64;
  p->reserved[0] = p->reserved[1] = 0;
}

int ocr_group_columns(ocr_det_t* det, const double* quads, const int32_t* word_img_offsets, int n_images, const ocr_column_params_t* params,
                      ocr_columns_t** out) {
  return guard([&] {
    using namespace ocr;
    if (!det || !word_img_offsets || !out) fail(OCR_ERR_INVALID, "group_columns: null argument");
    *out = nullptr;
    if (n_images < 1) fail(OCR_ERR_INVALID, "group_columns: %d images", n_images);
    ocr_column_params_t p;
    ocr_column_default_params(&p);
    if (params) p = *params;
    const ocr_line_params_t& lp = p.line;
    // (written so that a NaN is out of range)
    if (!(lp.line_tol > 0 && lp.line_tol <= 4) || !(lp.height_ratio >= 1 && lp.height_ratio <= 16) || !(lp.min_cos >= 0 && lp.min_cos <= 1) ||
        !(lp.max_gap >= 0 && lp.max_gap <= 64) || lp.reserved[0] || lp.reserved[1])
      fail(OCR_ERR_INVALID, "group_columns: line params line_tol=%g height_ratio=%g min_cos=%g max_gap=%g reserved=(%d, %d) (limits: line_tol "
           "(0, 4], height_ratio [1, 16], min_cos [0, 1], max_gap [0, 64], reserved 0)", lp.line_tol, lp.height_ratio, lp.min_cos, lp.max_gap,
           lp.reserved[0], lp.reserved[1]);
    if (!(p.row_gap >= lp.max_gap && p.row_gap <= 64) || !(p.min_gutter >= 0 && p.min_gutter <= 64) ||
        !(p.gutter_reach > 0 && p.gutter_reach <= 16) || !(p.min_overlap >= 0 && p.min_overlap <= 1) ||
        !(p.block_reach > 0 && p.block_reach <= 16) || p.min_rows < 1 || p.min_rows > 4096 || p.max_levels < 1 || p.max_levels > 256 ||
        p.reserved[0] || p.reserved[1])
      fail(OCR_ERR_INVALID, "group_columns: params row_gap=%g min_gutter=%g gutter_reach=%g min_overlap=%g block_reach=%g min_rows=%d "
           "max_levels=%d reserved=(%d, %d) (limits: row_gap [max_gap, 64], min_gutter [0, 64], gutter_reach (0, 16], min_overlap [0, 1], "
           "block_reach (0, 16], min_rows [1, 4096], max_levels [1, 256], reserved 0)", p.row_gap, p.min_gutter, p.gutter_reach,
           p.min_overlap, p.block_reach, p.min_rows, p.max_levels, p.reserved[0], p.reserved[1]);
    if (word_img_offsets[0] != 0) fail(OCR_ERR_INVALID, "group_columns: word offsets start at %d", word_img_offsets[0]);
    int max_words = 0;
    for (int b = 0; b < n_images; ++b) {
      const int64_t cnt = (int64_t)word_img_offsets[b + 1] - word_img_offsets[b];
      if (cnt < 0) fail(OCR_ERR_INVALID, "group_columns: word offsets decrease at image %d", b);
      if (cnt > OCR_LINE_MAX_WORDS) fail(OCR_ERR_INVALID, "group_columns: image %d has %lld words (limit %d)", b, (long long)cnt, OCR_LINE_MAX_WORDS);
      max_words = std::max(max_words, (int)cnt);
    }
    const int nw = word_img_offsets[n_images];
    if (nw > 0 && !quads) fail(OCR_ERR_INVALID, "group_columns: null quads");
    for (size_t e = 0; e < (size_t)nw * 8; ++e)
      if (!std::isfinite(quads[e])) fail(OCR_ERR_INVALID, "group_columns: word %zu has a non-finite coordinate", e / 8);
    std::unique_ptr<ColumnsOwned> c(new ColumnsOwned());
    c->img_offsets.assign(1, 0);
    c->block_offsets.assign(1, 0);
    c->line_offsets.assign(1, 0);
    if (nw == 0) {
      c->img_offsets.assign((size_t)n_images + 1, 0);
      c->finish();
      *out = &c.release()->view;
      return;
    }
    OCR_HIP(hipSetDevice(det->impl.device()));
    hipStream_t s = det->impl.stream();
    const size_t q_bytes = (size_t)nw * 64, off_bytes = ((size_t)n_images + 1) * 4, w4 = (size_t)nw * 4, w8 = (size_t)nw * 8;
    Carve cv;
    const size_t o_q = cv.take(q_bytes), o_off = cv.take(off_bytes);
    ColumnBuffers b;
    // (offsets first: the scratch block is fetched once the carve is complete)
    struct Slot { void** p; size_t off; };
    std::vector<Slot> slots;
    auto want = [&](auto*& ptr, size_t bytes) { slots.push_back({reinterpret_cast<void**>(&ptr), cv.take(bytes)}); };
    want(b.feat, (size_t)nw * kLineFeatBytes);
    want(b.link, 2 * w4);
    want(b.row_order, w4);
    want(b.flags, w4);
    want(b.row_start, w4);
    want(b.n_rows, (size_t)n_images * 4);
    want(b.row_gaps, w8);
    want(b.row_prev, w4);
    want(b.row_pos, w4);
    want(b.gap_state, w4);
    want(b.line_state, w4);
    want(b.line_head, w4);
    want(b.line_len, w4);
    want(b.line_cut, w4);
    want(b.gap_by_word, w8);
    want(b.gap_rec, (size_t)nw * kColumnGapBytes);
    want(b.line_rec, (size_t)nw * kColumnLineBytes);
    want(b.block_rec, (size_t)nw * kColumnBlockBytes);
    want(b.block_quads_by_slot, 8 * w8);
    want(b.pred_bits, (size_t)nw * ((max_words + 31) / 32) * 4);
    want(b.order, w4);
    want(b.line_start, w4);
    want(b.line_flags, w4);
    want(b.block_start, w4);
    want(b.block_levels, w4);
    want(b.counts, (size_t)n_images * 8);
    want(b.gaps, w8);
    want(b.block_quads, 8 * w8);
    char* sc = static_cast<char*>(det->impl.scratch(1, cv.end));
    for (const Slot& sl : slots) *sl.p = sc + sl.off;
    OCR_HIP(hipMemcpyAsync(sc + o_q, quads, q_bytes, hipMemcpyHostToDevice, s));
    OCR_HIP(hipMemcpyAsync(sc + o_off, word_img_offsets, off_bytes, hipMemcpyHostToDevice, s));
    launch_group_columns(at<const double>(sc, o_q), at<const int32_t>(sc, o_off), n_images, nw, max_words,
                         LineParams{lp.line_tol, lp.height_ratio, lp.min_cos, p.row_gap},
                         ColumnParams{lp.height_ratio, lp.min_cos, lp.max_gap, p.min_gutter, p.gutter_reach, p.min_overlap, p.block_reach,
                                      p.min_rows, p.max_levels}, b, s);
    std::vector<int32_t> line_start(nw), line_flags(nw), block_start(nw), block_levels(nw), counts(2 * (size_t)n_images);
    std::vector<double> block_quads(8 * (size_t)nw);
    c->order.resize(nw);
    c->word_flags.resize(nw);
    c->gaps.resize(nw);
    OCR_HIP(hipMemcpyAsync(c->order.data(), b.order, w4, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(c->word_flags.data(), b.flags, w4, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(c->gaps.data(), b.gaps, w8, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(line_start.data(), b.line_start, w4, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(line_flags.data(), b.line_flags, w4, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(block_start.data(), b.block_start, w4, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(block_levels.data(), b.block_levels, w4, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(block_quads.data(), b.block_quads, 8 * w8, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipMemcpyAsync(counts.data(), b.counts, (size_t)n_images * 8, hipMemcpyDeviceToHost, s));
    OCR_HIP(hipStreamSynchronize(s));
    // the kernels leave the lines and blocks of image b at the front of its own word slice; the CSRs over the batch are their
    // concatenation (block starts are image-local line numbers)
    c->line_offsets.clear();
    c->block_offsets.clear();
    for (int i = 0; i < n_images; ++i) {
      const int w0 = word_img_offsets[i], cnt = word_img_offsets[i + 1] - w0, nl = counts[2 * i], nb = counts[2 * i + 1];
      if (nl < 0 || nl > cnt || nb < 0 || nb > nl || (cnt > 0 && nb == 0))
        fail(OCR_ERR_INTERNAL, "group_columns: image %d reports %d lines in %d blocks of %d words", i, nl, nb, cnt);
      const int32_t l0 = (int32_t)c->line_offsets.size();
      for (int k = 0; k < nb; ++k) c->block_offsets.push_back(l0 + block_start[w0 + k]);
      c->line_offsets.insert(c->line_offsets.end(), line_start.begin() + w0, line_start.begin() + w0 + nl);
      c->line_flags.insert(c->line_flags.end(), line_flags.begin() + w0, line_flags.begin() + w0 + nl);
      c->block_levels.insert(c->block_levels.end(), block_levels.begin() + w0, block_levels.begin() + w0 + nb);
      c->block_quads.insert(c->block_quads.end(), block_quads.begin() + 8 * (size_t)w0, block_quads.begin() + 8 * ((size_t)w0 + nb));
      c->img_offsets.push_back((int32_t)c->block_offsets.size());
    }
    c->block_offsets.push_back((int32_t)c->line_offsets.size());
    c->line_offsets.push_back(nw);
    c->finish();
    *out = &c.release()->view;
  });
}

void ocr_columns_free(ocr_columns_t* c) {
  if (!c) return;
  delete reinterpret_cast<ocr::ColumnsOwned*>(reinterpret_cast<char*>(c) - offsetof(ocr::ColumnsOwned, view));
}

static std::vector<std::vector<ocr::geom::Pt>> csr_polys(const uint32_t* xy, const int32_t* offsets, int n) {
  std::vector<std::vector<ocr::geom::Pt>> out(n);
  for (int k = 0; k < n; ++k)
    for (int v = offsets[k]; v < offsets[k + 1]; ++v) out[k].push_back({(int)xy[2 * v], (int)xy[2 * v + 1]});
  return out;
}

int ocr_evaluate_image(const uint32_t* gt_xy, const int32_t* gt_offsets, int n_gt, const uint8_t* ignore_flags,
                       const uint32_t* pred_xy, const int32_t* pred_offsets, int n_pred, ocr_metrics_item_t* out) {
  return guard([&] {
    if (!out || n_gt < 0 || n_pred < 0 || (n_gt > 0 && (!gt_xy || !gt_offsets || !ignore_flags)) || (n_pred > 0 && (!pred_xy || !pred_offsets)))
      ocr::fail(OCR_ERR_INVALID, "evaluate_image: null argument");
    std::vector<bool> ign(n_gt);
    for (int i = 0; i < n_gt; ++i) ign[i] = ignore_flags[i] != 0;
    const ocr::geom::MetricsItem m = ocr::geom::evaluate_image(csr_polys(gt_xy, gt_offsets, n_gt), ign, csr_polys(pred_xy, pred_offsets, n_pred));
    out->precision = m.precision;
    out->recall = m.recall;
    out->hmean = m.hmean;
    out->gt_care = m.gt_care;
    out->det_care = m.det_care;
    out->det_matched = m.det_matched;
  });
}

int ocr_combine_results(const ocr_metrics_item_t* items, int n, double* precision, double* recall, double* hmean) {
  return guard([&] {
    if ((n > 0 && !items) || !precision || !recall || !hmean) ocr::fail(OCR_ERR_INVALID, "combine_results: null argument");
    std::vector<ocr::geom::MetricsItem> v(n);
    for (int i = 0; i < n; ++i) v[i] = {items[i].precision, items[i].recall, items[i].hmean, items[i].gt_care, items[i].det_care, items[i].det_matched};
    ocr::geom::combine_results(v.data(), n, precision, recall, hmean);
  });
}


int ocr_rec_create(const void* weights, size_t bytes, int device, ocr_rec_t** out) {
  return guard([&] {
    if (!out) ocr::fail(OCR_ERR_INVALID, "ocr_rec_create: out is null");
    *out = nullptr;
    *out = new ocr_rec(weights, bytes, device);
  });
}
int ocr_rec_create_from_varstore(const char* path, int device, ocr_rec_t** out) {
  return guard([&] {
    if (!out) ocr::fail(OCR_ERR_INVALID, "ocr_rec_create_from_varstore: out is null");
    *out = nullptr;
    const std::vector<uint8_t> blob = ocr::varstore_to_blob(path, 2);
    *out = new ocr_rec(blob.data(), blob.size(), device);
  });
}
void ocr_rec_destroy(ocr_rec_t* rec) { delete rec; }
int ocr_rec_set_stream(ocr_rec_t* rec, void* s) {
  return guard([&] {
    if (!rec) ocr::fail(OCR_ERR_INVALID, "null handle");
    rec->impl.set_stream(static_cast<hipStream_t>(s));
  });
}
int ocr_rec_set_options(ocr_rec_t* rec, const char* options) {
  return guard([&] {
    if (!rec) ocr::fail(OCR_ERR_INVALID, "null handle");
    rec->impl.set_options(options);
  });
}
int ocr_rec_synchronize(ocr_rec_t* rec) {
  return guard([&] {
    if (!rec) ocr::fail(OCR_ERR_INVALID, "null handle");
    rec->impl.synchronize();
  });
}
int ocr_rec_forward(ocr_rec_t* rec, const float* crops, int n, float* logits, int mem_kind) {
  return guard([&] {
    if (!rec || !crops || !logits) ocr::fail(OCR_ERR_INVALID, "null argument");
    if (n < 0) ocr::fail(OCR_ERR_INVALID, "negative crop count");
    if (mem_kind == OCR_MEM_HOST) rec->impl.forward_host(crops, n, logits, nullptr, nullptr);
    else {
      rec->impl.classify(crops, n, logits, nullptr, nullptr);
      rec->impl.synchronize();
    }
  });
}
int ocr_rec_classify_async(ocr_rec_t* rec, const float* crops, int n, float* logits, int32_t* labels, double* probs) {
  return guard([&] {
    if (!rec) ocr::fail(OCR_ERR_INVALID, "null handle");
    rec->impl.classify(crops, n, logits, labels, probs);
  });
}
int ocr_rec_classify_profile(ocr_rec_t* rec, const float* crops, int n, int32_t* labels, double* probs, int max_entries,
                             const char** names, float* ms, double* flops, double* bytes, int* n_entries) {
  return guard([&] {
    if (!rec || !n_entries) ocr::fail(OCR_ERR_INVALID, "null argument");
    std::vector<ocr::ProfileEntry> prof;
    rec->impl.classify(crops, n, nullptr, labels, probs, &prof);
    const int k = std::min<int>(max_entries, (int)prof.size());
    for (int i = 0; i < k; ++i) {
      if (names) names[i] = prof[i].name;
      if (ms) ms[i] = prof[i].ms;
      if (flops) flops[i] = prof[i].flops;
      if (bytes) bytes[i] = prof[i].bytes;
    }
    *n_entries = k;
  });
}
int ocr_rec_classify(ocr_rec_t* rec, const float* crops, int n, int32_t* labels, double* probs, int mem_kind) {
  return guard([&] {
    if (!rec || !crops) ocr::fail(OCR_ERR_INVALID, "null argument");
    if (n < 0) ocr::fail(OCR_ERR_INVALID, "negative crop count");
    if (mem_kind == OCR_MEM_HOST) rec->impl.forward_host(crops, n, nullptr, labels, probs);
    else {
      rec->impl.classify(crops, n, nullptr, labels, probs);
      rec->impl.synchronize();
    }
  });
}
int ocr_ctc_greedy_decode(ocr_rec_t* rec, const float* logits, int n, int t, int c, int blank, int mem_kind, int32_t* labels, int32_t* lengths) {
  return guard([&] {
    using namespace ocr;
    if (!rec || !logits || !labels || !lengths) fail(OCR_ERR_INVALID, "ctc_greedy_decode: null argument");
    if (mem_kind != OCR_MEM_HOST && mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "ctc_greedy_decode: mem_kind %d", mem_kind);
    if (n < 0 || t <= 0 || c <= 0 || blank < 0 || blank >= c) fail(OCR_ERR_INVALID, "ctc_greedy_decode: N=%d T=%d C=%d blank=%d", n, t, c, blank);
    if (n == 0) return;
    OCR_HIP(hipSetDevice(rec->impl.device()));
    hipStream_t s = rec->impl.stream();
    if (mem_kind == OCR_MEM_DEVICE) {   // enqueued on the handle's stream and awaited (the lengths are usually read right away)
      launch_ctc_greedy(logits, n, t, c, blank, labels, lengths, s);
      OCR_HIP(hipStreamSynchronize(s));
      return;
    }
    const CtcBlock blk({(size_t)n * t * c * 4, (size_t)n * t * 4, (size_t)n * 4});   // logits, labels, lengths
    blk.up(0, logits, s);
    launch_ctc_greedy(blk.piece<const float>(0), n, t, c, blank, blk.piece<int32_t>(1), blk.piece<int32_t>(2), s);
    blk.home(1, labels, s);
    blk.home(2, lengths, s);
    OCR_HIP(hipStreamSynchronize(s));
  });
}
int ocr_ctc_beam_decode(ocr_rec_t* rec, const float* logits, int n, int t, int c, int blank, int beam_width, int mem_kind, int32_t* labels,
                        int32_t* lengths, double* scores) {
  return guard([&] {
    using namespace ocr;
    if (!rec || !logits || !labels || !lengths || !scores) fail(OCR_ERR_INVALID, "ctc_beam_decode: null argument");
    if (mem_kind != OCR_MEM_HOST && mem_kind != OCR_MEM_DEVICE) fail(OCR_ERR_INVALID, "ctc_beam_decode: mem_kind %d", mem_kind);
    if (n < 0 || t < 1 || t > 1024 || c < 1 || c > 256 || blank < 0 || blank >= c || beam_width < 1 || beam_width > 32)
      fail(OCR_ERR_INVALID, "ctc_beam_decode: N=%d T=%d C=%d blank=%d beam_width=%d (limits: T 1..1024, C 1..256, beam_width 1..32)", n, t, c,
           blank, beam_width);
    if (n == 0) return;
    OCR_HIP(hipSetDevice(rec->impl.device()));
    hipStream_t s = rec->impl.stream();
    if (!rec->ctc_bad_crop) OCR_HIP(hipMalloc(reinterpret_cast<void**>(&rec->ctc_bad_crop), sizeof(int32_t)));
    constexpr int32_t kNone = 0x7F7F7F7F;   // what the byte memset leaves: above every crop index
    OCR_HIP(hipMemsetAsync(rec->ctc_bad_crop, 0x7F, sizeof(int32_t), s));
    int32_t bad = kNone;
    if (mem_kind == OCR_MEM_DEVICE) {   // enqueued on the handle's stream and awaited (the flag decides the return code)
      launch_ctc_beam(logits, n, t, c, blank, beam_width, labels, lengths, scores, rec->ctc_bad_crop, s);
      OCR_HIP(hipMemcpyAsync(&bad, rec->ctc_bad_crop, sizeof(bad), hipMemcpyDeviceToHost, s));
      OCR_HIP(hipStreamSynchronize(s));
    } else {
      const size_t nb = (size_t)n * beam_width;
      const CtcBlock blk({(size_t)n * t * c * 4, nb * t * 4, nb * 4, nb * 8});   // logits, labels, lengths, scores
      blk.up(0, logits, s);
      launch_ctc_beam(blk.piece<const float>(0), n, t, c, blank, beam_width, blk.piece<int32_t>(1), blk.piece<int32_t>(2), blk.piece<double>(3),
                      rec->ctc_bad_crop, s);
      OCR_HIP(hipMemcpyAsync(&bad, rec->ctc_bad_crop, sizeof(bad), hipMemcpyDeviceToHost, s));
      blk.home(1, labels, s);
      blk.home(2, lengths, s);
      blk.home(3, scores, s);
      OCR_HIP(hipStreamSynchronize(s));
    }
    if (bad != kNone) fail(OCR_ERR_INVALID, "ctc_beam_decode: non-finite logit in crop %d", bad);
  });
}
const char* ocr_rec_alphabet(void) { return "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789"; }

/* ---- multi-GPU exchange (comm.hip) */
struct ocr_comm {
  ocr::Comm* impl = nullptr;
  ~ocr_comm() { ocr::comm_destroy(impl); }
};

int ocr_comm_unique_id(uint8_t* id) {
  return guard([&] { ocr::comm_unique_id(id); });
}
int ocr_comm_rccl_version(int* version) {
  return guard([&] {
    if (!version) ocr::fail(OCR_ERR_INVALID, "null argument");
    *version = ocr::comm_rccl_version();
  });
}
int ocr_comm_create(const uint8_t* id, int world, int rank, int device, ocr_comm_t** out) {
  return guard([&] {
    if (!out) ocr::fail(OCR_ERR_INVALID, "ocr_comm_create: out is null");
    *out = nullptr;
    auto c = std::make_unique<ocr_comm>();
    c->impl = ocr::comm_create(id, world, rank, device);
    *out = c.release();
  });
}
void ocr_comm_destroy(ocr_comm_t* comm) { delete comm; }
int ocr_comm_all_gather_polygons(ocr_comm_t* comm, const ocr_polygons_t* local, ocr_polygons_t** all) {
  return guard([&] {
    if (!comm || !local || !all) ocr::fail(OCR_ERR_INVALID, "null argument");
    *all = nullptr;
    auto res = std::make_unique<PolygonsOwned>();
    ocr::comm_all_gather_polygons(comm->impl, *local, *res);
    *all = &res.release()->view;
  });
}
int ocr_comm_all_gather_labels(ocr_comm_t* comm, const int32_t* labels, int n_local, int32_t* all, int capacity,
                               int32_t* counts, int* n_all) {
  return guard([&] {
    if (!comm || !n_all) ocr::fail(OCR_ERR_INVALID, "null argument");
    std::vector<int32_t> a, c;
    ocr::comm_all_gather_labels(comm->impl, labels, n_local, a, c);
    *n_all = (int)a.size();
    if ((int)a.size() > capacity) ocr::fail(OCR_ERR_INVALID, "all_gather_labels: %zu labels, capacity %d", a.size(), capacity);
    if (!a.empty()) {
      if (!all) ocr::fail(OCR_ERR_INVALID, "null label buffer");
      std::memcpy(all, a.data(), a.size() * 4);
    }
    if (counts) std::memcpy(counts, c.data(), c.size() * 4);
  });
}

}  // extern "C"
