// Shared by the translation units that implement the extern "C" surface (api.hip, postprocess.hip, comm entry points) and by the
// test-hook library (test_hooks.hip -> libocr_amd_test.so, built from the same objects as libocr_amd.so).
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "engine.hpp"
#include "postproc_geom.hpp"

struct ocr_det {
  ocr::Detector impl;
  ocr_det(const void* b, size_t n, int d, const char* options = nullptr) : impl(b, n, d, options) {}
};
struct ocr_rec {
  ocr::Recognizer impl;
  int32_t* ctc_bad_crop = nullptr;   // device int of ocr_ctc_beam_decode: the lowest crop with a non-finite logit (allocated on first use)
  void* lex_ws = nullptr;            // device workspace of the lexicon and language-model calls: grown on demand
  size_t lex_ws_bytes = 0;
  ocr_rec(const void* b, size_t n, int d) : impl(b, n, d) {}
  ~ocr_rec() {
    if (ctc_bad_crop) (void)hipFree(ctc_bad_crop);
    if (lex_ws) (void)hipFree(lex_ws);
  }
};

struct ocr_char_lm {   // the character model of char_lm.hip, also read by lattice.hip
  int device = 0;
  float* dev = nullptr;   // the 64 x 64 model
  ~ocr_char_lm() {
    if (dev) {
      (void)hipSetDevice(device);
      (void)hipDeviceSynchronize();   // whatever was queued with the model has finished before its memory goes
      (void)hipFree(dev);
    }
  }
};

namespace ocr {

extern thread_local std::string g_last_error;  // what ocr_last_error() returns (api.hip)

// Nothing throws across the C boundary: every entry point runs inside guard().
template <typename F>
int guard(F&& f) {
  try {
    g_last_error.clear();
    f();
    return OCR_OK;
  } catch (const Error& e) {
    g_last_error = e.what();
    return e.code;
  } catch (const geom::DegeneratePolygon& e) {
    g_last_error = e.what();
    return OCR_ERR_DEGENERATE;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return OCR_ERR_INTERNAL;
  } catch (...) {
    g_last_error = "unknown failure";
    return OCR_ERR_INTERNAL;
  }
}

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }
// Running 256-byte-aligned offsets inside one block (a scratch slot, the pinned buffer, a device allocation): take() returns where
// the next piece starts, `end` is the size of what has been taken.  Kernels' launchers that carve a block themselves (candidates.hip)
// use the same chain, so both sides agree on where every piece lives.
struct Carve {
  size_t end = 0;
  size_t take(size_t bytes) {
    const size_t o = end;
    end = o + align256(bytes);
    return o;
  }
};
template <typename T>
T* at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }

// the recogniser's workspace of the lexicon and language-model calls (lexicon.hip, char_lm.hip): grown on demand, released with the handle
inline char* lex_workspace(ocr_rec* rec, size_t bytes) {
  if (bytes > rec->lex_ws_bytes) {
    OCR_HIP(hipStreamSynchronize(rec->impl.stream()));
    if (rec->lex_ws) OCR_HIP(hipFree(rec->lex_ws));
    rec->lex_ws = nullptr;
    rec->lex_ws_bytes = 0;
    const size_t want = bytes + bytes / 4;
    OCR_HIP(hipMalloc(&rec->lex_ws, want));
    rec->lex_ws_bytes = want;
  }
  return static_cast<char*>(rec->lex_ws);
}

// ctc_beam.hip (extension, no reference counterpart): CTC prefix beam search, one workgroup per crop; logits [n][t][c] f32 ->
// labels [n][beam][t] (-1 padded), lengths [n][beam] (-1: unused slot), scores [n][beam] f64.  *bad_crop_dev is lowered (atomicMin) to
// the index of every crop holding a non-finite logit; the caller presets it.
void launch_ctc_beam(const float* logits_dev, int n, int t, int c, int blank, int beam_width, int32_t* labels_dev, int32_t* lengths_dev,
                     double* scores_dev, int32_t* bad_crop_dev, hipStream_t s);

// the library-owned storage behind an ocr_polygons_t* (released by ocr_polygons_free)
struct PolygonsOwned {
  ocr_polygons_t view;
  std::vector<int32_t> img_offsets, poly_offsets;
  std::vector<uint32_t> xy;
  std::vector<double> scores;
  void finish() {
    view.n_images = (int32_t)img_offsets.size() - 1;
    view.n_polygons = (int32_t)scores.size();
    view.n_vertices = (int32_t)(xy.size() / 2);
    view.img_offsets = img_offsets.data();
    view.poly_offsets = poly_offsets.data();
    view.xy = xy.data();
    view.scores = scores.data();
  }
};

// the library-owned storage behind an ocr_glyphs_t* (released by ocr_glyphs_free)
struct GlyphsOwned {
  ocr_glyphs_t view;
  std::vector<int32_t> img_offsets, word_offsets, word_info, boxes;
  std::vector<float> word_levels;
  void finish() {
    view.n_images = (int32_t)img_offsets.size() - 1;
    view.n_words = (int32_t)word_offsets.size() - 1;
    view.n_glyphs = (int32_t)(boxes.size() / 4);
    view.img_offsets = img_offsets.data();
    view.word_offsets = word_offsets.data();
    view.word_info = word_info.data();
    view.word_levels = word_levels.data();
    view.boxes = boxes.data();
  }
};

// the library-owned storage behind an ocr_lines_t* (released by ocr_lines_free)
struct LinesOwned {
  ocr_lines_t view;
  std::vector<int32_t> img_offsets, line_offsets, order, word_flags;
  std::vector<double> gaps;
  void finish() {
    view.n_images = (int32_t)img_offsets.size() - 1;
    view.n_words = (int32_t)order.size();
    view.n_lines = (int32_t)line_offsets.size() - 1;
    view.img_offsets = img_offsets.data();
    view.line_offsets = line_offsets.data();
    view.order = order.data();
    view.word_flags = word_flags.data();
    view.gaps = gaps.data();
  }
};

// the library-owned storage behind an ocr_columns_t* (released by ocr_columns_free)
struct ColumnsOwned {
  ocr_columns_t view;
  std::vector<int32_t> img_offsets, block_offsets, line_offsets, order, word_flags, line_flags, block_levels;
  std::vector<double> gaps, block_quads;
  void finish() {
    view.n_images = (int32_t)img_offsets.size() - 1;
    view.n_words = (int32_t)order.size();
    view.n_lines = (int32_t)line_offsets.size() - 1;
    view.n_blocks = (int32_t)block_offsets.size() - 1;
    view.img_offsets = img_offsets.data();
    view.block_offsets = block_offsets.data();
    view.line_offsets = line_offsets.data();
    view.order = order.data();
    view.word_flags = word_flags.data();
    view.gaps = gaps.data();
    view.line_flags = line_flags.data();
    view.block_levels = block_levels.data();
    view.block_quads = block_quads.data();
  }
};

// comm.hip
class Comm;
std::vector<uint8_t> pack_shard(const ocr_polygons_t& p);
void assemble_shards(const uint8_t* const* shards, const size_t* bytes, int world, PolygonsOwned& out);
void comm_unique_id(uint8_t* id128);
int comm_rccl_version();
Comm* comm_create(const uint8_t* id, int world, int rank, int device);
void comm_destroy(Comm* c);
int comm_world(const Comm* c);
int comm_rank(const Comm* c);
void comm_all_gather_polygons(Comm* c, const ocr_polygons_t& local, PolygonsOwned& out);
void comm_all_gather_labels(Comm* c, const int32_t* labels, int n_local, std::vector<int32_t>& all, std::vector<int32_t>& counts);

}  // namespace ocr
