// Word strips: the host geometry of ocr_plan_word_strips and ocr_plan_curved_strips (word_strips.cpp; rules in include/ocr_amd.h,
// oracles tests/strip_oracle.py and tests/curved_strip_oracle.py).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/ocr_amd.h"

namespace ocr {

// the library-owned storage behind an ocr_word_strips_t* (released by ocr_word_strips_free)
struct WordStripsOwned {
  ocr_word_strips_t view;
  int32_t height = 0;
  int64_t total_width = 0;
  std::vector<int32_t> img_offsets, col_offsets, word_info;
  std::vector<double> quads, scores;
  std::vector<float> maps;
  void finish() {
    view.n_images = (int32_t)img_offsets.size() - 1;
    view.n_words = (int32_t)scores.size();
    view.height = height;
    view.total_width = (int32_t)total_width;
    view.img_offsets = img_offsets.data();
    view.col_offsets = col_offsets.data();
    view.word_info = word_info.data();
    view.quads = quads.data();
    view.maps = maps.data();
    view.scores = scores.data();
  }
};

// the library-owned storage behind an ocr_curved_strips_t* (released by ocr_curved_strips_free)
struct CurvedStripsOwned {
  ocr_curved_strips_t view;
  int32_t height = 0;
  int64_t total_width = 0;
  std::vector<int32_t> img_offsets, col_offsets, word_info;
  std::vector<float> knots, tscale;
  std::vector<double> half_heights, lengths, scores;
  void finish() {
    view.n_images = (int32_t)img_offsets.size() - 1;
    view.n_words = (int32_t)scores.size();
    view.height = height;
    view.total_width = (int32_t)total_width;
    view.img_offsets = img_offsets.data();
    view.col_offsets = col_offsets.data();
    view.word_info = word_info.data();
    view.knots = knots.data();
    view.tscale = tscale.data();
    view.half_heights = half_heights.data();
    view.lengths = lengths.data();
    view.scores = scores.data();
  }
};

constexpr int64_t kStripMaxAtlas = int64_t(1) << 31;   // atlas elements

// validates the arguments (ocr::Error OCR_ERR_INVALID) and plans every word; params already defaulted and checked
void plan_word_strips(const ocr_polygons_t& polys, const double* adj_xy, int n, const ocr_strip_params_t& p, WordStripsOwned& out);
void plan_curved_strips(const ocr_polygons_t& polys, const double* adj_xy, int n, const ocr_curve_params_t& p, CurvedStripsOwned& out);

}  // namespace ocr
