// Word strips: the host geometry of ocr_plan_word_strips (word_strips.cpp; rule in include/ocr_amd.h, oracle tests/strip_oracle.py).
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

constexpr int64_t kStripMaxAtlas = int64_t(1) << 31;   // atlas elements

// validates the arguments (ocr::Error OCR_ERR_INVALID) and plans every word; params already defaulted and checked
void plan_word_strips(const ocr_polygons_t& polys, const double* adj_xy, int n, const ocr_strip_params_t& p, WordStripsOwned& out);

}  // namespace ocr
