// Header-only C++ mirror of the reference's inference call sites over the C ABI
// (include/ocr_amd.h).  The reference is a Rust binary crate; Rust is not available
// in this image, so the host side above the C ABI is C++ with the reference's names,
// argument meaning and error behaviour (anyhow::Result -> ocr_rs::Error).
//
//   text_detection::resnet18(..) -> FuncT, FuncT::forward_t      model.rs:154-156, mod.rs:52-54
//   text_detection::preprocess_images                            image_ops.rs:188-220, a batch per call
//   text_detection::metrics::get_boxes_and_box_scores            metrics.rs:37-56
//   char_recognition::Net::{new_, forward_t}, utils::topk        model.rs:13-39, utils.rs:28-43
//   read_words: detected words -> glyphs -> text, the pipeline's segmentation step (README.md:20-26), which the reference never built
//   Lexicon / glyph_costs / lexicon_match / read_words(.., lexicon): words read as a whole against a word list (ocr_lexicon_match)
//   CharLm / lm_decode: words decoded under a character-bigram model from the same glyph costs, k best readings (ocr_lm_decode)
//   split_glyphs / glyph_spans / lattice_decode: wide glyphs cut into pieces, runs of pieces recognised, segmentation and classes
//     chosen together under the model (ocr_split_glyphs, ocr_glyph_spans, ocr_lattice_decode)
//   lexicon_lattice_match: the entries of a Lexicon matched over the pieces, a character reading a run of pieces (ocr_lexicon_lattice_match)
//   break_words / read_words(.., spaces): a polygon that holds several words cut at its inter-word gaps (ocr_break_words)
//   PhraseParams / phrase_match: the glyphs of a polygon segmented into lexicon words by one search (ocr_lexicon_phrase_match)
//   read_words_rectified: the same through upright word strips (ocr_plan_word_strips / ocr_extract_word_strips), for rotated words,
//     or through curved strips (ocr_plan_curved_strips / ocr_extract_curved_strips), for words that bend
//   group_lines / read_lines: the words of every page grouped into text lines in reading order (ocr_group_lines), the "output text" step
//   group_columns / read_columns: the same with columns: blocks in reading order, their lines top to bottom (ocr_group_columns)
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ocr_amd.h"

namespace ocr_rs {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
inline void check(int code) {
  if (code != OCR_OK) throw Error(code, ocr_last_error());
}

// N x C x H x W f32 host tensor (what a tch::Tensor of Kind::Float holds)
struct Tensor {
  std::vector<float> data;
  int n = 0, c = 0, h = 0, w = 0;
  Tensor() = default;
  Tensor(int n_, int c_, int h_, int w_) : data((size_t)n_ * c_ * h_ * w_), n(n_), c(c_), h(h_), w(w_) {}
};

namespace text_detection {

constexpr uint32_t DEFAULT_WIDTH = 800, DEFAULT_HEIGHT = 800;  // mod.rs:20-21

class FuncT {  // what resnet18(&nn::Path) returns
 public:
  FuncT(const void* weights, size_t bytes, int device) { check(ocr_det_create(weights, bytes, device, &h_)); }
  ~FuncT() { ocr_det_destroy(h_); }
  FuncT(const FuncT&) = delete;
  FuncT& operator=(const FuncT&) = delete;
  // ModuleT::forward_t(&self, xs, train)
  Tensor forward_t(const Tensor& xs, bool train) const {
    if (train) throw Error(OCR_ERR_INVALID, "inference-only build");
    if (xs.c != 1) throw Error(OCR_ERR_INVALID, "expected N x 1 x H x W");
    Tensor out(xs.n, 1, xs.h, xs.w);
    check(ocr_det_forward(h_, xs.data.data(), xs.n, xs.h, xs.w, out.data.data(), OCR_MEM_HOST));
    return out;
  }
  ocr_det_t* handle() const { return h_; }

 private:
  ocr_det_t* h_ = nullptr;
};
inline FuncT resnet18(const void* weights, size_t bytes, int device = 0) { return FuncT(weights, bytes, device); }

// image_ops::preprocess_image (image_ops.rs:188-220) after decoding, for a batch: every image's into_rgba() buffer (w x h, rows
// contiguous) -> N x 1 x H x W frames of raw 0..255 luma (the input of forward_t) and the adjust values x0, y0, x1, y1, ...
struct RgbaImage {
  const uint8_t* data;
  uint32_t width, height;
};
inline Tensor preprocess_images(const FuncT& net, const std::vector<RgbaImage>& images, std::vector<double>& adjust_values,
                                uint32_t width = DEFAULT_WIDTH, uint32_t height = DEFAULT_HEIGHT) {
  std::vector<ocr_image_t> descs(images.size());
  for (size_t i = 0; i < images.size(); ++i) descs[i] = {images[i].data, (int32_t)images[i].width, (int32_t)images[i].height, 0};
  Tensor out((int)images.size(), 1, (int)height, (int)width);
  adjust_values.assign(2 * images.size(), 0.0);
  check(ocr_preprocess_batch(net.handle(), descs.data(), (int)descs.size(), OCR_MEM_HOST, (int)width, (int)height, nullptr, out.data.data(),
                             OCR_MEM_HOST, adjust_values.data()));
  return out;
}

namespace metrics {
using Polygon = std::vector<std::pair<uint32_t, uint32_t>>;
using MultiPolygon = std::vector<Polygon>;
struct PolygonScores {  // metrics.rs:32-35
  std::vector<MultiPolygon> polygons;
  std::vector<std::vector<double>> scores;
};
// get_boxes_and_box_scores(pred: &Tensor, adjust_values: &Tensor) -> Result<PolygonScores>
inline PolygonScores get_boxes_and_box_scores(const FuncT& net, const Tensor& pred, const std::vector<double>& adjust_values) {
  if ((int)adjust_values.size() != 2 * pred.n) throw Error(OCR_ERR_INVALID, "adjust_values must be N x 2");
  ocr_polygons_t* r = nullptr;
  check(ocr_det_postprocess(net.handle(), pred.data.data(), pred.n, pred.h, pred.w, OCR_MEM_HOST, adjust_values.data(), nullptr, &r));
  PolygonScores out;
  for (int b = 0; b < r->n_images; ++b) {
    MultiPolygon mp;
    std::vector<double> sc;
    for (int k = r->img_offsets[b]; k < r->img_offsets[b + 1]; ++k) {
      Polygon p;
      for (int v = r->poly_offsets[k]; v < r->poly_offsets[k + 1]; ++v) p.emplace_back(r->xy[2 * v], r->xy[2 * v + 1]);
      mp.push_back(std::move(p));
      sc.push_back(r->scores[k]);
    }
    out.polygons.push_back(std::move(mp));
    out.scores.push_back(std::move(sc));
  }
  ocr_polygons_free(r);
  return out;
}
}  // namespace metrics
}  // namespace text_detection

namespace utils {
inline const char* VALUES() { return ocr_rec_alphabet(); }  // utils.rs:7
}

namespace char_recognition {
class Net {
 public:
  Net(const void* weights, size_t bytes, int device = 0) { check(ocr_rec_create(weights, bytes, device, &h_)); }
  ~Net() { ocr_rec_destroy(h_); }
  Net(const Net&) = delete;
  Net& operator=(const Net&) = delete;
  // forward_t: xs.view([-1, 1, 28, 28]) ... fc2 -> N x 62 logits
  std::vector<float> forward_t(const std::vector<float>& xs, bool train) const {
    if (train) throw Error(OCR_ERR_INVALID, "inference-only build");
    if (xs.size() % 784 != 0) throw Error(OCR_ERR_INVALID, "shape is invalid for view([-1, 1, 28, 28])");
    const int n = (int)(xs.size() / 784);
    std::vector<float> logits((size_t)n * 62);
    check(ocr_rec_forward(h_, xs.data(), n, logits.data(), OCR_MEM_HOST));
    return logits;
  }
  // run_prediction's tail: softmax(-1, Double) + topk(.., 1)[0]  (mod.rs:53-56)
  std::vector<std::pair<char, double>> predict(const std::vector<float>& xs) const {
    const int n = (int)(xs.size() / 784);
    std::vector<int32_t> labels(n);
    std::vector<double> probs(n);
    check(ocr_rec_classify(h_, xs.data(), n, labels.data(), probs.data(), OCR_MEM_HOST));
    std::vector<std::pair<char, double>> out;
    for (int i = 0; i < n; ++i) out.emplace_back(utils::VALUES()[labels[i]], probs[i]);
    return out;
  }
  ocr_rec_t* handle() const { return h_; }

 private:
  ocr_rec_t* h_ = nullptr;
};
}  // namespace char_recognition

// One detected word read glyph by glyph: its text (VALUES), the probability of every character, the glyph boxes (x0, y0, x1, y1
// frame pixels, half-open).
// With the `spaces` option the text carries one space in front of every inner word of the polygon, starts holds the sub-word ranges
// inside the polygon's glyphs (S + 1 values) and gap_pct the gap in front of every sub-word (S values, 0 first); both stay empty without it.
struct WordReading {
  std::string text;
  std::vector<double> probs;
  std::vector<std::array<int32_t, 4>> boxes;
  std::vector<int32_t> starts, gap_pct;
};
// ocr_break_words for the readers: per word of `g` its sub-word range (sub_offsets), per sub-word its first glyph (starts, batch
// glyph indices, n_glyphs appended) and the gap in front of it.
struct WordSpaces {
  std::vector<int32_t> sub_offsets, starts, gap_pct;
  // word k of the block the breaks were made of -> (starts relative to the word's first glyph, gap_pct)
  void of_word(int k, int32_t g0, std::vector<int32_t>& rel, std::vector<int32_t>& pct) const {
    for (int s = sub_offsets[k]; s <= sub_offsets[k + 1]; ++s) rel.push_back(starts[s] - g0);
    pct.assign(gap_pct.begin() + sub_offsets[k], gap_pct.begin() + sub_offsets[k + 1]);
  }
  bool starts_inside(int k, int32_t glyph) const {   // does an inner sub-word of word k start at this glyph?
    return std::binary_search(starts.begin() + sub_offsets[k] + 1, starts.begin() + sub_offsets[k + 1], glyph);
  }
};
inline WordSpaces word_spaces(const text_detection::FuncT& det_net, const ocr_glyphs_t* g, const ocr_break_params_t* spaces) {
  ocr_glyphs_t* words = nullptr;
  ocr_word_breaks_t* wb = nullptr;
  check(ocr_break_words(det_net.handle(), g, spaces, &words, &wb));
  WordSpaces out;
  out.sub_offsets.assign(wb->sub_offsets, wb->sub_offsets + wb->n_source + 1);
  out.starts.assign(words->word_offsets, words->word_offsets + words->n_words + 1);
  out.gap_pct.assign(wb->gap_pct, wb->gap_pct + wb->n_words);
  ocr_glyphs_free(words);
  ocr_word_breaks_free(wb);
  return out;
}
// The two glyph calls of both readers over host memory: the column rule (cc == nullptr), connected components (cc), or connected
// components with every crop masked by its glyph's components (cc and mask: ocr_segment_glyphs_cc_labelled ->
// ocr_extract_glyph_crops_masked; the label planes live on the GPU between the two calls).  mask without cc is OCR_ERR_INVALID.
// *g is the caller's to free; crops is resized to n_glyphs x 784.
inline void segment_and_crop(const text_detection::FuncT& det_net, const float* frames, int n, int h, int w, const ocr_polygons_t* polys,
                             const double* adjust_values, const ocr_segment_params_t* params, const ocr_cc_params_t* cc,
                             const ocr_mask_params_t* mask, ocr_glyphs_t** g, std::vector<float>& crops) {
  if (mask && !cc) throw Error(OCR_ERR_INVALID, "mask: masked crops need the connected-component rule (pass cc)");
  ocr_glyph_labels_t* labels = nullptr;
  struct FreeLabels {
    ocr_glyph_labels_t*& l;
    ~FreeLabels() { ocr_glyph_labels_free(l); }
  } free_l{labels};
  if (mask)
    check(ocr_segment_glyphs_cc_labelled(det_net.handle(), frames, n, h, w, OCR_MEM_HOST, polys, adjust_values, params, cc, g, &labels));
  else
    check(cc ? ocr_segment_glyphs_cc(det_net.handle(), frames, n, h, w, OCR_MEM_HOST, polys, adjust_values, params, cc, g)
             : ocr_segment_glyphs(det_net.handle(), frames, n, h, w, OCR_MEM_HOST, polys, adjust_values, params, g));
  crops.resize((size_t)(*g)->n_glyphs * 784);
  if ((*g)->n_glyphs == 0) return;
  check(mask ? ocr_extract_glyph_crops_masked(det_net.handle(), frames, n, h, w, OCR_MEM_HOST, *g, labels, params, mask, crops.data())
             : ocr_extract_glyph_crops(det_net.handle(), frames, n, h, w, OCR_MEM_HOST, *g, params, crops.data()));
}

// ocr_segment_glyphs -> ocr_extract_glyph_crops -> ocr_rec_classify over host memory: per image, per polygon of `ps`.  frames are the
// detector's input (N x 1 x H x W, raw 0..255), adjust_values N x 2 as given to get_boxes_and_box_scores; params == nullptr: defaults.
// cc == nullptr segments by the column rule; a pointer (see ocr_cc_default_params) segments by connected components
// (ocr_segment_glyphs_cc), which splits kerned letters.  mask == nullptr cuts every crop from its box alone; a pointer (see
// ocr_mask_default_params) needs cc and keeps a kerned neighbour's ink out of every crop (segment_and_crop).
inline std::vector<std::vector<WordReading>> read_words(const text_detection::FuncT& det_net, const char_recognition::Net& rec_net,
                                                        const Tensor& frames, const text_detection::metrics::PolygonScores& ps,
                                                        const std::vector<double>& adjust_values,
                                                        const ocr_segment_params_t* params = nullptr,
                                                        const ocr_cc_params_t* cc = nullptr,
                                                        const ocr_mask_params_t* mask = nullptr,
                                                        const ocr_break_params_t* spaces = nullptr) {
  if (frames.c != 1) throw Error(OCR_ERR_INVALID, "expected N x 1 x H x W");
  if ((int)ps.polygons.size() != frames.n || (int)adjust_values.size() != 2 * frames.n)
    throw Error(OCR_ERR_INVALID, "polygons / adjust_values do not match the frames");
  std::vector<int32_t> img_off{0}, poly_off{0};
  std::vector<uint32_t> xy;
  std::vector<double> scores;
  for (const auto& mp : ps.polygons) {
    for (const auto& p : mp) {
      for (const auto& v : p) {
        xy.push_back(v.first);
        xy.push_back(v.second);
      }
      poly_off.push_back((int32_t)(xy.size() / 2));
      scores.push_back(0.0);
    }
    img_off.push_back((int32_t)scores.size());
  }
  const ocr_polygons_t polys{frames.n, (int32_t)scores.size(), (int32_t)(xy.size() / 2), img_off.data(), poly_off.data(), xy.data(),
                             scores.data()};
  ocr_glyphs_t* g = nullptr;
  struct Free {
    ocr_glyphs_t*& g;
    ~Free() { ocr_glyphs_free(g); }
  } free_g{g};
  std::vector<float> crops;
  segment_and_crop(det_net, frames.data.data(), frames.n, frames.h, frames.w, &polys, adjust_values.data(), params, cc, mask, &g, crops);
  const int ng = g->n_glyphs;
  std::vector<int32_t> labels(ng);
  std::vector<double> probs(ng);
  if (ng > 0) {
    check(ocr_rec_classify(rec_net.handle(), crops.data(), ng, labels.data(), probs.data(), OCR_MEM_HOST));
  }
  WordSpaces sp;
  if (spaces) sp = word_spaces(det_net, g, spaces);
  std::vector<std::vector<WordReading>> out(frames.n);
  for (int b = 0; b < frames.n; ++b) {
    for (int k = g->img_offsets[b]; k < g->img_offsets[b + 1]; ++k) {
      WordReading r;
      if (spaces) sp.of_word(k, g->word_offsets[k], r.starts, r.gap_pct);
      for (int j = g->word_offsets[k]; j < g->word_offsets[k + 1]; ++j) {
        if (spaces && sp.starts_inside(k, j)) r.text.push_back(' ');
        r.text.push_back(utils::VALUES()[labels[j]]);
        r.probs.push_back(probs[j]);
        r.boxes.push_back({g->boxes[4 * j], g->boxes[4 * j + 1], g->boxes[4 * j + 2], g->boxes[4 * j + 3]});
      }
      out[b].push_back(std::move(r));
    }
  }
  return out;
}

// ---- lexicon matching (ocr_rec_glyph_costs, ocr_lexicon_create, ocr_lexicon_match; the rule is stated in ocr_amd.h)
// A word list over VALUES, uploaded once to the recogniser's GPU; results name the indices of `words`.
class Lexicon {
 public:
  Lexicon(const char_recognition::Net& rec_net, std::vector<std::string> words) : words_(std::move(words)) {
    std::string bytes;
    std::vector<int32_t> offsets{0};
    for (const auto& w : words_) {
      bytes += w;
      offsets.push_back((int32_t)bytes.size());
    }
    check(ocr_lexicon_create(rec_net.handle(), bytes.data(), offsets.data(), (int)words_.size(), &h_));
  }
  ~Lexicon() { ocr_lexicon_destroy(h_); }
  Lexicon(const Lexicon&) = delete;
  Lexicon& operator=(const Lexicon&) = delete;
  const std::vector<std::string>& words() const { return words_; }
  const ocr_lexicon_t* handle() const { return h_; }

 private:
  std::vector<std::string> words_;
  ocr_lexicon_t* h_ = nullptr;
};
// logits n x 62 (forward_t) -> costs n x 62: the negative log-softmax, computed in f64
inline std::vector<float> glyph_costs(const char_recognition::Net& rec_net, const std::vector<float>& logits) {
  if (logits.size() % 62 != 0) throw Error(OCR_ERR_INVALID, "logits are not n x 62");
  std::vector<float> costs(logits.size());
  if (!logits.empty()) check(ocr_rec_glyph_costs(rec_net.handle(), logits.data(), (int)(logits.size() / 62), costs.data(), OCR_MEM_HOST));
  return costs;
}
// entries / costs are n_words x top_k (-1 / +inf past the candidates); the other three are per word
struct LexiconMatches {
  int top_k = 1;
  std::vector<int32_t> entries, n_candidates, word_flags;
  std::vector<double> costs, raw_costs;
};
inline LexiconMatches lexicon_match(const char_recognition::Net& rec_net, const Lexicon& lex, const std::vector<float>& costs,
                                    const std::vector<int32_t>& word_offsets, const ocr_lexicon_params_t* params = nullptr) {
  if (word_offsets.empty() || costs.size() != 62 * (size_t)word_offsets.back()) throw Error(OCR_ERR_INVALID, "costs do not match the word offsets");
  ocr_lexicon_matches_t* m = nullptr;
  check(ocr_lexicon_match(rec_net.handle(), lex.handle(), costs.empty() ? nullptr : costs.data(), (int)(costs.size() / 62), OCR_MEM_HOST,
                          word_offsets.data(), (int)word_offsets.size() - 1, params, &m));
  LexiconMatches out;
  const size_t nw = (size_t)m->n_words, k = (size_t)m->top_k;
  out.top_k = m->top_k;
  out.entries.assign(m->entries, m->entries + nw * k);
  out.costs.assign(m->costs, m->costs + nw * k);
  out.raw_costs.assign(m->raw_costs, m->raw_costs + nw);
  out.n_candidates.assign(m->n_candidates, m->n_candidates + nw);
  out.word_flags.assign(m->word_flags, m->word_flags + nw);
  ocr_lexicon_matches_free(m);
  return out;
}
// ocr_lexicon_phrase_match: the glyphs of every line (a polygon's glyphs) segmented into lexicon words and out-of-vocabulary words by
// one search over the glyph costs.  PhraseParams starts from ocr_phrase_default_params; bound_cost and join_cost are per glyph (both
// empty: zeros).  word_offsets is an ordinary offset array over the glyph rows: lm_decode and lexicon_match take it.
struct PhraseParams : ocr_phrase_params_t {
  PhraseParams() { ocr_phrase_default_params(this); }
};
struct PhraseMatches {
  std::vector<int32_t> line_word_offsets, word_offsets, entries, line_flags;   // entries: -1 for an out-of-vocabulary word
  std::vector<double> word_costs, line_costs, raw_costs;
  // the text of line l: an entry's string for a lexicon word, raw[a, b) (the per-glyph reading of the whole block) for any other
  std::string text(const Lexicon& lex, const std::string& raw, size_t l) const {
    std::string out;
    for (int32_t w = line_word_offsets[l]; w < line_word_offsets[l + 1]; ++w) {
      if (w > line_word_offsets[l]) out += ' ';
      out += entries[w] >= 0 ? lex.words()[entries[w]] : raw.substr((size_t)word_offsets[w], (size_t)(word_offsets[w + 1] - word_offsets[w]));
    }
    return out;
  }
};
inline PhraseMatches phrase_match(const char_recognition::Net& rec_net, const Lexicon& lex, const std::vector<float>& costs,
                                  const std::vector<int32_t>& line_offsets, const std::vector<float>& bound_cost = {},
                                  const std::vector<float>& join_cost = {}, const ocr_phrase_params_t* params = nullptr) {
  if (line_offsets.empty() || costs.size() != 62 * (size_t)line_offsets.back()) throw Error(OCR_ERR_INVALID, "costs do not match the line offsets");
  const size_t ng = costs.size() / 62;
  const bool gaps = !bound_cost.empty() || !join_cost.empty();
  if (gaps && (bound_cost.size() != ng || join_cost.size() != ng)) throw Error(OCR_ERR_INVALID, "gap costs do not match the glyphs");
  ocr_phrase_matches_t* m = nullptr;
  check(ocr_lexicon_phrase_match(rec_net.handle(), lex.handle(), costs.empty() ? nullptr : costs.data(), (int)ng, OCR_MEM_HOST,
                                 line_offsets.data(), (int)line_offsets.size() - 1, gaps ? bound_cost.data() : nullptr,
                                 gaps ? join_cost.data() : nullptr, params, &m));
  PhraseMatches out;
  const size_t nl = (size_t)m->n_lines, nw = (size_t)m->n_words;
  out.line_word_offsets.assign(m->line_word_offsets, m->line_word_offsets + nl + 1);
  out.word_offsets.assign(m->word_offsets, m->word_offsets + nw + 1);
  out.entries.assign(m->entries, m->entries + nw);
  out.word_costs.assign(m->word_costs, m->word_costs + nw);
  out.line_costs.assign(m->line_costs, m->line_costs + nl);
  out.raw_costs.assign(m->raw_costs, m->raw_costs + nl);
  out.line_flags.assign(m->line_flags, m->line_flags + nl);
  ocr_phrase_matches_free(m);
  return out;
}
// A word read against a lexicon: text is the best entry's string when a candidate exists and cost - raw_cost <= max_penalty * G for
// its G glyphs, otherwise the raw reading; entry is the best candidate's index (-1 without one) with its cost, whether taken or not.
struct WordReadingLexicon : WordReading {
  int32_t entry = -1;
  double cost = 0, raw_cost = 0;
  std::string raw_text;
};
// read_words with a lexicon.  Over host memory the plain overload runs first and the glyph calls and the recogniser run a second
// time for the logits (ocr_rec_forward); callers with device-resident crops use ocr_rec_classify_async, which writes labels and
// logits in one pass, as reading.py does.
inline std::vector<std::vector<WordReadingLexicon>> read_words(const text_detection::FuncT& det_net, const char_recognition::Net& rec_net,
                                                               const Tensor& frames, const text_detection::metrics::PolygonScores& ps,
                                                               const std::vector<double>& adjust_values, const Lexicon& lexicon,
                                                               const ocr_lexicon_params_t* lexicon_params = nullptr, double max_penalty = 1.5,
                                                               const ocr_segment_params_t* params = nullptr,
                                                               const ocr_cc_params_t* cc = nullptr, const ocr_mask_params_t* mask = nullptr) {
  const auto plain = read_words(det_net, rec_net, frames, ps, adjust_values, params, cc, mask);
  std::vector<float> crops_flat;
  std::vector<int32_t> word_offsets{0};
  // the two glyph calls again for the crops and the word offsets, which the plain overload does not return
  std::vector<int32_t> img_off{0}, poly_off{0};
  std::vector<uint32_t> xy;
  std::vector<double> scores;
  for (const auto& mp : ps.polygons) {
    for (const auto& p : mp) {
      for (const auto& v : p) {
        xy.push_back(v.first);
        xy.push_back(v.second);
      }
      poly_off.push_back((int32_t)(xy.size() / 2));
      scores.push_back(0.0);
    }
    img_off.push_back((int32_t)scores.size());
  }
  const ocr_polygons_t polys{frames.n, (int32_t)scores.size(), (int32_t)(xy.size() / 2), img_off.data(), poly_off.data(), xy.data(),
                             scores.data()};
  ocr_glyphs_t* g = nullptr;
  struct Free {
    ocr_glyphs_t*& g;
    ~Free() { ocr_glyphs_free(g); }
  } free_g{g};
  segment_and_crop(det_net, frames.data.data(), frames.n, frames.h, frames.w, &polys, adjust_values.data(), params, cc, mask, &g, crops_flat);
  word_offsets.assign(g->word_offsets, g->word_offsets + g->n_words + 1);
  const std::vector<float> logits = g->n_glyphs ? rec_net.forward_t(crops_flat, false) : std::vector<float>();
  const LexiconMatches m = lexicon_match(rec_net, lexicon, glyph_costs(rec_net, logits), word_offsets, lexicon_params);
  std::vector<std::vector<WordReadingLexicon>> out(frames.n);
  size_t k = 0;
  for (int b = 0; b < frames.n; ++b) {
    for (const auto& w : plain[b]) {
      WordReadingLexicon r;
      static_cast<WordReading&>(r) = w;
      r.raw_text = w.text;
      r.entry = m.entries[k * m.top_k];
      r.cost = m.costs[k * m.top_k];
      r.raw_cost = m.raw_costs[k];
      if (r.entry >= 0 && r.cost - r.raw_cost <= max_penalty * (double)w.text.size()) r.text = lexicon.words()[r.entry];
      out[b].push_back(std::move(r));
      ++k;
    }
  }
  return out;
}

// ---- character language model (ocr_char_lm_create, ocr_lm_decode; the rule is stated in ocr_amd.h)
// A 64 x 64 table of transition costs over VALUES (row 62 begin-of-word, column 62 end-of-word), uploaded once to the recogniser's GPU.
class CharLm {
 public:
  CharLm(const char_recognition::Net& rec_net, const std::vector<float>& table) {
    if (table.size() != 64 * 64) throw Error(OCR_ERR_INVALID, "the model is not 64 x 64");
    check(ocr_char_lm_create(rec_net.handle(), table.data(), &h_));
  }
  ~CharLm() { ocr_char_lm_destroy(h_); }
  CharLm(const CharLm&) = delete;
  CharLm& operator=(const CharLm&) = delete;
  const ocr_char_lm_t* handle() const { return h_; }

 private:
  ocr_char_lm_t* h_ = nullptr;
};
// labels are top_k x n_glyphs (-1 in the rows of words that were not decoded), costs n_words x top_k (+inf for such words); the
// other two are per word
struct LmPaths {
  int top_k = 1, n_glyphs = 0;
  std::vector<int32_t> labels, word_flags;
  std::vector<double> costs, raw_costs;
  // hypothesis k of the word with glyph rows [g0, g1): "" when it was not decoded
  std::string text(int32_t g0, int32_t g1, int k = 0) const {
    std::string t;
    for (int32_t j = g0; j < g1; ++j) {
      const int32_t c = labels[(size_t)k * n_glyphs + j];
      if (c < 0) return std::string();
      t.push_back(utils::VALUES()[c]);
    }
    return t;
  }
};
inline LmPaths lm_decode(const char_recognition::Net& rec_net, const CharLm& lm, const std::vector<float>& costs,
                         const std::vector<int32_t>& word_offsets, const ocr_lm_params_t* params = nullptr) {
  if (word_offsets.empty() || costs.size() != 62 * (size_t)word_offsets.back()) throw Error(OCR_ERR_INVALID, "costs do not match the word offsets");
  ocr_lm_paths_t* m = nullptr;
  check(ocr_lm_decode(rec_net.handle(), lm.handle(), costs.empty() ? nullptr : costs.data(), (int)(costs.size() / 62), OCR_MEM_HOST,
                      word_offsets.data(), (int)word_offsets.size() - 1, params, &m));
  LmPaths out;
  const size_t nw = (size_t)m->n_words, k = (size_t)m->top_k, ng = (size_t)m->n_glyphs;
  out.top_k = m->top_k;
  out.n_glyphs = m->n_glyphs;
  out.labels.assign(m->labels, m->labels + k * ng);
  out.costs.assign(m->costs, m->costs + nw * k);
  out.raw_costs.assign(m->raw_costs, m->raw_costs + nw);
  out.word_flags.assign(m->word_flags, m->word_flags + nw);
  ocr_lm_paths_free(m);
  return out;
}

// ---- segmentation lattice (ocr_split_glyphs, ocr_glyph_spans, ocr_lattice_decode; the rules are stated in ocr_amd.h)
// A glyph block owned by the library (ocr_glyphs_free): what split_glyphs and glyph_spans return and every crop call takes.
struct GlyphBlock {
  ocr_glyphs_t* g = nullptr;
  GlyphBlock() = default;
  explicit GlyphBlock(ocr_glyphs_t* p) : g(p) {}
  GlyphBlock(GlyphBlock&& o) noexcept : g(o.g) { o.g = nullptr; }
  GlyphBlock& operator=(GlyphBlock&& o) noexcept {
    std::swap(g, o.g);
    return *this;
  }
  GlyphBlock(const GlyphBlock&) = delete;
  GlyphBlock& operator=(const GlyphBlock&) = delete;
  ~GlyphBlock() { ocr_glyphs_free(g); }
  const ocr_glyphs_t* get() const { return g; }
};
// ocr_break_words: the words of `glyphs` (polygons) re-cut at their inter-word gaps.  words is an ordinary glyph block over the same
// boxes (every crop, split, span and decode call takes it); source names the polygon of every sub-word, sub_offsets the sub-word range
// of every polygon, gap_pct the gap in front of every sub-word, source_info per polygon hw, rule, threshold, flags.
struct WordBreaks {
  GlyphBlock words;
  std::vector<int32_t> source, sub_offsets, gap_pct;
  std::vector<std::array<int32_t, 4>> source_info;
};
inline WordBreaks break_words(const text_detection::FuncT& det_net, const ocr_glyphs_t* glyphs, const ocr_break_params_t* params = nullptr) {
  ocr_glyphs_t* w = nullptr;
  ocr_word_breaks_t* b = nullptr;
  check(ocr_break_words(det_net.handle(), glyphs, params, &w, &b));
  WordBreaks out;
  out.words = GlyphBlock(w);
  out.source.assign(b->source, b->source + b->n_words);
  out.sub_offsets.assign(b->sub_offsets, b->sub_offsets + b->n_source + 1);
  out.gap_pct.assign(b->gap_pct, b->gap_pct + b->n_words);
  for (int32_t k = 0; k < b->n_source; ++k)
    out.source_info.push_back({b->source_info[4 * k], b->source_info[4 * k + 1], b->source_info[4 * k + 2], b->source_info[4 * k + 3]});
  ocr_word_breaks_free(b);
  return out;
}
// wide glyphs of `glyphs` cut at ink minima; piece_map (optional) receives per piece (source glyph, rank in it)
inline GlyphBlock split_glyphs(const text_detection::FuncT& det_net, const Tensor& frames, const ocr_glyphs_t* glyphs,
                               const ocr_split_params_t* params = nullptr, std::vector<std::array<int32_t, 2>>* piece_map = nullptr) {
  if (frames.c != 1) throw Error(OCR_ERR_INVALID, "expected N x 1 x H x W");
  ocr_glyphs_t* pieces = nullptr;
  ocr_piece_map_t* pm = nullptr;
  check(ocr_split_glyphs(det_net.handle(), frames.data.data(), frames.n, frames.h, frames.w, OCR_MEM_HOST, glyphs, params, &pieces, &pm));
  if (piece_map) {
    piece_map->clear();
    for (int32_t i = 0; i < pm->n_pieces; ++i) piece_map->push_back({pm->glyph[i], pm->rank[i]});
  }
  ocr_piece_map_free(pm);
  return GlyphBlock(pieces);
}
// every run of 1..max_span consecutive pieces of a word, ordered by (end, length): spans.get()->word_offsets are the span offsets of
// lattice_decode, piece_offsets the piece block's word_offsets
struct GlyphSpans {
  GlyphBlock spans;
  std::vector<int32_t> span_word, span_end, span_len, span_offsets, piece_offsets;
};
inline GlyphSpans glyph_spans(const ocr_glyphs_t* pieces, int max_span) {
  ocr_glyphs_t* s = nullptr;
  ocr_span_table_t* t = nullptr;
  check(ocr_glyph_spans(pieces, max_span, &s, &t));
  GlyphSpans out;
  out.spans = GlyphBlock(s);
  out.span_word.assign(t->span_word, t->span_word + t->n_spans);
  out.span_end.assign(t->span_end, t->span_end + t->n_spans);
  out.span_len.assign(t->span_len, t->span_len + t->n_spans);
  out.piece_offsets.assign(t->piece_offsets, t->piece_offsets + t->n_words + 1);
  out.span_offsets.assign(s->word_offsets, s->word_offsets + s->n_words + 1);
  ocr_span_table_free(t);
  return out;
}
// labels and seg_len are top_k x n_pieces: class and length at the first piece of every segment, -1 / 0 elsewhere; n_chars and costs
// n_words x top_k; the other two are per word.  Hypotheses are distinct (segmentation, classes) pairs: a string may come twice.
struct LatticePaths {
  int top_k = 1, n_pieces = 0;
  std::vector<int32_t> labels, seg_len, n_chars, word_flags;
  std::vector<double> costs, raw_costs;
  // hypothesis k of the word with pieces [p0, p1): "" when it was not decoded
  std::string text(int32_t p0, int32_t p1, int k = 0) const {
    std::string t;
    for (int32_t j = p0; j < p1; ++j) {
      const int32_t c = labels[(size_t)k * n_pieces + j];
      if (c >= 0) t.push_back(utils::VALUES()[c]);
    }
    return t;
  }
};
inline LatticePaths lattice_decode(const char_recognition::Net& rec_net, const CharLm& lm, const std::vector<float>& costs,
                                   const std::vector<int32_t>& span_offsets, const std::vector<int32_t>& piece_offsets,
                                   const ocr_lattice_params_t* params = nullptr) {
  if (span_offsets.empty() || span_offsets.size() != piece_offsets.size() || costs.size() != 62 * (size_t)span_offsets.back())
    throw Error(OCR_ERR_INVALID, "costs do not match the span offsets, or the two offset arrays differ in length");
  ocr_lattice_paths_t* m = nullptr;
  check(ocr_lattice_decode(rec_net.handle(), lm.handle(), costs.empty() ? nullptr : costs.data(), (int)(costs.size() / 62), OCR_MEM_HOST,
                           span_offsets.data(), piece_offsets.data(), (int)span_offsets.size() - 1, params, &m));
  LatticePaths out;
  const size_t nw = (size_t)m->n_words, k = (size_t)m->top_k, np = (size_t)m->n_pieces;
  out.top_k = m->top_k;
  out.n_pieces = m->n_pieces;
  out.labels.assign(m->labels, m->labels + k * np);
  out.seg_len.assign(m->seg_len, m->seg_len + k * np);
  out.n_chars.assign(m->n_chars, m->n_chars + nw * k);
  out.costs.assign(m->costs, m->costs + nw * k);
  out.raw_costs.assign(m->raw_costs, m->raw_costs + nw);
  out.word_flags.assign(m->word_flags, m->word_flags + nw);
  ocr_lattice_paths_free(m);
  return out;
}
// The joint search (ocr_lexicon_lattice_match): entries matched over the pieces, a character reading a span of 1..max_span pieces.
// entries, costs and n_ins are n_words x top_k; seg_len and seg_char top_k x n_pieces (m and the entry position at the first piece of
// a segment; seg_len 0 inside a segment, -1 at a deleted piece); the others are per word.
struct LexLatMatches {
  int top_k = 1, n_pieces = 0;
  std::vector<int32_t> entries, n_candidates, word_flags, seg_len, seg_char, n_ins;
  std::vector<double> costs, raw_costs;
};
inline LexLatMatches lexicon_lattice_match(const char_recognition::Net& rec_net, const Lexicon& lex, const std::vector<float>& costs,
                                           const std::vector<int32_t>& span_offsets, const std::vector<int32_t>& piece_offsets,
                                           const ocr_lexlat_params_t* params = nullptr) {
  if (span_offsets.empty() || span_offsets.size() != piece_offsets.size() || costs.size() != 62 * (size_t)span_offsets.back())
    throw Error(OCR_ERR_INVALID, "costs do not match the span offsets, or the two offset arrays differ in length");
  ocr_lexlat_matches_t* m = nullptr;
  check(ocr_lexicon_lattice_match(rec_net.handle(), lex.handle(), costs.empty() ? nullptr : costs.data(), (int)(costs.size() / 62),
                                  OCR_MEM_HOST, span_offsets.data(), piece_offsets.data(), (int)span_offsets.size() - 1, params, &m));
  LexLatMatches out;
  const size_t nw = (size_t)m->n_words, k = (size_t)m->top_k, np = (size_t)m->n_pieces;
  out.top_k = m->top_k;
  out.n_pieces = m->n_pieces;
  out.entries.assign(m->entries, m->entries + nw * k);
  out.costs.assign(m->costs, m->costs + nw * k);
  out.raw_costs.assign(m->raw_costs, m->raw_costs + nw);
  out.n_candidates.assign(m->n_candidates, m->n_candidates + nw);
  out.word_flags.assign(m->word_flags, m->word_flags + nw);
  out.seg_len.assign(m->seg_len, m->seg_len + k * np);
  out.seg_char.assign(m->seg_char, m->seg_char + k * np);
  out.n_ins.assign(m->n_ins, m->n_ins + nw * k);
  ocr_lexlat_matches_free(m);
  return out;
}

// One detected word read through its upright strip: text, the probability of every character, and every glyph box mapped back to the
// frame as a quad (x0, y0), (x1, y0), (x1, y1), (x0, y1) of strip pixels -> TL + cs * (U / Ws) + rs * (V / Hs), f64 frame coordinates.
// starts and gap_pct as in WordReading: filled by the `spaces` option, measured on the strip.
struct WordReadingRectified {
  std::string text;
  std::vector<double> probs;
  std::vector<std::array<double, 8>> quads;
  std::vector<int32_t> starts, gap_pct;
};
// ocr_plan_word_strips -> ocr_extract_word_strips -> ocr_word_strip_polygons -> ocr_segment_glyphs -> ocr_extract_glyph_crops ->
// ocr_rec_classify over host memory (the atlas is one frame of the glyph calls, adj = (1, 1)); per image, per polygon of `ps`.
// cc and mask as in read_words: a pointer segments the atlas by connected components / masks every crop by its glyph's components.
// curved: nullptr takes the straight strips; a pointer (ocr_curve_default_params for the defaults) takes ocr_plan_curved_strips ->
// ocr_extract_curved_strips -> ocr_curved_strip_polygons instead, strip_params is then not used, and the quads follow the centreline.
inline std::vector<std::vector<WordReadingRectified>> read_words_rectified(
    const text_detection::FuncT& det_net, const char_recognition::Net& rec_net, const Tensor& frames,
    const text_detection::metrics::PolygonScores& ps, const std::vector<double>& adjust_values,
    const ocr_strip_params_t* strip_params = nullptr, const ocr_segment_params_t* params = nullptr,
    const ocr_cc_params_t* cc = nullptr, const ocr_mask_params_t* mask = nullptr, const ocr_curve_params_t* curved = nullptr,
    const ocr_break_params_t* spaces = nullptr) {
  if (frames.c != 1) throw Error(OCR_ERR_INVALID, "expected N x 1 x H x W");
  if ((int)ps.polygons.size() != frames.n || (int)adjust_values.size() != 2 * frames.n)
    throw Error(OCR_ERR_INVALID, "polygons / adjust_values do not match the frames");
  std::vector<int32_t> img_off{0}, poly_off{0};
  std::vector<uint32_t> xy;
  std::vector<double> scores;
  for (size_t b = 0; b < ps.polygons.size(); ++b) {
    for (size_t k = 0; k < ps.polygons[b].size(); ++k) {
      for (const auto& v : ps.polygons[b][k]) {
        xy.push_back(v.first);
        xy.push_back(v.second);
      }
      poly_off.push_back((int32_t)(xy.size() / 2));
      scores.push_back(b < ps.scores.size() && k < ps.scores[b].size() ? ps.scores[b][k] : 0.0);
    }
    img_off.push_back((int32_t)scores.size());
  }
  const ocr_polygons_t polys{frames.n, (int32_t)scores.size(), (int32_t)(xy.size() / 2), img_off.data(), poly_off.data(), xy.data(),
                             scores.data()};
  ocr_word_strips_t* st = nullptr;
  ocr_curved_strips_t* cst = nullptr;
  struct FreeStrips {
    ocr_word_strips_t*& s;
    ocr_curved_strips_t*& c;
    ~FreeStrips() {
      ocr_word_strips_free(s);
      ocr_curved_strips_free(c);
    }
  } free_st{st, cst};
  if (curved)
    check(ocr_plan_curved_strips(&polys, adjust_values.data(), frames.n, frames.h, frames.w, curved, &cst));
  else
    check(ocr_plan_word_strips(&polys, adjust_values.data(), frames.n, frames.h, frames.w, strip_params, &st));
  std::vector<std::vector<WordReadingRectified>> out(frames.n);
  const int hs = curved ? cst->height : st->height, tw = curved ? cst->total_width : st->total_width;
  const int32_t* st_img = curved ? cst->img_offsets : st->img_offsets;
  const int32_t* st_col = curved ? cst->col_offsets : st->col_offsets;
  if (tw == 0) return out;
  std::vector<float> atlas((size_t)hs * tw);
  ocr_polygons_t* rects = nullptr;
  if (curved) {
    check(ocr_extract_curved_strips(det_net.handle(), frames.data.data(), frames.n, frames.h, frames.w, OCR_MEM_HOST, cst, atlas.data()));
    check(ocr_curved_strip_polygons(cst, &rects));
  } else {
    check(ocr_extract_word_strips(det_net.handle(), frames.data.data(), frames.n, frames.h, frames.w, OCR_MEM_HOST, st, atlas.data()));
    check(ocr_word_strip_polygons(st, &rects));
  }
  struct FreeRects {
    ocr_polygons_t* p;
    ~FreeRects() { ocr_polygons_free(p); }
  } free_r{rects};
  const double one[2] = {1.0, 1.0};
  ocr_glyphs_t* g = nullptr;
  struct FreeGlyphs {
    ocr_glyphs_t*& g;
    ~FreeGlyphs() { ocr_glyphs_free(g); }
  } free_g{g};
  std::vector<float> crops;
  segment_and_crop(det_net, atlas.data(), 1, hs, tw, rects, one, params, cc, mask, &g, crops);
  const int ng = g->n_glyphs;
  std::vector<int32_t> labels(ng);
  std::vector<double> probs(ng);
  if (ng > 0) {
    check(ocr_rec_classify(rec_net.handle(), crops.data(), ng, labels.data(), probs.data(), OCR_MEM_HOST));
  }
  WordSpaces sp;
  if (spaces) sp = word_spaces(det_net, g, spaces);
  for (int b = 0; b < frames.n; ++b) {
    for (int k = st_img[b]; k < st_img[b + 1]; ++k) {
      const double c0 = st_col[k], ws = st_col[k + 1] - st_col[k];
      const double* q = curved ? nullptr : st->quads + 8 * (size_t)k;
      const double cux = curved ? 0 : (q[2] - q[0]) / ws, cuy = curved ? 0 : (q[3] - q[1]) / ws;
      const double rvx = curved ? 0 : (q[6] - q[0]) / hs, rvy = curved ? 0 : (q[7] - q[1]) / hs;
      const float* kn = curved ? cst->knots + 4 * OCR_CURVE_KNOTS * (size_t)k : nullptr;
      WordReadingRectified r;
      if (spaces) sp.of_word(k, g->word_offsets[k], r.starts, r.gap_pct);
      for (int j = g->word_offsets[k]; j < g->word_offsets[k + 1]; ++j) {
        if (spaces && sp.starts_inside(k, j)) r.text.push_back(' ');
        r.text.push_back(utils::VALUES()[labels[j]]);
        r.probs.push_back(probs[j]);
        const int32_t* bx = g->boxes + 4 * (size_t)j;
        const double cs[4] = {bx[0] - c0, bx[2] - c0, bx[2] - c0, bx[0] - c0}, rs[4] = {(double)bx[1], (double)bx[1], (double)bx[3], (double)bx[3]};
        std::array<double, 8> quad;
        for (int c = 0; c < 4; ++c) {
          if (!curved) {
            quad[2 * c] = (q[0] + cs[c] * cux) + rs[c] * rvx;
            quad[2 * c + 1] = (q[1] + cs[c] * cuy) + rs[c] * rvy;
            continue;
          }
          // the sampling map of ocr_extract_curved_strips in f64 from the f32 knots, at t = (x - c0) * (32 / Ws) and row offset y - Hs / 2
          const double t = cs[c] * (32.0 / ws);
          const int kr = std::min(std::max((int)t, 0), 31);
          const double f = t - kr, o = rs[c] - hs / 2.0;
          double v[4];
          for (int e = 0; e < 4; ++e) v[e] = (double)kn[4 * kr + e] + f * ((double)kn[4 * kr + 4 + e] - (double)kn[4 * kr + e]);
          quad[2 * c] = v[0] + o * v[2];
          quad[2 * c + 1] = v[1] + o * v[3];
        }
        r.quads.push_back(quad);
      }
      out[b].push_back(std::move(r));
    }
  }
  return out;
}

// ocr_group_lines: quads 8 doubles per word (TL, TR, BR, BL: the quads of ocr_word_strips_t), word_img_offsets [n_images + 1].
// line l of image b is order[line_offsets[l] .. line_offsets[l + 1]) for l in [img_offsets[b], img_offsets[b + 1]).
struct Lines {
  std::vector<int32_t> img_offsets, line_offsets, order, word_flags;
  std::vector<double> gaps;
};
inline Lines group_lines(const text_detection::FuncT& det_net, const std::vector<double>& quads, const std::vector<int32_t>& word_img_offsets,
                         const ocr_line_params_t* params = nullptr) {
  if (word_img_offsets.empty() || quads.size() != 8 * (size_t)word_img_offsets.back())
    throw Error(OCR_ERR_INVALID, "quads do not match the word offsets");
  ocr_lines_t* l = nullptr;
  check(ocr_group_lines(det_net.handle(), quads.data(), word_img_offsets.data(), (int)word_img_offsets.size() - 1, params, &l));
  Lines out;
  out.img_offsets.assign(l->img_offsets, l->img_offsets + l->n_images + 1);
  out.line_offsets.assign(l->line_offsets, l->line_offsets + l->n_lines + 1);
  out.order.assign(l->order, l->order + l->n_words);
  out.word_flags.assign(l->word_flags, l->word_flags + l->n_words);
  out.gaps.assign(l->gaps, l->gaps + l->n_words);
  ocr_lines_free(l);
  return out;
}

// One text line: the non-empty word texts joined by one space, the image's polygon indices in reading order, and in front of every
// word its gap in units of the taller neighbour's height (0 for the first word).
struct LineReading {
  std::string text;
  std::vector<int32_t> word_indices;
  std::vector<double> gaps;
};
// The quads of every detected word (ocr_plan_word_strips; always: the curved plan carries none, and word order equals polygon order in
// every reading call) and the word range of every image.
inline std::vector<double> word_quads(const Tensor& frames, const text_detection::metrics::PolygonScores& ps,
                                      const std::vector<double>& adjust_values, const ocr_strip_params_t* strip_params,
                                      std::vector<int32_t>& img_off) {
  std::vector<int32_t> poly_off{0};
  std::vector<uint32_t> xy;
  std::vector<double> scores;
  img_off.assign(1, 0);
  for (const auto& image : ps.polygons) {
    for (const auto& poly : image) {
      for (const auto& v : poly) {
        xy.push_back(v.first);
        xy.push_back(v.second);
      }
      poly_off.push_back((int32_t)(xy.size() / 2));
      scores.push_back(0.0);
    }
    img_off.push_back((int32_t)scores.size());
  }
  const ocr_polygons_t polys{frames.n, (int32_t)scores.size(), (int32_t)(xy.size() / 2), img_off.data(), poly_off.data(), xy.data(),
                             scores.data()};
  ocr_word_strips_t* st = nullptr;
  check(ocr_plan_word_strips(&polys, adjust_values.data(), frames.n, frames.h, frames.w, strip_params, &st));
  const std::vector<double> quads(st->quads, st->quads + 8 * (size_t)st->n_words);
  ocr_word_strips_free(st);
  return quads;
}
// read_words_rectified for the texts, word_quads for the quads, ocr_group_lines for the lines; per image, its lines in reading order.
inline std::vector<std::vector<LineReading>> read_lines(
    const text_detection::FuncT& det_net, const char_recognition::Net& rec_net, const Tensor& frames,
    const text_detection::metrics::PolygonScores& ps, const std::vector<double>& adjust_values,
    const ocr_line_params_t* line_params = nullptr, const ocr_strip_params_t* strip_params = nullptr,
    const ocr_segment_params_t* params = nullptr, const ocr_cc_params_t* cc = nullptr, const ocr_mask_params_t* mask = nullptr,
    const ocr_curve_params_t* curved = nullptr) {
  const auto words = read_words_rectified(det_net, rec_net, frames, ps, adjust_values, strip_params, params, cc, mask, curved);
  std::vector<int32_t> img_off;
  const std::vector<double> quads = word_quads(frames, ps, adjust_values, strip_params, img_off);
  const Lines lines = group_lines(det_net, quads, img_off, line_params);
  std::vector<std::vector<LineReading>> out(frames.n);
  for (int b = 0; b < frames.n; ++b) {
    for (int l = lines.img_offsets[b]; l < lines.img_offsets[b + 1]; ++l) {
      LineReading r;
      for (int p = lines.line_offsets[l]; p < lines.line_offsets[l + 1]; ++p) {
        const int k = lines.order[p] - img_off[b];
        const std::string& t = words[b][k].text;
        if (!t.empty()) r.text += (r.text.empty() ? "" : " ") + t;
        r.word_indices.push_back(k);
        r.gaps.push_back(lines.gaps[p]);
      }
      out[b].push_back(std::move(r));
    }
  }
  return out;
}
inline std::string page_text(const std::vector<LineReading>& lines) {
  std::string s;
  for (size_t l = 0; l < lines.size(); ++l) s += (l ? "\n" : "") + lines[l].text;
  return s;
}

// ocr_group_columns: the arguments of group_lines.  Block k of image b, for k in [img_offsets[b], img_offsets[b + 1]), is the lines
// [block_offsets[k], block_offsets[k + 1]); line l is order[line_offsets[l] .. line_offsets[l + 1]).
struct Columns {
  std::vector<int32_t> img_offsets, block_offsets, line_offsets, order, word_flags, line_flags, block_levels;
  std::vector<double> gaps, block_quads;
};
inline Columns group_columns(const text_detection::FuncT& det_net, const std::vector<double>& quads,
                             const std::vector<int32_t>& word_img_offsets, const ocr_column_params_t* params = nullptr) {
  if (word_img_offsets.empty() || quads.size() != 8 * (size_t)word_img_offsets.back())
    throw Error(OCR_ERR_INVALID, "quads do not match the word offsets");
  ocr_columns_t* c = nullptr;
  check(ocr_group_columns(det_net.handle(), quads.data(), word_img_offsets.data(), (int)word_img_offsets.size() - 1, params, &c));
  Columns out;
  out.img_offsets.assign(c->img_offsets, c->img_offsets + c->n_images + 1);
  out.block_offsets.assign(c->block_offsets, c->block_offsets + c->n_blocks + 1);
  out.line_offsets.assign(c->line_offsets, c->line_offsets + c->n_lines + 1);
  out.order.assign(c->order, c->order + c->n_words);
  out.word_flags.assign(c->word_flags, c->word_flags + c->n_words);
  out.gaps.assign(c->gaps, c->gaps + c->n_words);
  out.line_flags.assign(c->line_flags, c->line_flags + c->n_lines);
  out.block_levels.assign(c->block_levels, c->block_levels + c->n_blocks);
  out.block_quads.assign(c->block_quads, c->block_quads + 8 * (size_t)c->n_blocks);
  ocr_columns_free(c);
  return out;
}
// read_lines with columns (ocr_group_columns): per image its blocks in reading order, per block its lines top to bottom.
inline std::vector<std::vector<std::vector<LineReading>>> read_columns(
    const text_detection::FuncT& det_net, const char_recognition::Net& rec_net, const Tensor& frames,
    const text_detection::metrics::PolygonScores& ps, const std::vector<double>& adjust_values,
    const ocr_column_params_t* column_params = nullptr, const ocr_strip_params_t* strip_params = nullptr,
    const ocr_segment_params_t* params = nullptr, const ocr_cc_params_t* cc = nullptr, const ocr_mask_params_t* mask = nullptr,
    const ocr_curve_params_t* curved = nullptr) {
  const auto words = read_words_rectified(det_net, rec_net, frames, ps, adjust_values, strip_params, params, cc, mask, curved);
  std::vector<int32_t> img_off;
  const std::vector<double> quads = word_quads(frames, ps, adjust_values, strip_params, img_off);
  const Columns cols = group_columns(det_net, quads, img_off, column_params);
  std::vector<std::vector<std::vector<LineReading>>> out(frames.n);
  for (int b = 0; b < frames.n; ++b) {
    for (int k = cols.img_offsets[b]; k < cols.img_offsets[b + 1]; ++k) {
      std::vector<LineReading> block;
      for (int l = cols.block_offsets[k]; l < cols.block_offsets[k + 1]; ++l) {
        LineReading r;
        for (int p = cols.line_offsets[l]; p < cols.line_offsets[l + 1]; ++p) {
          const int w = cols.order[p] - img_off[b];
          const std::string& t = words[b][w].text;
          if (!t.empty()) r.text += (r.text.empty() ? "" : " ") + t;
          r.word_indices.push_back(w);
          r.gaps.push_back(cols.gaps[p]);
        }
        block.push_back(std::move(r));
      }
      out[b].push_back(std::move(block));
    }
  }
  return out;
}
// the lines of every block joined with "\n", the blocks separated by an empty line
inline std::string page_text(const std::vector<std::vector<LineReading>>& blocks) {
  std::string s;
  for (size_t k = 0; k < blocks.size(); ++k) s += (k ? "\n\n" : "") + page_text(blocks[k]);
  return s;
}

}  // namespace ocr_rs
