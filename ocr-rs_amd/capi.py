"""ctypes binding of include/ocr_amd.h (the same C ABI the Rust shim of
INTEGRATION.md binds).  No torch types cross this boundary: device tensors are
passed as raw pointers (`tensor.data_ptr()`).

The product has NO CPU fallback: every compute entry point needs libocr_amd.so
and a gfx950 device and raises OcrError otherwise.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OCR_AMD_LIB") or os.path.join(_HERE, "lib", "libocr_amd.so")

MEM_HOST, MEM_DEVICE = 0, 1
ELEM_F32, ELEM_U8 = 0, 1
PRECISION_F32, PRECISION_BF16 = 0, 1

EXPORTS = [
    "ocr_last_error", "ocr_version", "ocr_device_count",
    "ocr_varstore_to_blob", "ocr_blob_free", "ocr_det_create_from_varstore", "ocr_rec_create_from_varstore",
    "ocr_det_create", "ocr_det_create_with_options", "ocr_det_destroy", "ocr_det_set_stream", "ocr_det_set_precision", "ocr_det_forward",
    "ocr_det_forward_u8", "ocr_host_alloc", "ocr_host_free", "ocr_det_detect_pipelined_host",
    "ocr_det_forward_async", "ocr_det_synchronize", "ocr_det_last_front_split", "ocr_det_last_top_side", "ocr_det_forward_profile",
    "ocr_preprocess_image", "ocr_preprocess_batch", "ocr_preprocess_batch_async", "ocr_postproc_default_params", "ocr_det_postprocess", "ocr_det_post_stats", "ocr_det_detect_pipelined", "ocr_polygons_free",
    "ocr_extract_crops", "ocr_segment_default_params", "ocr_segment_glyphs", "ocr_extract_glyph_crops", "ocr_glyphs_free",
    "ocr_cc_default_params", "ocr_segment_glyphs_cc",
    "ocr_mask_default_params", "ocr_segment_glyphs_cc_labelled", "ocr_glyph_labels_read", "ocr_extract_glyph_crops_masked",
    "ocr_glyph_labels_free",
    "ocr_strip_default_params", "ocr_plan_word_strips", "ocr_extract_word_strips", "ocr_word_strip_polygons", "ocr_word_strips_free",
    "ocr_curve_default_params", "ocr_plan_curved_strips", "ocr_extract_curved_strips", "ocr_curved_strip_polygons", "ocr_curved_strips_free",
    "ocr_line_default_params", "ocr_group_lines", "ocr_lines_free",
    "ocr_column_default_params", "ocr_group_columns", "ocr_columns_free",
    "ocr_evaluate_image", "ocr_combine_results",
    "ocr_rec_create", "ocr_rec_destroy", "ocr_rec_set_stream", "ocr_rec_set_options", "ocr_rec_synchronize",
    "ocr_rec_forward", "ocr_rec_classify_async", "ocr_rec_classify_profile", "ocr_rec_classify", "ocr_rec_alphabet", "ocr_ctc_greedy_decode",
    "ocr_rec_glyph_costs", "ocr_lexicon_create", "ocr_lexicon_size", "ocr_lexicon_destroy", "ocr_lexicon_default_params", "ocr_lexicon_match",
    "ocr_lexicon_matches_free",
    "ocr_char_lm_create", "ocr_char_lm_destroy", "ocr_lm_default_params", "ocr_lm_decode", "ocr_lm_paths_free",
    "ocr_split_default_params", "ocr_split_glyphs", "ocr_piece_map_free", "ocr_glyph_spans", "ocr_span_table_free",
    "ocr_lattice_default_params", "ocr_lattice_decode", "ocr_lattice_paths_free",
    "ocr_lexlat_default_params", "ocr_lexicon_lattice_match", "ocr_lexlat_matches_free",
    "ocr_break_default_params", "ocr_break_words", "ocr_word_breaks_free",
    "ocr_phrase_default_params", "ocr_lexicon_phrase_match", "ocr_phrase_matches_free",
    "ocr_ctc_beam_decode",
    "ocr_comm_unique_id", "ocr_comm_rccl_version", "ocr_comm_create", "ocr_comm_destroy",
    "ocr_comm_all_gather_polygons", "ocr_comm_all_gather_labels",
]


class OcrError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"ocr_amd error {code}: {msg}")
        self.code = code


class PostprocParams(C.Structure):
    _fields_ = [("thresh", C.c_double), ("box_thresh", C.c_double), ("min_size", C.c_double),
                ("unclip_ratio", C.c_double), ("skip_degenerate", C.c_int32), ("reserved", C.c_int32)]


class MetricsItem(C.Structure):
    _fields_ = [("precision", C.c_double), ("recall", C.c_double), ("hmean", C.c_double),
                ("gt_care", C.c_int32), ("det_care", C.c_int32), ("det_matched", C.c_int32)]


class Polygons(C.Structure):
    _fields_ = [("n_images", C.c_int32), ("n_polygons", C.c_int32), ("n_vertices", C.c_int32),
                ("img_offsets", C.POINTER(C.c_int32)), ("poly_offsets", C.POINTER(C.c_int32)),
                ("xy", C.POINTER(C.c_uint32)), ("scores", C.POINTER(C.c_double))]


class ImageDesc(C.Structure):
    """ocr_image_t: h rows of w RGBA pixels, stride_bytes apart (0 = 4 * w)."""
    _fields_ = [("rgba", C.c_void_p), ("w", C.c_int32), ("h", C.c_int32), ("stride_bytes", C.c_int64)]


class SegmentParams(C.Structure):
    _fields_ = [("polarity", C.c_int32), ("min_col_ink", C.c_int32), ("min_glyph_pixels", C.c_int32), ("max_glyphs", C.c_int32),
                ("glyph_box", C.c_int32), ("ink_high", C.c_int32)]


class CcParams(C.Structure):
    _fields_ = [("merge_overlap_pct", C.c_int32), ("min_height_pct", C.c_int32), ("reserved", C.c_int32 * 2)]


class Glyphs(C.Structure):
    _fields_ = [("n_images", C.c_int32), ("n_words", C.c_int32), ("n_glyphs", C.c_int32),
                ("img_offsets", C.POINTER(C.c_int32)), ("word_offsets", C.POINTER(C.c_int32)), ("word_info", C.POINTER(C.c_int32)),
                ("word_levels", C.POINTER(C.c_float)), ("boxes", C.POINTER(C.c_int32))]


class GlyphLabelsBlock(C.Structure):
    """ocr_glyph_labels_t: word_boxes and plane_offsets are host arrays, planes is device memory."""
    _fields_ = [("n_words", C.c_int32), ("device", C.c_int32), ("word_boxes", C.POINTER(C.c_int32)),
                ("plane_offsets", C.POINTER(C.c_int64)), ("planes", C.c_void_p)]


class MaskParams(C.Structure):
    _fields_ = [("halo", C.c_int32), ("reserved", C.c_int32 * 3)]


class StripParams(C.Structure):
    _fields_ = [("strip_height", C.c_int32), ("max_width", C.c_int32), ("reserved", C.c_int32 * 2)]


class Strips(C.Structure):
    _fields_ = [("n_images", C.c_int32), ("n_words", C.c_int32), ("height", C.c_int32), ("total_width", C.c_int32),
                ("img_offsets", C.POINTER(C.c_int32)), ("col_offsets", C.POINTER(C.c_int32)), ("word_info", C.POINTER(C.c_int32)),
                ("quads", C.POINTER(C.c_double)), ("maps", C.POINTER(C.c_float)), ("scores", C.POINTER(C.c_double))]


class CurveParams(C.Structure):
    _fields_ = [("strip_height", C.c_int32), ("max_width", C.c_int32), ("valid_pct", C.c_int32), ("reserved", C.c_int32)]


class CurvedStripsBlock(C.Structure):
    """ocr_curved_strips_t."""
    _fields_ = [("n_images", C.c_int32), ("n_words", C.c_int32), ("height", C.c_int32), ("total_width", C.c_int32),
                ("img_offsets", C.POINTER(C.c_int32)), ("col_offsets", C.POINTER(C.c_int32)), ("word_info", C.POINTER(C.c_int32)),
                ("knots", C.POINTER(C.c_float)), ("tscale", C.POINTER(C.c_float)), ("half_heights", C.POINTER(C.c_double)),
                ("lengths", C.POINTER(C.c_double)), ("scores", C.POINTER(C.c_double))]


CURVE_KNOTS = 33


class LineParams(C.Structure):
    _fields_ = [("line_tol", C.c_double), ("height_ratio", C.c_double), ("min_cos", C.c_double), ("max_gap", C.c_double),
                ("reserved", C.c_int32 * 2)]


class LinesBlock(C.Structure):
    """ocr_lines_t."""
    _fields_ = [("n_images", C.c_int32), ("n_words", C.c_int32), ("n_lines", C.c_int32),
                ("img_offsets", C.POINTER(C.c_int32)), ("line_offsets", C.POINTER(C.c_int32)), ("order", C.POINTER(C.c_int32)),
                ("word_flags", C.POINTER(C.c_int32)), ("gaps", C.POINTER(C.c_double))]


LINE_MAX_WORDS = 4096


class ColumnParams(C.Structure):
    """ocr_column_params_t."""
    _fields_ = [("line", LineParams), ("row_gap", C.c_double), ("min_gutter", C.c_double), ("gutter_reach", C.c_double),
                ("min_overlap", C.c_double), ("block_reach", C.c_double), ("min_rows", C.c_int32), ("max_levels", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class ColumnsBlock(C.Structure):
    """ocr_columns_t."""
    _fields_ = [("n_images", C.c_int32), ("n_words", C.c_int32), ("n_lines", C.c_int32), ("n_blocks", C.c_int32),
                ("img_offsets", C.POINTER(C.c_int32)), ("block_offsets", C.POINTER(C.c_int32)), ("line_offsets", C.POINTER(C.c_int32)),
                ("order", C.POINTER(C.c_int32)), ("word_flags", C.POINTER(C.c_int32)), ("gaps", C.POINTER(C.c_double)),
                ("line_flags", C.POINTER(C.c_int32)), ("block_levels", C.POINTER(C.c_int32)), ("block_quads", C.POINTER(C.c_double))]


class LexiconParams(C.Structure):
    """ocr_lexicon_params_t."""
    _fields_ = [("ins_cost", C.c_double), ("del_cost", C.c_double), ("max_len_diff", C.c_int32), ("fold_case", C.c_int32),
                ("top_k", C.c_int32), ("reserved", C.c_int32 * 3)]


class LexiconMatchesBlock(C.Structure):
    """ocr_lexicon_matches_t."""
    _fields_ = [("n_words", C.c_int32), ("top_k", C.c_int32), ("entries", C.POINTER(C.c_int32)), ("costs", C.POINTER(C.c_double)),
                ("raw_costs", C.POINTER(C.c_double)), ("n_candidates", C.POINTER(C.c_int32)), ("word_flags", C.POINTER(C.c_int32))]


class LmParams(C.Structure):
    """ocr_lm_params_t."""
    _fields_ = [("top_k", C.c_int32), ("reserved", C.c_int32 * 3)]


class LmPathsBlock(C.Structure):
    """ocr_lm_paths_t."""
    _fields_ = [("n_words", C.c_int32), ("top_k", C.c_int32), ("n_glyphs", C.c_int32), ("labels", C.POINTER(C.c_int32)),
                ("costs", C.POINTER(C.c_double)), ("raw_costs", C.POINTER(C.c_double)), ("word_flags", C.POINTER(C.c_int32))]


class SplitParams(C.Structure):
    """ocr_split_params_t."""
    _fields_ = [("aspect_pct", C.c_int32), ("max_pieces", C.c_int32), ("min_piece_w", C.c_int32), ("max_word_pieces", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class PieceMapBlock(C.Structure):
    """ocr_piece_map_t."""
    _fields_ = [("n_pieces", C.c_int32), ("glyph", C.POINTER(C.c_int32)), ("rank", C.POINTER(C.c_int32))]


class SpanTableBlock(C.Structure):
    """ocr_span_table_t."""
    _fields_ = [("n_words", C.c_int32), ("n_spans", C.c_int32), ("n_pieces", C.c_int32), ("max_span", C.c_int32),
                ("span_word", C.POINTER(C.c_int32)), ("span_end", C.POINTER(C.c_int32)), ("span_len", C.POINTER(C.c_int32)),
                ("piece_offsets", C.POINTER(C.c_int32))]


class LatticeParams(C.Structure):
    """ocr_lattice_params_t."""
    _fields_ = [("max_span", C.c_int32), ("top_k", C.c_int32), ("span_cost", C.c_double * 4), ("reserved", C.c_int32 * 2)]


class LatticePathsBlock(C.Structure):
    """ocr_lattice_paths_t."""
    _fields_ = [("n_words", C.c_int32), ("top_k", C.c_int32), ("n_pieces", C.c_int32), ("labels", C.POINTER(C.c_int32)),
                ("seg_len", C.POINTER(C.c_int32)), ("n_chars", C.POINTER(C.c_int32)), ("costs", C.POINTER(C.c_double)),
                ("raw_costs", C.POINTER(C.c_double)), ("word_flags", C.POINTER(C.c_int32))]


class LexLatParams(C.Structure):
    """ocr_lexlat_params_t."""
    _fields_ = [("ins_cost", C.c_double), ("del_cost", C.c_double), ("span_cost", C.c_double * 4), ("max_span", C.c_int32),
                ("max_len_diff", C.c_int32), ("fold_case", C.c_int32), ("top_k", C.c_int32), ("reserved", C.c_int32 * 2)]


class LexLatMatchesBlock(C.Structure):
    """ocr_lexlat_matches_t."""
    _fields_ = [("n_words", C.c_int32), ("top_k", C.c_int32), ("n_pieces", C.c_int32), ("entries", C.POINTER(C.c_int32)),
                ("costs", C.POINTER(C.c_double)), ("raw_costs", C.POINTER(C.c_double)), ("n_candidates", C.POINTER(C.c_int32)),
                ("word_flags", C.POINTER(C.c_int32)), ("seg_len", C.POINTER(C.c_int32)), ("seg_char", C.POINTER(C.c_int32)),
                ("n_ins", C.POINTER(C.c_int32))]


class BreakParams(C.Structure):
    """ocr_break_params_t."""
    _fields_ = [("mode", C.c_int32), ("space_pct", C.c_int32), ("min_space_pct", C.c_int32), ("sep_pct", C.c_int32),
                ("min_gaps", C.c_int32), ("reserved", C.c_int32 * 3)]


class WordBreaksBlock(C.Structure):
    """ocr_word_breaks_t."""
    _fields_ = [("n_source", C.c_int32), ("n_words", C.c_int32), ("source", C.POINTER(C.c_int32)), ("sub_offsets", C.POINTER(C.c_int32)),
                ("gap_pct", C.POINTER(C.c_int32)), ("source_info", C.POINTER(C.c_int32))]


class PhraseParams(C.Structure):
    """ocr_phrase_params_t."""
    _fields_ = [("word_cost", C.c_double), ("oov_word_cost", C.c_double), ("oov_glyph_cost", C.c_double), ("fold_case", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class PhraseMatchesBlock(C.Structure):
    """ocr_phrase_matches_t."""
    _fields_ = [("n_lines", C.c_int32), ("n_words", C.c_int32), ("n_glyphs", C.c_int32), ("line_word_offsets", C.POINTER(C.c_int32)),
                ("word_offsets", C.POINTER(C.c_int32)), ("entries", C.POINTER(C.c_int32)), ("word_costs", C.POINTER(C.c_double)),
                ("line_costs", C.POINTER(C.c_double)), ("raw_costs", C.POINTER(C.c_double)), ("line_flags", C.POINTER(C.c_int32))]


PHRASE_MAX_GLYPHS = 256
PHRASE_STARTS = 32           # starts per window of the phrase match kernel (csrc/lexicon_phrase.hip kPhraseStarts)
PHRASE_GROUP_WINDOWS = 2048  # windows per group of lines (kPhraseGroupWindows): batches around it take another launch sequence
BREAK_MAX_GLYPHS = 256
BREAK_WORDS = 4   # source words per workgroup of the break kernel (csrc/word_breaks.hip kBreakWaves): word counts around it change the grid

LEX_MAX_LEN = 32
LEX_MAX_ENTRIES = 1 << 22
LEX_CHUNK = 256   # entries per pass of a match workgroup (csrc/lexicon_host.hpp kLexChunk): lexicon sizes around it change the grid

LM_MAX_LEN = 32
LM_WORDS = 4      # words per workgroup of the decode kernel (csrc/char_lm_host.hpp kLmWords): word counts around it change the grid
LATTICE_MAX_SPAN = 4
LATTICE_MAX_PIECES = 32
LATTICE_WORDS = 4  # words per workgroup of the lattice decode kernel (csrc/lattice_host.hpp kLatWords)
LM_BEGIN = 62     # the model's row of begin-of-word
LM_END = 62       # ... and its column of end-of-word

_lib = None
_hip_shared = False


def _share_torch_hip_runtime() -> None:
    """One HIP runtime per process.  PyTorch-ROCm wheels carry their own libamdhip64.so (SONAME libamdhip64.so.7) and libhsa-runtime64.so and
    link to them by FILE name; libocr_amd.so needs `libamdhip64.so.7`.  Loaded after torch, the library binds to torch's copy (the SONAME
    matches) and the process has one runtime.  Loaded BEFORE torch, it brings /opt/rocm's copy in, torch then loads its own beside it (its
    NEEDED name matches no loaded SONAME) and the second runtime finds the device taken: torch's lazy init fails with "No HIP GPUs are
    available".  So this harness loads torch's copy first when a torch installation exists and has not been imported yet - without
    importing torch.  (A host that does not use torch - the Rust / C++ caller of INTEGRATION.md - has one runtime anyway.)"""
    global _hip_shared
    if _hip_shared:
        return
    _hip_shared = True
    import sys
    if "torch" in sys.modules:
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        p = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(p):
            C.CDLL(p, mode=C.RTLD_GLOBAL)
    except Exception:   # no torch, or an unusual layout: nothing to share
        pass


def lib() -> C.CDLL:
    """Loads libocr_amd.so; fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OcrError(-1, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)")
        _share_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        L.ocr_last_error.restype = C.c_char_p
        L.ocr_version.restype = C.c_char_p
        L.ocr_rec_alphabet.restype = C.c_char_p
        L.ocr_det_create.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]
        L.ocr_det_destroy.argtypes = [C.c_void_p]
        L.ocr_det_destroy.restype = None
        L.ocr_det_create_with_options.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_char_p, C.POINTER(C.c_void_p)]
        L.ocr_det_create_from_varstore.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        L.ocr_rec_create_from_varstore.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        L.ocr_varstore_to_blob.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.ocr_blob_free.argtypes = [C.c_void_p]
        L.ocr_blob_free.restype = None
        L.ocr_det_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.ocr_det_set_precision.argtypes = [C.c_void_p, C.c_int]
        L.ocr_det_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.ocr_det_forward_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.ocr_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
        L.ocr_host_free.argtypes = [C.c_void_p]
        L.ocr_host_free.restype = None
        L.ocr_det_detect_pipelined_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                    C.POINTER(C.c_double), C.POINTER(PostprocParams),
                                                    C.POINTER(C.POINTER(Polygons))]
        L.ocr_det_forward_async.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_float]
        L.ocr_det_synchronize.argtypes = [C.c_void_p]
        L.ocr_det_forward_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                              C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.POINTER(C.c_double),
                                              C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.ocr_preprocess_image.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.POINTER(C.c_double), C.c_int]
        L.ocr_preprocess_batch.argtypes = [C.c_void_p, C.POINTER(ImageDesc), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_int, C.POINTER(C.c_double)]
        L.ocr_preprocess_batch_async.argtypes = [C.c_void_p, C.POINTER(ImageDesc), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.POINTER(C.c_double)]
        L.ocr_postproc_default_params.argtypes = [C.POINTER(PostprocParams)]
        L.ocr_postproc_default_params.restype = None
        L.ocr_det_post_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.ocr_ctc_greedy_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.ocr_ctc_beam_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
        L.ocr_det_postprocess.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.POINTER(C.c_double), C.POINTER(PostprocParams),
                                          C.POINTER(C.POINTER(Polygons))]
        L.ocr_det_detect_pipelined.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                               C.POINTER(C.c_double), C.POINTER(PostprocParams),
                                               C.POINTER(C.POINTER(Polygons))]
        L.ocr_polygons_free.argtypes = [C.POINTER(Polygons)]
        L.ocr_polygons_free.restype = None
        L.ocr_evaluate_image.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.POINTER(MetricsItem)]
        L.ocr_combine_results.argtypes = [C.POINTER(MetricsItem), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(C.c_double)]
        L.ocr_extract_crops.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Polygons),
                                        C.POINTER(C.c_double), C.c_void_p]
        L.ocr_segment_default_params.argtypes = [C.POINTER(SegmentParams)]
        L.ocr_segment_default_params.restype = None
        L.ocr_segment_glyphs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Polygons),
                                         C.POINTER(C.c_double), C.POINTER(SegmentParams), C.POINTER(C.POINTER(Glyphs))]
        L.ocr_cc_default_params.argtypes = [C.POINTER(CcParams)]
        L.ocr_cc_default_params.restype = None
        L.ocr_segment_glyphs_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Polygons),
                                            C.POINTER(C.c_double), C.POINTER(SegmentParams), C.POINTER(CcParams),
                                            C.POINTER(C.POINTER(Glyphs))]
        L.ocr_extract_glyph_crops.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Glyphs),
                                              C.POINTER(SegmentParams), C.c_void_p]
        L.ocr_glyphs_free.argtypes = [C.POINTER(Glyphs)]
        L.ocr_glyphs_free.restype = None
        L.ocr_mask_default_params.argtypes = [C.POINTER(MaskParams)]
        L.ocr_mask_default_params.restype = None
        L.ocr_segment_glyphs_cc_labelled.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Polygons),
                                                     C.POINTER(C.c_double), C.POINTER(SegmentParams), C.POINTER(CcParams),
                                                     C.POINTER(C.POINTER(Glyphs)), C.POINTER(C.POINTER(GlyphLabelsBlock))]
        L.ocr_glyph_labels_read.argtypes = [C.c_void_p, C.POINTER(GlyphLabelsBlock), C.c_void_p]
        L.ocr_extract_glyph_crops_masked.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Glyphs),
                                                     C.POINTER(GlyphLabelsBlock), C.POINTER(SegmentParams), C.POINTER(MaskParams), C.c_void_p]
        L.ocr_glyph_labels_free.argtypes = [C.POINTER(GlyphLabelsBlock)]
        L.ocr_glyph_labels_free.restype = None
        L.ocr_strip_default_params.argtypes = [C.POINTER(StripParams)]
        L.ocr_strip_default_params.restype = None
        L.ocr_plan_word_strips.argtypes = [C.POINTER(Polygons), C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.POINTER(StripParams),
                                           C.POINTER(C.POINTER(Strips))]
        L.ocr_extract_word_strips.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Strips), C.c_void_p]
        L.ocr_word_strip_polygons.argtypes = [C.POINTER(Strips), C.POINTER(C.POINTER(Polygons))]
        L.ocr_word_strips_free.argtypes = [C.POINTER(Strips)]
        L.ocr_word_strips_free.restype = None
        L.ocr_curve_default_params.argtypes = [C.POINTER(CurveParams)]
        L.ocr_curve_default_params.restype = None
        L.ocr_plan_curved_strips.argtypes = [C.POINTER(Polygons), C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.POINTER(CurveParams),
                                             C.POINTER(C.POINTER(CurvedStripsBlock))]
        L.ocr_extract_curved_strips.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(CurvedStripsBlock),
                                                C.c_void_p]
        L.ocr_curved_strip_polygons.argtypes = [C.POINTER(CurvedStripsBlock), C.POINTER(C.POINTER(Polygons))]
        L.ocr_curved_strips_free.argtypes = [C.POINTER(CurvedStripsBlock)]
        L.ocr_curved_strips_free.restype = None
        L.ocr_line_default_params.argtypes = [C.POINTER(LineParams)]
        L.ocr_line_default_params.restype = None
        L.ocr_group_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(LineParams), C.POINTER(C.POINTER(LinesBlock))]
        L.ocr_lines_free.argtypes = [C.POINTER(LinesBlock)]
        L.ocr_lines_free.restype = None
        L.ocr_column_default_params.argtypes = [C.POINTER(ColumnParams)]
        L.ocr_column_default_params.restype = None
        L.ocr_group_columns.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(ColumnParams),
                                        C.POINTER(C.POINTER(ColumnsBlock))]
        L.ocr_columns_free.argtypes = [C.POINTER(ColumnsBlock)]
        L.ocr_columns_free.restype = None
        L.ocr_rec_glyph_costs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.ocr_lexicon_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.ocr_lexicon_size.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.ocr_lexicon_destroy.argtypes = [C.c_void_p]
        L.ocr_lexicon_destroy.restype = None
        L.ocr_lexicon_default_params.argtypes = [C.POINTER(LexiconParams)]
        L.ocr_lexicon_default_params.restype = None
        L.ocr_lexicon_match.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(LexiconParams),
                                        C.POINTER(C.POINTER(LexiconMatchesBlock))]
        L.ocr_lexicon_matches_free.argtypes = [C.POINTER(LexiconMatchesBlock)]
        L.ocr_lexicon_matches_free.restype = None
        L.ocr_char_lm_create.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.ocr_char_lm_destroy.argtypes = [C.c_void_p]
        L.ocr_char_lm_destroy.restype = None
        L.ocr_lm_default_params.argtypes = [C.POINTER(LmParams)]
        L.ocr_lm_default_params.restype = None
        L.ocr_lm_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(LmParams),
                                    C.POINTER(C.POINTER(LmPathsBlock))]
        L.ocr_lm_paths_free.argtypes = [C.POINTER(LmPathsBlock)]
        L.ocr_lm_paths_free.restype = None
        L.ocr_split_default_params.argtypes = [C.POINTER(SplitParams)]
        L.ocr_split_default_params.restype = None
        L.ocr_split_glyphs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Glyphs), C.POINTER(SplitParams),
                                       C.POINTER(C.POINTER(Glyphs)), C.POINTER(C.POINTER(PieceMapBlock))]
        L.ocr_piece_map_free.argtypes = [C.POINTER(PieceMapBlock)]
        L.ocr_piece_map_free.restype = None
        L.ocr_glyph_spans.argtypes = [C.POINTER(Glyphs), C.c_int, C.POINTER(C.POINTER(Glyphs)), C.POINTER(C.POINTER(SpanTableBlock))]
        L.ocr_span_table_free.argtypes = [C.POINTER(SpanTableBlock)]
        L.ocr_span_table_free.restype = None
        L.ocr_lattice_default_params.argtypes = [C.POINTER(LatticeParams)]
        L.ocr_lattice_default_params.restype = None
        L.ocr_lattice_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                         C.POINTER(LatticeParams), C.POINTER(C.POINTER(LatticePathsBlock))]
        L.ocr_lattice_paths_free.argtypes = [C.POINTER(LatticePathsBlock)]
        L.ocr_lattice_paths_free.restype = None
        L.ocr_lexlat_default_params.argtypes = [C.POINTER(LexLatParams)]
        L.ocr_lexlat_default_params.restype = None
        L.ocr_lexicon_lattice_match.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                C.POINTER(LexLatParams), C.POINTER(C.POINTER(LexLatMatchesBlock))]
        L.ocr_lexlat_matches_free.argtypes = [C.POINTER(LexLatMatchesBlock)]
        L.ocr_lexlat_matches_free.restype = None
        L.ocr_break_default_params.argtypes = [C.POINTER(BreakParams)]
        L.ocr_break_default_params.restype = None
        L.ocr_break_words.argtypes = [C.c_void_p, C.POINTER(Glyphs), C.POINTER(BreakParams), C.POINTER(C.POINTER(Glyphs)),
                                      C.POINTER(C.POINTER(WordBreaksBlock))]
        L.ocr_word_breaks_free.argtypes = [C.POINTER(WordBreaksBlock)]
        L.ocr_word_breaks_free.restype = None
        L.ocr_phrase_default_params.argtypes = [C.POINTER(PhraseParams)]
        L.ocr_phrase_default_params.restype = None
        L.ocr_lexicon_phrase_match.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                               C.c_void_p, C.POINTER(PhraseParams), C.POINTER(C.POINTER(PhraseMatchesBlock))]
        L.ocr_phrase_matches_free.argtypes = [C.POINTER(PhraseMatchesBlock)]
        L.ocr_phrase_matches_free.restype = None
        L.ocr_rec_create.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]
        L.ocr_rec_destroy.argtypes = [C.c_void_p]
        L.ocr_rec_destroy.restype = None
        L.ocr_rec_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.ocr_rec_synchronize.argtypes = [C.c_void_p]
        L.ocr_rec_set_options.argtypes = [C.c_void_p, C.c_char_p]
        L.ocr_rec_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.ocr_rec_classify_async.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ocr_rec_classify.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.ocr_rec_classify_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                               C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.POINTER(C.c_double),
                                               C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.ocr_comm_unique_id.argtypes = [C.c_void_p]
        L.ocr_comm_rccl_version.argtypes = [C.POINTER(C.c_int)]
        L.ocr_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.ocr_comm_destroy.argtypes = [C.c_void_p]
        L.ocr_comm_destroy.restype = None
        L.ocr_comm_all_gather_polygons.argtypes = [C.c_void_p, C.POINTER(Polygons), C.POINTER(C.POINTER(Polygons))]
        L.ocr_comm_all_gather_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                 C.POINTER(C.c_int)]
        _lib = L
    return _lib


_test_lib = None
TEST_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libocr_amd_test.so")


def test_lib() -> C.CDLL:
    """libocr_amd_test.so: the ocr_test_* hooks (kernel-level parity, host geometry, tuning aids).  A separate
    library built from the same objects plus test_hooks.o - nothing of it ships in libocr_amd.so, whose internals are
    not exported.  Hooks take the handles the product library created (same classes, same process)."""
    global _test_lib
    if _test_lib is None:
        lib()
        if not os.path.exists(TEST_LIB_PATH):
            raise OcrError(-1, f"{TEST_LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _share_torch_hip_runtime()
        L = C.CDLL(TEST_LIB_PATH)
        L.ocr_test_contour_candidates.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                  C.c_int, C.POINTER(C.c_int)]
        L.ocr_test_expand_polygon.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_int,
                                              C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.ocr_test_min_area_box.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
        L.ocr_test_box_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_void_p]
        L.ocr_test_box_scores_batch.argtypes = ([C.c_void_p, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_double] +
                                                [C.c_void_p] * 3)
        L.ocr_test_conv_bench.argtypes = [C.c_void_p] + [C.c_int] * 9 + [C.POINTER(C.c_float)]
        L.ocr_test_conv_run.argtypes = ([C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] +
                                        [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p] * 2)
        L.ocr_test_set_conv_tile.argtypes = [C.c_int]
        L.ocr_test_bf16_basic_block.argtypes = ([C.c_void_p, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 6 + [C.c_int] * 3 +
                                                [C.c_void_p, C.POINTER(C.c_float)])
        L.ocr_test_winograd_conv.argtypes = ([C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_int] +
                                             [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p])
        L.ocr_test_det_stage.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ocr_test_stem_run.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int]
        L.ocr_test_head_run.argtypes = ([C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_float, C.c_float] +
                                        [C.c_int, C.c_void_p, C.c_void_p, C.c_int])
        L.ocr_test_convt2_sigmoid.argtypes = ([C.c_void_p, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_int])
        L.ocr_test_binarize.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_int, C.c_void_p, C.c_int]
        L.ocr_test_binarize_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_int, C.c_void_p, C.c_int]
        L.ocr_test_rec_features.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_int]
        L.ocr_test_rec_fc1.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.ocr_test_rec_fc2.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int]
        L.ocr_test_comm_assemble.argtypes = [C.POINTER(C.POINTER(Polygons)), C.c_int, C.POINTER(C.POINTER(Polygons))]
        L.ocr_test_compose_taps.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.ocr_test_phase_weights.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.ocr_test_pyr4_weights.argtypes = [C.c_void_p] * 3
        L.ocr_test_phase_conv_run.argtypes = ([C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] +
                                              [C.c_int] * 3 + [C.c_void_p, C.c_int])
        L.ocr_test_pyr4_conv_run.argtypes = ([C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int])
        L.ocr_test_winograd_weights.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.ocr_test_winograd43_fragments.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.ocr_test_winograd_run.argtypes = ([C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 4 +
                                            [C.c_void_p, C.c_int])
        L.ocr_test_bf16_trunk_run.argtypes = ([C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_int] +
                                              [C.c_void_p] * 3 + [C.c_int] * 2 + [C.c_void_p] * 2 + [C.c_int])
        L.ocr_test_igemm_run.argtypes = ([C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 4 +
                                         [C.c_int] * 3 + [C.c_void_p] * 2 + [C.c_int])
        _test_lib = L
    return _test_lib


def check(code: int) -> None:
    if code != 0:
        msg = lib().ocr_last_error().decode()
        if not msg and _test_lib is not None:   # the failure came from a test hook: that library keeps its own message
            _test_lib.ocr_last_error.restype = C.c_char_p
            msg = _test_lib.ocr_last_error().decode()
        raise OcrError(code, msg)


def use_test_library() -> None:
    """Tuning tools whose hooks change library-wide state (tile override, ablation bits, stamp buffers) must run the
    detector from the SAME library the hooks live in: call this before the first lib() - libocr_amd_test.so carries the
    whole C ABI besides the hooks (it is built from the same objects)."""
    global LIB_PATH
    if _lib is not None:
        raise OcrError(-1, "use_test_library() must come before the first library call")
    LIB_PATH = TEST_LIB_PATH


def _ptr(a) -> int:
    """Raw address of a numpy array or of a torch tensor (host or device)."""
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()


def polygons_to_python(pp) -> Tuple[List[List[List[Tuple[int, int]]]], List[List[float]]]:
    """CSR block -> PolygonScores{polygons: Vec<MultiPolygon<u32>>, scores: Vec<Vec<f64>>}."""
    p = pp.contents
    ni, npoly, nv = p.n_images, p.n_polygons, p.n_vertices
    img = np.ctypeslib.as_array(p.img_offsets, shape=(ni + 1,)).tolist()
    po = np.ctypeslib.as_array(p.poly_offsets, shape=(npoly + 1,)).tolist() if npoly else [0]
    pts = list(map(tuple, np.ctypeslib.as_array(p.xy, shape=(2 * nv,)).reshape(-1, 2).tolist())) if nv else []
    sc = np.ctypeslib.as_array(p.scores, shape=(npoly,)).tolist() if npoly else []
    polys = [[pts[po[k]:po[k + 1]] for k in range(img[b], img[b + 1])] for b in range(ni)]
    scores = [sc[img[b]:img[b + 1]] for b in range(ni)]
    return polys, scores


VARSTORE_RAW, VARSTORE_DET, VARSTORE_REC = 0, 1, 2


def varstore_to_blob(path: str, kind: int = VARSTORE_RAW) -> bytes:
    """tch VarStore file -> OCRW blob through the library's own zip + pickle reader (host only, no torch)."""
    blob, n = C.c_void_p(), C.c_size_t(0)
    check(lib().ocr_varstore_to_blob(os.fsencode(path), kind, C.byref(blob), C.byref(n)))
    try:
        return C.string_at(blob, n.value)
    finally:
        lib().ocr_blob_free(blob)


def default_params(skip_degenerate: bool = False) -> PostprocParams:
    p = PostprocParams()
    lib().ocr_postproc_default_params(C.byref(p))
    p.skip_degenerate = 1 if skip_degenerate else 0
    return p


def segment_params(**fields) -> SegmentParams:
    """ocr_segment_default_params with the given fields overridden (polarity, min_col_ink, min_glyph_pixels, max_glyphs, glyph_box,
    ink_high)."""
    p = SegmentParams()
    lib().ocr_segment_default_params(C.byref(p))
    for k, v in fields.items():
        if k not in dict(SegmentParams._fields_):
            raise TypeError(f"unknown segment parameter {k!r}")
        setattr(p, k, int(v))
    return p


def _as_segment_params(params) -> Optional[SegmentParams]:
    if params is None or isinstance(params, SegmentParams):
        return params
    return segment_params(**params)


def cc_params(**fields) -> CcParams:
    """ocr_cc_default_params with the given fields overridden (merge_overlap_pct, min_height_pct)."""
    p = CcParams()
    lib().ocr_cc_default_params(C.byref(p))
    for k, v in fields.items():
        if k not in ("merge_overlap_pct", "min_height_pct"):
            raise TypeError(f"unknown cc parameter {k!r}")
        setattr(p, k, int(v))
    return p


def _as_cc_params(cc) -> Optional[CcParams]:
    if cc is None or isinstance(cc, CcParams):
        return cc
    return cc_params(**cc)


class GlyphSet:
    """The arrays of an ocr_glyphs_t, copied into numpy: img_offsets [n_images+1], word_offsets [n_words+1], word_info n_words x 4
    (frame, t, polarity used, truncated - from segment_glyphs(cc=...) a bit set: 1 truncated, 2 column fallback), word_levels n_words x 2 f32 (bg, ink), boxes n_glyphs x 4 (x0, y0, x1, y1, half-open)."""

    def __init__(self, img_offsets, word_offsets, word_info, word_levels, boxes):
        self.img_offsets = np.ascontiguousarray(img_offsets, dtype=np.int32)
        self.word_offsets = np.ascontiguousarray(word_offsets, dtype=np.int32)
        self.word_info = np.ascontiguousarray(word_info, dtype=np.int32).reshape(-1, 4)
        self.word_levels = np.ascontiguousarray(word_levels, dtype=np.float32).reshape(-1, 2)
        self.boxes = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)

    @property
    def n_images(self) -> int:
        return len(self.img_offsets) - 1

    @property
    def n_words(self) -> int:
        return len(self.word_offsets) - 1

    @property
    def n_glyphs(self) -> int:
        return int(self.word_offsets[-1])

    @staticmethod
    def from_block(gp) -> "GlyphSet":
        g = gp.contents
        ni, nw, ng = g.n_images, g.n_words, g.n_glyphs

        def arr(ptr, n, dt):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, dt)
        return GlyphSet(arr(g.img_offsets, ni + 1, np.int32), arr(g.word_offsets, nw + 1, np.int32), arr(g.word_info, 4 * nw, np.int32),
                        arr(g.word_levels, 2 * nw, np.float32), arr(g.boxes, 4 * ng, np.int32))

    def block(self) -> Glyphs:
        """An ocr_glyphs_t viewing these arrays (valid while this object lives)."""
        def p(a, t):
            return a.ctypes.data_as(C.POINTER(t))
        return Glyphs(self.n_images, self.n_words, self.n_glyphs, p(self.img_offsets, C.c_int32), p(self.word_offsets, C.c_int32),
                      p(self.word_info, C.c_int32), p(self.word_levels, C.c_float), p(self.boxes, C.c_int32))


def mask_params(**fields) -> MaskParams:
    """ocr_mask_default_params with the given fields overridden (halo)."""
    p = MaskParams()
    lib().ocr_mask_default_params(C.byref(p))
    for k, v in fields.items():
        if k != "halo":
            raise TypeError(f"unknown mask parameter {k!r}")
        setattr(p, k, int(v))
    return p


def _as_mask_params(mask) -> Optional[MaskParams]:
    """None or True -> the defaults (a null pointer); MaskParams as it is; a dict of its fields -> mask_params(**mask)."""
    if mask is None or mask is True:
        return None
    if isinstance(mask, MaskParams):
        return mask
    if not isinstance(mask, dict):
        raise TypeError(f"mask: expected None, True, a MaskParams or a dict of its fields, got {mask!r} (the unmasked call is extract_glyph_crops)")
    return mask_params(**mask)


class GlyphLabels:
    """Owner of an ocr_glyph_labels_t: the label planes of one ocr_segment_glyphs_cc_labelled call, resident on the detector's GPU
    until free() (or the end of a `with` block).  word_boxes n_words x 4 (X0, Y0, X1, Y1) and plane_offsets [n_words+1] are numpy
    copies; read() brings the planes to the host."""

    def __init__(self, det: "Detector", block):
        self._det, self._p = det, block
        b = block.contents
        nw = b.n_words
        self.n_words, self.device = nw, b.device
        self.word_boxes = (np.ctypeslib.as_array(b.word_boxes, shape=(4 * nw,)).copy() if nw else np.zeros(0, np.int32)).reshape(-1, 4)
        self.plane_offsets = np.ctypeslib.as_array(b.plane_offsets, shape=(nw + 1,)).copy()

    @property
    def block(self):
        """The ocr_glyph_labels_t* for the C calls."""
        if self._p is None:
            raise OcrError(1, "glyph labels already freed")
        return self._p

    def read(self) -> np.ndarray:
        """All planes, plane_offsets[n_words] uint16: word k is read()[plane_offsets[k]:plane_offsets[k + 1]].reshape(bh, bw)."""
        planes = np.zeros(int(self.plane_offsets[-1]), np.uint16)
        check(lib().ocr_glyph_labels_read(self._det._h, self.block, _ptr(planes)))
        return planes

    def plane(self, planes: np.ndarray, k: int) -> np.ndarray:
        """Word k's bh x bw view of what read() returned."""
        x0, y0, x1, y1 = (int(v) for v in self.word_boxes[k])
        return planes[int(self.plane_offsets[k]):int(self.plane_offsets[k + 1])].reshape(y1 - y0, x1 - x0)

    def free(self) -> None:
        if self._p is not None:
            lib().ocr_glyph_labels_free(self._p)
            self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def strip_params(**fields) -> StripParams:
    """ocr_strip_default_params with the given fields overridden (strip_height, max_width)."""
    p = StripParams()
    lib().ocr_strip_default_params(C.byref(p))
    for k, v in fields.items():
        if k == "reserved":
            p.reserved[0], p.reserved[1] = (int(x) for x in v)
        elif k in dict(StripParams._fields_):
            setattr(p, k, int(v))
        else:
            raise TypeError(f"unknown strip parameter {k!r}")
    return p


def _as_strip_params(params) -> Optional[StripParams]:
    if params is None or isinstance(params, StripParams):
        return params
    return strip_params(**params)


class WordStrips:
    """The arrays of an ocr_word_strips_t, copied into numpy: img_offsets [n_images+1], col_offsets [n_words+1], word_info n_words x 2
    (frame, flags: 1 squeezed, 2 degenerate), quads n_words x 8 f64 (TL, TR, BR, BL in frame coordinates), maps n_words x 6 f32 (ox, oy,
    ux, uy, vx, vy), scores [n_words] f64; height and total_width of the atlas."""

    def __init__(self, img_offsets, col_offsets, word_info, quads, maps, scores, height: int):
        self.img_offsets = np.ascontiguousarray(img_offsets, dtype=np.int32)
        self.col_offsets = np.ascontiguousarray(col_offsets, dtype=np.int32)
        self.word_info = np.ascontiguousarray(word_info, dtype=np.int32).reshape(-1, 2)
        self.quads = np.ascontiguousarray(quads, dtype=np.float64).reshape(-1, 8)
        self.maps = np.ascontiguousarray(maps, dtype=np.float32).reshape(-1, 6)
        self.scores = np.ascontiguousarray(scores, dtype=np.float64)
        self.height = int(height)

    @property
    def n_images(self) -> int:
        return len(self.img_offsets) - 1

    @property
    def n_words(self) -> int:
        return len(self.col_offsets) - 1

    @property
    def total_width(self) -> int:
        return int(self.col_offsets[-1])

    @staticmethod
    def from_block(sp) -> "WordStrips":
        s = sp.contents
        ni, nw = s.n_images, s.n_words

        def arr(ptr, n, dt):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, dt)
        return WordStrips(arr(s.img_offsets, ni + 1, np.int32), arr(s.col_offsets, nw + 1, np.int32), arr(s.word_info, 2 * nw, np.int32),
                          arr(s.quads, 8 * nw, np.float64), arr(s.maps, 6 * nw, np.float32), arr(s.scores, nw, np.float64), s.height)

    def block(self) -> Strips:
        """An ocr_word_strips_t viewing these arrays (valid while this object lives)."""
        def p(a, t):
            return a.ctypes.data_as(C.POINTER(t))
        return Strips(self.n_images, self.n_words, self.height, self.total_width, p(self.img_offsets, C.c_int32),
                      p(self.col_offsets, C.c_int32), p(self.word_info, C.c_int32), p(self.quads, C.c_double), p(self.maps, C.c_float),
                      p(self.scores, C.c_double))

    @contextlib.contextmanager
    def polygon_block(self):
        """ocr_word_strip_polygons as the library's own block (a Polygons, valid inside the with statement): the atlas rectangles
        without a round trip through Python lists."""
        blk = self.block()
        out = C.POINTER(Polygons)()
        check(lib().ocr_word_strip_polygons(C.byref(blk), C.byref(out)))
        try:
            yield out.contents
        finally:
            lib().ocr_polygons_free(out)

    def polygons(self):
        """ocr_word_strip_polygons: (one image of n_words atlas rectangles, their scores) as postprocess returns polygons."""
        with self.polygon_block() as p:
            return polygons_to_python(C.pointer(p))


def plan_word_strips(polys, adjust_values, h: int, w: int, params=None, scores=None) -> WordStrips:
    """ocr_plan_word_strips (host only, no GPU): polys per image in original-image pixels (or a Polygons block), adjust_values N x 2,
    the frame size H x W; params: StripParams, a dict of its fields, or None (defaults); scores: per image per polygon, or None (0)."""
    if isinstance(polys, Polygons):
        st, n = polys, polys.n_images
    else:
        st, keep = python_to_polygons(polys, scores if scores is not None else [[0.0] * len(p) for p in polys])
        n = len(polys)
    adj = np.ascontiguousarray(adjust_values, dtype=np.float64).reshape(-1, 2)
    prm = _as_strip_params(params)
    out = C.POINTER(Strips)()
    check(lib().ocr_plan_word_strips(C.byref(st), adj.ctypes.data_as(C.POINTER(C.c_double)), n, h, w,
                                     C.byref(prm) if prm is not None else None, C.byref(out)))
    try:
        return WordStrips.from_block(out)
    finally:
        lib().ocr_word_strips_free(out)


def curve_params(**fields) -> CurveParams:
    """ocr_curve_default_params with the given fields overridden (strip_height, max_width, valid_pct)."""
    p = CurveParams()
    lib().ocr_curve_default_params(C.byref(p))
    for k, v in fields.items():
        if k in dict(CurveParams._fields_):
            setattr(p, k, int(v))
        else:
            raise TypeError(f"unknown curve parameter {k!r}")
    return p


def _as_curve_params(params) -> Optional[CurveParams]:
    if params is None or isinstance(params, CurveParams):
        return params
    return curve_params(**params)


class CurvedStrips:
    """The arrays of an ocr_curved_strips_t, copied into numpy: img_offsets [n_images+1], col_offsets [n_words+1], word_info
    n_words x 2 (frame, flags: 1 squeezed, 2 degenerate, 4 folded, 8 steep, 16 straight fallback), knots n_words x 33 x 4 f32 (px, py,
    nx, ny), tscale [n_words] f32, half_heights, lengths and scores [n_words] f64; height and total_width of the atlas."""

    def __init__(self, img_offsets, col_offsets, word_info, knots, tscale, half_heights, lengths, scores, height: int):
        self.img_offsets = np.ascontiguousarray(img_offsets, dtype=np.int32)
        self.col_offsets = np.ascontiguousarray(col_offsets, dtype=np.int32)
        self.word_info = np.ascontiguousarray(word_info, dtype=np.int32).reshape(-1, 2)
        self.knots = np.ascontiguousarray(knots, dtype=np.float32).reshape(-1, CURVE_KNOTS, 4)
        self.tscale = np.ascontiguousarray(tscale, dtype=np.float32)
        self.half_heights = np.ascontiguousarray(half_heights, dtype=np.float64)
        self.lengths = np.ascontiguousarray(lengths, dtype=np.float64)
        self.scores = np.ascontiguousarray(scores, dtype=np.float64)
        self.height = int(height)

    @property
    def n_images(self) -> int:
        return len(self.img_offsets) - 1

    @property
    def n_words(self) -> int:
        return len(self.col_offsets) - 1

    @property
    def total_width(self) -> int:
        return int(self.col_offsets[-1])

    @staticmethod
    def from_block(sp) -> "CurvedStrips":
        s = sp.contents
        ni, nw = s.n_images, s.n_words

        def arr(ptr, n, dt):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, dt)
        return CurvedStrips(arr(s.img_offsets, ni + 1, np.int32), arr(s.col_offsets, nw + 1, np.int32), arr(s.word_info, 2 * nw, np.int32),
                            arr(s.knots, 4 * CURVE_KNOTS * nw, np.float32), arr(s.tscale, nw, np.float32),
                            arr(s.half_heights, nw, np.float64), arr(s.lengths, nw, np.float64), arr(s.scores, nw, np.float64), s.height)

    def block(self) -> CurvedStripsBlock:
        """An ocr_curved_strips_t viewing these arrays (valid while this object lives)."""
        def p(a, t):
            return a.ctypes.data_as(C.POINTER(t))
        return CurvedStripsBlock(self.n_images, self.n_words, self.height, self.total_width, p(self.img_offsets, C.c_int32),
                                 p(self.col_offsets, C.c_int32), p(self.word_info, C.c_int32), p(self.knots, C.c_float),
                                 p(self.tscale, C.c_float), p(self.half_heights, C.c_double), p(self.lengths, C.c_double),
                                 p(self.scores, C.c_double))

    @contextlib.contextmanager
    def polygon_block(self):
        """ocr_curved_strip_polygons as the library's own block (a Polygons, valid inside the with statement)."""
        blk = self.block()
        out = C.POINTER(Polygons)()
        check(lib().ocr_curved_strip_polygons(C.byref(blk), C.byref(out)))
        try:
            yield out.contents
        finally:
            lib().ocr_polygons_free(out)

    def polygons(self):
        """ocr_curved_strip_polygons: (one image of n_words atlas rectangles, their scores) as postprocess returns polygons."""
        with self.polygon_block() as p:
            return polygons_to_python(C.pointer(p))


def plan_curved_strips(polys, adjust_values, h: int, w: int, params=None, scores=None) -> CurvedStrips:
    """ocr_plan_curved_strips (host only, no GPU): arguments as plan_word_strips; params: CurveParams, a dict of its fields (strip_height,
    max_width, valid_pct), or None (defaults)."""
    if isinstance(polys, Polygons):
        st, n = polys, polys.n_images
    else:
        st, keep = python_to_polygons(polys, scores if scores is not None else [[0.0] * len(p) for p in polys])
        n = len(polys)
    adj = np.ascontiguousarray(adjust_values, dtype=np.float64).reshape(-1, 2)
    prm = _as_curve_params(params)
    out = C.POINTER(CurvedStripsBlock)()
    check(lib().ocr_plan_curved_strips(C.byref(st), adj.ctypes.data_as(C.POINTER(C.c_double)), n, h, w,
                                       C.byref(prm) if prm is not None else None, C.byref(out)))
    try:
        return CurvedStrips.from_block(out)
    finally:
        lib().ocr_curved_strips_free(out)


def line_params(**fields) -> LineParams:
    """ocr_line_default_params with the given fields overridden (line_tol, height_ratio, min_cos, max_gap)."""
    p = LineParams()
    lib().ocr_line_default_params(C.byref(p))
    for k, v in fields.items():
        if k == "reserved":
            p.reserved[0], p.reserved[1] = (int(x) for x in v)
        elif k in dict(LineParams._fields_):
            setattr(p, k, float(v))
        else:
            raise TypeError(f"unknown line parameter {k!r}")
    return p


def _as_line_params(params) -> Optional[LineParams]:
    if params is None or isinstance(params, LineParams):
        return params
    return line_params(**params)


class Lines:
    """The arrays of an ocr_lines_t, copied into numpy: img_offsets [n_images+1] (line range per image), line_offsets [n_lines+1]
    (range of `order` per line), order [n_words] (batch-global word indices in reading order), word_flags [n_words] by word index
    (1 isolated, 2 a cycle was cut in front of this word), gaps [n_words] f64 by position in `order` (g / hmax of the link that leads to
    the word, 0.0 for the head of a line)."""

    def __init__(self, img_offsets, line_offsets, order, word_flags, gaps):
        self.img_offsets = np.ascontiguousarray(img_offsets, dtype=np.int32)
        self.line_offsets = np.ascontiguousarray(line_offsets, dtype=np.int32)
        self.order = np.ascontiguousarray(order, dtype=np.int32)
        self.word_flags = np.ascontiguousarray(word_flags, dtype=np.int32)
        self.gaps = np.ascontiguousarray(gaps, dtype=np.float64)

    @property
    def n_images(self) -> int:
        return len(self.img_offsets) - 1

    @property
    def n_lines(self) -> int:
        return len(self.line_offsets) - 1

    @property
    def n_words(self) -> int:
        return len(self.order)

    @staticmethod
    def from_block(lp) -> "Lines":
        s = lp.contents

        def arr(ptr, n, dt):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, dt)
        return Lines(arr(s.img_offsets, s.n_images + 1, np.int32), arr(s.line_offsets, s.n_lines + 1, np.int32),
                     arr(s.order, s.n_words, np.int32), arr(s.word_flags, s.n_words, np.int32), arr(s.gaps, s.n_words, np.float64))

    def lines(self, b: int) -> List[Tuple[np.ndarray, np.ndarray]]:
        """image b: per line (batch-global word indices in reading order, their gaps)"""
        out = []
        for l in range(int(self.img_offsets[b]), int(self.img_offsets[b + 1])):
            p0, p1 = int(self.line_offsets[l]), int(self.line_offsets[l + 1])
            out.append((self.order[p0:p1].copy(), self.gaps[p0:p1].copy()))
        return out


def column_params(**fields) -> ColumnParams:
    """ocr_column_default_params with the given fields overridden: the line fields (line_tol, height_ratio, min_cos, max_gap), row_gap,
    min_gutter, gutter_reach, min_overlap, block_reach, min_rows, max_levels; `reserved` is the column block's, `line_reserved` the
    embedded line block's."""
    p = ColumnParams()
    lib().ocr_column_default_params(C.byref(p))
    own = dict(ColumnParams._fields_)
    for k, v in fields.items():
        if k == "reserved":
            p.reserved[0], p.reserved[1] = (int(x) for x in v)
        elif k == "line_reserved":
            p.line.reserved[0], p.line.reserved[1] = (int(x) for x in v)
        elif k in ("min_rows", "max_levels"):
            setattr(p, k, int(v))
        elif k in own and k != "line":
            setattr(p, k, float(v))
        elif k in dict(LineParams._fields_):
            setattr(p.line, k, float(v))
        else:
            raise TypeError(f"unknown column parameter {k!r}")
    return p


def _as_column_params(params) -> Optional[ColumnParams]:
    if params is None or isinstance(params, ColumnParams):
        return params
    return column_params(**params)


class Columns:
    """The arrays of an ocr_columns_t, copied into numpy: img_offsets [n_images+1] (block range per image), block_offsets [n_blocks+1]
    (line range per block), line_offsets [n_lines+1] (range of `order` per line), order [n_words], word_flags [n_words] by word index
    (1 isolated, 2 cycle cut, 4 gutter cut), gaps [n_words] by position, line_flags [n_lines], block_levels [n_blocks], block_quads
    [n_blocks, 8] (TL, TR, BR, BL)."""
    FIELDS = (("img_offsets", np.int32), ("block_offsets", np.int32), ("line_offsets", np.int32), ("order", np.int32),
              ("word_flags", np.int32), ("gaps", np.float64), ("line_flags", np.int32), ("block_levels", np.int32),
              ("block_quads", np.float64))

    def __init__(self, **arrays):
        for name, dt in self.FIELDS:
            setattr(self, name, np.ascontiguousarray(arrays[name], dtype=dt))
        self.block_quads = self.block_quads.reshape(-1, 8)

    @property
    def n_images(self) -> int:
        return len(self.img_offsets) - 1

    @property
    def n_blocks(self) -> int:
        return len(self.block_offsets) - 1

    @property
    def n_lines(self) -> int:
        return len(self.line_offsets) - 1

    @property
    def n_words(self) -> int:
        return len(self.order)

    @staticmethod
    def from_block(cp) -> "Columns":
        s = cp.contents
        sizes = {"img_offsets": s.n_images + 1, "block_offsets": s.n_blocks + 1, "line_offsets": s.n_lines + 1, "order": s.n_words,
                 "word_flags": s.n_words, "gaps": s.n_words, "line_flags": s.n_lines, "block_levels": s.n_blocks,
                 "block_quads": s.n_blocks * 8}
        return Columns(**{name: (np.ctypeslib.as_array(getattr(s, name), shape=(sizes[name],)).copy() if sizes[name] else np.zeros(0, dt))
                          for name, dt in Columns.FIELDS})

    def blocks(self, b: int) -> List[List[Tuple[np.ndarray, np.ndarray]]]:
        """image b: per block, per line (batch-global word indices in reading order, their gaps)"""
        out = []
        for k in range(int(self.img_offsets[b]), int(self.img_offsets[b + 1])):
            lines = []
            for l in range(int(self.block_offsets[k]), int(self.block_offsets[k + 1])):
                p0, p1 = int(self.line_offsets[l]), int(self.line_offsets[l + 1])
                lines.append((self.order[p0:p1].copy(), self.gaps[p0:p1].copy()))
            out.append(lines)
        return out


def lexicon_params(**fields) -> LexiconParams:
    """ocr_lexicon_default_params with the given fields overridden (ins_cost, del_cost, max_len_diff, fold_case, top_k)."""
    p = LexiconParams()
    lib().ocr_lexicon_default_params(C.byref(p))
    for k, v in fields.items():
        if k == "reserved":
            p.reserved[0], p.reserved[1], p.reserved[2] = (int(x) for x in v)
        elif k in ("ins_cost", "del_cost"):
            setattr(p, k, float(v))
        elif k in ("max_len_diff", "fold_case", "top_k"):
            setattr(p, k, int(v))
        else:
            raise TypeError(f"unknown lexicon parameter {k!r}")
    return p


def _as_lexicon_params(params) -> Optional[LexiconParams]:
    if params is None or isinstance(params, LexiconParams):
        return params
    return lexicon_params(**params)


class LexiconMatches:
    """The arrays of an ocr_lexicon_matches_t, copied into numpy: entries n_words x top_k int32 (the caller's entry index, -1 past the
    candidates), costs n_words x top_k f64 (+inf past the candidates), raw_costs [n_words] f64 (the greedy reading), n_candidates
    [n_words], word_flags [n_words] (1 no glyphs, 2 more than 32 glyphs, 4 no entry of an admissible length)."""

    def __init__(self, entries, costs, raw_costs, n_candidates, word_flags):
        self.entries = np.ascontiguousarray(entries, dtype=np.int32)
        self.costs = np.ascontiguousarray(costs, dtype=np.float64)
        self.raw_costs = np.ascontiguousarray(raw_costs, dtype=np.float64)
        self.n_candidates = np.ascontiguousarray(n_candidates, dtype=np.int32)
        self.word_flags = np.ascontiguousarray(word_flags, dtype=np.int32)

    @property
    def n_words(self) -> int:
        return self.entries.shape[0]

    @property
    def top_k(self) -> int:
        return self.entries.shape[1]

    @staticmethod
    def from_block(mp) -> "LexiconMatches":
        s = mp.contents
        nw, k = s.n_words, s.top_k

        def arr(ptr, n, dt):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, dt)
        return LexiconMatches(arr(s.entries, nw * k, np.int32).reshape(nw, k), arr(s.costs, nw * k, np.float64).reshape(nw, k),
                              arr(s.raw_costs, nw, np.float64), arr(s.n_candidates, nw, np.int32), arr(s.word_flags, nw, np.int32))


def phrase_params(**fields) -> PhraseParams:
    """ocr_phrase_default_params with the given fields overridden (word_cost, oov_word_cost, oov_glyph_cost, fold_case, reserved)."""
    p = PhraseParams()
    lib().ocr_phrase_default_params(C.byref(p))
    for k, v in fields.items():
        if k == "reserved":
            p.reserved[0], p.reserved[1], p.reserved[2] = (int(x) for x in v)
        elif k in ("word_cost", "oov_word_cost", "oov_glyph_cost"):
            setattr(p, k, float(v))
        elif k == "fold_case":
            p.fold_case = int(v)
        else:
            raise TypeError(f"unknown phrase parameter {k!r}")
    return p


def _as_phrase_params(params) -> Optional[PhraseParams]:
    if params is None or isinstance(params, PhraseParams):
        return params
    return phrase_params(**params)


class PhraseMatches:
    """The arrays of an ocr_phrase_matches_t, copied into numpy: line_word_offsets [n_lines+1] the word range of every line,
    word_offsets [n_words+1] the glyph rows of every word (an ordinary offset array: lm_decode and lexicon_match take it), entries
    [n_words] int32 (the caller's entry index, -1 for an out-of-vocabulary word), word_costs [n_words] f64, line_costs and raw_costs
    [n_lines] f64, line_flags [n_lines] (1 no glyphs, 2 more than PHRASE_MAX_GLYPHS glyphs)."""

    def __init__(self, line_word_offsets, word_offsets, entries, word_costs, line_costs, raw_costs, line_flags):
        self.line_word_offsets = np.ascontiguousarray(line_word_offsets, dtype=np.int32)
        self.word_offsets = np.ascontiguousarray(word_offsets, dtype=np.int32)
        self.entries = np.ascontiguousarray(entries, dtype=np.int32)
        self.word_costs = np.ascontiguousarray(word_costs, dtype=np.float64)
        self.line_costs = np.ascontiguousarray(line_costs, dtype=np.float64)
        self.raw_costs = np.ascontiguousarray(raw_costs, dtype=np.float64)
        self.line_flags = np.ascontiguousarray(line_flags, dtype=np.int32)

    @property
    def n_lines(self) -> int:
        return len(self.line_flags)

    @property
    def n_words(self) -> int:
        return len(self.entries)

    def line(self, l: int) -> "PhraseMatches":
        """The rows of line l as a block of one line: word_offsets relative to the line's first glyph."""
        w0, w1 = int(self.line_word_offsets[l]), int(self.line_word_offsets[l + 1])
        return PhraseMatches([0, w1 - w0], self.word_offsets[w0:w1 + 1] - self.word_offsets[w0], self.entries[w0:w1],
                             self.word_costs[w0:w1], self.line_costs[l:l + 1], self.raw_costs[l:l + 1], self.line_flags[l:l + 1])

    @staticmethod
    def from_block(mp) -> "PhraseMatches":
        s = mp.contents
        nl, nw = s.n_lines, s.n_words

        def arr(ptr, n, dt):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, dt)
        return PhraseMatches(arr(s.line_word_offsets, nl + 1, np.int32), arr(s.word_offsets, nw + 1, np.int32), arr(s.entries, nw, np.int32),
                             arr(s.word_costs, nw, np.float64), arr(s.line_costs, nl, np.float64), arr(s.raw_costs, nl, np.float64),
                             arr(s.line_flags, nl, np.int32))


def phrase_gap_costs(sub, breaks=None, break_penalty: float = 2.0, join_penalty: float = 2.0):
    """The gap costs of ocr_lexicon_phrase_match from the result of Detector.break_words (sub: the sub-words' GlyphSet, breaks: its
    WordBreaks): at a glyph that starts a sub-word the bound costs 0 and the join join_penalty - the gaps say a word starts there -,
    at every other glyph the bound costs break_penalty and the join 0.  -> (bound_cost, join_cost), f32 [n_glyphs]."""
    ng = sub.n_glyphs
    bound = np.full(ng, break_penalty, np.float32)
    join = np.zeros(ng, np.float32)
    starts = np.asarray(sub.word_offsets[:-1], np.int64)
    starts = starts[starts < ng]
    bound[starts] = 0.0
    join[starts] = join_penalty
    return bound, join


class Lexicon:
    """Owner of an ocr_lexicon_t: a word list over the recogniser's alphabet, uploaded once to the recogniser's GPU and resident there
    until close() (or the end of a `with` block).  words keeps the caller's list: results name its indices."""

    def __init__(self, rec: "Recognizer", words: Sequence[str]):
        self._h = C.c_void_p()
        self.words = list(words)
        raw = [w.encode("latin-1", "replace") if isinstance(w, str) else bytes(w) for w in self.words]
        offsets = np.zeros(len(raw) + 1, np.int64)
        offsets[1:] = np.cumsum(np.array([len(b) for b in raw], np.int64))
        if offsets[-1] > 0x7FFFFFFF:
            raise OcrError(1, "lexicon: more than 2^31 bytes")
        self._create(rec, b"".join(raw), offsets.astype(np.int32), len(raw))

    def _create(self, rec, blob: bytes, offsets: np.ndarray, n: int) -> None:
        buf = np.frombuffer(blob, np.uint8) if blob else np.zeros(1, np.uint8)
        check(lib().ocr_lexicon_create(rec._h, _ptr(buf), _ptr(offsets), n, C.byref(self._h)))

    @classmethod
    def from_bytes(cls, rec: "Recognizer", blob: bytes, offsets, n_entries: Optional[int] = None) -> "Lexicon":
        """The C call's own arguments: entry k is blob[offsets[k]:offsets[k + 1]] (nothing is checked here)."""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        n = len(off) - 1 if n_entries is None else int(n_entries)
        self.words = [blob[int(off[k]):int(off[k + 1])].decode("latin-1") for k in range(max(min(n, len(off) - 1), 0))]
        self._create(rec, blob, off, n)
        return self

    @property
    def handle(self):
        if not self._h:
            raise OcrError(1, "lexicon already closed")
        return self._h

    def __len__(self) -> int:
        n = C.c_int32(0)
        check(lib().ocr_lexicon_size(self.handle, C.byref(n)))
        return n.value

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            lib().ocr_lexicon_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_ALPHABET = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789"


def char_lm_table(words, counts=None, alpha: float = 0.5, weight: float = 1.0) -> np.ndarray:
    """A bigram model for ocr_char_lm_create from a word list, on the host: 64 x 64 f32, [p, c] the cost of class c behind class p, row 62
    begin-of-word, column 62 end-of-word.  Every word contributes its bigrams (begin, c_0), (c_0, c_1) .. (c_last, end), counts[k] times
    (once without counts); a row's 63 successors - the 62 classes and end-of-word, for the begin row the 62 classes - are smoothed by
    adding alpha to each count, and the cost is -log(probability) in f64 times weight, rounded to f32.  An empty word adds nothing.  A
    character outside the alphabet is OcrError."""
    if not (alpha > 0 and np.isfinite(alpha)) or not (weight >= 0 and np.isfinite(weight)):
        raise OcrError(1, f"char_lm_table: alpha={alpha} weight={weight} (alpha > 0, weight >= 0, both finite)")
    words = list(words)
    cnt = np.ones(len(words), np.float64) if counts is None else np.asarray(counts, np.float64).reshape(-1)
    if len(cnt) != len(words) or not np.all(np.isfinite(cnt)) or np.any(cnt < 0):
        raise OcrError(1, "char_lm_table: counts must be finite, >= 0 and one per word")
    cls = {ch: k for k, ch in enumerate(_ALPHABET)}
    n = np.zeros((64, 64), np.float64)
    for k, w in enumerate(words):
        if isinstance(w, bytes):
            w = w.decode("latin-1")
        prev = LM_BEGIN
        for ch in w:
            c = cls.get(ch)
            if c is None:
                raise OcrError(1, f"char_lm_table: word {k} holds {ch!r}, which is not in the alphabet")
            n[prev, c] += cnt[k]
            prev = c
        if w:
            n[prev, LM_END] += cnt[k]
    used = np.zeros((64, 64), bool)
    used[:63, :63] = True
    used[LM_BEGIN, LM_END] = False
    sm = np.where(used, n + float(alpha), 0.0)
    prob = sm / np.maximum(sm.sum(axis=1, keepdims=True), np.finfo(np.float64).tiny)
    with np.errstate(divide="ignore"):
        cost = np.where(used, -np.log(np.where(used, prob, 1.0)) * float(weight), 0.0)
    return np.where(used, np.maximum(cost, 0.0), 0.0).astype(np.float32)


def lm_params(**fields) -> LmParams:
    """ocr_lm_default_params with the given fields overridden (top_k)."""
    p = LmParams()
    lib().ocr_lm_default_params(C.byref(p))
    for k, v in fields.items():
        if k == "reserved":
            p.reserved[0], p.reserved[1], p.reserved[2] = (int(x) for x in v)
        elif k == "top_k":
            p.top_k = int(v)
        else:
            raise TypeError(f"unknown language-model parameter {k!r}")
    return p


def _as_lm_params(params) -> Optional[LmParams]:
    if params is None or isinstance(params, LmParams):
        return params
    return lm_params(**params)


class LmPaths:
    """The arrays of an ocr_lm_paths_t, copied into numpy: labels top_k x n_glyphs int32 (the class of every glyph row per hypothesis, -1
    where the word was not decoded), costs n_words x top_k f64 (+inf where it was not), raw_costs [n_words] f64 (the greedy reading under
    the model), word_flags [n_words] (1 no glyphs, 2 more than 32 glyphs)."""

    def __init__(self, labels, costs, raw_costs, word_flags):
        self.labels = np.ascontiguousarray(labels, dtype=np.int32)
        self.costs = np.ascontiguousarray(costs, dtype=np.float64)
        self.raw_costs = np.ascontiguousarray(raw_costs, dtype=np.float64)
        self.word_flags = np.ascontiguousarray(word_flags, dtype=np.int32)

    @property
    def n_words(self) -> int:
        return self.costs.shape[0]

    @property
    def top_k(self) -> int:
        return self.costs.shape[1]

    def text(self, word_offsets, w: int, k: int = 0) -> str:
        """hypothesis k of word w as a string ("" for a word that was not decoded)"""
        g0, g1 = int(word_offsets[w]), int(word_offsets[w + 1])
        lab = self.labels[k, g0:g1]
        return "".join(_ALPHABET[int(c)] for c in lab) if len(lab) and lab[0] >= 0 else ""

    def texts(self, word_offsets, k: int = 0) -> list:
        """hypothesis k of every word as a string ("" for a word that was not decoded), in one pass over the labels"""
        off = np.asarray(word_offsets, np.int64)
        lab = self.labels[k] if self.labels.shape[1] else np.zeros(0, np.int32)
        flat = np.frombuffer((_ALPHABET + "?").encode(), np.uint8)[np.where(lab >= 0, lab, 62)].tobytes().decode()
        return [flat[int(off[w]):int(off[w + 1])] if self.word_flags[w] == 0 else "" for w in range(len(off) - 1)]

    @staticmethod
    def from_block(mp) -> "LmPaths":
        s = mp.contents
        nw, k, ng = s.n_words, s.top_k, s.n_glyphs

        def arr(ptr, n, dt):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, dt)
        return LmPaths(arr(s.labels, k * ng, np.int32).reshape(k, ng), arr(s.costs, nw * k, np.float64).reshape(nw, k),
                       arr(s.raw_costs, nw, np.float64), arr(s.word_flags, nw, np.int32))


def split_params(**fields) -> SplitParams:
    """ocr_split_default_params with the given fields overridden (aspect_pct, max_pieces, min_piece_w, max_word_pieces, reserved)."""
    p = SplitParams()
    lib().ocr_split_default_params(C.byref(p))
    for k, v in fields.items():
        if k == "reserved":
            for i, x in enumerate(v):
                p.reserved[i] = int(x)
        elif k in ("aspect_pct", "max_pieces", "min_piece_w", "max_word_pieces"):
            setattr(p, k, int(v))
        else:
            raise TypeError(f"unknown split parameter {k!r}")
    return p


def _as_split_params(params) -> Optional[SplitParams]:
    if params is None or isinstance(params, SplitParams):
        return params
    return split_params(**params)


def break_params(**fields) -> BreakParams:
    """ocr_break_default_params with the given fields overridden (mode, space_pct, min_space_pct, sep_pct, min_gaps, reserved)."""
    p = BreakParams()
    lib().ocr_break_default_params(C.byref(p))
    for k, v in fields.items():
        if k == "reserved":
            for i, x in enumerate(v):
                p.reserved[i] = int(x)
        elif k in ("mode", "space_pct", "min_space_pct", "sep_pct", "min_gaps"):
            setattr(p, k, int(v))
        else:
            raise TypeError(f"unknown break parameter {k!r}")
    return p


def _as_break_params(params) -> Optional[BreakParams]:
    if params is None or isinstance(params, BreakParams):
        return params
    return break_params(**params)


class WordBreaks:
    """The arrays of an ocr_word_breaks_t, copied into numpy: source [n_words] the source word of every sub-word, sub_offsets
    [n_source+1] the sub-word range of every source word, gap_pct [n_words] the gap in front of a sub-word in percent of the source
    word's median glyph height (0 for the first of a source word), source_info n_source x 4 (hw, rule 0 / 1 / 2, threshold in pixels,
    flags: 2 = more than BREAK_MAX_GLYPHS glyphs, not broken)."""

    def __init__(self, source, sub_offsets, gap_pct, source_info):
        self.source = np.ascontiguousarray(source, dtype=np.int32)
        self.sub_offsets = np.ascontiguousarray(sub_offsets, dtype=np.int32)
        self.gap_pct = np.ascontiguousarray(gap_pct, dtype=np.int32)
        self.source_info = np.ascontiguousarray(source_info, dtype=np.int32).reshape(-1, 4)

    @property
    def n_source(self) -> int:
        return len(self.sub_offsets) - 1

    @property
    def n_words(self) -> int:
        return len(self.source)

    @staticmethod
    def from_block(bp) -> "WordBreaks":
        b = bp.contents

        def arr(ptr, n):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, np.int32)
        return WordBreaks(arr(b.source, b.n_words), arr(b.sub_offsets, b.n_source + 1), arr(b.gap_pct, b.n_words),
                          arr(b.source_info, 4 * b.n_source))


def lattice_params(**fields) -> LatticeParams:
    """ocr_lattice_default_params with the given fields overridden (max_span, top_k, span_cost: up to 4 values, reserved)."""
    p = LatticeParams()
    lib().ocr_lattice_default_params(C.byref(p))
    for k, v in fields.items():
        if k in ("reserved", "span_cost"):
            for i, x in enumerate(v):
                getattr(p, k)[i] = int(x) if k == "reserved" else float(x)
        elif k in ("max_span", "top_k"):
            setattr(p, k, int(v))
        else:
            raise TypeError(f"unknown lattice parameter {k!r}")
    return p


def _as_lattice_params(params) -> Optional[LatticeParams]:
    if params is None or isinstance(params, LatticeParams):
        return params
    return lattice_params(**params)


class SpanTable:
    """The arrays of an ocr_span_table_t, copied into numpy: span_word, span_end (e), span_len (m) per span, piece_offsets
    [n_words+1]; span_offsets [n_words+1] is the span block's word_offsets, kept beside them for the decode call."""

    def __init__(self, span_word, span_end, span_len, piece_offsets, span_offsets, max_span: int):
        self.span_word = np.ascontiguousarray(span_word, dtype=np.int32)
        self.span_end = np.ascontiguousarray(span_end, dtype=np.int32)
        self.span_len = np.ascontiguousarray(span_len, dtype=np.int32)
        self.piece_offsets = np.ascontiguousarray(piece_offsets, dtype=np.int32)
        self.span_offsets = np.ascontiguousarray(span_offsets, dtype=np.int32)
        self.max_span = int(max_span)

    @property
    def n_spans(self) -> int:
        return len(self.span_word)


def glyph_spans(pieces: "GlyphSet", max_span: int):
    """ocr_glyph_spans (host only): -> (the span block as a GlyphSet, whose word_offsets are the span ranges, and the SpanTable)."""
    blk = pieces.block()
    out, tab = C.POINTER(Glyphs)(), C.POINTER(SpanTableBlock)()
    check(lib().ocr_glyph_spans(C.byref(blk), int(max_span), C.byref(out), C.byref(tab)))
    try:
        spans = GlyphSet.from_block(out)
        t = tab.contents

        def arr(ptr, n):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, np.int32)
        return spans, SpanTable(arr(t.span_word, t.n_spans), arr(t.span_end, t.n_spans), arr(t.span_len, t.n_spans),
                                arr(t.piece_offsets, t.n_words + 1), spans.word_offsets, t.max_span)
    finally:
        lib().ocr_glyphs_free(out)
        lib().ocr_span_table_free(tab)


class LatticePaths:
    """The arrays of an ocr_lattice_paths_t, copied into numpy: labels and seg_len top_k x n_pieces int32 (class and length at the first
    piece of every segment, -1 / 0 elsewhere), n_chars n_words x top_k, costs n_words x top_k f64 (+inf where the word was not decoded),
    raw_costs [n_words] f64 (the all-singletons reading), word_flags [n_words] (1 no pieces, 2 more than 32 pieces)."""

    def __init__(self, labels, seg_len, n_chars, costs, raw_costs, word_flags):
        self.labels = np.ascontiguousarray(labels, dtype=np.int32)
        self.seg_len = np.ascontiguousarray(seg_len, dtype=np.int32)
        self.n_chars = np.ascontiguousarray(n_chars, dtype=np.int32)
        self.costs = np.ascontiguousarray(costs, dtype=np.float64)
        self.raw_costs = np.ascontiguousarray(raw_costs, dtype=np.float64)
        self.word_flags = np.ascontiguousarray(word_flags, dtype=np.int32)

    @property
    def n_words(self) -> int:
        return self.costs.shape[0]

    @property
    def top_k(self) -> int:
        return self.costs.shape[1]

    def text(self, piece_offsets, w: int, k: int = 0) -> str:
        """hypothesis k of word w as a string: the classes at the segment starts ("" for a word that was not decoded)"""
        lab = self.labels[k, int(piece_offsets[w]):int(piece_offsets[w + 1])]
        return "".join(_ALPHABET[int(c)] for c in lab if c >= 0)

    def texts(self, piece_offsets, k: int = 0) -> list:
        """hypothesis k of every word as a string ("" for a word that was not decoded)"""
        return [self.text(piece_offsets, w, k) for w in range(len(piece_offsets) - 1)]

    def segments(self, piece_offsets, w: int, k: int = 0) -> list:
        """hypothesis k of word w as [(first piece, length, class)] with piece indices into the block"""
        p0, p1 = int(piece_offsets[w]), int(piece_offsets[w + 1])
        return [(p, int(self.seg_len[k, p]), int(self.labels[k, p])) for p in range(p0, p1) if self.seg_len[k, p] > 0]

    @staticmethod
    def from_block(mp) -> "LatticePaths":
        s = mp.contents
        nw, k, n = s.n_words, s.top_k, s.n_pieces

        def arr(ptr, n, dt):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, dt)
        return LatticePaths(arr(s.labels, k * n, np.int32).reshape(k, n), arr(s.seg_len, k * n, np.int32).reshape(k, n),
                            arr(s.n_chars, nw * k, np.int32).reshape(nw, k), arr(s.costs, nw * k, np.float64).reshape(nw, k),
                            arr(s.raw_costs, nw, np.float64), arr(s.word_flags, nw, np.int32))


def lexlat_params(**fields) -> LexLatParams:
    """ocr_lexlat_default_params with the given fields overridden (ins_cost, del_cost, span_cost: up to 4 values, max_span,
    max_len_diff, fold_case, top_k, reserved)."""
    p = LexLatParams()
    lib().ocr_lexlat_default_params(C.byref(p))
    for k, v in fields.items():
        if k in ("reserved", "span_cost"):
            for i, x in enumerate(v):
                getattr(p, k)[i] = int(x) if k == "reserved" else float(x)
        elif k in ("ins_cost", "del_cost"):
            setattr(p, k, float(v))
        elif k in ("max_span", "max_len_diff", "fold_case", "top_k"):
            setattr(p, k, int(v))
        else:
            raise TypeError(f"unknown lexicon-lattice parameter {k!r}")
    return p


def _as_lexlat_params(params) -> Optional[LexLatParams]:
    if params is None or isinstance(params, LexLatParams):
        return params
    return lexlat_params(**params)


class LexLatMatches:
    """The arrays of an ocr_lexlat_matches_t, copied into numpy: entries and costs n_words x top_k (-1 and +inf past the candidates),
    raw_costs [n_words] f64 (the cheapest free segmentation), n_candidates and word_flags [n_words] (1 no pieces, 2 more than 32
    pieces, 4 no entry of an admissible length), seg_len and seg_char top_k x n_pieces int32 (m and the entry position at the first
    piece of a segment; seg_len 0 inside a segment, -1 at a deleted piece), n_ins n_words x top_k (entry characters without a
    segment)."""

    def __init__(self, entries, costs, raw_costs, n_candidates, word_flags, seg_len, seg_char, n_ins):
        self.entries = np.ascontiguousarray(entries, dtype=np.int32)
        self.costs = np.ascontiguousarray(costs, dtype=np.float64)
        self.raw_costs = np.ascontiguousarray(raw_costs, dtype=np.float64)
        self.n_candidates = np.ascontiguousarray(n_candidates, dtype=np.int32)
        self.word_flags = np.ascontiguousarray(word_flags, dtype=np.int32)
        self.seg_len = np.ascontiguousarray(seg_len, dtype=np.int32)
        self.seg_char = np.ascontiguousarray(seg_char, dtype=np.int32)
        self.n_ins = np.ascontiguousarray(n_ins, dtype=np.int32)

    @property
    def n_words(self) -> int:
        return self.entries.shape[0]

    @property
    def top_k(self) -> int:
        return self.entries.shape[1]

    def segments(self, piece_offsets, w: int, k: int = 0) -> list:
        """alignment k of word w as [(first piece, length, entry position)] with piece indices into the block"""
        p0, p1 = int(piece_offsets[w]), int(piece_offsets[w + 1])
        return [(p, int(self.seg_len[k, p]), int(self.seg_char[k, p])) for p in range(p0, p1) if self.seg_len[k, p] > 0]

    @staticmethod
    def from_block(mp) -> "LexLatMatches":
        s = mp.contents
        nw, k, n = s.n_words, s.top_k, s.n_pieces

        def arr(ptr, n, dt):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, dt)
        return LexLatMatches(arr(s.entries, nw * k, np.int32).reshape(nw, k), arr(s.costs, nw * k, np.float64).reshape(nw, k),
                             arr(s.raw_costs, nw, np.float64), arr(s.n_candidates, nw, np.int32), arr(s.word_flags, nw, np.int32),
                             arr(s.seg_len, k * n, np.int32).reshape(k, n), arr(s.seg_char, k * n, np.int32).reshape(k, n),
                             arr(s.n_ins, nw * k, np.int32).reshape(nw, k))


class CharLm:
    """Owner of an ocr_char_lm_t: a 64 x 64 bigram cost table (char_lm_table), uploaded once to the recogniser's GPU and resident there
    until close() (or the end of a `with` block)."""

    def __init__(self, rec: "Recognizer", table):
        self._h = C.c_void_p()
        t = np.ascontiguousarray(table, dtype=np.float32)
        if t.size != 64 * 64:
            raise OcrError(1, f"char lm: expected a 64 x 64 table, got shape {tuple(t.shape)}")
        self.table = t.reshape(64, 64).copy()
        check(lib().ocr_char_lm_create(rec._h, _ptr(self.table), C.byref(self._h)))

    @classmethod
    def from_words(cls, rec: "Recognizer", words, counts=None, alpha: float = 0.5, weight: float = 1.0) -> "CharLm":
        return cls(rec, char_lm_table(words, counts, alpha, weight))

    @property
    def handle(self):
        if not self._h:
            raise OcrError(1, "char lm already closed")
        return self._h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            lib().ocr_char_lm_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostBuffer:
    """Pinned host memory from ocr_host_alloc, viewed as a numpy array (frames / maps of the host-memory entry points)."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self._p = C.c_void_p()
        check(lib().ocr_host_alloc(self.nbytes, C.byref(self._p)))
        buf = (C.c_char * self.nbytes).from_address(self._p.value)
        self.array = np.frombuffer(buf, dtype=self.dtype).reshape(self.shape)

    def close(self) -> None:
        if self._p:
            self.array = None
            lib().ocr_host_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Detector:
    """Owns an ocr_det_t.  Mirrors `resnet18(&vs.root())` + `vs.load(..)`
    (/root/reference/src/text_detection/mod.rs:35-44)."""

    def __init__(self, weights_blob: Optional[bytes], device: int = 0, varstore_path: Optional[str] = None,
                 options: Optional[str] = None):
        """options: "key=value;..." engine options of ocr_det_create_with_options (None = defaults)."""
        self._h = C.c_void_p()
        self._blob = weights_blob
        self.device = device
        if varstore_path is not None:   # `vs.load(file)`: the library reads the tch archive itself
            check(lib().ocr_det_create_from_varstore(os.fsencode(varstore_path), device, C.byref(self._h)))
        else:
            check(lib().ocr_det_create_with_options(weights_blob, len(weights_blob), device,
                                                    options.encode() if options else None, C.byref(self._h)))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            lib().ocr_det_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, raw_stream: Optional[int]) -> None:
        check(lib().ocr_det_set_stream(self._h, C.c_void_p(raw_stream or 0)))

    def set_precision(self, precision: int) -> None:
        """PRECISION_F32 (default, the parity configuration) or PRECISION_BF16 (trunk + FPN in bf16)."""
        check(lib().ocr_det_set_precision(self._h, precision))

    def synchronize(self) -> None:
        check(lib().ocr_det_synchronize(self._h))

    def last_front_split(self) -> int:
        """Frames of the first frame group of the most recent forward (option front_split); 0 = it ran unsplit."""
        k = C.c_int32(-1)
        f = lib().ocr_det_last_front_split   # (bound here: A/B runs load libraries built before this entry point existed)
        f.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        check(f(self._h, C.byref(k)))
        return int(k.value)

    def last_top_side(self) -> int:
        """The moves of option top_side that the most recent forward took (a mask of 1 | 2 | 4); 0 = today's order."""
        m = C.c_int32(-1)
        f = lib().ocr_det_last_top_side   # (bound here, like last_front_split)
        f.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        check(f(self._h, C.byref(m)))
        return int(m.value)

    def forward_host(self, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)
        n, c, h, w = x.shape
        assert c == 1
        prob = np.empty((n, 1, h, w), np.float32)
        check(lib().ocr_det_forward(self._h, _ptr(x), n, h, w, _ptr(prob), MEM_HOST))
        return prob

    def forward_host_u8(self, x: np.ndarray) -> np.ndarray:
        """ocr_det_forward_u8 on a host batch of raw u8 luma frames (the reference's image type)."""
        x = np.ascontiguousarray(x, dtype=np.uint8)
        n, c, h, w = x.shape
        assert c == 1
        prob = np.empty((n, 1, h, w), np.float32)
        check(lib().ocr_det_forward_u8(self._h, _ptr(x), n, h, w, _ptr(prob), MEM_HOST))
        return prob

    def forward_u8_device(self, x_ptr: int, n: int, h: int, w: int, prob_ptr: int) -> None:
        """ocr_det_forward_u8 on device pointers (blocking)."""
        check(lib().ocr_det_forward_u8(self._h, x_ptr, n, h, w, prob_ptr, MEM_DEVICE))

    def detect_pipelined_host(self, x, n: int = 0, h: int = 0, w: int = 0, adjust_values=None, prob_out=None,
                              params: Optional[PostprocParams] = None, convert: bool = True):
        """ocr_det_detect_pipelined_host: x is a host array of frames (float32 or uint8, N x 1 x H x W; a HostBuffer view
        keeps the copy asynchronous) or None to flush.  Returns the PREVIOUS batch's polygons (None on the first call)."""
        adj_p = None
        xp, elem = None, ELEM_F32
        if x is not None:
            assert x.flags["C_CONTIGUOUS"] and x.dtype in (np.float32, np.uint8)
            n, _, h, w = x.shape
            elem = ELEM_U8 if x.dtype == np.uint8 else ELEM_F32
            xp = _ptr(x)
            adj = np.ascontiguousarray(adjust_values, dtype=np.float64).reshape(n, 2)
            adj_p = adj.ctypes.data_as(C.POINTER(C.c_double))
        out = C.POINTER(Polygons)()
        check(lib().ocr_det_detect_pipelined_host(self._h, xp, elem, n, h, w, _ptr(prob_out) if prob_out is not None else None, adj_p,
                                                  C.byref(params) if params is not None else None, C.byref(out)))
        if not out:
            return None
        try:
            return polygons_to_python(out) if convert else (out.contents.n_polygons, out.contents.n_vertices)
        finally:
            lib().ocr_polygons_free(out)

    def forward_device(self, x_ptr: int, n: int, h: int, w: int, prob_ptr: int, bitmap_ptr: int = 0,
                       thresh: float = 0.6) -> None:
        """Enqueue only (device pointers)."""
        check(lib().ocr_det_forward_async(self._h, x_ptr, n, h, w, prob_ptr, bitmap_ptr or None, thresh))

    def forward_profile(self, x_ptr: int, n: int, h: int, w: int, prob_ptr: int):
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        fl = (C.c_double * cap)()
        by = (C.c_double * cap)()
        cnt = C.c_int(0)
        check(lib().ocr_det_forward_profile(self._h, x_ptr, n, h, w, prob_ptr, cap, names, ms, fl, by, C.byref(cnt)))
        return [(names[i].decode(), float(ms[i]), float(fl[i]), float(by[i])) for i in range(cnt.value)]

    def postprocess_and_crops(self, prob: np.ndarray, frames: np.ndarray, adjust_values: np.ndarray,
                              params: Optional[PostprocParams] = None):
        """get_boxes_and_box_scores followed by the detect -> recognise crop step (host arrays):
        returns (polygons, scores, crops[P x 784])."""
        prob = np.ascontiguousarray(prob, dtype=np.float32)
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        n, _, h, w = prob.shape
        adj = np.ascontiguousarray(adjust_values, dtype=np.float64).reshape(n, 2)
        adj_p = adj.ctypes.data_as(C.POINTER(C.c_double))
        out = C.POINTER(Polygons)()
        check(lib().ocr_det_postprocess(self._h, _ptr(prob), n, h, w, MEM_HOST, adj_p,
                                        C.byref(params) if params is not None else None, C.byref(out)))
        try:
            crops = np.zeros((out.contents.n_polygons, 784), np.float32)
            check(lib().ocr_extract_crops(self._h, _ptr(frames), n, h, w, MEM_HOST, out, adj_p, _ptr(crops)))
            polys, scores = polygons_to_python(out)
            return polys, scores, crops
        finally:
            lib().ocr_polygons_free(out)

    def postprocess_and_crops_device(self, prob_ptr: int, frames_ptr: int, n: int, h: int, w: int, adjust_values,
                                     alloc_crops, params: Optional[PostprocParams] = None):
        """The same on device-resident tensors: prob / frames are device pointers (N x 1 x H x W f32),
        `alloc_crops(P)` returns the device pointer of a P x 784 f32 buffer once the polygon count P is known.
        Returns (polygons, scores, P)."""
        adj = np.ascontiguousarray(adjust_values, dtype=np.float64).reshape(n, 2)
        adj_p = adj.ctypes.data_as(C.POINTER(C.c_double))
        out = C.POINTER(Polygons)()
        check(lib().ocr_det_postprocess(self._h, prob_ptr, n, h, w, MEM_DEVICE, adj_p,
                                        C.byref(params) if params is not None else None, C.byref(out)))
        try:
            npoly = out.contents.n_polygons
            if npoly:
                check(lib().ocr_extract_crops(self._h, frames_ptr, n, h, w, MEM_DEVICE, out, adj_p, alloc_crops(npoly)))
            polys, scores = polygons_to_python(out)
            return polys, scores, npoly
        finally:
            lib().ocr_polygons_free(out)

    def _segment(self, frames_ptr, n: int, h: int, w: int, mem_kind: int, polys, adjust_values, params, cc=None) -> GlyphSet:
        st, keep = python_to_polygons(polys, [[0.0] * len(p) for p in polys]) if not isinstance(polys, Polygons) else (polys, None)
        adj = np.ascontiguousarray(adjust_values, dtype=np.float64).reshape(-1, 2)
        prm = _as_segment_params(params)
        out = C.POINTER(Glyphs)()
        prm_p = C.byref(prm) if prm is not None else None
        adj_p = adj.ctypes.data_as(C.POINTER(C.c_double))
        if cc is None:
            check(lib().ocr_segment_glyphs(self._h, frames_ptr, n, h, w, mem_kind, C.byref(st), adj_p, prm_p, C.byref(out)))
        else:
            ccp = _as_cc_params(cc)
            check(lib().ocr_segment_glyphs_cc(self._h, frames_ptr, n, h, w, mem_kind, C.byref(st), adj_p, prm_p, C.byref(ccp), C.byref(out)))
        try:
            return GlyphSet.from_block(out)
        finally:
            lib().ocr_glyphs_free(out)

    def segment_glyphs(self, frames: np.ndarray, polys, adjust_values, params=None, cc=None) -> GlyphSet:
        """Glyph segmentation of the words `polys` (per image the polygons in original-image pixels, as postprocess returns them, or a
        Polygons block) on host frames N x 1 x H x W f32.  params: SegmentParams, a dict of its fields, or None (defaults).
        cc: None for the column rule (ocr_segment_glyphs); CcParams or a dict of its fields ({} for the defaults) for the
        connected-component rule (ocr_segment_glyphs_cc), which splits kerned letters."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        n, _, h, w = frames.shape
        return self._segment(_ptr(frames), n, h, w, MEM_HOST, polys, adjust_values, params, cc)

    def segment_glyphs_device(self, frames_ptr: int, n: int, h: int, w: int, polys, adjust_values, params=None, cc=None) -> GlyphSet:
        """The same on device-resident frames (a device pointer to N x 1 x H x W f32)."""
        return self._segment(C.c_void_p(frames_ptr), n, h, w, MEM_DEVICE, polys, adjust_values, params, cc)

    def _split(self, frames_ptr, n: int, h: int, w: int, mem_kind: int, glyphs: GlyphSet, params):
        blk = glyphs.block()
        prm = _as_split_params(params)
        out, pm = C.POINTER(Glyphs)(), C.POINTER(PieceMapBlock)()
        check(lib().ocr_split_glyphs(self._h, frames_ptr, n, h, w, mem_kind, C.byref(blk), C.byref(prm) if prm is not None else None,
                                     C.byref(out), C.byref(pm)))
        try:
            m = pm.contents

            def arr(ptr):
                return np.ctypeslib.as_array(ptr, shape=(m.n_pieces,)).copy() if m.n_pieces else np.zeros(0, np.int32)
            return GlyphSet.from_block(out), np.stack([arr(m.glyph), arr(m.rank)], axis=1)
        finally:
            lib().ocr_glyphs_free(out)
            lib().ocr_piece_map_free(pm)

    def split_glyphs(self, frames: np.ndarray, glyphs: GlyphSet, params=None):
        """ocr_split_glyphs on host frames N x 1 x H x W f32: wide glyphs of `glyphs` cut at ink minima.  params: SplitParams, a dict of
        its fields, or None (defaults).  -> (the pieces as a GlyphSet, the piece map n_pieces x 2: source glyph, rank in it)."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        n, _, h, w = frames.shape
        return self._split(_ptr(frames), n, h, w, MEM_HOST, glyphs, params)

    def split_glyphs_device(self, frames_ptr: int, n: int, h: int, w: int, glyphs: GlyphSet, params=None):
        """The same on device-resident frames (a device pointer to N x 1 x H x W f32)."""
        return self._split(C.c_void_p(frames_ptr), n, h, w, MEM_DEVICE, glyphs, params)

    def break_words(self, glyphs: GlyphSet, params=None):
        """ocr_break_words: the words of `glyphs` (polygons) re-cut at their inter-word gaps.  params: BreakParams, a dict of its fields
        ({} = the defaults), or None (defaults).  -> (the sub-words as a GlyphSet over the same boxes, the WordBreaks map)."""
        blk = glyphs.block()
        prm = _as_break_params(params)
        out, wb = C.POINTER(Glyphs)(), C.POINTER(WordBreaksBlock)()
        check(lib().ocr_break_words(self._h, C.byref(blk), C.byref(prm) if prm is not None else None, C.byref(out), C.byref(wb)))
        try:
            return GlyphSet.from_block(out), WordBreaks.from_block(wb)
        finally:
            lib().ocr_glyphs_free(out)
            lib().ocr_word_breaks_free(wb)

    def _segment_labelled(self, frames_ptr, n: int, h: int, w: int, mem_kind: int, polys, adjust_values, params, cc):
        st, keep = python_to_polygons(polys, [[0.0] * len(p) for p in polys]) if not isinstance(polys, Polygons) else (polys, None)
        adj = np.ascontiguousarray(adjust_values, dtype=np.float64).reshape(-1, 2)
        prm, ccp = _as_segment_params(params), _as_cc_params(cc)
        out, lab = C.POINTER(Glyphs)(), C.POINTER(GlyphLabelsBlock)()
        check(lib().ocr_segment_glyphs_cc_labelled(self._h, frames_ptr, n, h, w, mem_kind, C.byref(st), adj.ctypes.data_as(C.POINTER(C.c_double)),
                                                   C.byref(prm) if prm is not None else None, C.byref(ccp) if ccp is not None else None,
                                                   C.byref(out), C.byref(lab)))
        try:
            return GlyphSet.from_block(out), GlyphLabels(self, lab)
        finally:
            lib().ocr_glyphs_free(out)

    def segment_glyphs_cc_labelled(self, frames: np.ndarray, polys, adjust_values, params=None, cc=None):
        """segment_glyphs(cc=...) on host frames that also keeps which glyph every ink pixel went to (ocr_segment_glyphs_cc_labelled):
        (GlyphSet, GlyphLabels).  cc: CcParams, a dict of its fields, or None for the defaults.  The labels live on the GPU until freed
        and are what extract_glyph_crops_masked needs."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        n, _, h, w = frames.shape
        return self._segment_labelled(_ptr(frames), n, h, w, MEM_HOST, polys, adjust_values, params, cc)

    def segment_glyphs_cc_labelled_device(self, frames_ptr: int, n: int, h: int, w: int, polys, adjust_values, params=None, cc=None):
        """The same on device-resident frames (a device pointer to N x 1 x H x W f32)."""
        return self._segment_labelled(C.c_void_p(frames_ptr), n, h, w, MEM_DEVICE, polys, adjust_values, params, cc)

    def extract_glyph_crops_masked(self, frames: np.ndarray, glyphs: GlyphSet, labels: GlyphLabels, params=None, mask=None) -> np.ndarray:
        """extract_glyph_crops through the label planes (ocr_extract_glyph_crops_masked): a kerned neighbour's ink inside a glyph's box
        reads as background.  mask: MaskParams, a dict of its fields ({"halo": 0}), or None / True for the defaults."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        n, _, h, w = frames.shape
        crops = np.empty((glyphs.n_glyphs, 784), np.float32)
        blk = glyphs.block()
        prm, mp = _as_segment_params(params), _as_mask_params(mask)
        check(lib().ocr_extract_glyph_crops_masked(self._h, _ptr(frames), n, h, w, MEM_HOST, C.byref(blk), labels.block,
                                                   C.byref(prm) if prm is not None else None, C.byref(mp) if mp is not None else None,
                                                   _ptr(crops)))
        return crops

    def extract_glyph_crops_masked_device(self, frames_ptr: int, n: int, h: int, w: int, glyphs: GlyphSet, labels: GlyphLabels,
                                          crops_ptr: int, params=None, mask=None) -> None:
        """The same on device memory: crops_ptr points at n_glyphs x 784 f32."""
        blk = glyphs.block()
        prm, mp = _as_segment_params(params), _as_mask_params(mask)
        check(lib().ocr_extract_glyph_crops_masked(self._h, C.c_void_p(frames_ptr), n, h, w, MEM_DEVICE, C.byref(blk), labels.block,
                                                   C.byref(prm) if prm is not None else None, C.byref(mp) if mp is not None else None,
                                                   C.c_void_p(crops_ptr)))

    def extract_glyph_crops(self, frames: np.ndarray, glyphs: GlyphSet, params=None) -> np.ndarray:
        """The 28 x 28 crop of every glyph (host frames) -> n_glyphs x 784 f32."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        n, _, h, w = frames.shape
        crops = np.empty((glyphs.n_glyphs, 784), np.float32)
        blk = glyphs.block()
        prm = _as_segment_params(params)
        check(lib().ocr_extract_glyph_crops(self._h, _ptr(frames), n, h, w, MEM_HOST, C.byref(blk), C.byref(prm) if prm is not None else None,
                                            _ptr(crops)))
        return crops

    def extract_glyph_crops_device(self, frames_ptr: int, n: int, h: int, w: int, glyphs: GlyphSet, crops_ptr: int, params=None) -> None:
        """The same on device memory: crops_ptr points at n_glyphs x 784 f32."""
        blk = glyphs.block()
        prm = _as_segment_params(params)
        check(lib().ocr_extract_glyph_crops(self._h, C.c_void_p(frames_ptr), n, h, w, MEM_DEVICE, C.byref(blk),
                                            C.byref(prm) if prm is not None else None, C.c_void_p(crops_ptr)))

    def plan_word_strips(self, polys, adjust_values, h: int, w: int, params=None, scores=None) -> WordStrips:
        """capi.plan_word_strips (host geometry; the handle is not used)."""
        return plan_word_strips(polys, adjust_values, h, w, params, scores)

    def extract_word_strips(self, frames: np.ndarray, strips: WordStrips) -> np.ndarray:
        """The atlas of `strips` from host frames N x 1 x H x W f32 -> height x total_width f32."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        n, _, h, w = frames.shape
        atlas = np.empty((strips.height, strips.total_width), np.float32)
        blk = strips.block()
        check(lib().ocr_extract_word_strips(self._h, _ptr(frames), n, h, w, MEM_HOST, C.byref(blk), _ptr(atlas) if atlas.size else None))
        return atlas

    def plan_curved_strips(self, polys, adjust_values, h: int, w: int, params=None, scores=None) -> CurvedStrips:
        """capi.plan_curved_strips (host geometry; the handle is not used)."""
        return plan_curved_strips(polys, adjust_values, h, w, params, scores)

    def extract_curved_strips(self, frames: np.ndarray, strips: CurvedStrips) -> np.ndarray:
        """The atlas of `strips` from host frames N x 1 x H x W f32 -> height x total_width f32."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        n, _, h, w = frames.shape
        atlas = np.empty((strips.height, strips.total_width), np.float32)
        blk = strips.block()
        check(lib().ocr_extract_curved_strips(self._h, _ptr(frames), n, h, w, MEM_HOST, C.byref(blk), _ptr(atlas) if atlas.size else None))
        return atlas

    def extract_curved_strips_device(self, frames_ptr: int, n: int, h: int, w: int, strips: CurvedStrips, atlas_ptr: int) -> None:
        """Device-memory form: frames and atlas are device pointers; blocking."""
        blk = strips.block()
        check(lib().ocr_extract_curved_strips(self._h, C.c_void_p(frames_ptr), n, h, w, MEM_DEVICE, C.byref(blk), C.c_void_p(atlas_ptr or None)))

    def extract_word_strips_device(self, frames_ptr: int, n: int, h: int, w: int, strips: WordStrips, atlas_ptr: int) -> None:
        """The same on device memory: atlas_ptr points at height x total_width f32."""
        blk = strips.block()
        check(lib().ocr_extract_word_strips(self._h, C.c_void_p(frames_ptr), n, h, w, MEM_DEVICE, C.byref(blk), C.c_void_p(atlas_ptr or None)))

    def group_lines(self, quads, img_offsets, params=None) -> Lines:
        """ocr_group_lines: quads n_words x 8 f64 (TL, TR, BR, BL, the quads of a WordStrips), img_offsets [n_images+1] the word range
        per image; params: LineParams, a dict of its fields, or None (defaults).  Blocking, on the handle's stream."""
        q = np.ascontiguousarray(quads, dtype=np.float64).reshape(-1)
        off = np.ascontiguousarray(img_offsets, dtype=np.int32).reshape(-1)
        prm = _as_line_params(params)
        out = C.POINTER(LinesBlock)()
        check(lib().ocr_group_lines(self._h, _ptr(q) if q.size else None, _ptr(off) if off.size else None, len(off) - 1,
                                    C.byref(prm) if prm is not None else None, C.byref(out)))
        try:
            return Lines.from_block(out)
        finally:
            lib().ocr_lines_free(out)

    def group_columns(self, quads, img_offsets, params=None) -> Columns:
        """ocr_group_columns: the arguments of group_lines; params: ColumnParams, a dict of its fields and the line fields, or None
        (defaults).  Blocking, on the handle's stream."""
        q = np.ascontiguousarray(quads, dtype=np.float64).reshape(-1)
        off = np.ascontiguousarray(img_offsets, dtype=np.int32).reshape(-1)
        prm = _as_column_params(params)
        out = C.POINTER(ColumnsBlock)()
        check(lib().ocr_group_columns(self._h, _ptr(q) if q.size else None, _ptr(off) if off.size else None, len(off) - 1,
                                      C.byref(prm) if prm is not None else None, C.byref(out)))
        try:
            return Columns.from_block(out)
        finally:
            lib().ocr_columns_free(out)

    def debug_stage(self, stage_id: int, shape_nhwc) -> np.ndarray:
        """Test hook: NHWC intermediate of the last forward, returned as NCHW."""
        n = C.c_size_t(0)
        check(test_lib().ocr_test_det_stage(self._h, stage_id, None, 0, C.byref(n)))
        out = np.empty(n.value, np.float32)
        check(test_lib().ocr_test_det_stage(self._h, stage_id, _ptr(out), n.value, C.byref(n)))
        return np.ascontiguousarray(out.reshape(shape_nhwc).transpose(0, 3, 1, 2))

    def preprocess_image(self, rgba: np.ndarray, target_w: int, target_h: int, want_f32: bool = False):
        """image_ops::preprocess_image after decoding: rgba h x w x 4 u8 -> (gray HxW u8[, f32 frame], adj_x, adj_y)."""
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        h, w = rgba.shape[:2]
        gray = np.empty((target_h, target_w), np.uint8)
        f32 = np.empty((1, 1, target_h, target_w), np.float32) if want_f32 else None
        adj = (C.c_double * 2)()
        check(lib().ocr_preprocess_image(self._h, _ptr(rgba), w, h, target_w, target_h, _ptr(gray),
                                         _ptr(f32) if want_f32 else None, adj, MEM_HOST))
        return (gray, f32, adj[0], adj[1]) if want_f32 else (gray, adj[0], adj[1])

    @staticmethod
    def _image_descs(images):
        """images: h x w x 4 u8 numpy arrays, or CUDA u8 tensors of that shape -> (ImageDesc array, mem kind, what keeps the pixels alive).
        A row stride that the ABI takes (pixels contiguous, rows a multiple of 4 bytes apart and not overlapping) is passed through as
        stride_bytes; anything else is copied to a contiguous array first."""
        kinds = {isinstance(im, np.ndarray) for im in images}
        if len(kinds) > 1:
            raise TypeError("preprocess_batch: numpy arrays and device tensors in one batch")
        host = kinds != {False}
        descs, keep = (ImageDesc * max(1, len(images)))(), []
        for i, im in enumerate(images):
            if im.ndim != 3 or im.shape[2] != 4 or (im.dtype != np.uint8 if host else str(im.dtype) != "torch.uint8"):
                raise TypeError(f"preprocess_batch: image {i} is not h x w x 4 uint8")
            if not host and not im.is_cuda:
                raise TypeError(f"preprocess_batch: image {i} is a host tensor (pass numpy arrays or CUDA tensors)")
            h, w = int(im.shape[0]), int(im.shape[1])
            st = tuple(im.strides) if host else tuple(int(v) for v in im.stride())
            if not (st[2] == 1 and st[1] == 4 and (st[0] >= 4 * w and st[0] % 4 == 0 or h == 1)):
                im = np.ascontiguousarray(im) if host else im.contiguous()
                st = (4 * w, 4, 1)
            keep.append(im)
            descs[i] = ImageDesc(_ptr(im), w, h, st[0] if h > 1 else 0)
        return descs, (MEM_HOST if host else MEM_DEVICE), keep

    def preprocess_batch(self, images, target_w: int, target_h: int, want_u8: bool = True, want_f32: bool = False, device_out: bool = False):
        """ocr_preprocess_batch: decoded images of differing sizes -> (gray N x H x W u8 or None, frames N x 1 x H x W f32 or None,
        adjust N x 2 f64), every frame bit for bit preprocess_image's.  images: a list of h x w x 4 u8 numpy arrays, or of CUDA u8
        tensors (whose producers must have finished: the handle's stream does not order against torch's); row strides are passed
        through, not copied.  The outputs are numpy arrays, or with device_out CUDA tensors.  Blocking."""
        descs, src_kind, keep = self._image_descs(images)
        n = len(images)
        if device_out:
            import torch
            dev = torch.device("cuda", self.device)
            gray = torch.empty((n, target_h, target_w), dtype=torch.uint8, device=dev) if want_u8 else None
            f32 = torch.empty((n, 1, target_h, target_w), dtype=torch.float32, device=dev) if want_f32 else None
        else:
            gray = np.empty((n, target_h, target_w), np.uint8) if want_u8 else None
            f32 = np.empty((n, 1, target_h, target_w), np.float32) if want_f32 else None
        adj = np.zeros((n, 2), np.float64)
        check(lib().ocr_preprocess_batch(self._h, descs, n, src_kind, target_w, target_h, _ptr(gray) if want_u8 else None,
                                         _ptr(f32) if want_f32 else None, MEM_DEVICE if device_out else MEM_HOST,
                                         adj.ctypes.data_as(C.POINTER(C.c_double))))
        del keep
        return gray, f32, adj

    def preprocess_batch_async(self, images, target_w: int, target_h: int, gray=None, f32=None) -> np.ndarray:
        """ocr_preprocess_batch_async: CUDA u8 tensors in, frames into the CUDA tensors gray (N x H x W u8) and / or f32 (N x 1 x H x W),
        queued on the handle's stream; returns the N x 2 adjust array (valid at once).  Images and outputs must stay alive and
        unchanged until synchronize()."""
        descs, src_kind, keep = self._image_descs(images)
        if src_kind != MEM_DEVICE and images:
            raise TypeError("preprocess_batch_async takes device tensors")
        n = len(images)
        adj = np.zeros((n, 2), np.float64)
        check(lib().ocr_preprocess_batch_async(self._h, descs, n, target_w, target_h, _ptr(gray) if gray is not None else None,
                                               _ptr(f32) if f32 is not None else None, adj.ctypes.data_as(C.POINTER(C.c_double))))
        self._pre_keep = keep   # (a .contiguous() copy made above lives until the next call)
        return adj

    def debug_conv_bench(self, n, h, w, cin, cout, ks=3, stride=1, src_mode=0, iters=5) -> float:
        """Test hook: average milliseconds of one conv_igemm launch of this shape."""
        ms = C.c_float(0.0)
        check(test_lib().ocr_test_conv_bench(self._h, n, h, w, cin, cout, ks, stride, src_mode, iters, C.byref(ms)))
        return ms.value

    def debug_conv_run(self, x_nhwc, wgt_ohwi, stride=1, scale=None, bias=None, residual=None, up_residual=None,
                       relu=False, cat4_shape=None, in_bf16=False, out_bf16=False, want_out=True, want_out2=False, variant=0):
        """One conv_igemm launch on caller data (test hook).  x_nhwc: N x H x W x Cin f32, or with
        cat4_shape=(n, h, w) the flat concatenation p5|p4|p3|p2.  Returns (out, out2) as N x Ho x Wo x Cout f32."""
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        x, wg = f(x_nhwc), f(wgt_ohwi)
        cout, kk, cin = wg.shape
        ks = int(round(kk ** 0.5))
        n, h, w = cat4_shape if cat4_shape else x.shape[:3]
        pad = (ks - 1) // 2
        ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
        out = np.empty((n, ho, wo, cout), np.float32) if want_out else None
        out2 = np.empty((n, ho, wo, cout), np.float32) if want_out2 else None
        sc, bi, rs, ur = f(scale), f(bias), f(residual), f(up_residual)
        p = lambda a: None if a is None else _ptr(a)
        check(test_lib().ocr_test_conv_run(self._h, int(in_bf16), int(out_bf16), _ptr(x), n, h, w, cin, _ptr(wg), cout, ks,
                                           stride, p(sc), p(bi), p(rs), p(ur), int(relu), int(bool(cat4_shape)), int(variant),
                                           p(out), p(out2)))
        return out, out2

    def debug_phase_conv_run(self, form, x_nhwc, wphase, up, win=0, out_bf16=False, bias=None, relu=False, residual=None, poison=False,
                             guard=64, sentinel=-7.0):
        """One conv_igemm launch with STORE_PHASE on caller data (test hook): form 0 exact f32, 1 split bf16, 2 bf16 operands (rounded
        inside).  x: N x h x w x Cin; wphase: [up*up][Cout][2x2][Cin] (phase_weights); residual: N x up h x up w x Cout, added IN PLACE (it is
        what the output buffer holds before the launch, as the engine runs it); without one the buffer holds `sentinel`.  poison: the guard
        regions around the source inside its allocation hold NaN instead of zeros.  Returns (out N x up h x up w x Cout f32, the `guard`
        rows of Cout elements behind it, which went to the device as `sentinel`)."""
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        x, wg, bi = f(x_nhwc), f(wphase), f(bias)
        n, h, w, cin = x.shape
        cout = wg.shape[1]
        assert wg.shape == (up * up, cout, 4, cin), wg.shape
        px = n * up * h * up * w
        io = np.full((px + guard, cout), sentinel, np.float32)
        if residual is not None:
            io[:px] = np.asarray(residual, np.float32).reshape(px, cout)
        check(test_lib().ocr_test_phase_conv_run(self._h, int(form), int(bool(out_bf16)), _ptr(x), n, h, w, cin, _ptr(wg), cout, int(up), int(win),
                                                 None if bi is None else _ptr(bi), int(bool(relu)), int(residual is not None), int(bool(poison)),
                                                 _ptr(io), int(guard)))
        return io[:px].reshape(n, up * h, up * w, cout), io[px:]

    def debug_pyr4_conv_run(self, form, levels, wpyr, nsrc=4, out_bf16=False, bias=None, relu=False, residual=None, launches=0, poison=False,
                            guard=64, sentinel=-7.0):
        """One (or, launches = 3, two) conv_igemm launches with SRC_PYR4 on caller data (test hook): form as above; levels = (p5, p4, p3, p2) as
        N x (h << i) x (w << i) x 64 (p2 may be None with nsrc 3); wpyr: [64][64][21][64] (pyr4_weights); residual: N x 8h x 8w x 64, a separate
        array; launches: 0 = pyr_group 0, 1 / 2 = that group alone, 3 = group 1 then 2.  poison: the gaps around the four sources inside their
        shared allocation hold NaN.  Returns (out N x 8h x 8w x 64 f32, guard rows); the output buffer holds `sentinel` before the launch."""
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        lv = [f(a) for a in levels]
        n, h, w, _ = lv[0].shape
        for i, a in enumerate(lv):
            assert a is None or a.shape == (n, h << i, w << i, 64), (i, a.shape)
        wg, bi, rs = f(wpyr), f(bias), f(residual)
        assert wg.shape == (64, 64, 21, 64), wg.shape
        px = n * 8 * h * 8 * w
        assert rs is None or rs.size == px * 64
        io = np.full((px + guard, 64), sentinel, np.float32)
        p = lambda a: None if a is None else _ptr(a)
        check(test_lib().ocr_test_pyr4_conv_run(self._h, int(form), int(bool(out_bf16)), p(lv[0]), p(lv[1]), p(lv[2]), p(lv[3]), n, h, w, _ptr(wg),
                                                int(nsrc), p(bi), int(bool(relu)), p(rs), int(launches), int(bool(poison)), _ptr(io), int(guard)))
        return io[:px].reshape(n, 8 * h, 8 * w, 64), io[px:]

    def debug_stem_run(self, form, frames, w64x49, scale64, bias64, poison=0, guard=None, sentinel=-7.0):
        """The stem alone on caller data (test hook): form 0 exact f32, 1 bf16 precision, 2 split bf16.  frames: N x H x W, uint8 (raw luma)
        or f32; w64x49: conv1.weight as [64][49].  Returns N x H/4 x W/4 x 64 f32 (form 1: the bf16 output widened).
        The frames sit between two leads of zeros, of quiet NaN (poison=1; uint8 frames: 255) or of +inf (poison=2; uint8: 255).  With
        guard=g the result is (out, the g rows of 64 behind it), which went to the device as `sentinel` and come back as the kernel left them."""
        x = np.ascontiguousarray(frames)
        if x.dtype != np.uint8:
            x = np.ascontiguousarray(x, dtype=np.float32)
        n, h, w = x.shape
        f = lambda a, shape: np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(shape))
        wg, sc, bi = f(w64x49, (64, 49)), f(scale64, (64,)), f(bias64, (64,))
        rows, g = n * (h // 4) * (w // 4), int(guard or 0)
        io = np.full((rows + g, 64), sentinel, np.float32)
        check(test_lib().ocr_test_stem_run(self._h, int(form), _ptr(x), int(x.dtype == np.uint8), n, h, w, _ptr(wg), _ptr(sc), _ptr(bi), int(poison),
                                           _ptr(io), g))
        out = io[:rows].reshape(n, h // 4, w // 4, 64)
        return out if guard is None else (out, io[rows:])

    def debug_head_run(self, form, y_nhwc, wt1, s4, b4, w2t, bias2=0.0, thresh=0.5, want_bitmap=True, poison=0, guard=None, sentinel=-7.0,
                       bitmap_sentinel=9):
        """The fused head alone on caller data (test hook): form 0 f32 MFMA, 1 bf16 operands (y and wt1 rounded inside), 2 split bf16.
        y: N x h4 x w4 x 64; wt1: [4 taps a*2+b][64 co][64 ci]; s4 / b4: [256] (tap * 64 + co); w2t: [64 co][4 u = c'*2+d'].
        Returns (prob N x 4 h4 x 4 w4 f32, bitmap u8 or None).
        y sits between two leads of zeros, quiet NaN (poison=1) or +inf (poison=2).  With guard=g the result is (prob, bitmap or None, prob's
        guard g x 4 w4, bitmap's guard or None): rows that went to the device as the sentinels and come back as the kernel left them."""
        y = np.ascontiguousarray(y_nhwc, dtype=np.float32)
        n, h4, w4, c = y.shape
        assert c == 64
        f = lambda a, shape: np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(shape))
        wt, s, b, w2 = f(wt1, (4, 64, 64)), f(s4, (256,)), f(b4, (256,)), f(w2t, (64, 4))
        rows, g = n * 4 * h4, int(guard or 0)
        pio = np.full((rows + g, 4 * w4), sentinel, np.float32)
        bio = np.full((rows + g, 4 * w4), bitmap_sentinel, np.uint8) if want_bitmap else None
        check(test_lib().ocr_test_head_run(self._h, int(form), _ptr(y), n, h4, w4, _ptr(wt), _ptr(s), _ptr(b), _ptr(w2), float(bias2), float(thresh),
                                           int(poison), _ptr(pio), _ptr(bio) if want_bitmap else None, g))
        prob = pio[:rows].reshape(n, 4 * h4, 4 * w4)
        bm = bio[:rows].reshape(n, 4 * h4, 4 * w4) if want_bitmap else None
        return (prob, bm) if guard is None else (prob, bm, pio[rows:], bio[rows:] if want_bitmap else None)

    def debug_convt2_sigmoid(self, x_nhwc, w4x64, bias=0.0, thresh=0.5, want_bitmap=True, poison=0, guard=8, sentinel=-7.0, bitmap_sentinel=9):
        """convt2_sigmoid_kernel alone on caller data (test hook): x N x H2 x W2 x 64 f32 between two leads (zeros, NaN or +inf as poison = 0, 1,
        2); w4x64 [4 taps a*2+b][64].  Returns (prob N x 2 H2 x 2 W2 f32, bitmap u8 or None, prob's guard rows, bitmap's guard rows or None)."""
        x = np.ascontiguousarray(x_nhwc, dtype=np.float32)
        n, h2, w2, c = x.shape
        assert c == 64
        wt = np.ascontiguousarray(np.asarray(w4x64, dtype=np.float32).reshape(4, 64))
        rows, g = n * 2 * h2, int(guard)
        pio = np.full((rows + g, 2 * w2), sentinel, np.float32)
        bio = np.full((rows + g, 2 * w2), bitmap_sentinel, np.uint8) if want_bitmap else None
        check(test_lib().ocr_test_convt2_sigmoid(self._h, _ptr(x), n, h2, w2, _ptr(wt), float(bias), float(thresh), int(poison), _ptr(pio),
                                                 _ptr(bio) if want_bitmap else None, g))
        return (pio[:rows].reshape(n, 2 * h2, 2 * w2), bio[:rows].reshape(n, 2 * h2, 2 * w2) if want_bitmap else None, pio[rows:],
                bio[rows:] if want_bitmap else None)

    def debug_binarize(self, prob, thresh, poison=0, guard=64, sentinel=9):
        """launch_binarize on caller data (test hook): prob, any shape, f32, between two leads.  Returns (bitmap u8 [size], its guard bytes)."""
        x = np.ascontiguousarray(prob, dtype=np.float32).reshape(-1)
        io = np.full(x.size + int(guard), sentinel, np.uint8)
        check(test_lib().ocr_test_binarize(self._h, _ptr(x), x.size, float(thresh), int(poison), _ptr(io), int(guard)))
        return io[:x.size], io[x.size:]

    def debug_binarize_pack(self, prob, thresh, poison=0, guard=8, sentinel=0xA5A5A5A5):
        """launch_binarize_pack on caller data (test hook): prob n_images x px_per_image f32 between two leads.  Returns (words u32
        [n_images][2 ceil(px / 64)], the guard words behind them)."""
        x = np.ascontiguousarray(prob, dtype=np.float32)
        n, px = x.shape
        words = n * ((px + 63) // 64 * 2)
        io = np.full(words + int(guard), sentinel, np.uint32)
        check(test_lib().ocr_test_binarize_pack(self._h, _ptr(x), n, px, float(thresh), int(poison), _ptr(io), int(guard)))
        return io[:words].reshape(n, -1), io[words:]

    def debug_bf16_basic_block(self, x_nhwc, w1, w2, scale1=None, bias1=None, scale2=None, bias2=None, fused=True, num_cus=0, iters=1):
        """one BasicBlock 64 -> 64 of the bf16 precision (test hook): fused = basic_block_bf16_c64.hip (one launch), otherwise two
        conv3x3_bf16_c64 launches.  x N x H x W x 64 f32 (rounded to bf16 inside), w [64][9][64].  Returns (out f32, ms per block)."""
        x = np.ascontiguousarray(x_nhwc, dtype=np.float32)
        n, h, w, c = x.shape
        assert c == 64
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        p = lambda a: None if a is None else _ptr(a)
        w1, w2, s1, b1, s2, b2 = f(w1), f(w2), f(scale1), f(bias1), f(scale2), f(bias2)
        out = np.empty_like(x)
        ms = C.c_float(0.0)
        check(test_lib().ocr_test_bf16_basic_block(self._h, _ptr(x), n, h, w, _ptr(w1), p(s1), p(b1), _ptr(w2), p(s2), p(b2), int(bool(fused)),
                                                   int(num_cus), int(iters), _ptr(out), C.byref(ms)))
        return out, ms.value

    def debug_gemm_batched(self, x_bmk, w_bnk, variant=2, scale=None, bias=None, relu=False):
        """B independent GEMMs out[b] = x[b] @ w[b].T through conv_igemm's batched 1x1 mode (test hook; what the Winograd GEMMs of layer3 /
        layer4 launch): x B x M x K, w B x N x K -> B x M x N.  variant 0 f32 MFMA, 2 split-bf16 128-wide tiles, 3 the 256 x 128 form."""
        x = np.ascontiguousarray(x_bmk, dtype=np.float32)
        wg = np.ascontiguousarray(w_bnk, dtype=np.float32)
        b, m, k = x.shape
        _, nn, _ = wg.shape
        out = np.empty((b, m, nn), np.float32)
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        sc, bi = f(scale), f(bias)
        p = lambda a: None if a is None else _ptr(a)
        check(test_lib().ocr_test_conv_run(self._h, 0, 0, _ptr(x), 1, 1, m, k, _ptr(wg), nn, 1, 1, p(sc), p(bi), None, None, int(relu), 0,
                                           int(variant) | (b << 8), _ptr(out), None))
        return out

    def debug_winograd_conv(self, x_nhwc, wgt_ohwi, scale=None, bias=None, residual=None, relu=False, unfused=False):
        """3x3 s1 p1 conv through the Winograd path on caller data (test hook): N x H x W x Cout f32."""
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        x, wg = f(x_nhwc), f(wgt_ohwi)
        n, h, w, cin = x.shape
        cout = wg.shape[0]
        assert wg.shape == (cout, 9, cin)
        sc, bi, rs = f(scale), f(bias), f(residual)
        p = lambda a: None if a is None else _ptr(a)
        out = np.empty((n, h, w, cout), np.float32)
        check(test_lib().ocr_test_winograd_conv(self._h, _ptr(x), n, h, w, cin, _ptr(wg), cout, p(sc), p(bi), p(rs),
                                                int(relu), int(unfused), _ptr(out)))
        return out

    def debug_winograd_run(self, form, x_nhwc, wgt_ohwi, scale=None, bias=None, residual=None, relu=False, inplace=False, num_cus=0,
                           guard=64, poison=False, sentinel=-7.0):
        """One 3x3 s1 p1 conv through a Winograd form on caller data (test hook): form 0 the fused F(4x4,3x3) kernel (num_cus sizes its grid),
        1 the three launches of F(4x4,3x3) with the 36 split-bf16 GEMMs as the engine runs them, 2 the same with exact-f32 GEMMs, 3 the three
        launches of F(2x2,3x3).  x: N x H x W x Cin; wgt: [Cout][9][Cin]; residual: N x H x W x Cout - with inplace it is what the output buffer
        holds before the launch and the launch gets residual == y, otherwise a separate buffer; without one the buffer holds `sentinel`.
        poison: the regions around the source inside its allocation hold NaN instead of zeros.  Returns (out N x H x W x Cout f32, the `guard`
        rows of Cout elements behind it, which went to the device as `sentinel`)."""
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        x, wg, sc, bi = f(x_nhwc), f(wgt_ohwi), f(scale), f(bias)
        n, h, w, cin = x.shape
        cout = wg.shape[0]
        assert wg.shape == (cout, 9, cin), wg.shape
        assert not inplace or residual is not None
        px = n * h * w
        io = np.full((px + guard, cout), sentinel, np.float32)
        rs = None
        if residual is not None:
            rs = np.ascontiguousarray(np.asarray(residual, np.float32).reshape(px, cout))
            if inplace:
                io[:px] = rs
                rs = None
        p = lambda a: None if a is None else _ptr(a)
        check(test_lib().ocr_test_winograd_run(self._h, int(form), _ptr(x), n, h, w, cin, _ptr(wg), cout, p(sc), p(bi), p(rs), int(bool(relu)),
                                               int(bool(inplace)), int(num_cus), int(bool(poison)), _ptr(io), int(guard)))
        return io[:px].reshape(n, h, w, cout), io[px:]

    def debug_winograd_topdown(self, x_nhwc, low_nhwc=None, guard=64, sentinel=-7.0):
        """The F(4x4) input transform alone (test hook): with low (N x H/2 x W/2 x C) the engine's top_side form, which adds up2(low) on load;
        without it the plain transform of x.  Both sources sit between NaN regions of their allocations.  Returns (V [36][T][C], the `guard`
        elements behind it, which went to the device as `sentinel`)."""
        x = np.ascontiguousarray(x_nhwc, dtype=np.float32)
        low = None if low_nhwc is None else np.ascontiguousarray(low_nhwc, dtype=np.float32)
        n, h, w, c = x.shape
        assert low is None or low.shape == (n, h // 2, w // 2, c), low.shape
        T = n * ((h + 3) // 4) * ((w + 3) // 4)
        io = np.full(36 * T * c + guard, sentinel, np.float32)
        f = test_lib().ocr_test_winograd_topdown
        f.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p, C.c_int]
        check(f(self._h, _ptr(x), None if low is None else _ptr(low), n, h, w, c, _ptr(io), int(guard)))
        return io[:36 * T * c].reshape(36, T, c), io[36 * T * c:]

    def debug_bf16_trunk_run(self, form, x_nhwc, wgt_ohwi, scale=None, bias=None, residual=None, relu=False, stride=1, up_residual=None, want_out=True,
                             wgt2=None, scale2=None, bias2=None, num_cus=0, guard=64, poison=False, sentinel=-7.0, claim=None):
        """One launch of the bf16 precision's trunk on caller data (test hook): form 0 conv3x3_bf16_c64 (grid 2 x num_cus), 1 basic_block_bf16_c64
        (conv (wgt, scale, bias) + ReLU, conv (wgt2, scale2, bias2), + x, ReLU; grid num_cus), 2 conv_igemm with bf16 operands and results
        (kernel 1x1 or 3x3 by wgt's shape, stride 1 or 2; with up_residual [N][Ho / 2][Wo / 2][Cout] the second output is value + its nearest
        upsample, and want_out=False stores that sum only).  Arrays are f32 and are rounded to bf16 on the way in.  poison: the regions around
        the source inside its allocation hold NaN instead of zeros.  Returns (out or None, out2 or None, guard): N x Ho x Wo x Cout f32 each, and
        the `guard` rows of Cout elements behind every output, one after the other, which went to the device as `sentinel`.  claim: an (N, H, W)
        handed to the hook instead of x's own, for shapes the launchers refuse by their arguments alone - the outputs are not allocated."""
        f = lambda a, shape=None: None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape or np.shape(a)))
        x, wg = f(x_nhwc), f(wgt_ohwi)
        n, h, w, cin = x.shape
        cout, taps = wg.shape[0], wg.shape[1]
        ks = {1: 1, 9: 3}[taps]
        assert wg.shape == (cout, taps, cin), wg.shape
        pad = (ks - 1) // 2
        ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
        px = n * ho * wo
        if claim is not None:
            n, h, w = claim
            px = 0
        io = np.full((px + guard, cout), sentinel, np.float32) if want_out else None
        io2 = np.full((px + guard, cout), sentinel, np.float32) if up_residual is not None else None
        p = lambda a: None if a is None else _ptr(a)
        ops = [f(scale), f(bias), f(residual, (-1, cout)), f(up_residual, (-1, cout)), f(wgt2), f(scale2), f(bias2)]
        check(test_lib().ocr_test_bf16_trunk_run(self._h, int(form), _ptr(x), n, h, w, cin, _ptr(wg), cout, ks, int(stride), p(ops[0]), p(ops[1]), p(ops[2]),
                                                 p(ops[3]), int(bool(relu)), p(ops[4]), p(ops[5]), p(ops[6]), int(num_cus), int(bool(poison)), p(io), p(io2),
                                                 int(guard)))
        outs = [None if a is None else a[:px].reshape(-1, ho, wo, cout) for a in (io, io2)]
        return outs[0], outs[1], np.concatenate([a[px:] for a in (io, io2) if a is not None])

    def debug_igemm_run(self, form, x, wgt, out_bf16=False, stride=1, src_mode=0, store_mode=0, scale=None, bias=None, residual=None, up_residual=None,
                        want_out=True, want_out2=False, relu=False, tile=0, poison=False, guard=64, sentinel=-7.0, claim=None):
        """One launch_conv_igemm with a SRC_PLAIN (0) / SRC_CAT4 (2) source and a STORE_NHWC (0) / STORE_SHUFFLE2 (1) store on caller data (test
        hook).  form 0 exact f32, 1 split bf16, 2 bf16 operands; out_bf16: bf16 results and residuals.  x: [N][H][W][Cin], [B][N][H][W][Cin] for the
        batched GEMM of B problems, or for CAT4 the four levels (p5, p4, p3, p2) of 64 channels; wgt: [Cout][ks ks][Cin] ([B][Cout][1][Cin]).
        want_out2: the second output, value + nearest_up2(up_residual [N][Ho / 2][Wo / 2][Cout]).  tile: 0 automatic, 1 128 x 128, 2 128 x 64,
        3 64 x 64, for this launch only.  poison: the regions around the source (and between the levels) inside its allocation hold NaN instead of
        zeros.  Returns (out or None, out2 or None, guard): f32 arrays [N][Ho][Wo][Cout] ([B][N].. batched; [N][2 Ho][2 Wo][64] shuffled) and the
        `guard` rows behind every output, one after the other, which went to the device as `sentinel`.  claim: an (N, H, W) handed to the hook
        instead of x's own, for shapes the launcher refuses by their size alone - nothing is allocated."""
        f = lambda a, shape=None: None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape or np.shape(a)))
        wg = f(wgt)
        batch = wg.shape[0] if wg.ndim == 4 else 1
        cout, taps, cin = wg.shape[-3:]
        ks = {1: 1, 9: 3}[taps]
        if src_mode == 2:
            levels = [f(a) for a in x]
            n, h, w, _ = levels[3].shape
            assert [a.shape for a in levels] == [(n, h >> (3 - l), w >> (3 - l), 64) for l in range(4)], [a.shape for a in levels]
            xs = np.concatenate([a.reshape(-1) for a in levels])
        else:
            xs = f(x)
            assert xs.ndim == (5 if wg.ndim == 4 else 4) and xs.shape[-1] == cin and (wg.ndim == 3 or xs.shape[0] == batch), (xs.shape, wg.shape)
            n, h, w = xs.shape[-4:-1]
        pad = (ks - 1) // 2
        ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
        shape = (n, 2 * ho, 2 * wo, 64) if store_mode == 1 else ((batch,) if wg.ndim == 4 else ()) + (n, ho, wo, cout)
        rows, row = int(np.prod(shape[:-1])), shape[-1]
        if claim is not None:
            n, h, w = claim
            rows = 0
        io = np.full((rows + guard, row), sentinel, np.float32) if want_out else None
        io2 = np.full((rows + guard, row), sentinel, np.float32) if want_out2 else None
        p = lambda a: None if a is None else _ptr(a)
        ops = [f(scale), f(bias), f(residual), f(up_residual)]
        check(test_lib().ocr_test_igemm_run(self._h, int(form), int(bool(out_bf16)), _ptr(xs), n, h, w, cin, _ptr(wg), cout, ks, int(stride), int(src_mode),
                                            int(store_mode), batch, p(ops[0]), p(ops[1]), p(ops[2]), p(ops[3]), int(bool(relu)), int(tile), int(bool(poison)),
                                            p(io), p(io2), int(guard)))
        outs = [None if a is None else a[:rows].reshape(shape) for a in (io, io2)]
        return outs[0], outs[1], np.concatenate([a[rows:] for a in (io, io2) if a is not None])

    def debug_box_scores(self, pred_hw: np.ndarray, polys):
        """Test hook: raw (sum, count) of the GPU box-score kernel for given polygons."""
        pred = np.ascontiguousarray(pred_hw, dtype=np.float32)
        h, w = pred.shape
        xy = np.asarray([c for p in polys for pt in p for c in pt], dtype=np.int32)
        cnt = np.asarray([len(p) for p in polys], dtype=np.int32)
        sums = np.empty(len(polys), np.float64)
        counts = np.empty(len(polys), np.float64)
        check(test_lib().ocr_test_box_scores(self._h, _ptr(pred), h, w, _ptr(xy), _ptr(cnt), len(polys), _ptr(sums),
                                        _ptr(counts)))
        return sums, counts

    BOX_SCORE_SENTINEL = -7.0

    def debug_box_scores_batch(self, preds_nhw: np.ndarray, polys, images=None, grid: int = 0, dev_count: Optional[int] = None, slack: int = 0):
        """Test hook: the box-score kernel on n maps (N x H x W, or one H x W) for polygons with an image index each (default 0).
        grid == 0 is the plain launch; grid > 0 the counted one with that many workgroups and `dev_count` (default: all polygons) as the
        job count in device memory.  `slack` more job and result slots lie behind the list (copies of job 0).  Every result slot holds
        BOX_SCORE_SENTINEL before the launch.  Returns (sums, counts, boxes as (min_x, min_y, bw, bh), slack_sums, slack_counts)."""
        pred = np.ascontiguousarray(preds_nhw, dtype=np.float32)
        if pred.ndim == 2:
            pred = pred[None]
        n, h, w = pred.shape
        npoly = len(polys)
        xy = np.asarray([c for p in polys for pt in p for c in pt] or [0, 0], dtype=np.int32)
        cnt = np.asarray([len(p) for p in polys] or [0], dtype=np.int32)
        img = np.zeros(max(npoly, 1), np.int32) if images is None else np.ascontiguousarray(list(images) or [0], dtype=np.int32)
        assert images is None or len(images) == npoly
        sums = np.empty(max(npoly + slack, 1), np.float64)
        counts = np.empty(max(npoly + slack, 1), np.float64)
        box = np.empty((max(npoly, 1), 4), np.int32)
        check(test_lib().ocr_test_box_scores_batch(self._h, _ptr(pred), n, h, w, _ptr(xy), _ptr(cnt), _ptr(img), npoly, int(grid),
                                                   npoly if dev_count is None else int(dev_count), int(slack), self.BOX_SCORE_SENTINEL,
                                                   _ptr(sums), _ptr(counts), _ptr(box)))
        return sums[:npoly], counts[:npoly], [tuple(int(v) for v in b) for b in box[:npoly]], sums[npoly:npoly + slack], counts[npoly:npoly + slack]

    def detect_pipelined(self, x_ptr: int, n: int, h: int, w: int, prob_ptr: int, adjust_values=None,
                         params: Optional[PostprocParams] = None, convert: bool = True):
        """ocr_det_detect_pipelined: enqueue this batch's forward, get the PREVIOUS batch's polygons (None on the first
        call); x_ptr = 0 flushes.  convert=False returns (n_polygons, n_vertices) instead of Python lists."""
        adj_p = None
        if x_ptr:
            adj = np.ascontiguousarray(adjust_values, dtype=np.float64).reshape(n, 2)
            adj_p = adj.ctypes.data_as(C.POINTER(C.c_double))
        out = C.POINTER(Polygons)()
        check(lib().ocr_det_detect_pipelined(self._h, x_ptr or None, n, h, w, prob_ptr or None, adj_p,
                                             C.byref(params) if params is not None else None, C.byref(out)))
        if not out:
            return None
        try:
            return polygons_to_python(out) if convert else (out.contents.n_polygons, out.contents.n_vertices)
        finally:
            lib().ocr_polygons_free(out)

    def detect_pipelined_block(self, x_ptr: int, n: int, h: int, w: int, prob_ptr: int, adjust_values=None,
                               params: Optional[PostprocParams] = None):
        """ocr_det_detect_pipelined returning the PREVIOUS batch's ocr_polygons_t block itself (a ctypes pointer, None on the
        first call; release it with free_block) - what extract_crops_block consumes without a detour through Python lists."""
        adj_p = None
        if x_ptr:
            adj = np.ascontiguousarray(adjust_values, dtype=np.float64).reshape(n, 2)
            adj_p = adj.ctypes.data_as(C.POINTER(C.c_double))
        out = C.POINTER(Polygons)()
        check(lib().ocr_det_detect_pipelined(self._h, x_ptr or None, n, h, w, prob_ptr or None, adj_p,
                                             C.byref(params) if params is not None else None, C.byref(out)))
        return out if out else None

    def extract_crops_block(self, block, frames_ptr: int, n: int, h: int, w: int, adjust_values, crops_ptr: int) -> int:
        """ocr_extract_crops for a polygon block on device-resident frames; returns the number of crops written."""
        adj = np.ascontiguousarray(adjust_values, dtype=np.float64).reshape(n, 2)
        if block.contents.n_polygons:
            check(lib().ocr_extract_crops(self._h, frames_ptr, n, h, w, MEM_DEVICE, block, adj.ctypes.data_as(C.POINTER(C.c_double)), crops_ptr))
        return block.contents.n_polygons

    @staticmethod
    def free_block(block) -> None:
        if block:
            lib().ocr_polygons_free(block)

    def postprocess_counts(self, prob, n: int, h: int, w: int, adjust_values: np.ndarray, mem_kind: int = MEM_HOST,
                           params: Optional[PostprocParams] = None) -> Tuple[int, int]:
        """get_boxes_and_box_scores without turning the CSR block into Python objects: (polygons, vertices).
        What a benchmark times when it wants the library, not the harness."""
        adj = np.ascontiguousarray(adjust_values, dtype=np.float64).reshape(n, 2)
        out = C.POINTER(Polygons)()
        check(lib().ocr_det_postprocess(self._h, _ptr(prob), n, h, w, mem_kind,
                                        adj.ctypes.data_as(C.POINTER(C.c_double)),
                                        C.byref(params) if params is not None else None, C.byref(out)))
        try:
            return out.contents.n_polygons, out.contents.n_vertices
        finally:
            lib().ocr_polygons_free(out)

    def post_stats(self) -> dict:
        """Cumulative counters of where this handle's polygon chain ran (ocr_det_post_stats)."""
        a = (C.c_int64 * 6)()
        check(lib().ocr_det_post_stats(self._h, a))
        return dict(zip(("images_device_traced", "images_host_traced", "candidates_device", "candidates_host", "images_device_chain", "passes"),
                        (int(v) for v in a)))

    def postprocess(self, prob, n: int, h: int, w: int, adjust_values: np.ndarray, mem_kind: int = MEM_HOST,
                    params: Optional[PostprocParams] = None):
        adj = np.ascontiguousarray(adjust_values, dtype=np.float64).reshape(n, 2)
        out = C.POINTER(Polygons)()
        check(lib().ocr_det_postprocess(self._h, _ptr(prob), n, h, w, mem_kind,
                                        adj.ctypes.data_as(C.POINTER(C.c_double)),
                                        C.byref(params) if params is not None else None, C.byref(out)))
        try:
            return polygons_to_python(out)
        finally:
            lib().ocr_polygons_free(out)


class Recognizer:
    """Owns an ocr_rec_t.  Mirrors `Net::new(&weights.root())` + `weights.load(..)`
    (/root/reference/src/char_recognition/mod.rs:44-46)."""

    def __init__(self, weights_blob: Optional[bytes], device: int = 0, varstore_path: Optional[str] = None,
                 options: Optional[str] = None):
        self._h = C.c_void_p()
        self.device = device
        if varstore_path is not None:
            check(lib().ocr_rec_create_from_varstore(os.fsencode(varstore_path), device, C.byref(self._h)))
        else:
            check(lib().ocr_rec_create(weights_blob, len(weights_blob), device, C.byref(self._h)))
        if options:
            self.set_options(options)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            lib().ocr_rec_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, raw_stream: Optional[int]) -> None:
        check(lib().ocr_rec_set_stream(self._h, C.c_void_p(raw_stream or 0)))

    def synchronize(self) -> None:
        check(lib().ocr_rec_synchronize(self._h))

    def debug_rec_features(self, form, crops, w1, b1, w2, b2, crops_per_block=0, poison=0, guard=None, sentinel=-7.0):
        """conv1 + pool + conv2 + pool on caller weights (test hook): form 0 the exact-f32 kernel, 1 the small-batch split-bf16 one.
        crops: n x 784; w1 [32][25], b1 [32], w2 [64][32][25], b2 [64].  Returns n x 1024 f32 in the order co * 16 + p.
        crops_per_block (form 0): 0 = chosen by n as shipped, 1, 2 or 4 = that instantiation of rec_conv_kernel.  The crops sit between two
        leads of four crops: zeros, quiet NaN (poison=1) or +inf (poison=2).  With guard=g the result is (feat, the rows behind it), rows
        that went to the device as `sentinel` and come back as the kernel left them: g rows for form 0; for form 1 the pad rows of the last
        16-crop tile and max(1, ceil(g / 16)) further tiles."""
        f = lambda a, shape: np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(shape))
        x = f(crops, (-1, 784))
        n = x.shape[0]
        w1, b1, w2, b2 = f(w1, (32, 25)), f(b1, (32,)), f(w2, (64, 32, 25)), f(b2, (64,))
        g = int(guard or 0)
        rows = n + g if int(form) == 0 else 16 * ((n + 15) // 16 + max(1, (g + 15) // 16))
        io = np.full((rows, 1024), sentinel, np.float32)
        check(test_lib().ocr_test_rec_features(self._h, int(form), int(crops_per_block), _ptr(x), n, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), int(poison),
                                               _ptr(io), g))
        return io[:n] if guard is None else (io[:n], io[n:])

    def debug_rec_fc1(self, form, feat, w, bias, poison=False, guard=8, sentinel=-7.0):
        """fc1 + bias + ReLU on caller weights (test hook): form 0 the large-batch conv_igemm GEMM, 1 rec_fc1_ksplit_kernel.  feat: n x 1024;
        w [512][1024], bias [512]; poison: the rows the kernel may read past the batch hold NaN instead of zero.  Returns (n + guard) x 512 f32:
        the result and, behind it, `guard` rows that went to the device as `sentinel` and come back as the kernel left them."""
        f = lambda a, shape: np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(shape))
        x = f(feat, (-1, 1024))
        n = x.shape[0]
        w, bias = f(w, (512, 1024)), f(bias, (512,))
        hid = np.full((n + guard, 512), sentinel, np.float32)
        check(test_lib().ocr_test_rec_fc1(self._h, int(form), _ptr(x), n, _ptr(w), _ptr(bias), int(bool(poison)), _ptr(hid), int(guard)))
        return hid

    def debug_rec_fc2(self, form, hid, w, bias, want=("logits", "labels", "probs"), guard=8, sentinel=-7):
        """fc2 + bias + softmax(f64) + top-1 on caller weights (test hook): form 0 rec_fc2_softmax_kernel, 1 rec_fc2_small_kernel.  hid: n x 512;
        w [62][512], bias [62].  Returns (logits (n + guard) x 62 f32, labels (n + guard) i32, probs (n + guard) f64), None for an output not in
        `want` (the kernel then gets a null pointer); each went to the device filled with `sentinel`."""
        f = lambda a, shape: np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(shape))
        x = f(hid, (-1, 512))
        n = x.shape[0]
        w, bias = f(w, (62, 512)), f(bias, (62,))
        logits = np.full((n + guard, 62), sentinel, np.float32) if "logits" in want else None
        labels = np.full(n + guard, sentinel, np.int32) if "labels" in want else None
        probs = np.full(n + guard, sentinel, np.float64) if "probs" in want else None
        check(test_lib().ocr_test_rec_fc2(self._h, int(form), _ptr(x), n, _ptr(w), _ptr(bias), *(None if a is None else _ptr(a) for a in (logits, labels, probs)),
                                          int(guard)))
        return logits, labels, probs

    def set_options(self, options: str) -> None:
        """`small_batch=0`: every batch on the throughput kernels (bit-exact batch-size invariance)."""
        check(lib().ocr_rec_set_options(self._h, options.encode()))

    def forward_host(self, crops: np.ndarray) -> np.ndarray:
        crops = np.ascontiguousarray(crops, dtype=np.float32).reshape(-1, 784)
        n = crops.shape[0]
        logits = np.empty((n, 62), np.float32)
        check(lib().ocr_rec_forward(self._h, _ptr(crops), n, _ptr(logits), MEM_HOST))
        return logits

    def classify_host(self, crops: np.ndarray):
        crops = np.ascontiguousarray(crops, dtype=np.float32).reshape(-1, 784)
        n = crops.shape[0]
        labels = np.empty(n, np.int32)
        probs = np.empty(n, np.float64)
        check(lib().ocr_rec_classify(self._h, _ptr(crops), n, _ptr(labels), _ptr(probs), MEM_HOST))
        return labels, probs

    def ctc_greedy_decode(self, logits: np.ndarray, blank: int):
        """EXTENSION (no reference counterpart): logits N x T x C f32 in host memory -> (labels N x T int32 padded with -1, lengths N)."""
        x = np.ascontiguousarray(logits, dtype=np.float32)
        n, t, c = x.shape
        labels = np.empty((n, t), np.int32)
        lengths = np.empty(n, np.int32)
        check(lib().ocr_ctc_greedy_decode(self._h, _ptr(x), n, t, c, int(blank), MEM_HOST, _ptr(labels), _ptr(lengths)))
        return labels, lengths

    def ctc_greedy_decode_device(self, logits_ptr: int, n: int, t: int, c: int, blank: int, labels_ptr: int, lengths_ptr: int) -> None:
        check(lib().ocr_ctc_greedy_decode(self._h, C.c_void_p(logits_ptr), n, t, c, int(blank), MEM_DEVICE, C.c_void_p(labels_ptr), C.c_void_p(lengths_ptr)))

    def ctc_beam_decode(self, logits: np.ndarray, blank: int, beam_width: int):
        """EXTENSION (no reference counterpart): CTC prefix beam search over N x T x C f32 logits in host memory -> (labels N x B x T
        int32 padded with -1, lengths N x B (-1: no such hypothesis), scores N x B f64 log-probabilities), hypotheses in rank order."""
        x = np.ascontiguousarray(logits, dtype=np.float32)
        n, t, c = x.shape
        b = int(beam_width)
        labels = np.empty((n, max(b, 0), t), np.int32)
        lengths = np.empty((n, max(b, 0)), np.int32)
        scores = np.empty((n, max(b, 0)), np.float64)
        check(lib().ocr_ctc_beam_decode(self._h, _ptr(x), n, t, c, int(blank), b, MEM_HOST, _ptr(labels), _ptr(lengths), _ptr(scores)))
        return labels, lengths, scores

    def ctc_beam_decode_device(self, logits_ptr: int, n: int, t: int, c: int, blank: int, beam_width: int, labels_ptr: int, lengths_ptr: int,
                               scores_ptr: int, mem_kind: int = MEM_DEVICE) -> None:
        check(lib().ocr_ctc_beam_decode(self._h, C.c_void_p(logits_ptr), n, t, c, int(blank), int(beam_width), int(mem_kind),
                                        C.c_void_p(labels_ptr), C.c_void_p(lengths_ptr), C.c_void_p(scores_ptr)))

    def classify_profile(self, crops_ptr: int, n: int, labels_ptr: int = 0, probs_ptr: int = 0):
        """[(kernel, ms, executed flops, bytes)] of one classify pass (device pointers)."""
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        fl = (C.c_double * cap)()
        by = (C.c_double * cap)()
        cnt = C.c_int(0)
        check(lib().ocr_rec_classify_profile(self._h, crops_ptr, n, labels_ptr or None, probs_ptr or None, cap, names, ms,
                                             fl, by, C.byref(cnt)))
        return [(names[i].decode(), float(ms[i]), float(fl[i]), float(by[i])) for i in range(cnt.value)]

    def classify_device(self, crops_ptr: int, n: int, logits_ptr: int, labels_ptr: int, probs_ptr: int) -> None:
        check(lib().ocr_rec_classify_async(self._h, crops_ptr, n, logits_ptr or None, labels_ptr or None,
                                           probs_ptr or None))

    def glyph_costs(self, logits: np.ndarray) -> np.ndarray:
        """ocr_rec_glyph_costs: logits n x 62 f32 in host memory -> costs n x 62 f32, the negative log-softmax computed in f64."""
        x = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1, 62)
        costs = np.empty_like(x)
        if x.shape[0]:
            check(lib().ocr_rec_glyph_costs(self._h, _ptr(x), x.shape[0], _ptr(costs), MEM_HOST))
        return costs

    def glyph_costs_device(self, logits_ptr: int, n: int, costs_ptr: int) -> None:
        check(lib().ocr_rec_glyph_costs(self._h, C.c_void_p(logits_ptr or None), n, C.c_void_p(costs_ptr or None), MEM_DEVICE))

    def _lexicon_match(self, lex, costs_ptr, n_glyphs: int, mem_kind: int, word_offsets, params) -> LexiconMatches:
        off = np.ascontiguousarray(word_offsets, dtype=np.int32).reshape(-1)
        prm = _as_lexicon_params(params)
        out = C.POINTER(LexiconMatchesBlock)()
        check(lib().ocr_lexicon_match(self._h, lex.handle if isinstance(lex, Lexicon) else lex, costs_ptr, n_glyphs, mem_kind,
                                      _ptr(off) if off.size else None, len(off) - 1, C.byref(prm) if prm is not None else None, C.byref(out)))
        try:
            return LexiconMatches.from_block(out)
        finally:
            lib().ocr_lexicon_matches_free(out)

    def lexicon_match(self, lex: "Lexicon", costs: np.ndarray, word_offsets, params=None) -> LexiconMatches:
        """ocr_lexicon_match: costs n_glyphs x 62 f32 in host memory (glyph_costs), word_offsets [n_words+1] the glyph range per word
        (GlyphSet.word_offsets); params: LexiconParams, a dict of its fields, or None (defaults).  Blocking, on the handle's stream."""
        x = np.ascontiguousarray(costs, dtype=np.float32).reshape(-1, 62)
        return self._lexicon_match(lex, _ptr(x) if x.size else None, x.shape[0], MEM_HOST, word_offsets, params)

    def lexicon_match_device(self, lex: "Lexicon", costs_ptr: int, n_glyphs: int, word_offsets, params=None) -> LexiconMatches:
        return self._lexicon_match(lex, C.c_void_p(costs_ptr or None), n_glyphs, MEM_DEVICE, word_offsets, params)

    def _phrase_match(self, lex, costs_ptr, n_glyphs: int, mem_kind: int, line_offsets, bound_cost, join_cost, params) -> PhraseMatches:
        off = np.ascontiguousarray(line_offsets, dtype=np.int32).reshape(-1)
        prm = _as_phrase_params(params)
        bound = None if bound_cost is None else np.ascontiguousarray(bound_cost, dtype=np.float32).reshape(-1)
        join = None if join_cost is None else np.ascontiguousarray(join_cost, dtype=np.float32).reshape(-1)
        for name, a in (("bound_cost", bound), ("join_cost", join)):
            if a is not None and a.size != n_glyphs:
                raise OcrError(1, f"phrase_match: {name} has {a.size} values for {n_glyphs} glyphs")
        pad = np.zeros(1, np.float32)   # an array without glyphs still passes a pointer: NULL means "no gap costs"
        out = C.POINTER(PhraseMatchesBlock)()
        check(lib().ocr_lexicon_phrase_match(self._h, lex.handle if isinstance(lex, Lexicon) else lex, costs_ptr, n_glyphs, mem_kind,
                                             _ptr(off) if off.size else None, len(off) - 1,
                                             None if bound is None else _ptr(bound if bound.size else pad),
                                             None if join is None else _ptr(join if join.size else pad),
                                             C.byref(prm) if prm is not None else None, C.byref(out)))
        try:
            return PhraseMatches.from_block(out)
        finally:
            lib().ocr_phrase_matches_free(out)

    def phrase_match(self, lex: "Lexicon", costs: np.ndarray, line_offsets, bound_cost=None, join_cost=None, params=None) -> PhraseMatches:
        """ocr_lexicon_phrase_match: costs n_glyphs x 62 f32 in host memory (glyph_costs), line_offsets [n_lines+1] the glyph range of
        every line (a polygon's glyphs: GlyphSet.word_offsets); bound_cost and join_cost f32 [n_glyphs] (phrase_gap_costs) or both None
        for zeros; params: PhraseParams, a dict of its fields, or None (defaults).  Blocking, on the handle's stream."""
        x = np.ascontiguousarray(costs, dtype=np.float32).reshape(-1, 62)
        return self._phrase_match(lex, _ptr(x) if x.size else None, x.shape[0], MEM_HOST, line_offsets, bound_cost, join_cost, params)

    def phrase_match_device(self, lex: "Lexicon", costs_ptr: int, n_glyphs: int, line_offsets, bound_cost=None, join_cost=None,
                            params=None) -> PhraseMatches:
        return self._phrase_match(lex, C.c_void_p(costs_ptr or None), n_glyphs, MEM_DEVICE, line_offsets, bound_cost, join_cost, params)

    def _lm_decode(self, lm, costs_ptr, n_glyphs: int, mem_kind: int, word_offsets, params) -> LmPaths:
        off = np.ascontiguousarray(word_offsets, dtype=np.int32).reshape(-1)
        prm = _as_lm_params(params)
        out = C.POINTER(LmPathsBlock)()
        check(lib().ocr_lm_decode(self._h, lm.handle if isinstance(lm, CharLm) else lm, costs_ptr, n_glyphs, mem_kind,
                                  _ptr(off) if off.size else None, len(off) - 1, C.byref(prm) if prm is not None else None, C.byref(out)))
        try:
            return LmPaths.from_block(out)
        finally:
            lib().ocr_lm_paths_free(out)

    def lm_decode(self, lm: "CharLm", costs: np.ndarray, word_offsets, params=None) -> LmPaths:
        """ocr_lm_decode: costs n_glyphs x 62 f32 in host memory (glyph_costs), word_offsets [n_words+1] the glyph range per word
        (GlyphSet.word_offsets); params: LmParams, a dict of its fields, or None (defaults).  Blocking, on the handle's stream."""
        x = np.ascontiguousarray(costs, dtype=np.float32).reshape(-1, 62)
        return self._lm_decode(lm, _ptr(x) if x.size else None, x.shape[0], MEM_HOST, word_offsets, params)

    def lm_decode_device(self, lm: "CharLm", costs_ptr: int, n_glyphs: int, word_offsets, params=None) -> LmPaths:
        return self._lm_decode(lm, C.c_void_p(costs_ptr or None), n_glyphs, MEM_DEVICE, word_offsets, params)

    def _lattice_decode(self, lm, costs_ptr, n_spans: int, mem_kind: int, span_offsets, piece_offsets, params) -> LatticePaths:
        so = np.ascontiguousarray(span_offsets, dtype=np.int32).reshape(-1)
        po = np.ascontiguousarray(piece_offsets, dtype=np.int32).reshape(-1)
        if len(so) != len(po):
            raise ValueError(f"{len(so)} span offsets, {len(po)} piece offsets")
        prm = _as_lattice_params(params)
        out = C.POINTER(LatticePathsBlock)()
        check(lib().ocr_lattice_decode(self._h, lm.handle if isinstance(lm, CharLm) else lm, costs_ptr, n_spans, mem_kind,
                                       _ptr(so) if so.size else None, _ptr(po) if po.size else None, len(so) - 1,
                                       C.byref(prm) if prm is not None else None, C.byref(out)))
        try:
            return LatticePaths.from_block(out)
        finally:
            lib().ocr_lattice_paths_free(out)

    def lattice_decode(self, lm: "CharLm", costs: np.ndarray, span_offsets, piece_offsets, params=None) -> LatticePaths:
        """ocr_lattice_decode: costs n_spans x 62 f32 in host memory (glyph_costs of the span crops), span_offsets and piece_offsets
        [n_words+1] (SpanTable); params: LatticeParams, a dict of its fields, or None (defaults).  Blocking, on the handle's stream."""
        x = np.ascontiguousarray(costs, dtype=np.float32).reshape(-1, 62)
        return self._lattice_decode(lm, _ptr(x) if x.size else None, x.shape[0], MEM_HOST, span_offsets, piece_offsets, params)

    def lattice_decode_device(self, lm: "CharLm", costs_ptr: int, n_spans: int, span_offsets, piece_offsets, params=None) -> LatticePaths:
        return self._lattice_decode(lm, C.c_void_p(costs_ptr or None), n_spans, MEM_DEVICE, span_offsets, piece_offsets, params)

    def _lexicon_lattice_match(self, lex, costs_ptr, n_spans: int, mem_kind: int, span_offsets, piece_offsets, params) -> LexLatMatches:
        so = np.ascontiguousarray(span_offsets, dtype=np.int32).reshape(-1)
        po = np.ascontiguousarray(piece_offsets, dtype=np.int32).reshape(-1)
        if len(so) != len(po):
            raise ValueError(f"{len(so)} span offsets, {len(po)} piece offsets")
        prm = _as_lexlat_params(params)
        out = C.POINTER(LexLatMatchesBlock)()
        check(lib().ocr_lexicon_lattice_match(self._h, lex.handle if isinstance(lex, Lexicon) else lex, costs_ptr, n_spans, mem_kind,
                                              _ptr(so) if so.size else None, _ptr(po) if po.size else None, len(so) - 1,
                                              C.byref(prm) if prm is not None else None, C.byref(out)))
        try:
            return LexLatMatches.from_block(out)
        finally:
            lib().ocr_lexlat_matches_free(out)

    def lexicon_lattice_match(self, lex: "Lexicon", costs: np.ndarray, span_offsets, piece_offsets, params=None) -> LexLatMatches:
        """ocr_lexicon_lattice_match: costs n_spans x 62 f32 in host memory (glyph_costs of the span crops), span_offsets and
        piece_offsets [n_words+1] (SpanTable); params: LexLatParams, a dict of its fields, or None (defaults).  Blocking, on the
        handle's stream."""
        x = np.ascontiguousarray(costs, dtype=np.float32).reshape(-1, 62)
        return self._lexicon_lattice_match(lex, _ptr(x) if x.size else None, x.shape[0], MEM_HOST, span_offsets, piece_offsets, params)

    def lexicon_lattice_match_device(self, lex: "Lexicon", costs_ptr: int, n_spans: int, span_offsets, piece_offsets,
                                     params=None) -> LexLatMatches:
        return self._lexicon_lattice_match(lex, C.c_void_p(costs_ptr or None), n_spans, MEM_DEVICE, span_offsets, piece_offsets, params)


def python_to_polygons(polys, scores):
    """PolygonScores as Python lists -> (Polygons struct, keep-alive arrays) for the calls that take a block."""
    img = np.cumsum([0] + [len(p) for p in polys]).astype(np.int32)
    flat = [pg for p in polys for pg in p]
    po = np.cumsum([0] + [len(pg) for pg in flat]).astype(np.int32)
    xy = np.asarray([c for pg in flat for v in pg for c in v], dtype=np.uint32)
    sc = np.asarray([s for ss in scores for s in ss], dtype=np.float64)
    st = Polygons(len(polys), len(flat), int(po[-1]), img.ctypes.data_as(C.POINTER(C.c_int32)),
                  po.ctypes.data_as(C.POINTER(C.c_int32)), xy.ctypes.data_as(C.POINTER(C.c_uint32)),
                  sc.ctypes.data_as(C.POINTER(C.c_double)))
    return st, (img, po, xy, sc)


class Comm:
    """Owns an ocr_comm_t: the RCCL communicator behind the C ABI (one per rank; creation is collective)."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        check(lib().ocr_comm_unique_id(buf))
        return bytes(buf)

    @staticmethod
    def rccl_version() -> int:
        v = C.c_int(0)
        check(lib().ocr_comm_rccl_version(C.byref(v)))
        return v.value

    def __init__(self, unique_id: bytes, world: int, rank: int, device: int = 0):
        self._h = C.c_void_p()
        self.world, self.rank = world, rank
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        check(lib().ocr_comm_create(buf, world, rank, device, C.byref(self._h)))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            lib().ocr_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def all_gather_polygons(self, polys, scores):
        st, keep = python_to_polygons(polys, scores)
        out = C.POINTER(Polygons)()
        check(lib().ocr_comm_all_gather_polygons(self._h, C.byref(st), C.byref(out)))
        try:
            return polygons_to_python(out)
        finally:
            lib().ocr_polygons_free(out)

    def all_gather_labels(self, labels: np.ndarray, capacity: int):
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        out = np.empty(capacity, np.int32)
        counts = np.zeros(self.world, np.int32)
        n = C.c_int(0)
        check(lib().ocr_comm_all_gather_labels(self._h, _ptr(labels), labels.size, _ptr(out), capacity, _ptr(counts), C.byref(n)))
        return out[:n.value].copy(), counts


def comm_assemble(shards):
    """Test hook: what ocr_comm_all_gather_polygons returns for these per-rank (polys, scores) shards, without RCCL."""
    structs, keep = [], []
    for polys, scores in shards:
        st, k = python_to_polygons(polys, scores)
        structs.append(st)
        keep.append(k)
    arr = (C.POINTER(Polygons) * len(structs))(*[C.pointer(s) for s in structs])
    out = C.POINTER(Polygons)()
    check(test_lib().ocr_test_comm_assemble(arr, len(structs), C.byref(out)))
    try:
        return polygons_to_python(out)
    finally:
        lib().ocr_polygons_free(out)


# ---- the weight builders of the composed FPN (engine.hip; CPU only, through the test library)
def compose_taps(out_ohwi, in_oi) -> np.ndarray:
    """out (3x3, [cout][9][mid]) after in (1x1, [mid][cin]) -> f64 taps [cout][9][cin]."""
    o = np.ascontiguousarray(out_ohwi, dtype=np.float32)
    i = np.ascontiguousarray(in_oi, dtype=np.float32)
    cout, nine, mid = o.shape
    assert nine == 9 and i.shape[0] == mid
    t = np.empty((cout, 9, i.shape[1]), np.float64)
    check(test_lib().ocr_test_compose_taps(_ptr(o), cout, mid, _ptr(i), i.shape[1], _ptr(t)))
    return t


def phase_weights(taps, up: int) -> np.ndarray:
    """f64 taps [cout][9][cin] of a 3x3 conv of the nearest-x-up upsample -> f32 [up*up][cout][2x2][cin] as the engine builds them."""
    t = np.ascontiguousarray(taps, dtype=np.float64)
    cout, nine, cin = t.shape
    assert nine == 9
    w = np.empty((up * up, cout, 4, cin), np.float32)
    check(test_lib().ocr_test_phase_weights(_ptr(t), cout, cin, int(up), _ptr(w)))
    return w


def pyr4_weights(bin1_ohwi, scale64) -> np.ndarray:
    """bin_conv1 [64][9][256] and bin_bn1's folded scale [64] -> f32 [64 phases][64][21 slots][64] as the engine builds them."""
    o = np.ascontiguousarray(bin1_ohwi, dtype=np.float32)
    sc = np.ascontiguousarray(scale64, dtype=np.float32)
    assert o.shape == (64, 9, 256) and sc.shape == (64,)
    w = np.empty((64, 64, 21, 64), np.float32)
    check(test_lib().ocr_test_pyr4_weights(_ptr(o), _ptr(sc), _ptr(w)))
    return w


# ---- the host side of the Winograd convs (engine.hip, winograd43_fused.hip; CPU only, through the test library)
def winograd_weights(wgt_ohwi, m: int = 4) -> np.ndarray:
    """[cout][9][cin] -> U = G g G^T as f32 [(m+2)^2][cout][cin], as the engine builds it (f64, rounded once)."""
    g = np.ascontiguousarray(wgt_ohwi, dtype=np.float32)
    cout, nine, cin = g.shape
    assert nine == 9
    u = np.empty(((m + 2) ** 2, cout, cin), np.float32)
    check(test_lib().ocr_test_winograd_weights(_ptr(g), cout, cin, int(m), _ptr(u)))
    return u


def winograd43_fragments(u) -> np.ndarray:
    """U [36][cout][cin] -> the fused kernel's MFMA B-fragment order [cout/64][cin/16][36][4 waves][64 lanes][4]."""
    u = np.ascontiguousarray(u, dtype=np.float32)
    comps, cout, cin = u.shape
    assert comps == 36
    f = np.empty(u.size, np.float32)
    check(test_lib().ocr_test_winograd43_fragments(_ptr(u), cout, cin, _ptr(f)))
    return f.reshape(cout // 64, cin // 16, 36, 4, 64, 4)


# ---- host-geometry hooks (CPU only; used by tests to pin the C++ geometry to the KATs)
def host_contour_candidates(bitmap01: np.ndarray) -> List[List[Tuple[int, int]]]:
    bm = np.ascontiguousarray(bitmap01, dtype=np.uint8)
    h, w = bm.shape
    max_pts, max_polys = 1 << 20, 1 << 16
    xy = np.empty(2 * max_pts, np.int32)
    cnt = np.empty(max_polys, np.int32)
    n = C.c_int(0)
    check(test_lib().ocr_test_contour_candidates(_ptr(bm), h, w, _ptr(xy), _ptr(cnt), max_pts, max_polys, C.byref(n)))
    out, pos = [], 0
    for k in range(n.value):
        c = int(cnt[k])
        out.append([(int(xy[2 * (pos + i)]), int(xy[2 * (pos + i) + 1])) for i in range(c)])
        pos += c
    return out


def _contours_call(fn, bitmap01, extra_status=False, max_pts=1 << 20, max_polys=1 << 16, tail=(), extra_out=0):
    bm = np.ascontiguousarray(bitmap01, dtype=np.uint8)
    h, w = bm.shape
    xy = np.empty(2 * max_pts, np.int32)
    cnt = np.empty(max_polys, np.int32)
    n, st = C.c_int(0), C.c_int(0)
    extra = [C.c_int(0) for _ in range(extra_out)]
    args = [_ptr(bm), h, w, _ptr(xy), _ptr(cnt), max_pts, max_polys, C.byref(n)] + ([C.byref(st)] if extra_status else []) + list(tail)
    check(fn(*args, *[C.byref(e) for e in extra]))
    out, pos = [], 0
    for k in range(n.value):
        c = int(cnt[k])
        out.append([(int(xy[2 * (pos + i)]), int(xy[2 * (pos + i) + 1])) for i in range(c)])
        pos += c
    if extra_out:
        return (out, st.value, *(e.value for e in extra))
    return (out, st.value) if extra_status else out


def host_contours(bitmap01: np.ndarray):
    """Raw contours of the host tracer (postproc_geom.cpp::find_contours)."""
    L = test_lib()
    L.ocr_test_host_contours.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    return _contours_call(L.ocr_test_host_contours, bitmap01)


def device_contours(bitmap01: np.ndarray, max_pts: int = 1 << 20, max_polys: int = 1 << 16, sequential: bool = False, report: bool = False):
    """Raw contours of the device tracer (contours.hip; the parallel form, or the one-wave-per-image form) and its status
    (0 ok, 1 buffers too small, 2 guard, 3 parallel form: a start outside its list of plausible starts).  report: also the form that
    ran (contour_trace_form: 1 one wave, else the parallel instantiation's LDS words) and the parallel form's count of plausible
    starts K (0 for the one-wave form) - (contours, status, form, K)."""
    L = test_lib()
    L.ocr_test_device_contours.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                           C.POINTER(C.c_int), C.POINTER(C.c_int)]
    r = _contours_call(L.ocr_test_device_contours, bitmap01, True, max_pts, max_polys, tail=(int(sequential),), extra_out=2)
    return r if report else r[:2]


def contour_trace_form(h: int, w: int, sequential: bool = False, have_spec: bool = True) -> int:
    """The form the device tracer runs for an h x w map (contour_trace_form; needs no GPU): 0 the map does not fit, 1 the one-wave
    form, else the LDS words of the parallel form's instantiation (14336, 22528 or 35840)."""
    L = test_lib()
    L.ocr_test_contour_trace_form.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    f = C.c_int(-1)
    check(L.ocr_test_contour_trace_form(h, w, int(sequential), int(have_spec), C.byref(f)))
    return f.value


def device_candidates(contours, h: int, w: int, max_pts: int = 1 << 18, max_polys: int = 1 << 14):
    """candidates.hip on the given contours of one h x w map (lists of (x, y)): the candidate polygons after arc length, Douglas-Peucker
    and the >= 4 points filter, in list order, and their clamped job boxes (min_x, min_y, bw, bh)."""
    L = test_lib()
    L.ocr_test_device_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                             C.POINTER(C.c_int)]
    lens = np.asarray([len(c) for c in contours] or [0], np.int32)
    flat = np.asarray([v for c in contours for q in c for v in q] or [0, 0], np.int32)
    xy = np.empty(2 * max_pts, np.int32)
    cnt = np.empty(max_polys, np.int32)
    box = np.empty(4 * max_polys, np.int32)
    n = C.c_int(0)
    check(L.ocr_test_device_candidates(_ptr(flat), _ptr(lens), len(contours), h, w, _ptr(xy), _ptr(cnt), _ptr(box), max_pts, max_polys, C.byref(n)))
    out, boxes, pos = [], [], 0
    for k in range(n.value):
        c = int(cnt[k])
        out.append([(int(xy[2 * (pos + i)]), int(xy[2 * (pos + i) + 1])) for i in range(c)])
        boxes.append(tuple(int(v) for v in box[4 * k:4 * k + 4]))
        pos += c
    return out, boxes


def device_candidates_batch(images, h: int, w: int, cap: int, maxc: int, max_jobs: int, max_pts: int, scratch_fill: int = 0, guard: int = 0,
                            poison: int = 0x5A5AC3C3):
    """candidates.hip on a batch laid out as the device tracer leaves it, nothing interpreted (ocr_test_candidates_batch).  images: a
    list of (status, contours), contours lists of (x, y); image i's points sit at i * cap, its starts row is maxc + 1 long.  The whole
    scratch is filled with the byte scratch_fill, the lists and `guard` jobs / points behind them with the word poison.  Returns
    (tot [n][2], totals [3], jobs [max_jobs + guard][7], points [max_pts + guard][2]) as int32 arrays."""
    L = test_lib()
    L.ocr_test_candidates_batch.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    n = len(images)
    status = np.asarray([st for st, _ in images] or [0], np.int32)
    ncs = np.asarray([len(cs) for _, cs in images] or [0], np.int32)
    lens = np.asarray([len(c) for _, cs in images for c in cs] or [0], np.int32)
    parts = [np.asarray(c, np.int32).reshape(-1) for _, cs in images for c in cs if len(c)]
    flat = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(2, np.int32), dtype=np.int32)
    tot = np.empty((max(n, 1), 2), np.int32)
    totals = np.empty(3, np.int32)
    jobs = np.empty((max_jobs + guard, 7), np.int32)
    pts = np.empty((max_pts + guard, 2), np.int32)
    check(L.ocr_test_candidates_batch(n, h, w, _ptr(status), _ptr(ncs), _ptr(lens), _ptr(flat), cap, maxc, max_jobs, max_pts, scratch_fill, guard, poison,
                                      _ptr(tot), _ptr(totals), _ptr(jobs), _ptr(pts)))
    return tot, totals, jobs, pts


def host_expand_polygon(pts: Sequence[Tuple[int, int]], factor: float = 2.0):
    a = np.asarray(pts, dtype=np.int32).reshape(-1)
    out = np.empty(8192, np.int32)
    n = C.c_int(0)
    ss = C.c_double(0.0)
    check(test_lib().ocr_test_expand_polygon(_ptr(a), len(pts), factor, _ptr(out), 4096, C.byref(n), C.byref(ss)))
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n.value)], ss.value


def host_min_area_box(pts: Sequence[Tuple[int, int]]):
    a = np.asarray(pts, dtype=np.int32).reshape(-1)
    box = np.empty(8, np.int32)
    ss = C.c_double(0.0)
    check(test_lib().ocr_test_min_area_box(_ptr(a), len(pts), _ptr(box), C.byref(ss)))
    return [(int(box[2 * i]), int(box[2 * i + 1])) for i in range(4)], ss.value
