"""Page -> text: the reference pipeline's missing middle (README.md:20-26: text detection -> character segmentation -> character
recognition -> output text), composed over the C ABI.

    read_words(det_net, rec_net, frames, polygon_scores, adjust_values)
        ocr_segment_glyphs        every detected word (polygon) -> glyph boxes          (csrc/glyphs.hip, segment_kernel)
        ocr_extract_glyph_crops   every glyph -> one 28 x 28 crop, on the device         (csrc/glyphs.hip, glyph_crop_kernel)
        ocr_rec_classify          every crop -> label in VALUES (utils.rs:7) and its probability

The segmentation rule is build-defined (the reference never built the step): include/ocr_amd.h, restated in tests/glyph_oracle.py.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from . import capi
from .char_recognition import VALUES


def _handle(net, kind):
    h = getattr(net, "handle", net)
    if not isinstance(h, kind):
        raise TypeError(f"expected a {kind.__name__} or a wrapper with .handle, got {type(net).__name__}")
    return h


def read_words(det_net, rec_net, frames, polygon_scores, adjust_values, params=None
               ) -> List[List[Tuple[str, np.ndarray, np.ndarray]]]:
    """Reads every detected word of a batch.

    det_net: text_detection.FuncT or capi.Detector (supplies the GPU and stream of the segmentation); rec_net: char_recognition.Net
    or capi.Recognizer.  frames: the detector's input, N x 1 x H x W f32 raw 0..255, a numpy array or a CUDA tensor.
    polygon_scores: what get_boxes_and_box_scores returned (or its per-image polygon lists); adjust_values: N x 2 as given to it.
    params: capi.SegmentParams, a dict of its fields, or None for the defaults.
    Returns per image, per polygon: (text, probability of every character (f64), glyph boxes k x 4 int32 x0, y0, x1, y1 in frame
    pixels, half-open).  A flat word reads as ""."""
    import torch

    det = _handle(det_net, capi.Detector)
    rec = _handle(rec_net, capi.Recognizer)
    polys = getattr(polygon_scores, "polygons", polygon_scores)
    if isinstance(frames, np.ndarray):
        dev = torch.device("cuda", det.device)
        x = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32)).to(dev)
    else:
        if not (frames.is_cuda and frames.dtype == torch.float32):
            raise capi.OcrError(1, "frames: expected a numpy array or a CUDA f32 tensor N x 1 x H x W")
        dev = frames.device
        x = frames.contiguous()
    if x.dim() != 4 or x.shape[1] != 1:
        raise capi.OcrError(1, f"frames: expected N x 1 x H x W, got {tuple(x.shape)}")
    n, _, h, w = x.shape
    # the library's calls run on their handles' streams: whatever torch queued to produce x is finished first
    torch.cuda.current_stream(dev).synchronize()
    glyphs = det.segment_glyphs_device(x.data_ptr(), n, h, w, polys, adjust_values, params)
    ng = glyphs.n_glyphs
    labels = np.zeros(0, np.int32)
    probs = np.zeros(0, np.float64)
    if ng:
        crops = torch.empty((ng, 784), dtype=torch.float32, device=dev)
        det.extract_glyph_crops_device(x.data_ptr(), n, h, w, glyphs, crops.data_ptr(), params)   # blocking
        lab = torch.empty(ng, dtype=torch.int32, device=dev)
        pr = torch.empty(ng, dtype=torch.float64, device=dev)
        rec.classify_device(crops.data_ptr(), ng, 0, lab.data_ptr(), pr.data_ptr())
        rec.synchronize()
        labels, probs = lab.cpu().numpy(), pr.cpu().numpy()
    out = []
    for b in range(n):
        words = []
        for k in range(int(glyphs.img_offsets[b]), int(glyphs.img_offsets[b + 1])):
            g0, g1 = int(glyphs.word_offsets[k]), int(glyphs.word_offsets[k + 1])
            words.append(("".join(VALUES[int(c)] for c in labels[g0:g1]), probs[g0:g1].copy(), glyphs.boxes[g0:g1].copy()))
        out.append(words)
    return out


def glyph_crops(det_net, frames: np.ndarray, polygon_scores, adjust_values, params: Optional[dict] = None):
    """Host-memory form of the first two stages: (capi.GlyphSet, n_glyphs x 784 f32 crops)."""
    det = _handle(det_net, capi.Detector)
    polys = getattr(polygon_scores, "polygons", polygon_scores)
    glyphs = det.segment_glyphs(frames, polys, adjust_values, params)
    return glyphs, det.extract_glyph_crops(frames, glyphs, params)
