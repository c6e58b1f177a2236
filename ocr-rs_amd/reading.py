"""Page -> text: the reference pipeline's missing middle (README.md:20-26: text detection -> character segmentation -> character
recognition -> output text), composed over the C ABI.

    read_words(det_net, rec_net, frames, polygon_scores, adjust_values)
        ocr_segment_glyphs        every detected word (polygon) -> glyph boxes          (csrc/glyphs.hip, segment_kernel)
          or, with cc=..., ocr_segment_glyphs_cc: connected components, kerned letters split   (csrc/glyph_cc.hip)
        ocr_extract_glyph_crops   every glyph -> one 28 x 28 crop, on the device         (csrc/glyphs.hip, glyph_crop_kernel)
          or, with cc=... and mask=..., ocr_segment_glyphs_cc_labelled and ocr_extract_glyph_crops_masked: the crop of a glyph holds
          its own components' ink only
        ocr_rec_classify          every crop -> label in VALUES (utils.rs:7) and its probability

    read_words_rectified(det_net, rec_net, frames, polygon_scores, adjust_values)
        ocr_plan_word_strips      every word -> its minimum-area rectangle, upright      (csrc/word_strips.cpp, host)
        ocr_extract_word_strips   every word -> one strip of the atlas, on the device    (csrc/strips.hip)
        then the three calls above on the atlas, through the rectangles of ocr_word_strip_polygons
      with curved=True (or a dict of capi.CurveParams' fields), words that bend are read along their own centreline:
        ocr_plan_curved_strips    every word -> 33 knots of its centreline with normals   (csrc/word_strips.cpp, host)
        ocr_extract_curved_strips every word -> one strip of the atlas, on the device     (csrc/curved_strips.hip)

    read_lines(det_net, rec_net, frames, polygon_scores, adjust_values)
        read_words_rectified (or read_words) for the texts, then
        ocr_plan_word_strips      every word -> its oriented rectangle                    (the quads)
        ocr_group_lines           the words of every page -> text lines in reading order  (csrc/lines.hip)
    read_columns(det_net, rec_net, frames, polygon_scores, adjust_values)
        the same with ocr_group_columns in place of ocr_group_lines: blocks (columns) in reading order, lines within (csrc/columns.hip)
    page_text(lines) joins the lines of one image with "\n"; page_text(blocks, columns=True) separates blocks by an empty line.

    Every reading call takes lexicon=capi.Lexicon (with lexicon_params and max_penalty): the glyph posteriors of every word are then
    matched against the word list on the device, between the classify call and the texts:
        ocr_rec_glyph_costs       the classify call's logits -> negative log-softmax costs (csrc/lexicon.hip)
        ocr_lexicon_match         every word against every entry of an admissible length  (csrc/lexicon.hip)
    ... and lm=capi.CharLm (with lm_params): every word is decoded under a character-bigram model from the same costs, which reads
    words that no list contains:
        ocr_lm_decode             every word -> its k cheapest readings under glyph + transition cost  (csrc/char_lm.hip)
    read_words(..., lattice={}) does not trust the segmentation: wide glyphs are cut, every run of up to max_span pieces is
    recognised, and glyph cost plus model cost choose segmentation and classes together:
        ocr_split_glyphs          wide glyphs -> pieces, cut at ink minima                 (csrc/glyph_split.hip)
        ocr_glyph_spans           pieces -> every run of 1..max_span pieces, a glyph block (csrc/lattice_host.cpp, host)
        ocr_extract_glyph_crops, ocr_rec_classify, ocr_rec_glyph_costs on the spans
        ocr_lattice_decode        every word -> its k cheapest (segmentation, classes) pairs (csrc/lattice.hip)
    ... and with lattice_lexicon=capi.Lexicon the word list is searched over the same pieces:
        ocr_lexicon_lattice_match every word's pieces against every entry, a character reading a run of pieces (csrc/lexicon_lattice.hip)
    read_words(..., spaces={}) and read_words_rectified(..., spaces={}) cut a polygon that holds several words at its inter-word gaps,
    between the crops and the classify call; the lexicon and the model then see every word on its own:
        ocr_break_words           the words of a glyph block -> the words inside them      (csrc/word_breaks.hip)
    read_words(..., phrases={"lexicon": lex}) and read_words_rectified(..., phrases=...) segment the glyphs of every polygon into
    lexicon words and out-of-vocabulary words after the classify call; with spaces= the gaps enter as soft costs, not as cuts:
        ocr_lexicon_phrase_match  the glyph costs of every polygon -> its words and their entries (csrc/lexicon_phrase.hip)

The segmentation, strip and line rules are build-defined (the reference never built the step): include/ocr_amd.h, restated in
tests/glyph_oracle.py, tests/glyph_cc_oracle.py, tests/glyph_mask_oracle.py, tests/strip_oracle.py, tests/curved_strip_oracle.py and
tests/line_oracle.py; the lexicon rule likewise, restated in tests/lexicon_oracle.py, the language model's in tests/char_lm_oracle.py
the word-break rule in tests/word_break_oracle.py and the phrase rule in tests/phrase_oracle.py.
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


def _device_frames(det, frames):
    """frames (numpy or CUDA f32 tensor, N x 1 x H x W) -> a contiguous CUDA tensor, with torch's queued work finished."""
    import torch
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
    # the library's calls run on their handles' streams: whatever torch queued to produce x is finished first
    torch.cuda.current_stream(dev).synchronize()
    return x


def _masked(mask, cc) -> bool:
    """mask: None / False -> the unmasked path; True, a dict of capi.MaskParams' fields or a capi.MaskParams -> masked, which needs cc."""
    if mask is None or mask is False:
        return False
    if cc is None:
        raise capi.OcrError(1, "mask: masked crops need the connected-component rule (cc={} for its defaults)")
    return True


def _segment_and_crop(det, frames_ptr, n, h, w, polys, adjust_values, params, cc, mask, dev):
    """The two glyph calls on device frames -> (GlyphSet, crops tensor or None when there is no glyph); blocking."""
    import torch
    if not _masked(mask, cc):
        glyphs = det.segment_glyphs_device(frames_ptr, n, h, w, polys, adjust_values, params, cc)
        if not glyphs.n_glyphs:
            return glyphs, None
        crops = torch.empty((glyphs.n_glyphs, 784), dtype=torch.float32, device=dev)
        det.extract_glyph_crops_device(frames_ptr, n, h, w, glyphs, crops.data_ptr(), params)
        return glyphs, crops
    glyphs, labels = det.segment_glyphs_cc_labelled_device(frames_ptr, n, h, w, polys, adjust_values, params, cc)
    with labels:
        if not glyphs.n_glyphs:
            return glyphs, None
        crops = torch.empty((glyphs.n_glyphs, 784), dtype=torch.float32, device=dev)
        det.extract_glyph_crops_masked_device(frames_ptr, n, h, w, glyphs, labels, crops.data_ptr(), params, mask)
    return glyphs, crops


def _classify(rec, crops, ng: int, dev, word_offsets, lexicon, lexicon_params, lm=None, lm_params=None):
    """classify on device crops -> (labels, probs, LexiconMatches or None, LmPaths or None); with a lexicon or a language model the
    same call also writes the logits, and the costs, the match and the decode stay on the device."""
    import torch
    if lexicon is not None and not isinstance(lexicon, capi.Lexicon):
        raise TypeError(f"lexicon: expected a capi.Lexicon, got {type(lexicon).__name__}")
    if lm is not None and not isinstance(lm, capi.CharLm):
        raise TypeError(f"lm: expected a capi.CharLm, got {type(lm).__name__}")
    want_costs = lexicon is not None or lm is not None
    labels = np.zeros(0, np.int32)
    probs = np.zeros(0, np.float64)
    costs_ptr = 0
    if ng:
        lab = torch.empty(ng, dtype=torch.int32, device=dev)
        pr = torch.empty(ng, dtype=torch.float64, device=dev)
        logits = torch.empty((ng, 62), dtype=torch.float32, device=dev) if want_costs else None
        rec.classify_device(crops.data_ptr(), ng, logits.data_ptr() if logits is not None else 0, lab.data_ptr(), pr.data_ptr())
        if want_costs:
            costs = torch.empty((ng, 62), dtype=torch.float32, device=dev)
            rec.glyph_costs_device(logits.data_ptr(), ng, costs.data_ptr())   # blocking, behind the classify call
            costs_ptr = costs.data_ptr()
        else:
            rec.synchronize()
        labels, probs = lab.cpu().numpy(), pr.cpu().numpy()
    matches = None
    if lexicon is not None:
        matches = rec.lexicon_match_device(lexicon, costs_ptr, ng, word_offsets, lexicon_params)
    paths = None
    if lm is not None:
        paths = rec.lm_decode_device(lm, costs_ptr, ng, word_offsets, lm_params)
        paths.best = paths.texts(word_offsets)   # hypothesis 0 of every word, for _word
    return labels, probs, matches, paths


def _word(text: str, probs, where, k: int, n_glyphs: int, matches, lexicon, max_penalty: float, paths=None):
    """The tuple of word k: without a lexicon (text, probs, where); with one the text is the best entry's string when a candidate
    exists and cost - raw_cost <= max_penalty * G (f64), and (entry index or -1, cost, raw_cost, raw text) is appended.  With a
    language model the text of a decoded word that the lexicon did not take is hypothesis 0's string, and (cost of hypothesis 0, the
    greedy reading's cost under the model, raw text) is appended last."""
    if matches is None and paths is None:
        return (text, probs, where)
    out, extra, take = text, [], False
    if matches is not None:
        e, c, r = int(matches.entries[k, 0]), float(matches.costs[k, 0]), float(matches.raw_costs[k])
        take = e >= 0 and c - r <= float(max_penalty) * n_glyphs
        if take:
            out = lexicon.words[e]
        extra.append((e, c, r, text))
    if paths is not None:
        if not take and int(paths.word_flags[k]) == 0:
            out = paths.best[k]
        extra.append((float(paths.costs[k, 0]), float(paths.raw_costs[k]), text))
    return (out, probs, where, *extra)


def _spaced_word(text: str, probs, where, k: int, g0: int, sub, breaks, matches, lexicon, max_penalty: float, paths=None):
    """The tuple of polygon k read with spaces=: its sub-words (the words of `sub`, an ocr_break_words block; `breaks` maps them to the
    polygons) each go through _word, the texts are joined by one space, the lexicon and model elements become lists with one entry per
    sub-word, and (starts, gap_pct) is appended: starts int32 [S+1], the sub-word ranges inside the polygon's glyphs, gap_pct int32 [S]."""
    s0, s1 = int(breaks.sub_offsets[k]), int(breaks.sub_offsets[k + 1])
    off = sub.word_offsets[s0:s1 + 1] - np.int32(g0)     # (int32 - int32: a new int32 array)
    o = off.tolist()
    parts = [_word(text[o[i]:o[i + 1]], None, None, s0 + i, o[i + 1] - o[i], matches, lexicon, max_penalty, paths) for i in range(s1 - s0)]
    extras = [list(e) for e in zip(*[p[3:] for p in parts])]
    return (" ".join(p[0] for p in parts), probs, where, *extras, (off, breaks.gap_pct[s0:s1].copy()))


_PHRASE_KEYS = ("lexicon", "params", "break_penalty", "join_penalty")


def _check_phrases(phrases, lexicon, lattice=None):
    """phrases=: a dict with `lexicon` (a capi.Lexicon) and optionally `params`, `break_penalty`, `join_penalty`; not with lexicon= or
    lattice=, whose matches read a fixed word."""
    if lattice is not None:
        raise capi.OcrError(1, "phrases: the composition with lattice= is not built (the phrase search reads glyphs, not pieces)")
    if lexicon is not None:
        raise capi.OcrError(1, "phrases: lexicon= matches every word on its own; give the word list as phrases['lexicon'] alone")
    if not isinstance(phrases, dict) or any(k not in _PHRASE_KEYS for k in phrases):
        raise TypeError(f"phrases: expected a dict with the keys {_PHRASE_KEYS}, got {phrases!r}")
    if not isinstance(phrases.get("lexicon"), capi.Lexicon):
        raise TypeError(f"phrases: 'lexicon' must be a capi.Lexicon, got {type(phrases.get('lexicon')).__name__}")


def _classify_phrases(rec, crops, ng: int, dev, glyphs, sub, breaks, phrases, lm=None, lm_params=None):
    """classify on device crops, glyph costs, the phrase match over the polygons of `glyphs` and - with a language model - the decode
    of the words the match found -> (labels, probs, PhraseMatches, LmPaths or None).  `sub` and `breaks` are the result of
    ocr_break_words or None: with them the gaps enter as costs (capi.phrase_gap_costs), without them the gap costs are zeros."""
    import torch
    if lm is not None and not isinstance(lm, capi.CharLm):
        raise TypeError(f"lm: expected a capi.CharLm, got {type(lm).__name__}")
    labels = np.zeros(0, np.int32)
    probs = np.zeros(0, np.float64)
    costs_ptr = 0
    if ng:
        lab = torch.empty(ng, dtype=torch.int32, device=dev)
        pr = torch.empty(ng, dtype=torch.float64, device=dev)
        logits = torch.empty((ng, 62), dtype=torch.float32, device=dev)
        rec.classify_device(crops.data_ptr(), ng, logits.data_ptr(), lab.data_ptr(), pr.data_ptr())
        costs = torch.empty((ng, 62), dtype=torch.float32, device=dev)
        rec.glyph_costs_device(logits.data_ptr(), ng, costs.data_ptr())   # blocking, behind the classify call
        costs_ptr = costs.data_ptr()
        labels, probs = lab.cpu().numpy(), pr.cpu().numpy()
    bound = join = None
    if breaks is not None:
        bound, join = capi.phrase_gap_costs(sub, breaks, float(phrases.get("break_penalty", 2.0)), float(phrases.get("join_penalty", 2.0)))
    pm = rec.phrase_match_device(phrases["lexicon"], costs_ptr, ng, glyphs.word_offsets, bound, join, phrases.get("params"))
    paths = None
    if lm is not None:
        paths = rec.lm_decode_device(lm, costs_ptr, ng, pm.word_offsets, lm_params)
        paths.best = paths.texts(pm.word_offsets)   # hypothesis 0 of every word of the match
    return labels, probs, pm, paths


def _phrase_word(text: str, probs, where, k: int, pm, lexicon, paths=None):
    """The tuple of polygon k read with phrases=: its words (the rows of line k of the match) joined by one space, a lexicon word as the
    entry's string, an out-of-vocabulary word as its per-glyph argmax or - with a language model and at most 32 glyphs - hypothesis 0
    of the decode; the polygon's rows of the match (PhraseMatches.line) are appended."""
    w0, w1 = int(pm.line_word_offsets[k]), int(pm.line_word_offsets[k + 1])
    o = (pm.word_offsets[w0:w1 + 1] - pm.word_offsets[w0]).tolist()
    parts = []
    for i in range(w1 - w0):
        e = int(pm.entries[w0 + i])
        if e >= 0:
            parts.append(lexicon.words[e])
        elif paths is not None and int(paths.word_flags[w0 + i]) == 0:
            parts.append(paths.best[w0 + i])
        else:
            parts.append(text[o[i]:o[i + 1]])
    return (" ".join(parts), probs, where, pm.line(k))


def _read_words_lattice(det, rec, x, n, h, w, dev, polys, adjust_values, params, cc, lm, lattice, split, lattice_lexicon=None,
                        lattice_lexicon_params=None, max_penalty=1.5):
    """segment -> split -> spans -> crops -> classify + costs -> decode, everything between the calls on the device; per word
    (text, probs, where, (cost, raw_cost, raw_text, seg_len)) with text, probs and where (the union boxes) along hypothesis 0's segments.
    With lattice_lexicon the joint match runs on the same span costs, and a word it accepts takes the entry's string, with probs and
    where along the match's segments; every tuple then gains (entry or -1, cost, raw_cost, seg_len of the match over the word's pieces)."""
    import torch
    if lm is not None and not isinstance(lm, capi.CharLm):
        raise TypeError(f"lm: expected a capi.CharLm, got {type(lm).__name__}")
    if lattice_lexicon is not None and not isinstance(lattice_lexicon, capi.Lexicon):
        raise TypeError(f"lattice_lexicon: expected a capi.Lexicon, got {type(lattice_lexicon).__name__}")
    prm = capi._as_lattice_params(lattice)
    glyphs = det.segment_glyphs_device(x.data_ptr(), n, h, w, polys, adjust_values, params, cc)
    pieces, _ = det.split_glyphs_device(x.data_ptr(), n, h, w, glyphs, split)
    spans, table = capi.glyph_spans(pieces, prm.max_span)
    ns = spans.n_glyphs
    labels, probs, costs_ptr = np.zeros(0, np.int32), np.zeros(0, np.float64), 0
    if ns:
        crops = torch.empty((ns, 784), dtype=torch.float32, device=dev)
        det.extract_glyph_crops_device(x.data_ptr(), n, h, w, spans, crops.data_ptr(), params)
        lab = torch.empty(ns, dtype=torch.int32, device=dev)
        pr = torch.empty(ns, dtype=torch.float64, device=dev)
        logits = torch.empty((ns, 62), dtype=torch.float32, device=dev)
        costs = torch.empty((ns, 62), dtype=torch.float32, device=dev)
        rec.classify_device(crops.data_ptr(), ns, logits.data_ptr(), lab.data_ptr(), pr.data_ptr())
        rec.glyph_costs_device(logits.data_ptr(), ns, costs.data_ptr())   # blocking, behind the classify call
        costs_ptr = costs.data_ptr()
        labels, probs = lab.cpu().numpy(), pr.cpu().numpy()
    so, po = table.span_offsets, table.piece_offsets
    if lm is not None:
        paths = rec.lattice_decode_device(lm, costs_ptr, ns, so, po, prm)
    else:
        with capi.CharLm(rec, np.zeros((64, 64), np.float32)) as zero:
            paths = rec.lattice_decode_device(zero, costs_ptr, ns, so, po, prm)
    matches = None
    if lattice_lexicon is not None:
        given = capi._as_lexlat_params(lattice_lexicon_params)
        mp = capi.LexLatParams.from_buffer_copy(given) if given is not None else capi.lexlat_params()
        mp.max_span = prm.max_span              # the lattice's spans and span costs: both searches read the same rows
        for i in range(4):
            mp.span_cost[i] = prm.span_cost[i]
        matches = rec.lexicon_lattice_match_device(lattice_lexicon, costs_ptr, ns, so, po, mp)
    M = prm.max_span
    base = lambda e: e * (e + 1) // 2 if e <= M else M * (M + 1) // 2 + (e - M) * M   # the spans in front of end e + 1
    out = []
    for b in range(n):
        words = []
        for k in range(int(pieces.img_offsets[b]), int(pieces.img_offsets[b + 1])):
            p0, G, s0 = int(po[k]), int(po[k + 1] - po[k]), int(so[k])
            single = [s0 + base(e - 1) for e in range(1, G + 1)]
            raw_text = "".join(VALUES[int(labels[r])] for r in single)
            segs = [(p - p0, m) for p, m, _ in paths.segments(po, k)] if int(paths.word_flags[k]) == 0 else [(i, 1) for i in range(G)]
            rows = [s0 + base(i + m - 1) + (m - 1) for i, m in segs]
            text = paths.text(po, k) if int(paths.word_flags[k]) == 0 else raw_text
            extra = [(float(paths.costs[k, 0]), float(paths.raw_costs[k]), raw_text, tuple(m for _, m in segs))]
            if matches is not None:
                e, c, r = int(matches.entries[k, 0]), float(matches.costs[k, 0]), float(matches.raw_costs[k])
                if e >= 0 and c - r <= float(max_penalty) * G:
                    text = lattice_lexicon.words[e]
                    rows = [s0 + base(p - p0 + m - 1) + (m - 1) for p, m, _ in matches.segments(po, k)]
                extra.append((e, c, r, tuple(int(v) for v in matches.seg_len[0, p0:p0 + G])))
            words.append((text, probs[rows].copy() if rows else np.zeros(0, np.float64), spans.boxes[rows].reshape(-1, 4).copy(), *extra))
        out.append(words)
    return out


def read_words(det_net, rec_net, frames, polygon_scores, adjust_values, params=None, cc=None, mask=None, lexicon=None,
               lexicon_params=None, max_penalty=1.5, lm=None, lm_params=None, lattice=None,
               split=None, lattice_lexicon=None, lattice_lexicon_params=None, spaces=None, phrases=None) -> List[List[Tuple[str, np.ndarray, np.ndarray]]]:
    """Reads every detected word of a batch.

    det_net: text_detection.FuncT or capi.Detector (supplies the GPU and stream of the segmentation); rec_net: char_recognition.Net
    or capi.Recognizer.  frames: the detector's input, N x 1 x H x W f32 raw 0..255, a numpy array or a CUDA tensor.
    polygon_scores: what get_boxes_and_box_scores returned (or its per-image polygon lists); adjust_values: N x 2 as given to it.
    params: capi.SegmentParams, a dict of its fields, or None for the defaults.  cc: None segments by the column rule; capi.CcParams
    or a dict of its fields ({} for the defaults) segments by connected components (ocr_segment_glyphs_cc), which splits kerned letters.
    mask: None or False cuts every crop from its box alone; True, {} or {"halo": 0} (capi.MaskParams' fields) needs cc and masks every
    crop by its glyph's components (ocr_segment_glyphs_cc_labelled, ocr_extract_glyph_crops_masked): a kerned neighbour's ink stays out.
    Returns per image, per polygon: (text, probability of every character (f64), glyph boxes k x 4 int32 x0, y0, x1, y1 in frame
    pixels, half-open).  A flat word reads as "".
    lexicon: None, or a capi.Lexicon on the recogniser's GPU: every word is matched against it (ocr_lexicon_match with lexicon_params:
    capi.LexiconParams, a dict of its fields or None) and its tuple gains a fourth element (entry index or -1, cost, raw_cost, raw
    text); the text becomes the entry's string when a candidate exists and cost - raw_cost <= max_penalty * G for the word's G glyphs,
    otherwise the raw text stays.  With lexicon=None nothing changes.
    lm: None, or a capi.CharLm on the recogniser's GPU: every word is decoded under it (ocr_lm_decode with lm_params: capi.LmParams, a
    dict of its fields or None), the text of a decoded word becomes hypothesis 0's string, and the tuple gains (lm_cost, raw_cost,
    raw_text) as its last element: the cost of hypothesis 0, the cost of the greedy reading under the model, the greedy text.  With
    both lexicon and lm a word the lexicon accepted keeps the entry's string, the others take the model's, and the lexicon's element
    comes first.  With lm=None nothing changes.
    lattice: None, or capi.LatticeParams, a dict of its fields or {} for the defaults: the segmentation is searched too.  The glyphs
    are cut into pieces (ocr_split_glyphs with split: capi.SplitParams, a dict of its fields or None), every run of up to max_span
    pieces is cropped and classified, and ocr_lattice_decode picks segments and classes together under lm (lm=None: a zero model
    created for the call; lm_params is not used, top_k is the lattice's).  The text is hypothesis 0's, probs and where follow its
    segments (where holds the union box of every segment), and the tuple gains (cost, raw_cost, raw_text, seg_len) as its last
    element: raw_text is the reading of the pieces one by one, seg_len the pieces per character.  Masked crops with a lattice raise
    OcrError (labels do not map to pieces), and so does lexicon= (the match over a fixed segmentation; the joint search is
    lattice_lexicon=).  With lattice=None nothing changes.
    lattice_lexicon: None, or a capi.Lexicon on the recogniser's GPU, with lattice= only: after the decode the entries are matched
    over the pieces on the same span costs (ocr_lexicon_lattice_match with lattice_lexicon_params: capi.LexLatParams, a dict of its
    fields or None; max_span and span_cost are always the lattice's).  A word takes the best entry's string when an entry exists and
    cost - raw_cost <= max_penalty * G for its G pieces (f64); its probs and where then follow the match's segments (an inserted
    character has none, and neither has a deleted piece).  Every tuple gains (entry index or -1, cost, raw_cost, seg_len) as its last
    element, seg_len being the match's per piece: m at the first piece of a segment, 0 inside it, -1 at a deleted piece.  With
    lattice_lexicon=None nothing changes.
    spaces: None, or capi.BreakParams, a dict of its fields or {} for the defaults: a polygon that holds several words is cut at its
    inter-word gaps (ocr_break_words) between the crops and the classify call.  Segmentation and crops run on the polygons (masked
    crops keep working: the labels are per polygon); lexicon= and lm= then match and decode every sub-word on its own.  The text of a
    polygon is its sub-word texts joined by one space, probs and where stay per glyph, the lexicon's and the model's elements become
    lists with one entry per sub-word, and the tuple gains (starts, gap_pct) as its last element: starts int32 [S+1], the sub-word
    ranges inside the polygon's glyphs, and gap_pct int32 [S], the gap in front of every sub-word in percent of the polygon's median
    glyph height (0 for the first).  lattice= with spaces= raises OcrError: the composition is not built.  With spaces=None nothing
    changes.
    phrases: None, or a dict with `lexicon` (a capi.Lexicon) and optionally `params` (capi.PhraseParams or a dict of its fields),
    `break_penalty` and `join_penalty` (default 2.0 each): the glyphs of every polygon are segmented into lexicon words and
    out-of-vocabulary words by one search over the glyph costs (ocr_lexicon_phrase_match), after the classify call.  With spaces= the
    breaks of ocr_break_words enter as costs (capi.phrase_gap_costs: starting a word where the gaps found none costs break_penalty,
    reading across a found break costs join_penalty) and cut nothing; without it the gap costs are zeros.  The polygon's text is its
    words joined by one space: a lexicon word is the entry's string, an out-of-vocabulary word its per-glyph argmax or, with lm=, the
    model's best reading of it (words of at most 32 glyphs).  probs and where stay per glyph, and the tuple's last element is the
    polygon's rows of the match (capi.PhraseMatches.line: word_offsets relative to the polygon, entries, word_costs, line_costs,
    raw_costs, line_flags).  phrases= with lexicon= or lattice= raises OcrError.  With phrases=None nothing changes."""
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
    if phrases is not None:
        _check_phrases(phrases, lexicon, lattice)
    if lattice is not None:
        if spaces is not None:
            raise capi.OcrError(1, "lattice: the composition with spaces= is not built (break the words, then call the lattice calls on the block)")
        if _masked(mask, cc):
            raise capi.OcrError(1, "lattice: masked crops are not built for pieces (labels do not map to them)")
        if lexicon is not None:
            raise capi.OcrError(1, "lattice: lexicon= matches a fixed segmentation; the joint search is lattice_lexicon=")
        return _read_words_lattice(det, rec, x, n, h, w, dev, polys, adjust_values, params, cc, lm, lattice, split, lattice_lexicon,
                                   lattice_lexicon_params, max_penalty)
    if lattice_lexicon is not None:
        raise capi.OcrError(1, "lattice_lexicon: the joint search needs lattice= ({} for its defaults)")
    glyphs, crops = _segment_and_crop(det, x.data_ptr(), n, h, w, polys, adjust_values, params, cc, mask, dev)   # blocking
    ng = glyphs.n_glyphs
    sub, breaks = det.break_words(glyphs, spaces) if spaces is not None else (glyphs, None)
    if phrases is not None:
        labels, probs, pm, paths = _classify_phrases(rec, crops, ng, dev, glyphs, sub, breaks, phrases, lm, lm_params)
    else:
        labels, probs, matches, paths = _classify(rec, crops, ng, dev, sub.word_offsets, lexicon, lexicon_params, lm, lm_params)
    out = []
    for b in range(n):
        words = []
        for k in range(int(glyphs.img_offsets[b]), int(glyphs.img_offsets[b + 1])):
            g0, g1 = int(glyphs.word_offsets[k]), int(glyphs.word_offsets[k + 1])
            text = "".join(VALUES[int(c)] for c in labels[g0:g1])
            if phrases is not None:
                words.append(_phrase_word(text, probs[g0:g1].copy(), glyphs.boxes[g0:g1].copy(), k, pm, phrases["lexicon"], paths))
            elif breaks is None:
                words.append(_word(text, probs[g0:g1].copy(), glyphs.boxes[g0:g1].copy(), k, g1 - g0, matches, lexicon, max_penalty, paths))
            else:
                words.append(_spaced_word(text, probs[g0:g1].copy(), glyphs.boxes[g0:g1].copy(), k, g0, sub, breaks, matches, lexicon,
                                          max_penalty, paths))
        out.append(words)
    return out


def glyph_crops(det_net, frames: np.ndarray, polygon_scores, adjust_values, params: Optional[dict] = None):
    """Host-memory form of the first two stages: (capi.GlyphSet, n_glyphs x 784 f32 crops)."""
    det = _handle(det_net, capi.Detector)
    polys = getattr(polygon_scores, "polygons", polygon_scores)
    glyphs = det.segment_glyphs(frames, polys, adjust_values, params)
    return glyphs, det.extract_glyph_crops(frames, glyphs, params)


def strip_glyph_quads(strips: "capi.WordStrips", words: np.ndarray, boxes: np.ndarray) -> np.ndarray:
    """Glyph boxes (x0, y0, x1, y1, half-open atlas pixels), glyph g of strip words[g] -> k x 4 x 2 f64 frame coordinates of the
    corners (x0, y0), (x1, y0), (x1, y1), (x0, y1): TL + cs * (U / Ws) + rs * (V / Hs), in that order, with cs = x - col_offsets[word]
    and U, V the sides of the word's quad."""
    words = np.asarray(words, np.int64)
    q = strips.quads[words]
    c0 = strips.col_offsets[words].astype(np.float64)[:, None]
    ws = (strips.col_offsets[words + 1] - strips.col_offsets[words]).astype(np.float64)
    hs = float(strips.height)
    cux, cuy = ((q[:, 2] - q[:, 0]) / ws)[:, None], ((q[:, 3] - q[:, 1]) / ws)[:, None]
    rvx, rvy = ((q[:, 6] - q[:, 0]) / hs)[:, None], ((q[:, 7] - q[:, 1]) / hs)[:, None]
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    cs = np.stack([b[:, 0], b[:, 2], b[:, 2], b[:, 0]], axis=1).astype(np.float64) - c0
    rs = np.stack([b[:, 1], b[:, 1], b[:, 3], b[:, 3]], axis=1).astype(np.float64)
    return np.stack([(q[:, 0:1] + cs * cux) + rs * rvx, (q[:, 1:2] + cs * cuy) + rs * rvy], axis=2)


def curved_glyph_quads(strips: "capi.CurvedStrips", words: np.ndarray, boxes: np.ndarray) -> np.ndarray:
    """strip_glyph_quads for curved strips: glyph g of strip words[g] -> k x 4 x 2 f64 frame coordinates of the corners (x0, y0), (x1, y0),
    (x1, y1), (x0, y1).  The sampling map of ocr_extract_curved_strips in f64 from the f32 knots: t = (x - c0) * (32 / Ws),
    r = min(int(t), 31), f = t - r, (px, py, nx, ny) = knot_r + f * (knot_(r+1) - knot_r), the point (px + o * nx, py + o * ny) at the
    row offset o = y - Hs / 2."""
    words = np.asarray(words, np.int64)
    c0 = strips.col_offsets[words].astype(np.float64)[:, None]
    ws = (strips.col_offsets[words + 1] - strips.col_offsets[words]).astype(np.float64)[:, None]
    hs = float(strips.height)
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    xs = np.stack([b[:, 0], b[:, 2], b[:, 2], b[:, 0]], axis=1).astype(np.float64)
    ys = np.stack([b[:, 1], b[:, 1], b[:, 3], b[:, 3]], axis=1).astype(np.float64)
    t = (xs - c0) * (32.0 / ws)
    r = np.clip(t.astype(np.int64), 0, 31)
    f = (t - r.astype(np.float64))[..., None]
    kn = strips.knots.astype(np.float64)
    k0, k1 = kn[words[:, None], r], kn[words[:, None], r + 1]
    kv = k0 + f * (k1 - k0)
    o = ys - hs / 2
    return np.stack([kv[..., 0] + o * kv[..., 2], kv[..., 1] + o * kv[..., 3]], axis=2)


def _curved(curved, strip_params):
    """curved: None / False -> None (the straight strips); True, {} , a dict of capi.CurveParams' fields or a capi.CurveParams -> the
    CurveParams, which take strip_height and max_width from strip_params where the dict does not name them."""
    if curved is None or curved is False:
        return None
    if isinstance(curved, capi.CurveParams):
        return curved
    fields = {}
    if isinstance(strip_params, capi.StripParams):
        fields.update(strip_height=strip_params.strip_height, max_width=strip_params.max_width)
    elif strip_params:
        fields.update(strip_params)
    if curved is not True:
        fields.update(curved)
    return capi.curve_params(**fields)


def read_words_rectified(det_net, rec_net, frames, polygon_scores, adjust_values, strip_params=None, params=None, cc=None, mask=None,
                         curved=None, lexicon=None, lexicon_params=None, max_penalty=1.5, lm=None, lm_params=None, spaces=None,
                         phrases=None) -> List[List[Tuple[str, np.ndarray, np.ndarray]]]:
    """Reads every detected word of a batch through its upright strip: rotated words are read along their own axis, and with
    curved=True (or {} or a dict of capi.CurveParams' fields: strip_height, max_width, valid_pct) words that bend are read along their
    own centreline (ocr_plan_curved_strips, ocr_extract_curved_strips; the glyph quads then come from curved_glyph_quads).  curved=None
    or False takes the straight strips.

    Arguments as read_words; strip_params: capi.StripParams, a dict of its fields (strip_height, max_width) or None for the defaults;
    params, cc and mask: the segmentation parameters, rule and crop masking as in read_words, applied to the atlas.  Returns per image, per polygon: (text, probability of every character
    (f64), glyph quads k x 4 x 2 f64: the corners (x0, y0), (x1, y0), (x1, y1), (x0, y1) of every glyph box mapped back to frame
    coordinates, strip_glyph_quads).  A flat word reads as "".  lexicon, lexicon_params, max_penalty, lm and lm_params as in read_words; spaces likewise, applied to the atlas' glyph block (a strip is upright, so the
    gaps are measured along the word's own axis), and phrases likewise (the tuple's last element is then the polygon's rows of the match)."""
    import torch

    det = _handle(det_net, capi.Detector)
    rec = _handle(rec_net, capi.Recognizer)
    polys = getattr(polygon_scores, "polygons", polygon_scores)
    scores = getattr(polygon_scores, "scores", None)
    x = _device_frames(det, frames)
    dev = x.device
    n, _, h, w = x.shape
    cp = _curved(curved, strip_params)
    if phrases is not None:
        _check_phrases(phrases, lexicon)
    if cp is None:
        strips = det.plan_word_strips(polys, adjust_values, h, w, strip_params, scores)
    else:
        strips = det.plan_curved_strips(polys, adjust_values, h, w, cp, scores)
    if strips.total_width == 0:
        return [[] for _ in range(n)]
    atlas = torch.empty((strips.height, strips.total_width), dtype=torch.float32, device=dev)
    if cp is None:
        det.extract_word_strips_device(x.data_ptr(), n, h, w, strips, atlas.data_ptr())      # blocking
    else:
        det.extract_curved_strips_device(x.data_ptr(), n, h, w, strips, atlas.data_ptr())    # blocking
    hs, tw = strips.height, strips.total_width
    with strips.polygon_block() as rects:
        glyphs, crops = _segment_and_crop(det, atlas.data_ptr(), 1, hs, tw, rects, [[1.0, 1.0]], params, cc, mask, dev)
    ng = glyphs.n_glyphs
    sub, breaks = det.break_words(glyphs, spaces) if spaces is not None else (glyphs, None)
    if phrases is not None:
        labels, probs, pm, paths = _classify_phrases(rec, crops, ng, dev, glyphs, sub, breaks, phrases, lm, lm_params)
    else:
        labels, probs, matches, paths = _classify(rec, crops, ng, dev, sub.word_offsets, lexicon, lexicon_params, lm, lm_params)
    quads = (strip_glyph_quads if cp is None else curved_glyph_quads)(
        strips, np.repeat(np.arange(glyphs.n_words), np.diff(glyphs.word_offsets)), glyphs.boxes)
    text = "".join(VALUES[int(c)] for c in labels)
    out = []
    for b in range(n):
        words = []
        for k in range(int(strips.img_offsets[b]), int(strips.img_offsets[b + 1])):
            g0, g1 = int(glyphs.word_offsets[k]), int(glyphs.word_offsets[k + 1])
            if phrases is not None:
                words.append(_phrase_word(text[g0:g1], probs[g0:g1].copy(), quads[g0:g1].copy(), k, pm, phrases["lexicon"], paths))
            elif breaks is None:
                words.append(_word(text[g0:g1], probs[g0:g1].copy(), quads[g0:g1].copy(), k, g1 - g0, matches, lexicon, max_penalty, paths))
            else:
                words.append(_spaced_word(text[g0:g1], probs[g0:g1].copy(), quads[g0:g1].copy(), k, g0, sub, breaks, matches, lexicon,
                                          max_penalty, paths))
        out.append(words)
    return out


def _words_and_strips(who, det_net, rec_net, frames, polygon_scores, adjust_values, rectified, reading_kwargs):
    """the words of a batch read (rectified or not) and the word strips planned for their quads -> (detector handle, words, strips)"""
    det = _handle(det_net, capi.Detector)
    if rectified:
        words = read_words_rectified(det_net, rec_net, frames, polygon_scores, adjust_values, **reading_kwargs)
    else:
        if "strip_params" in reading_kwargs or "curved" in reading_kwargs:
            raise TypeError(f"{who}: strip_params and curved belong to rectified=True")
        words = read_words(det_net, rec_net, frames, polygon_scores, adjust_values, **reading_kwargs)
    polys = getattr(polygon_scores, "polygons", polygon_scores)
    _, _, h, w = frames.shape
    strips = det.plan_word_strips(polys, adjust_values, h, w, reading_kwargs.get("strip_params"), getattr(polygon_scores, "scores", None))
    return det, words, strips


def read_lines(det_net, rec_net, frames, polygon_scores, adjust_values, line_params=None, rectified=True, **reading_kwargs
               ) -> List[List[Tuple[str, np.ndarray, np.ndarray]]]:
    """Reads every detected word of a batch and groups the words of every image into text lines in reading order (ocr_group_lines).

    Arguments as read_words_rectified (rectified=True, the default) or read_words (rectified=False); strip_params, params, cc, mask and
    curved go to that call unchanged, and so do lexicon, lexicon_params, max_penalty, lm and lm_params (the lines then join the matched or decoded texts) and spaces (a polygon's text then carries its inner spaces, in place) and phrases (likewise).  line_params: capi.LineParams, a dict of its fields (line_tol, height_ratio, min_cos, max_gap) or
    None for the defaults.  The quads always come from ocr_plan_word_strips (with strip_params where given): word order equals polygon
    order in every reading call, and the curved plan carries no quads.
    Returns per image a list of lines (text, word_indices, gaps): word_indices are the image's polygon indices in reading order (int32),
    gaps[k] the gap in front of word k of the line in units of the taller neighbour's height (0.0 for the first), text the non-empty
    word texts joined by one space."""
    det, words, strips = _words_and_strips("read_lines", det_net, rec_net, frames, polygon_scores, adjust_values, rectified, reading_kwargs)
    n = frames.shape[0]
    lines = det.group_lines(strips.quads, strips.img_offsets, line_params)
    # one pass over the lines of the batch: slices of the batch's arrays (views), the texts by batch-global word index
    texts = [wd[0] for page in words for wd in page]
    order = lines.order.tolist()
    local = lines.order - np.repeat(strips.img_offsets[:-1], np.diff(strips.img_offsets))[lines.order]
    img_off, line_off = lines.img_offsets.tolist(), lines.line_offsets.tolist()
    out = []
    for b in range(n):
        page = []
        for l in range(img_off[b], img_off[b + 1]):
            p0, p1 = line_off[l], line_off[l + 1]
            page.append((" ".join(filter(None, [texts[k] for k in order[p0:p1]])), local[p0:p1], lines.gaps[p0:p1]))
        out.append(page)
    return out


def read_columns(det_net, rec_net, frames, polygon_scores, adjust_values, column_params=None, rectified=True, **reading_kwargs
                 ) -> List[List[List[Tuple[str, np.ndarray, np.ndarray]]]]:
    """read_lines with columns: the words of every image as blocks (columns, paragraphs) in reading order (ocr_group_columns), so that a
    two-column page reads down its left column before its right one.

    Arguments as read_lines; column_params: capi.ColumnParams, a dict of its fields (the line fields among them) or None for the
    defaults.  Returns per image a list of blocks, each a list of lines (text, word_indices, gaps) as read_lines returns them, top to
    bottom."""
    det, words, strips = _words_and_strips("read_columns", det_net, rec_net, frames, polygon_scores, adjust_values, rectified, reading_kwargs)
    cols = det.group_columns(strips.quads, strips.img_offsets, column_params)
    texts = [wd[0] for page in words for wd in page]
    order = cols.order.tolist()
    local = cols.order - np.repeat(strips.img_offsets[:-1], np.diff(strips.img_offsets))[cols.order]
    img_off, blk_off, line_off = cols.img_offsets.tolist(), cols.block_offsets.tolist(), cols.line_offsets.tolist()
    out = []
    for b in range(frames.shape[0]):
        page = []
        for k in range(img_off[b], img_off[b + 1]):
            block = []
            for l in range(blk_off[k], blk_off[k + 1]):
                p0, p1 = line_off[l], line_off[l + 1]
                block.append((" ".join(filter(None, [texts[w] for w in order[p0:p1]])), local[p0:p1], cols.gaps[p0:p1]))
            page.append(block)
        out.append(page)
    return out


def page_text(lines, columns=False) -> str:
    """The lines of one image (an element of read_lines' result) joined with "\n".  columns=True takes an element of read_columns'
    result: the lines of every block joined with "\n", the blocks separated by an empty line."""
    if columns:
        return "\n\n".join("\n".join(text for text, _, _ in block) for block in lines)
    return "\n".join(text for text, _, _ in lines)
