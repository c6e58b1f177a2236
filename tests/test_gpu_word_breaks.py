"""ocr_break_words on the MI355X (csrc/word_breaks.hip) against tests/word_break_oracle.py: every array of both results bit for bit,
over the lane, slot and limit edges of the word length, the workgroup edges of the word count, images without words, coordinates up
to 2^22, heavy ties and the ends of every parameter; the output block through the crop, split and span calls; read_words,
read_words_rectified and read_lines with spaces=; every OCR_ERR_INVALID case with the handle used again; two handles from two threads."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import word_break_jobs as J
from tests import word_break_oracle as WB

pytestmark = pytest.mark.gpu

INVALID = 1      # OCR_ERR_INVALID (include/ocr_amd.h)


@pytest.fixture(scope="module")
def det():
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def rec():
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    r = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    yield r
    r.close()


def _set(blk):
    from ocr_rs_amd import capi
    return capi.GlyphSet(blk["img_offsets"], blk["word_offsets"], blk["word_info"], blk["word_levels"], blk["boxes"])


def _as_dict(gs):
    return dict(img_offsets=gs.img_offsets, word_offsets=gs.word_offsets, word_info=gs.word_info, word_levels=gs.word_levels, boxes=gs.boxes)


def _differs(got, want):
    """the first array of (words, breaks) that is not the oracle's bit for bit, or None"""
    words, breaks = got
    ww, wb = want
    for name in ("img_offsets", "word_offsets", "word_info", "boxes"):
        a, b = getattr(words, name).reshape(-1), np.asarray(ww[name]).reshape(-1)
        if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(a, b):
            return name
    if not np.array_equal(words.word_levels.view(np.uint32).reshape(-1), ww["word_levels"].view(np.uint32).reshape(-1)):
        return "word_levels"
    for name in ("source", "sub_offsets", "gap_pct", "source_info"):
        a, b = getattr(breaks, name), wb[name]
        if a.reshape(-1).shape != b.reshape(-1).shape or not np.array_equal(a.reshape(-1), b.reshape(-1)):
            return name
    return None


_WANT = {}


def _want(name, blk, params):
    """the oracle's result, computed once per (block, parameters)"""
    key = (name, tuple(sorted((params or {}).items())))
    if key not in _WANT:
        _WANT[key] = WB.break_words(blk, params)
    return _WANT[key]


def _check(det, name, blk, params):
    got = det.break_words(_set(blk), params)
    want = _want(name, blk, params)
    d = _differs(got, want)
    assert d is None, (name, params, d)
    return got


@pytest.mark.parametrize("mode", [0, 1])
def test_word_lengths_at_lane_slot_and_limit_edges(det, mode):
    words, breaks = _check(det, "edges", J.edges(), {"mode": mode})
    assert breaks.n_source == len(J.EDGE_LENGTHS) and breaks.source_info[-1].tolist() == [0, 0, 0, 2]
    assert breaks.sub_offsets[-1] - breaks.sub_offsets[-2] == 1                       # 257 glyphs: one sub-word holding all of them
    assert breaks.n_words > breaks.n_source and set(breaks.source_info[:, 1].tolist()) == ({0, 1, 2} if mode else {0, 1})
    # every length alone as well: a batch of one word
    for G in J.EDGE_LENGTHS:
        one = J.block_of([J.edges()["boxes"][J.edges()["word_offsets"][J.EDGE_LENGTHS.index(G)]:][:G].tolist()])
        _check(det, f"edge {G}", one, {"mode": mode})


@pytest.mark.parametrize("nw", J.BATCHES)
def test_word_counts_at_workgroup_edges_with_mixed_lengths(det, nw):
    for mode in (0, 1):
        words, breaks = _check(det, f"batch {nw}", J.batch(nw), {"mode": mode})
        assert breaks.n_source == nw and words.n_images == 4


def test_images_without_words_and_empty_blocks(det):
    blk = J.block_of([J.row([2, 2, 9, 2]), [], J.row([3])], n_images=5, cuts=[0, 1, 1, 3])
    words, breaks = _check(det, "holes", blk, None)
    assert words.img_offsets.tolist() == [0, 0, 2, 2, 4, 4] and breaks.sub_offsets.tolist() == [0, 2, 3, 4]
    # no glyphs at all: nothing is launched, every word is one empty sub-word
    none = J.block_of([[], []], n_images=3, cuts=[1, 1])
    words, breaks = _check(det, "no glyphs", none, None)
    assert words.n_glyphs == 0 and words.word_offsets.tolist() == [0, 0, 0] and breaks.source_info.tolist() == [[0, 0, 0, 0]] * 2
    words, breaks = _check(det, "no words", J.block_of([], n_images=2, cuts=[0]), None)
    assert words.n_words == 0 and words.img_offsets.tolist() == [0, 0, 0] and breaks.sub_offsets.tolist() == [0]


@pytest.mark.parametrize("params", [None, {"mode": 0}, {"space_pct": 1000, "sep_pct": 1000, "min_space_pct": 1000},
                                    {"space_pct": 1, "sep_pct": 100, "min_space_pct": 1}])
def test_coordinates_up_to_2_to_the_22(det, params):
    words, breaks = _check(det, "wide", J.wide(), params)
    if params is None:
        assert breaks.source_info[-1].tolist() == [1, 2, (1 << 22) - 6, 0] and int(breaks.gap_pct.max()) == ((1 << 22) - 6) * 100


@pytest.mark.parametrize("params", [None, {"mode": 0}, {"sep_pct": 100, "min_space_pct": 1}])
def test_heavy_ties(det, params):
    words, breaks = _check(det, "ties", J.ties(), params)
    if params is None:
        assert {1, 2} <= set(breaks.source_info[:, 1].tolist())


@pytest.mark.parametrize("field,values", [("space_pct", (1, 1000)), ("min_space_pct", (1, 1000)), ("sep_pct", (100, 1000)), ("min_gaps", (3, 255))])
def test_parameters_at_both_ends(det, field, values):
    from ocr_rs_amd import capi
    for v in values:
        _check(det, "edges", J.edges(), {field: v})
        _check(det, "ties", J.ties(), {field: v})
    got = det.break_words(_set(J.ties()), capi.break_params(**{field: values[0]}))            # the struct form of the same
    assert _differs(got, _want("ties", J.ties(), {field: values[0]})) is None


def test_the_broken_block_is_an_ordinary_glyph_block(det):
    from ocr_rs_amd import capi
    fr, polys, adj = J.two_groups()
    src = det.segment_glyphs(fr, polys, adj)
    assert src.n_words == 1 and src.boxes[:, 0].tolist() == [20, 31, 42, 64, 75, 86]
    words, breaks = det.break_words(src)
    assert _differs((words, breaks), WB.break_words(_as_dict(src))) is None
    assert words.word_offsets.tolist() == [0, 3, 6] and breaks.source.tolist() == [0, 0] and breaks.gap_pct.tolist() == [0, 58]
    assert breaks.source_info.tolist() == [[24, 2, 14, 0]]
    crops = det.extract_glyph_crops(fr, words)
    assert np.array_equal(crops.view(np.uint32), det.extract_glyph_crops(fr, src).view(np.uint32)) and crops.shape == (6, 784)
    pieces, pmap = det.split_glyphs(fr, words)
    spans, table = capi.glyph_spans(pieces, 2)
    assert pieces.n_words == 2 and table.span_offsets.tolist() == [0, 5, 10]
    assert not np.any((spans.boxes[:, 0] < 50) & (spans.boxes[:, 2] > 64))          # no span reaches across the break


def _plain(pages):
    return [[(wd[0], wd[1].tolist(), np.asarray(wd[2]).tolist()) for wd in pg] for pg in pages]


def test_read_words_with_spaces(det, rec):
    from ocr_rs_amd import capi, reading
    fr, polys, adj = J.two_groups()
    before = reading.read_words(det, rec, fr, polys, adj)
    got = reading.read_words(det, rec, fr, polys, adj, spaces={})
    (t0, p0, b0), (text, pr, where, (starts, pct)) = before[0][0], got[0][0]
    assert len(t0) == 6 and text == t0[:3] + " " + t0[3:] and text.count(" ") == 1
    assert np.array_equal(pr, p0) and np.array_equal(where, b0)
    assert starts.dtype == np.int32 and starts.tolist() == [0, 3, 6] and pct.tolist() == [0, 58]
    assert _plain(reading.read_words(det, rec, fr, polys, adj, spaces=None)) == _plain(before)
    for form in (capi.break_params(), {"mode": 1}):
        assert reading.read_words(det, rec, fr, polys, adj, spaces=form)[0][0][0] == text
    assert reading.read_words(det, rec, fr, polys, adj, spaces={"mode": 0, "space_pct": 100})[0][0][0] == t0       # 14 px < 24 px
    masked = reading.read_words(det, rec, fr, polys, adj, cc={}, mask=True, spaces={})
    assert masked[0][0][0].count(" ") == 1 and masked[0][0][0][3] == " "
    rect0 = reading.read_words_rectified(det, rec, fr, polys, adj)
    rect = reading.read_words_rectified(det, rec, fr, polys, adj, spaces={})
    assert rect[0][0][0].replace(" ", "") == rect0[0][0][0] and rect[0][0][0].count(" ") == 1 and rect[0][0][0][3] == " "
    assert np.array_equal(rect[0][0][1], rect0[0][0][1]) and np.array_equal(rect[0][0][2], rect0[0][0][2])
    with pytest.raises(capi.OcrError, match="not built"):
        reading.read_words(det, rec, fr, polys, adj, lattice={}, spaces={})
    # read_lines forwards the option: the inner space is in the line's text
    for rectified in (False, True):
        lines = reading.read_lines(det, rec, fr, polys, adj, rectified=rectified, spaces={})
        assert len(lines[0]) == 1 and lines[0][0][0].count(" ") == 1 and lines[0][0][0][3] == " "
        assert " " not in reading.read_lines(det, rec, fr, polys, adj, rectified=rectified)[0][0][0]
        assert reading.page_text(lines[0]) == lines[0][0][0]


def test_a_line_of_forty_glyphs_is_decoded_once_it_is_broken(det, rec):
    from ocr_rs_amd import capi, reading
    from tests import lexicon_oracle as LX
    fr, polys, adj = J.forty_bars()
    seg = dict(max_glyphs=64)
    table = capi.char_lm_table(LX.random_words(np.random.default_rng(6), 400, 1, 9), weight=3.0)
    words = LX.random_words(np.random.default_rng(4), 50, 18, 22)
    with capi.CharLm(rec, table) as lm, capi.Lexicon(rec, words) as lex:
        whole = reading.read_words(det, rec, fr, polys, adj, params=seg, lm=lm)
        text, pr, where, (cost, raw, raw_text) = whole[0][0]
        assert len(raw_text) == 40 and text == raw_text and cost == np.inf          # more than 32 glyphs: flagged 2, not decoded
        got = reading.read_words(det, rec, fr, polys, adj, params=seg, lm=lm, spaces={})
        text, pr2, where2, model, (starts, pct) = got[0][0]
        assert starts.tolist() == [0, 20, 40] and len(model) == 2 and all(np.isfinite(c) and c <= r for c, r, _ in model)
        assert [len(t) for t in text.split(" ")] == [20, 20] and [m[2] for m in model] == [raw_text[:20], raw_text[20:]]
        assert np.array_equal(pr2, pr) and np.array_equal(where2, where)
        both = reading.read_words(det, rec, fr, polys, adj, params=seg, lexicon=lex, lm=lm, spaces={})
        _, _, _, matched, model2, (starts2, _) = both[0][0]
        assert len(matched) == 2 and len(model2) == 2 and starts2.tolist() == [0, 20, 40]       # one row of the match block per sub-word
        assert all(np.isfinite(c) and r > 0 for e, c, r, _ in matched) and [m[3] for m in matched] == [raw_text[:20], raw_text[20:]]
        # the calls by hand on the broken block
        glyphs, crops = reading.glyph_crops(det, fr, polys, adj, seg)
        sub, breaks = det.break_words(glyphs)
        costs = rec.glyph_costs(rec.forward_host(crops))
        m = rec.lexicon_match(lex, costs, sub.word_offsets)
        assert m.n_words == 2 and [(int(m.entries[k, 0]), float(m.costs[k, 0])) for k in range(2)] == [(e, c) for e, c, _, _ in matched]
        assert rec.lm_decode(lm, costs, glyphs.word_offsets).word_flags.tolist() == [2]
        assert rec.lm_decode(lm, costs, sub.word_offsets).word_flags.tolist() == [0, 0]


def _invalid(fn, *needles):
    from ocr_rs_amd import capi
    with pytest.raises(capi.OcrError) as e:
        fn()
    assert e.value.code == INVALID, e.value
    for n in needles:
        assert n in str(e.value), e.value


def test_invalid_arguments(det):
    from ocr_rs_amd import capi
    L = capi.lib()
    blk = J.block_of([J.row([2, 3, 2, 9, 2, 3, 2]), J.row([4])], n_images=2, cuts=[1])
    gs = _set(blk)
    good = lambda: det.break_words(gs)[0].word_offsets.tolist() == [0, 4, 8, 10]
    assert good()
    b = gs.block()
    out, wb = C.POINTER(capi.Glyphs)(), C.POINTER(capi.WordBreaksBlock)()
    raw = lambda *a: capi.check(L.ocr_break_words(*a))
    ok = (det._h, C.byref(b), None, C.byref(out), C.byref(wb))
    for k in (0, 1, 3, 4):      # det, glyphs, words, breaks
        args = list(ok)
        args[k] = None
        _invalid(lambda: raw(*args), "null")
        assert good()
    for name in ("img_offsets", "word_offsets", "word_info", "word_levels", "boxes"):
        nb = gs.block()
        setattr(nb, name, C.POINTER(C.c_float if name == "word_levels" else C.c_int32)())
        _invalid(lambda: raw(det._h, C.byref(nb), None, C.byref(out), C.byref(wb)), "null array")
    assert good()

    def with_offsets(word=None, img=None):
        bad = _set(blk)
        if word is not None:
            bad.word_offsets = np.asarray(word, np.int32)
        if img is not None:
            bad.img_offsets = np.asarray(img, np.int32)
        return bad
    _invalid(lambda: det.break_words(with_offsets(word=[1, 8, 10])), "span")                  # do not start at 0
    _invalid(lambda: det.break_words(with_offsets(word=[0, 11, 10])), "decrease")
    nb = gs.block()
    nb.n_glyphs = 9                                                                             # do not span the glyphs
    _invalid(lambda: raw(det._h, C.byref(nb), None, C.byref(out), C.byref(wb)), "span")
    _invalid(lambda: det.break_words(with_offsets(img=[1, 1, 2])), "span")
    _invalid(lambda: det.break_words(with_offsets(img=[0, 3, 2])), "decrease")
    _invalid(lambda: det.break_words(with_offsets(img=[0, 1, 1])), "span")
    assert good()
    top = 1 << 22
    for bad in ((5, 0, 5, 9), (6, 0, 5, 9), (0, 4, 9, 4), (0, 5, 9, 4), (-1, 0, 5, 9), (0, -1, 5, 9), (0, 0, top + 1, 9), (0, 0, 5, top + 1)):
        _invalid(lambda: det.break_words(_set(J.block_of([[(0, 0, 4, 4), bad]]))), "glyph 1")
        assert good()
    det.break_words(_set(J.block_of([[(0, 0, top, top)]])))                                    # the limit itself is inside
    for field, vals in (("mode", (-1, 2)), ("space_pct", (0, 1001)), ("min_space_pct", (0, 1001)), ("sep_pct", (99, 1001)), ("min_gaps", (2, 256))):
        for v in vals:
            _invalid(lambda: det.break_words(gs, {field: v}), "params")
    for i in range(3):
        _invalid(lambda: det.break_words(gs, dict(reserved=[int(j == i) for j in range(3)])), "params")
    assert good()
    L.ocr_word_breaks_free(None)
    L.ocr_break_default_params(None)
    p = capi.break_params()
    assert (p.mode, p.space_pct, p.min_space_pct, p.sep_pct, p.min_gaps, list(p.reserved)) == (1, 35, 25, 200, 3, [0, 0, 0])
    with pytest.raises(TypeError):
        capi.break_params(gap=3)


@pytest.mark.timeout(120)
def test_two_handles_from_two_threads_give_the_single_thread_bits():
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    jobs = [J.job(k) for k in range(2)]
    want = [_want(f"job {k}", *jobs[k]) for k in range(2)]
    errors = [[], []]
    start = threading.Barrier(2)

    def work(t):
        d = None
        try:
            d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
            gs = _set(jobs[t][0])
            start.wait(60)
            for rnd in range(6):
                diff = _differs(d.break_words(gs, jobs[t][1]), want[t])
                if diff:
                    errors[t].append(f"thread {t}, round {rnd}: {diff}")
            try:     # a refused call on this thread raises on this thread
                d.break_words(gs, {"min_gaps": 2})
                errors[t].append(f"thread {t}: min_gaps 2 was not refused")
            except capi.OcrError as e:
                if e.code != INVALID:
                    errors[t].append(f"thread {t}: {e!r}")
        except Exception as e:   # noqa: BLE001
            start.abort()
            errors[t].append(f"thread {t}: {e!r}")
        finally:
            if d is not None:
                d.close()

    threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(100)
        assert not th.is_alive(), "a thread did not return"     # (nothing more is started after a failed join)
    assert errors == [[], []], errors
