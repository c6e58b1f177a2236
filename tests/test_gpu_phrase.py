"""ocr_lexicon_phrase_match on the MI355X (csrc/lexicon_phrase.hip) against tests/phrase_oracle.py: every array of the result bit for
bit, over the window edges and both flags of the line length, the pass and chunk edges of the lexicon size, lexicons with all, missing,
repeated and single lengths, batches with empty lines and more than one group of lines, both fold_case values, gap costs, the ends of
every parameter, host and device costs; what the tree could not read before; read_words, read_words_rectified and read_lines with
phrases=; every OCR_ERR_INVALID case with the handle used again; two handles from two threads."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import lexicon_oracle as LX
from tests import phrase_oracle as PO
from tests import word_break_jobs as J
from tests.test_word_break_oracle import row

pytestmark = pytest.mark.gpu

INVALID = 1      # OCR_ERR_INVALID (include/ocr_amd.h)
KEYS = ("line_word_offsets", "word_offsets", "entries", "word_costs", "line_costs", "raw_costs", "line_flags")
EDGE_LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257]   # the window edges (32 starts, 63 rows) and both flags


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


def _differs(got, want):
    """the first array that is not the oracle's bit for bit, or None"""
    for name in KEYS:
        a, b = getattr(got, name), want[name]
        if a.dtype != b.dtype or a.shape != b.shape:
            return f"{name}: {a.dtype}{a.shape} against {b.dtype}{b.shape}"
        same = np.array_equal(a.view(np.uint64), b.view(np.uint64)) if a.dtype == np.float64 else np.array_equal(a, b)
        if not same:
            return name
    return None


def _text_costs(rng, text):
    """glyph costs of random logits with the text's class favoured: what ocr_rec_glyph_costs gives for a readable line"""
    lg = (rng.standard_normal((len(text), 62)) * 2).astype(np.float32)
    if len(text):
        lg[np.arange(len(text)), [LX.CLASS_OF[ch] for ch in text]] += 8
    return LX.glyph_costs(lg)


def _line_text(rng, words, G):
    """G characters: entries of the lexicon in a row, now and then a run that is in no lexicon, cut at G"""
    t = ""
    while len(t) < G:
        t += words[int(rng.integers(len(words)))] if rng.random() < 0.8 else "".join(LX.random_words(rng, 1, 1, 5))
    return t[:G]


def _case(seed, words, gs, integer=False, gaps=False):
    """-> (costs, line_offsets, bound, join): one line per glyph count of gs, read from the lexicon's own words"""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(np.asarray(gs, np.int64))]).astype(np.int32)
    ng = int(off[-1])
    if integer:
        cost = LX.make_costs(rng, ng, integer=True)
    else:
        cost = np.concatenate([_text_costs(rng, _line_text(rng, words, int(g))) for g in gs] + [np.zeros((0, 62), np.float32)])
    bound = join = None
    if gaps:
        bound = rng.integers(0, 3, ng).astype(np.float32) if integer else (rng.random(ng) * 3).astype(np.float32)
        join = rng.integers(0, 3, ng).astype(np.float32) if integer else (rng.random(ng) * 3).astype(np.float32)
    return cost, off, bound, join


def _check(rec, lex, words, case, prm=None, device=False):
    cost, off, bound, join = case
    if device:
        import torch
        t = torch.from_numpy(cost).to(f"cuda:{rec.device}") if cost.size else None
        got = rec.phrase_match_device(lex, t.data_ptr() if t is not None else 0, cost.shape[0], off, bound, join, prm)
    else:
        got = rec.phrase_match(lex, cost, off, bound, join, prm)
    want = PO.phrase_match(cost, off, words, bound, join, **(prm or {}))
    d = _differs(got, want)
    assert d is None, (d, prm)
    return got


def _mixed_words(seed, n, min_len=1, max_len=LX.MAX_LEN):
    return LX.random_words(np.random.default_rng(seed), n, min_len, max_len)


def test_the_new_symbols_resolve():
    from ocr_rs_amd import capi
    L = capi.lib()
    for name in ("ocr_phrase_default_params", "ocr_lexicon_phrase_match", "ocr_phrase_matches_free"):
        assert getattr(L, name) is not None and name in capi.EXPORTS
    p = capi.phrase_params()
    assert (p.word_cost, p.oov_word_cost, p.oov_glyph_cost, p.fold_case, list(p.reserved)) == (1.0, 6.0, 1.0, 1, [0, 0, 0])
    assert C.sizeof(capi.PhraseParams) == 40 and capi.PHRASE_MAX_GLYPHS == 256
    L.ocr_phrase_default_params(None)
    L.ocr_phrase_matches_free(None)
    with pytest.raises(TypeError):
        capi.phrase_params(top_k=2)


@pytest.mark.parametrize("gaps", [False, True], ids=["zero gaps", "gaps"])
def test_line_lengths_at_window_edges_and_both_flags(rec, gaps):
    from ocr_rs_amd import capi
    words = _mixed_words(11, 600)             # lengths 1..32
    with capi.Lexicon(rec, words) as lex:
        case = _case(12, words, EDGE_LENGTHS, gaps=gaps)
        got = _check(rec, lex, words, case)
        assert got.line_flags.tolist() == [1] + [0] * 10 + [2] and got.n_lines == 12
        assert np.any(got.entries >= 0) and np.any(got.entries[1:-1] < 0)            # lexicon words and OOV words both occur
        assert got.word_costs[-1] == np.inf and got.line_costs[-1] == np.inf and got.line_costs[0] == 0.0
        for k, G in enumerate(EDGE_LENGTHS):     # every length alone as well: a batch of one line
            c, off, bound, join = case
            g0, g1 = int(off[k]), int(off[k + 1])
            one = (c[g0:g1], np.array([0, G], np.int32), None if bound is None else bound[g0:g1], None if join is None else join[g0:g1])
            _check(rec, lex, words, one, device=bool(k % 2))


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 5000])
def test_lexicon_sizes_at_pass_and_chunk_edges(rec, n):
    """One length only: all n entries are one run of the sorted lexicon, so 255 / 256 / 257 are the edges of a pass of 256 lanes; mixed
    short lengths: several chunks per length.  The 5 000 are 1 667 entries three times over with whole-number costs: every minimum
    is reached by three entries of three different chunks (they lie more than 256 positions apart), and the lowest index must win."""
    from ocr_rs_amd import capi
    single = ["".join(LX.ALPHABET[c] for c in w) for w in np.random.default_rng(20 + n).integers(0, 4, (n, 3))]
    with capi.Lexicon(rec, single) as lex:
        got = _check(rec, lex, single, _case(21, single, [3, 5, 33, 70], integer=True, gaps=True))
        _check(rec, lex, single, _case(22, single, [7, 64]))
    if n >= 255:
        base = _mixed_words(23, (n + 2) // 3, 1, 4)
        mixed = (base * 3)[:n]
        with capi.Lexicon(rec, mixed) as lex:
            got = _check(rec, lex, mixed, _case(24, mixed, [4, 40, 100], integer=True), dict(word_cost=0.0))
            lexw = got.entries[got.entries >= 0]
            assert len(lexw) and int(lexw.max()) < len(base)        # a later copy of an entry never wins
            _check(rec, lex, mixed, _case(25, mixed, [9, 65], gaps=True), device=True)


def test_equal_costs_in_every_wave_of_three_chunks_go_to_the_smaller_index(rec):
    """One line of 3 glyphs whose cost rows are constant against 600 distinct entries of 3 characters (behind four of other lengths):
    every one of them costs the same, in all four waves of the three chunks of length 3, so the wave's butterflies, the read-back of
    the waves' slots and the minimum over the chunks all see equal costs and the index alone decides."""
    from ocr_rs_amd import capi
    words = ["a", "bc", "defg", "hijkl"] + ["".join(LX.ALPHABET[37 * n // d % 62] for d in (3844, 62, 1)) for n in range(600)]
    assert len(set(words)) == 604
    with capi.Lexicon(rec, words) as lex:
        got = _check(rec, lex, words, (np.full((3, 62), 0.5, np.float32), np.array([0, 3], np.int32), None, None))
    assert got.entries.tolist() == [4] and got.word_offsets.tolist() == [0, 3] and got.line_costs.tolist() == [2.5]


@pytest.mark.parametrize("name,lens", [("all lengths", list(range(1, 33))), ("missing lengths", [2, 5, 9, 32]), ("one length", [4]),
                                        ("long only", [31, 32])])
def test_lexicon_length_sets(rec, name, lens):
    from ocr_rs_amd import capi
    rng = np.random.default_rng(30 + len(lens))
    words = ["".join(LX.ALPHABET[c] for c in rng.integers(0, 62, int(m))) for m in rng.choice(lens, 300)]
    words += words[:40]                                       # duplicates
    with capi.Lexicon(rec, words) as lex:
        got = _check(rec, lex, words, _case(31, words, [1, 3, 31, 32, 33, 64, 100], gaps=True))
        assert np.any(got.entries >= 0) or name == "long only"
        _check(rec, lex, words, _case(32, words, [2, 8, 40], integer=True), dict(fold_case=0))


@pytest.mark.parametrize("nl", [1, 3, 257])
def test_batches_with_empty_lines_between(rec, nl):
    from ocr_rs_amd import capi
    words = _mixed_words(41, 200, 1, 9)
    gs = np.random.default_rng(42 + nl).choice([0, 0, 1, 3, 7, 12, 40, 70], nl).tolist()
    if nl == 3:
        gs = [5, 0, 9]
    with capi.Lexicon(rec, words) as lex:
        got = _check(rec, lex, words, _case(43, words, gs, gaps=True))
        assert got.n_lines == nl and got.word_offsets[-1] == sum(gs) and np.all(np.diff(got.line_word_offsets) >= 1)
        _check(rec, lex, words, _case(44, words, gs, integer=True), device=True)
        # no lines, and lines without any glyph: nothing to search
        none = rec.phrase_match(lex, np.zeros((0, 62), np.float32), [0])
        assert none.n_lines == 0 and none.n_words == 0 and none.word_offsets.tolist() == [0] and none.line_word_offsets.tolist() == [0]
        _check(rec, lex, words, (np.zeros((0, 62), np.float32), np.zeros(4, np.int32), None, None))


def test_more_lines_than_one_group_holds(rec):
    """2 048 windows are one group of lines (capi.PHRASE_GROUP_WINDOWS): 2 060 lines of one window each, and 300 of eight, take more."""
    from ocr_rs_amd import capi
    words = _mixed_words(51, 60, 1, 3)
    with capi.Lexicon(rec, words) as lex:
        gs = np.random.default_rng(52).integers(1, 4, capi.PHRASE_GROUP_WINDOWS + 12).tolist()
        _check(rec, lex, words, _case(53, words, gs, integer=True))
    few = ["".join(LX.ALPHABET[c] for c in w) for w in np.random.default_rng(54).integers(0, 62, (8, 2))]
    with capi.Lexicon(rec, few) as lex:
        rng = np.random.default_rng(55)
        gs = [256] * 300
        cost = LX.make_costs(rng, 256 * 300, integer=True)
        off = np.arange(301, dtype=np.int32) * 256
        got = rec.phrase_match(lex, cost, off)
        # the oracle on the lines around the group edge (line 256 opens the second group) and on the last one
        for l in (0, 255, 256, 257, 299):
            want = PO.phrase_match(cost[l * 256:(l + 1) * 256], [0, 256], few)
            assert _differs(got.line(l), want) is None, l


@pytest.mark.parametrize("prm", [dict(fold_case=0), dict(fold_case=1), dict(word_cost=0.0), dict(word_cost=1e300),
                                 dict(oov_word_cost=0.0), dict(oov_word_cost=1e300), dict(oov_glyph_cost=0.0), dict(oov_glyph_cost=1e300),
                                 dict(word_cost=0.0, oov_word_cost=0.0, oov_glyph_cost=0.0)],
                         ids=lambda p: " ".join(f"{k}={v:g}" for k, v in p.items()))
def test_parameters_at_both_ends(rec, prm):
    from ocr_rs_amd import capi
    words = _mixed_words(61, 300, 1, 8)
    with capi.Lexicon(rec, words) as lex:
        _check(rec, lex, words, _case(62, words, [1, 6, 33, 90], gaps=True), prm)
        _check(rec, lex, words, _case(63, words, [4, 64], integer=True, gaps=True), prm)
        got = rec.phrase_match(lex, *_case(62, words, [1, 6, 33, 90], gaps=True), capi.phrase_params(**prm))      # the struct form
        assert _differs(got, PO.phrase_match(*_case(62, words, [1, 6, 33, 90], gaps=True)[:2], words,
                                             *_case(62, words, [1, 6, 33, 90], gaps=True)[2:], **prm)) is None


# ---- what the tree could not read before

def test_inthebox_reads_in_the_box(rec):
    from ocr_rs_amd import capi
    words = ["in", "the", "box"]
    cost = PO.costs_for_phrase("inthebox", np.random.default_rng(5), noise=0.5)
    with capi.Lexicon(rec, words) as lex:
        got = rec.phrase_match(lex, cost, [0, 8])
        assert _differs(got, PO.phrase_match(cost, [0, 8], words)) is None
        assert " ".join(words[e] for e in got.entries) == "in the box" and got.word_offsets.tolist() == [0, 2, 5, 8]
        # the word match on the same polygon: no entry of an admissible length (8 glyphs against 2 and 3 characters), flag 4
        whole = rec.lexicon_match(lex, cost, [0, 8])
        want = LX.match(cost, [0, 8], words)
        assert whole.word_flags.tolist() == want["word_flags"].tolist() == [4] and whole.entries.tolist() == want["entries"].tolist() == [[-1]]


def test_a_letter_spaced_word_comes_back_as_one_entry(det, rec):
    from ocr_rs_amd import capi
    text = "SPACED"
    blk = J.block_of([row([12] * 5)])            # equal, wide gaps: 60 % of the glyph height each
    gs = capi.GlyphSet(blk["img_offsets"], blk["word_offsets"], blk["word_info"], blk["word_levels"], blk["boxes"])
    sub, breaks = det.break_words(gs)
    assert breaks.source_info[0, 1] == 1 and sub.word_offsets.tolist() == list(range(7))       # rule 1 broke it at every letter
    # (no set of entries tiles the word: with every gap a found break, a join costs 2.0 and a further word 1.0, so `SPA` + `CED` or
    # single letters would come out cheaper than the one entry, as the rule says they must)
    words = ["SPA", "ACE", "SPACED", "PACE"]
    cost = PO.costs_for_phrase(text, np.random.default_rng(6), noise=0.5)
    bound, join = capi.phrase_gap_costs(sub, breaks)
    assert bound.tolist() == [0.0] * 6 and join.tolist() == [2.0] * 6
    wb, wj = PO.gap_costs(sub.word_offsets, 6)
    assert np.array_equal(bound, wb) and np.array_equal(join, wj)
    with capi.Lexicon(rec, words) as lex:
        got = rec.phrase_match(lex, cost, gs.word_offsets, bound, join)
        assert _differs(got, PO.phrase_match(cost, gs.word_offsets, words, bound, join)) is None
        assert got.entries.tolist() == [2] and got.word_offsets.tolist() == [0, 6]
        # the word match on the broken block sees six words of one glyph: no entry of that length, and nothing puts them together
        apart = rec.lexicon_match(lex, cost, sub.word_offsets, dict(max_len_diff=0))
        want = LX.match(cost, sub.word_offsets, words, max_len_diff=0)
        assert apart.word_flags.tolist() == want["word_flags"].tolist() == [4] * 6 and apart.entries[:, 0].tolist() == [-1] * 6


def test_a_polygon_of_forty_glyphs_is_read_as_its_words(rec):
    from ocr_rs_amd import capi
    words = _mixed_words(71, 50, 18, 22)
    text = (words[7] + words[31])[:40].ljust(40, "x")
    cost = _text_costs(np.random.default_rng(72), text)
    with capi.Lexicon(rec, words) as lex:
        assert rec.lexicon_match(lex, cost, [0, 40]).word_flags.tolist() == [2]
        got = rec.phrase_match(lex, cost, [0, 40])
        assert _differs(got, PO.phrase_match(cost, [0, 40], words)) is None
        assert got.entries[0] == 7 and got.line_flags.tolist() == [0] and got.word_offsets[1] == len(words[7])


# ---- the reading chain

def _plain(pages):
    return [[(wd[0], wd[1].tolist(), np.asarray(wd[2]).tolist()) for wd in pg] for pg in pages]


def _compose(pm, k, raw, words, best=None, flags=None):
    """the text of polygon k from the C calls' results: entries as the lexicon's strings, OOV words as the raw text or the model's"""
    w0, w1 = int(pm.line_word_offsets[k]), int(pm.line_word_offsets[k + 1])
    g0 = int(pm.word_offsets[w0])
    parts = []
    for w in range(w0, w1):
        a, b, e = int(pm.word_offsets[w]) - g0, int(pm.word_offsets[w + 1]) - g0, int(pm.entries[w])
        parts.append(words[e] if e >= 0 else best[w] if best is not None and flags[w] == 0 else raw[a:b])
    return " ".join(parts)


def test_read_words_with_phrases(det, rec):
    from ocr_rs_amd import capi, reading
    fr, polys, adj = J.two_groups()
    before = reading.read_words(det, rec, fr, polys, adj)
    t0 = before[0][0][0]
    assert len(t0) == 6
    words = [t0[:3], t0[3:], t0[:2], "Zq9"]
    glyphs, crops = reading.glyph_crops(det, fr, polys, adj)
    costs = rec.glyph_costs(rec.forward_host(crops))
    sub, breaks = det.break_words(glyphs)
    with capi.Lexicon(rec, words) as lex:
        assert _plain(reading.read_words(det, rec, fr, polys, adj, phrases=None)) == _plain(before)
        # without spaces=: zero gap costs
        got = reading.read_words(det, rec, fr, polys, adj, phrases={"lexicon": lex})
        text, pr, where, rows = got[0][0]
        pm = rec.phrase_match(lex, costs, glyphs.word_offsets)
        assert text == _compose(pm, 0, t0, words) and np.array_equal(pr, before[0][0][1]) and np.array_equal(where, before[0][0][2])
        assert _differs(rows, {k: getattr(pm.line(0), k) for k in KEYS}) is None
        assert _differs(rows, PO.phrase_match(costs, glyphs.word_offsets, words)) is None
        # with spaces=: the gap costs of the break call
        bound, join = capi.phrase_gap_costs(sub, breaks, 1.5, 0.5)
        pm2 = rec.phrase_match(lex, costs, glyphs.word_offsets, bound, join, dict(word_cost=0.5))
        got2 = reading.read_words(det, rec, fr, polys, adj, spaces={}, phrases=dict(lexicon=lex, params=dict(word_cost=0.5), break_penalty=1.5,
                                                                                     join_penalty=0.5))
        assert got2[0][0][0] == _compose(pm2, 0, t0, words) and _differs(got2[0][0][3], {k: getattr(pm2.line(0), k) for k in KEYS}) is None
        assert got2[0][0][0] == t0[:3] + " " + t0[3:] and [words[e] for e in got2[0][0][3].entries] == [t0[:3], t0[3:]]
        # rectified, and through read_lines
        rect0 = reading.read_words_rectified(det, rec, fr, polys, adj)
        assert _plain(reading.read_words_rectified(det, rec, fr, polys, adj, phrases=None)) == _plain(rect0)
        rect = reading.read_words_rectified(det, rec, fr, polys, adj, spaces={}, phrases={"lexicon": lex})
        rt, rp, rq, rrows = rect[0][0]
        assert rt == _compose(rrows, 0, rect0[0][0][0], words) and np.array_equal(rp, rect0[0][0][1]) and np.array_equal(rq, rect0[0][0][2])
        assert rrows.word_offsets[-1] == len(rect0[0][0][0]) and rrows.line_flags.tolist() == [0]
        for rectified in (False, True):
            lines = reading.read_lines(det, rec, fr, polys, adj, rectified=rectified, spaces={}, phrases={"lexicon": lex})
            assert len(lines[0]) == 1 and lines[0][0][0] == (rt if rectified else reading.read_words(
                det, rec, fr, polys, adj, spaces={}, phrases={"lexicon": lex})[0][0][0])
            assert _plain_lines(reading.read_lines(det, rec, fr, polys, adj, rectified=rectified, phrases=None)) == \
                _plain_lines(reading.read_lines(det, rec, fr, polys, adj, rectified=rectified))
        with pytest.raises(capi.OcrError, match="lattice"):
            reading.read_words(det, rec, fr, polys, adj, lattice={}, phrases={"lexicon": lex})
        with pytest.raises(capi.OcrError, match="lexicon="):
            reading.read_words(det, rec, fr, polys, adj, lexicon=lex, phrases={"lexicon": lex})
        with pytest.raises(capi.OcrError, match="lexicon="):
            reading.read_words_rectified(det, rec, fr, polys, adj, lexicon=lex, phrases={"lexicon": lex})
        with pytest.raises(TypeError):
            reading.read_words(det, rec, fr, polys, adj, phrases={"lexicon": lex, "top_k": 2})
        with pytest.raises(TypeError):
            reading.read_words(det, rec, fr, polys, adj, phrases={"lexicon": words})


def _plain_lines(pages):
    return [[(t, np.asarray(i).tolist(), np.asarray(g).tolist()) for t, i, g in pg] for pg in pages]


def test_forty_glyphs_with_phrases_and_a_language_model(det, rec):
    from ocr_rs_amd import capi, reading
    fr, polys, adj = J.forty_bars()
    seg = dict(max_glyphs=64)
    raw = reading.read_words(det, rec, fr, polys, adj, params=seg)[0][0][0]
    assert len(raw) == 40
    words = [raw[:20], "Zq9"]
    table = capi.char_lm_table(LX.random_words(np.random.default_rng(6), 400, 1, 9), weight=3.0)
    glyphs, crops = reading.glyph_crops(det, fr, polys, adj, seg)
    costs = rec.glyph_costs(rec.forward_host(crops))
    with capi.CharLm(rec, table) as lm, capi.Lexicon(rec, words) as lex:
        pm = rec.phrase_match(lex, costs, glyphs.word_offsets)
        assert _differs(pm, PO.phrase_match(costs, glyphs.word_offsets, words)) is None
        assert pm.entries[0] == 0 and pm.word_offsets[1] == 20 and pm.line_flags.tolist() == [0]
        got = reading.read_words(det, rec, fr, polys, adj, params=seg, phrases={"lexicon": lex})
        assert got[0][0][0] == _compose(pm, 0, raw, words) and got[0][0][0].startswith(raw[:20] + " ")
        paths = rec.lm_decode(lm, costs, pm.word_offsets)
        with_lm = reading.read_words(det, rec, fr, polys, adj, params=seg, phrases={"lexicon": lex}, lm=lm)
        assert with_lm[0][0][0] == _compose(pm, 0, raw, words, paths.texts(pm.word_offsets), paths.word_flags.tolist())
        assert _differs(with_lm[0][0][3], {k: getattr(pm.line(0), k) for k in KEYS}) is None


# ---- refused calls

def _invalid(fn, *needles):
    from ocr_rs_amd import capi
    with pytest.raises(capi.OcrError) as e:
        fn()
    assert e.value.code == INVALID, e.value
    for n in needles:
        assert n in str(e.value), e.value


def test_invalid_arguments(rec):
    import torch
    from ocr_rs_amd import capi
    L = capi.lib()
    words = ["in", "the", "box"]
    cost = PO.costs_for_phrase("intheboxQ", np.random.default_rng(8), noise=0.5)
    off = np.array([0, 8, 9], np.int32)
    z = np.zeros(9, np.float32)
    with capi.Lexicon(rec, words) as lex:
        good = lambda: rec.phrase_match(lex, cost, off).entries.tolist() == [0, 1, 2, -1]
        assert good()
        out = C.POINTER(capi.PhraseMatchesBlock)()
        raw = lambda *a: capi.check(L.ocr_lexicon_phrase_match(*a))
        ok = [rec._h, lex.handle, cost.ctypes.data, 9, capi.MEM_HOST, off.ctypes.data, 2, None, None, None, C.byref(out)]
        for k in (0, 1, 2, 5, 10):      # rec, lex, costs, line_offsets, out
            args = list(ok)
            args[k] = None
            _invalid(lambda: raw(*args), "null")
            assert good()
        for k in (7, 8):                # exactly one of bound_cost / join_cost
            args = list(ok)
            args[k] = z.ctypes.data
            _invalid(lambda: raw(*args), "together")
        assert good()
        args = list(ok)
        args[4] = 7
        _invalid(lambda: raw(*args), "mem_kind")
        _invalid(lambda: rec.phrase_match(lex, cost, [1, 8, 9]), "start")
        _invalid(lambda: rec.phrase_match(lex, cost, [0, 9, 8, 9]), "decrease")
        _invalid(lambda: rec.phrase_match(lex, cost, [0, 8]), "end")
        args = list(ok)
        args[6] = -1
        _invalid(lambda: raw(*args), "lines")
        assert good()
        for field in ("word_cost", "oov_word_cost", "oov_glyph_cost"):
            for v in (-1.0, np.nan, np.inf):
                _invalid(lambda: rec.phrase_match(lex, cost, off, params={field: v}), "params")
        for v in (-1, 2):
            _invalid(lambda: rec.phrase_match(lex, cost, off, params=dict(fold_case=v)), "params")
        for i in range(3):
            _invalid(lambda: rec.phrase_match(lex, cost, off, params=dict(reserved=[int(j == i) for j in range(3)])), "params")
        assert good()
        for v in (np.nan, np.inf, -np.inf, -1.0):
            for name in ("bound_cost", "join_cost"):
                a = z.copy()
                a[4] = v
                b, j = (a, z) if name == "bound_cost" else (z, a)
                _invalid(lambda: rec.phrase_match(lex, cost, off, b, j), name + "[4]")
            bad = cost.copy()
            bad[8, 61] = v                                    # the last class of the last row: line 1
            _invalid(lambda: rec.phrase_match(lex, bad, off), "line 1")
            t = torch.from_numpy(bad).to(f"cuda:{rec.device}")
            _invalid(lambda: rec.phrase_match_device(lex, t.data_ptr(), 9, off), "line 1")
            bad[0, 0] = v                                     # the first bad line is named
            _invalid(lambda: rec.phrase_match(lex, bad, off), "line 0")
            assert good()
        with pytest.raises(capi.OcrError):
            rec.phrase_match(lex, cost, off, z[:5], z[:5])    # gap costs of another glyph count: refused before the call
        assert good()
        if torch.cuda.device_count() > 1:
            from ocr_rs_amd import weights as W
            other = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 1)
            try:
                _invalid(lambda: other.phrase_match(lex, cost, off), "device")
            finally:
                other.close()
            assert good()


@pytest.mark.timeout(120)
def test_two_handles_from_two_threads_give_the_single_thread_bits():
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    lexs = [_mixed_words(81, 500, 1, 10), _mixed_words(82, 90, 2, 32)]
    cases = [_case(83, lexs[0], [3, 0, 40, 256, 7], gaps=True), _case(84, lexs[1], [65] * 9 + [1, 2], integer=True)]
    prms = [dict(), dict(fold_case=0, word_cost=0.0)]
    want = [PO.phrase_match(cases[t][0], cases[t][1], lexs[t], cases[t][2], cases[t][3], **prms[t]) for t in range(2)]
    errors = [[], []]
    start = threading.Barrier(2)

    def work(t):
        r = lex = None
        try:
            r = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
            lex = capi.Lexicon(r, lexs[t])
            start.wait(60)
            for rnd in range(6):
                diff = _differs(r.phrase_match(lex, *cases[t], prms[t]), want[t])
                if diff:
                    errors[t].append(f"thread {t}, round {rnd}: {diff}")
            try:     # a refused call on this thread raises on this thread
                r.phrase_match(lex, *cases[t], dict(word_cost=-1.0))
                errors[t].append(f"thread {t}: word_cost -1 was not refused")
            except capi.OcrError as e:
                if e.code != INVALID:
                    errors[t].append(f"thread {t}: {e!r}")
        except Exception as e:   # noqa: BLE001
            start.abort()
            errors[t].append(f"thread {t}: {e!r}")
        finally:
            if lex is not None:
                lex.close()
            if r is not None:
                r.close()

    threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(100)
        assert not th.is_alive(), "a thread did not return"     # (nothing more is started after a failed join)
    assert errors == [[], []], errors
