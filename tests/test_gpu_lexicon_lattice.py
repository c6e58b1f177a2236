"""The joint lexicon and lattice search on the MI355X (ocr_lexicon_lattice_match; csrc/lexicon_lattice.hip) against
tests/lexicon_lattice_oracle.py: entries, candidates, flags, segment lengths, entry positions and inserted counts equal, every cost
bit-equal (compared as uint64), for words of 0..33 pieces at max_span 1, 2, 4 and top_k 1, 2, 8, word counts 1..9 and 257, lexicon
sizes either side of a chunk, ties, extreme span costs, max_span 1 against ocr_lexicon_match from the device, both memory kinds and
every OCR_ERR_INVALID case; read_words composed with lattice_lexicon against the calls made by hand."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import lattice_oracle as LO
from tests import lexicon_lattice_oracle as O
from tests import lexicon_oracle as LX

pytestmark = pytest.mark.gpu

INVALID = 1      # OCR_ERR_INVALID (include/ocr_amd.h)


@pytest.fixture(scope="module")
def rec():
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    r = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    yield r
    r.close()


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want):
    for name in O.ARRAYS:
        assert getattr(got, name).shape == want[name].shape, name
        assert np.array_equal(getattr(got, name), want[name]), name
    for name in O.F64_ARRAYS:
        assert np.array_equal(_u64(getattr(got, name)), _u64(want[name])), name


def _check(rec, cost, so, po, words, lex=None, **prm):
    from ocr_rs_amd import capi
    want = O.match(cost, so, po, words, **prm)
    if lex is not None:
        got = rec.lexicon_lattice_match(lex, cost, so, po, prm)
    else:
        with capi.Lexicon(rec, words) as lx:
            got = rec.lexicon_lattice_match(lx, cost, so, po, prm)
    _same(got, want)
    return got, want


def test_constants_match_the_kernel():
    from ocr_rs_amd import capi
    assert capi.LEX_CHUNK == 256 and capi.LATTICE_MAX_PIECES == O.MAX_PIECES == 32 and capi.LATTICE_MAX_SPAN == O.MAX_SPAN == 4
    assert capi.LEX_MAX_LEN == O.MAX_LEN == 32


# 4, 5 and 8, 31, 32 are either side of the groups of 4 rows behind one branch; 0 and 33 are the two flags that need no lexicon
GS = [0, 1, 2, 3, 4, 5, 8, 31, 32, 33]


@functools.lru_cache(maxsize=None)
def _shapes(M):
    rng = np.random.default_rng(140 + M)
    words = LX.random_words(rng, 300, 1, 32)
    po = O.offsets(GS)
    so = O.span_offsets(po, M)
    return LX.make_costs(rng, int(so[-1])), so, po, words


# a call whose span costs are all zero takes the instantiation without their adds: both kinds at every max_span and best-k
@pytest.mark.parametrize("sc", [[0.5, 0.25, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0]], ids=["span_costs", "zero_span_costs"])
@pytest.mark.parametrize("top_k", [1, 2, 8])
@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_word_shapes(rec, M, top_k, sc):
    cost, so, po, words = _shapes(M)
    got, want = _check(rec, cost, so, po, words, max_span=M, top_k=top_k, span_cost=sc, max_len_diff=3)
    assert want["word_flags"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0, 2]
    assert np.all(np.isinf(got.costs[[0, 9]])) and np.all(np.isfinite(got.costs[1:9])) and np.all(got.entries[1:9] >= 0)
    assert got.raw_costs[0] == 0.0 and got.raw_costs[9] > 0 and not got.seg_len[:, po[9]:].any()
    if M > 1:
        assert got.seg_len.max() > 1   # some alignment does merge pieces


@pytest.mark.parametrize("integer", [False, True], ids=["floats", "whole"])
def test_against_every_alignment_path(rec, integer):
    """G = 1..4 at M = 1..3 against the enumeration of every alignment path of every entry (L <= 3): the device's costs are the path
    minima, bit for bit."""
    for M in (1, 2, 3):
        rng = np.random.default_rng(150 + M + 10 * integer)
        words = LX.random_words(rng, 8, 1, 3)
        po = O.offsets([1, 2, 3, 4])
        so = O.span_offsets(po, M)
        cost = LX.make_costs(rng, int(so[-1]), integer=integer)
        prm = dict(max_span=M, top_k=8, max_len_diff=8, ins_cost=2.0 if integer else 1.75, del_cost=1.0 if integer else 2.25,
                   span_cost=[0.0, 1.0, 2.0] if integer else [0.25, 0.0, 1.5], fold_case=M % 2)
        got, _ = _check(rec, cost, so, po, words, **prm)
        sub = O._fold(cost, prm["fold_case"])
        for w in range(4):
            rows = sub[so[w]:so[w + 1]]
            all_cost = sorted((O.brute_force(rows, LX.classes(wd), w + 1, M, prm["ins_cost"], prm["del_cost"], prm["span_cost"] + [0.0]), k)
                              for k, wd in enumerate(words))
            assert np.array_equal(_u64(got.costs[w]), _u64([c for c, _ in all_cost])) and got.entries[w].tolist() == [k for _, k in all_cost]


@pytest.mark.parametrize("n_words", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_word_counts(rec, n_words):
    rng = np.random.default_rng(160 + n_words)
    cost, so, po, words = O.fuzz(160 + n_words, 120, rng.integers(0, 9, n_words).tolist(), 3, 1, 10, integer=bool(n_words % 2))
    _check(rec, cost, so, po, words, max_span=3, top_k=8, span_cost=[0.0, 1.0, 0.0])


@pytest.mark.parametrize("M,top_k", [(1, 8), (2, 1), (4, 8)])
def test_257_words(rec, M, top_k):
    rng = np.random.default_rng(170 + M)
    cost, so, po, words = O.fuzz(170 + M, 150, rng.integers(0, 8, 257).tolist(), M, 1, 9, integer=(M == 2))
    _check(rec, cost, so, po, words, max_span=M, top_k=top_k)


# one admissible length: every entry is a candidate of the word, so the sizes are the chunk's 256 and one either side of it
@pytest.mark.parametrize("n_entries", [1, 255, 256, 257])
def test_lexicon_sizes_around_a_chunk(rec, n_entries):
    rng = np.random.default_rng(180 + n_entries)
    words = LX.random_words(rng, n_entries, 4, 4)
    po = O.offsets([4, 6])
    so = O.span_offsets(po, 2)
    cost = LX.make_costs(rng, int(so[-1]), integer=True)
    got, want = _check(rec, cost, so, po, words, max_span=2, top_k=8, max_len_diff=1)
    assert want["n_candidates"].tolist() == [n_entries, n_entries]


def test_three_chunks_with_a_ragged_last_one(rec):
    rng = np.random.default_rng(190)
    words = LX.random_words(rng, 700, 3, 6)               # 700 candidates of one word: chunks of 256, 256 and 188
    po = O.offsets([4, 5, 9])
    so = O.span_offsets(po, 2)
    for integer in (False, True):
        cost = LX.make_costs(rng, int(so[-1]), integer=integer)
        got, want = _check(rec, cost, so, po, words, max_span=2, top_k=8)
        assert want["n_candidates"][:2].tolist() == [700, 700]


def test_no_admissible_length_and_top_k_past_the_candidates(rec):
    po = O.offsets([8, 2, 8])
    so = O.span_offsets(po, 4)
    cost = LX.make_costs(np.random.default_rng(191), int(so[-1]))
    got, want = _check(rec, cost, so, po, ["a", "ab", "abc"], max_span=4, top_k=8, max_len_diff=0)   # G = 8 admits 2..8, G = 2 admits 1..2
    assert want["word_flags"].tolist() == [0, 0, 0] and want["n_candidates"].tolist() == [2, 2, 2]
    assert np.all(got.entries[:, 2:] == -1) and np.all(np.isinf(got.costs[:, 2:])) and not got.seg_len[2:].any()
    got, want = _check(rec, cost, so, po, ["a"], max_span=4, top_k=2, max_len_diff=0)               # the lexicon gives the words of 8 nothing
    assert want["word_flags"].tolist() == [4, 0, 4] and np.all(got.raw_costs > 0)
    got, want = _check(rec, cost, so, po, ["a" * 20], max_span=4, top_k=2, max_len_diff=0)          # ... and here nobody anything: no launch
    assert want["word_flags"].tolist() == [4, 4, 4] and np.all(got.entries == -1) and np.all(got.raw_costs > 0)


def test_duplicates(rec):
    cost, so, po, _, _ = O.hand_cases()["rn_span"]
    got, _ = _check(rec, cost, so, po, ["com", "corn", "com", "com"], max_span=2, top_k=4)
    assert got.entries.tolist() == [[0, 2, 3, 1]] and got.costs.tolist() == [[0.5, 0.5, 0.5, 2.0]]
    assert np.array_equal(got.seg_len[0], got.seg_len[1]) and np.array_equal(got.seg_len[0], got.seg_len[2])


def test_rank_ties_and_trace_ties_go_by_the_written_order(rec):
    fz, prm = O.TIE_CASE
    cost, so, po, words = O.fuzz(**fz)
    got, want = _check(rec, cost, so, po, words, **prm)
    assert want["ties"] >= 20 and want["trace_ties"] >= 1
    cost, so, po, words, prm = O.hand_cases()["trace_tie"]
    got, want = _check(rec, cost, so, po, words, **prm)
    assert want["trace_ties"] == 1 and got.seg_len.tolist() == [[-1, 1]] and got.seg_char.tolist() == [[-1, 0]] and got.costs.tolist() == [[4.0]]


@pytest.mark.parametrize("top_k", [1, 8])
def test_equal_costs_in_every_wave_of_three_chunks_go_to_the_smaller_index(rec, top_k):
    """One word of 3 pieces whose span rows are constant against 600 distinct entries of 3 characters (behind four of other lengths):
    every one of them costs the same, in all four waves of three chunks, so the wave's butterfly, the read-back of the waves' slots
    and the merge over the chunks all see equal costs and the index alone decides."""
    words = ["a", "defg", "hijkl", "mnop"] + ["".join(LX.ALPHABET[37 * n // d % 62] for d in (3844, 62, 1)) for n in range(600)]
    assert len(set(words)) == 604   # (none of 2 characters: it would read two of the pieces as one and be cheaper)
    po = O.offsets([3])
    so = O.span_offsets(po, 2)
    got, want = _check(rec, np.full((int(so[-1]), 62), 1.5, np.float32), so, po, words, max_span=2, top_k=top_k)
    assert want["n_candidates"].tolist() == [604] and got.entries.tolist() == [list(range(4, 4 + top_k))] and np.all(got.costs == 4.5)
    assert np.all(got.seg_len == 1) and got.seg_char.tolist() == [[0, 1, 2]] * top_k


def test_hand_cases(rec):
    res = {}
    for name, (cost, so, po, words, prm) in O.hand_cases().items():
        res[name], _ = _check(rec, cost, so, po, words, **prm)
    r = res["rn_span"]
    assert r.entries.tolist() == [[1, 0]] and r.costs.tolist() == [[0.5, 2.0]] and r.raw_costs.tolist() == [0.5]
    assert r.seg_len.tolist() == [[1, 1, 2, 0], [1, 1, 1, 1]] and r.seg_char.tolist() == [[0, 1, 2, -1], [0, 1, 2, 3]]
    assert r.segments([0, 4], 0, 0) == [(0, 1, 0), (1, 1, 1), (2, 2, 2)]
    r = res["rn_span_cost"]
    assert r.entries.tolist() == [[0, 1]] and r.costs.tolist() == [[2.0, 3.5]] and r.raw_costs.tolist() == [2.0]
    r = res["rn_m1"]
    assert r.costs.tolist() == [[2.0, 10.0]] and r.seg_len[1].tolist() == [1, 1, -1, 1] and r.seg_char[1].tolist() == [0, 1, -1, 2]
    r = res["m_cut_m1"]
    assert r.costs.tolist() == [[0.0, 10.0]] and r.seg_char[1].tolist() == [0, 1, 3] and r.n_ins.tolist() == [[0, 1]]
    r = res["inserted"]
    assert r.costs.tolist() == [[4.0]] and r.seg_len.tolist() == [[1, 1]] and r.seg_char.tolist() == [[0, 2]] and r.n_ins.tolist() == [[1]]
    assert res["fold_on"].costs.tolist() == [[0.0, 6.0]] and res["fold_off"].costs.tolist() == [[6.0, 6.0]]
    assert res["fold_off"].entries.tolist() == [[0, 1]]


def test_span_costs_zero_huge_and_subnormal(rec):
    from ocr_rs_amd import capi
    cost, so, po, words = O.fuzz(195, 200, [1, 2, 4, 6], 4, 1, 8)
    tiny = float(np.nextafter(0.0, 1.0))
    with capi.Lexicon(rec, words) as lex:
        for sc in ([0.0, 0.0, 0.0, 0.0], [1e30, 0.0, 0.0, 0.0], [0.0, 1e30, 1e30, 1e30], [tiny, 0.0, tiny, 0.0], [tiny, 1e30, 0.0, tiny]):
            got, _ = _check(rec, cost, so, po, words, lex, max_span=4, top_k=8, span_cost=sc)
        got, _ = _check(rec, cost, so, po, words, lex, max_span=4, top_k=1, span_cost=[0.0, 1e30, 1e30, 1e30])
        assert got.seg_len.max() == 1                                       # merging costs 1e30: the cut stays
    zero = np.zeros((3, 62), np.float32)
    got, _ = _check(rec, zero, [0, 3], [0, 2], ["a", "ab"], max_span=2, top_k=2, span_cost=[tiny, 0.0])
    assert got.costs.tolist() == [[0.0, 2 * tiny]] and got.seg_len.tolist() == [[2, 0], [1, 1]]   # the merge is free, the cuts are not


@pytest.mark.parametrize("top_k", [1, 2, 8])
def test_max_span_1_is_lexicon_match_from_the_device(rec, top_k):
    from ocr_rs_amd import capi
    rng = np.random.default_rng(196)
    off = O.offsets([0, 1, 2, 3, 9, 31, 32, 33] + rng.integers(0, 12, 40).tolist())
    words = LX.random_words(rng, 900, 1, 32)
    for integer in (False, True):
        cost = LX.make_costs(rng, int(off[-1]), integer=integer)
        with capi.Lexicon(rec, words) as lex:
            a = rec.lexicon_match(lex, cost, off, dict(top_k=top_k, ins_cost=3.5, del_cost=2.25, fold_case=int(integer)))
            b = rec.lexicon_lattice_match(lex, cost, off, off, dict(max_span=1, top_k=top_k, ins_cost=3.5, del_cost=2.25, fold_case=int(integer)))
        assert np.array_equal(a.entries, b.entries) and np.array_equal(_u64(a.costs), _u64(b.costs))
        assert np.array_equal(_u64(a.raw_costs), _u64(b.raw_costs))
        assert np.array_equal(a.n_candidates, b.n_candidates) and np.array_equal(a.word_flags, b.word_flags)
        assert set(a.word_flags.tolist()) >= {0, 1, 2} and np.all(np.isin(b.seg_len, (-1, 0, 1)))


def test_no_words(rec):
    from ocr_rs_amd import capi
    with capi.Lexicon(rec, ["a"]) as lex:
        got = rec.lexicon_lattice_match(lex, np.zeros((0, 62), np.float32), [0], [0])
        assert got.n_words == 0 and got.seg_len.shape == (1, 0)
        got = rec.lexicon_lattice_match(lex, np.zeros((0, 62), np.float32), [0, 0, 0], [0, 0, 0], dict(top_k=3))
        assert got.word_flags.tolist() == [1, 1] and np.all(np.isinf(got.costs)) and got.costs.shape == (2, 3)


def test_memory_kinds(rec):
    import torch
    from ocr_rs_amd import capi
    cost, so, po, words = _shapes(2)
    prm = dict(max_span=2, top_k=8)
    want = O.match(cost, so, po, words, **prm)
    d = torch.from_numpy(cost).cuda()
    torch.cuda.synchronize()
    with capi.Lexicon(rec, words) as lex:
        _same(rec.lexicon_lattice_match_device(lex, d.data_ptr(), cost.shape[0], so, po, prm), want)
        _same(rec.lexicon_lattice_match(lex, cost, so, po, prm), want)      # the same handle and workspace, host memory
        _same(rec.lexicon_lattice_match_device(lex, d.data_ptr(), cost.shape[0], so, po, capi.lexlat_params(**prm)), want)


# ---- errors: bad arguments only, and the handle is used again after each

def _invalid(fn, *needles):
    from ocr_rs_amd import capi
    with pytest.raises(capi.OcrError) as e:
        fn()
    assert e.value.code == INVALID, e.value
    for n in needles:
        assert n in str(e.value), e.value


def test_invalid_calls(rec):
    from ocr_rs_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(199)
    po = np.array([0, 5, 8], np.int32)
    so = LO.span_offsets(po, 2)                      # [0, 9, 14]
    cost = LX.make_costs(rng, int(so[-1]))
    words = LX.random_words(rng, 40, 2, 9)
    prm = dict(max_span=2, top_k=2)
    want = O.match(cost, so, po, words, **prm)
    with capi.Lexicon(rec, words) as lex:
        match = lambda c=cost, s=so, p=po, q=prm: rec.lexicon_lattice_match(lex, c, s, p, q)
        good = lambda: _same(match(), want)
        good()
        out = C.POINTER(capi.LexLatMatchesBlock)()
        p = capi.lexlat_params(**prm)
        raw = lambda *a: capi.check(L.ocr_lexicon_lattice_match(*a))
        ok = (rec._h, lex.handle, cost.ctypes.data, 14, capi.MEM_HOST, so.ctypes.data, po.ctypes.data, 2, C.byref(p), C.byref(out))
        for k in (0, 1, 2, 5, 6, 9):      # rec, lex, costs, span_offsets, piece_offsets, out
            args = list(ok)
            args[k] = None
            _invalid(lambda: raw(*args), "null")
            good()
        args = list(ok)                   # params == NULL means the defaults, which are these spans' max_span
        args[8] = None
        raw(*args)
        assert out.contents.top_k == 1 and out.contents.n_words == 2
        L.ocr_lexlat_matches_free(out)
        _invalid(lambda: raw(*ok[:4], 5, *ok[5:]), "mem_kind")
        _invalid(lambda: match(s=[1, 9, 14]), "start at 1")
        _invalid(lambda: match(p=[1, 5, 8]), "start at")
        _invalid(lambda: match(p=[0, 5, 4]), "decrease at word 1")
        _invalid(lambda: match(s=[0, 9, 13]), "word 1", "holds 4 spans")      # a wrong span count
        _invalid(lambda: match(s=[0, 8, 14]), "word 0", "holds 8 spans")
        _invalid(lambda: match(q=dict(max_span=3, top_k=2)), "holds 9 spans", "gives 12")   # counted for M = 2
        _invalid(lambda: match(c=cost[:13]), "end at 14")
        _invalid(lambda: match(c=np.concatenate([cost, cost[:1]])), "end at 14")
        good()
        for bad in (dict(top_k=0), dict(top_k=9), dict(max_span=0), dict(max_span=5), dict(max_span=-1), dict(reserved=(1, 0)),
                    dict(reserved=(0, 5)), dict(max_len_diff=-1), dict(max_len_diff=9), dict(fold_case=2), dict(fold_case=-1),
                    dict(ins_cost=-1.0), dict(ins_cost=np.nan), dict(ins_cost=np.inf), dict(del_cost=-1e-300), dict(del_cost=np.nan),
                    dict(del_cost=-np.inf)):
            _invalid(lambda: match(q=dict(prm, **bad)), "params")
        for bad in (np.nan, np.inf, -np.inf, -1.0, -1e-300):
            for slot in range(4):
                sc = [0.0] * 4
                sc[slot] = bad
                _invalid(lambda: match(q=dict(prm, span_cost=sc)), f"span_cost[{slot}]")
        good()
        for bad in (np.nan, np.inf, -np.inf, -1.0):
            c = cost.copy()
            c[12, 61] = bad
            _invalid(lambda: match(c=c, q=dict(max_span=2, top_k=8)), "word 1")
            c[2, 0] = bad                              # a merged span's row (e = 2, m = 2) of word 0
            _invalid(lambda: match(c=c, q=dict(max_span=2)), "word 0")
            good()
        po3 = np.array([0, 5, 8, 41], np.int32)          # ... also in a word that is too long to be matched
        so3 = LO.span_offsets(po3, 2)
        c = np.concatenate([cost, LX.make_costs(rng, int(so3[-1] - so3[2]))])
        c[40, 3] = np.nan
        _invalid(lambda: match(c=c, s=so3, p=po3), "word 2")
        good()
        with pytest.raises(ValueError):
            match(p=[0, 8])
        if L.ocr_device_count() > 1:
            from ocr_rs_amd import weights as W
            other = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 1)
            try:
                _invalid(lambda: other.lexicon_lattice_match(lex, cost, so, po, prm), "device")
            finally:
                other.close()
            good()
    L.ocr_lexlat_matches_free(None)
    L.ocr_lexlat_default_params(None)
    with pytest.raises(TypeError):
        capi.lexlat_params(beam=3)


# ---- read_words composed

def _plain(pages):
    return [[(wd[0], wd[1].tolist(), np.asarray(wd[2]).tolist(), *wd[3:]) for wd in pg] for pg in pages]


def test_read_words_with_a_lattice_lexicon(rec):
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    from tests.test_gpu_glyphs import _synthetic_pages
    det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    try:
        frames, polys = _synthetic_pages(2, 320, 320, 25, seed=33)
        adj = np.ones((2, 2))
        split = dict(aspect_pct=60, max_pieces=3)
        lat = dict(max_span=3, top_k=2, span_cost=[0.5, 0.0, 0.0])
        mprm = dict(top_k=2, max_len_diff=3, ins_cost=3.0)
        before = reading.read_words(det, rec, frames, polys, adj, lattice=lat, split=split)
        # the calls by hand
        glyphs = det.segment_glyphs(frames, polys, adj)
        pieces, _ = det.split_glyphs(frames, glyphs, split)
        spans, tab = capi.glyph_spans(pieces, 3)
        crops = det.extract_glyph_crops(frames, spans)
        costs = rec.glyph_costs(rec.forward_host(crops))
        _, probs = rec.classify_host(crops)
        po, so = tab.piece_offsets, tab.span_offsets
        # a word list drawn from what the lattice reads, so that some words are accepted, and entries that nothing resembles
        texts = [wd[0] for pg in before for wd in pg if wd[0]]
        words = sorted(set(texts[::2])) + ["zzzzzzzzzzzzzzzzzzzzzzzz", "Q"]
        with capi.Lexicon(rec, words) as lex:
            assert _plain(reading.read_words(det, rec, frames, polys, adj, lattice=lat, split=split, lattice_lexicon=None)) == _plain(before)
            got = reading.read_words(det, rec, frames, polys, adj, lattice=lat, split=split, lattice_lexicon=lex,
                                     lattice_lexicon_params=mprm, max_penalty=1.0)
            m = rec.lexicon_lattice_match(lex, costs, so, po, dict(mprm, max_span=3, span_cost=lat["span_cost"]))
            with pytest.raises(capi.OcrError):
                reading.read_words(det, rec, frames, polys, adj, lattice_lexicon=lex)           # the joint search needs lattice=
            with pytest.raises(capi.OcrError):
                reading.read_words(det, rec, frames, polys, adj, lexicon=lex, lattice={})       # lexicon= stays the fixed segmentation's
            with pytest.raises(TypeError):
                reading.read_words(det, rec, frames, polys, adj, lattice={}, lattice_lexicon=words)
        _same(m, O.match(costs, so, po, words, max_span=3, span_cost=lat["span_cost"], **mprm))
        k = taken = 0
        for pg, pg0 in zip(got, before):
            assert len(pg) == len(pg0)
            for wd, wd0 in zip(pg, pg0):
                text, pr, where, lat_el, (entry, cost, raw, seg_len) = wd
                G = int(po[k + 1] - po[k])
                assert lat_el == wd0[3] and len(wd0) == 4
                assert (entry, cost, raw) == (int(m.entries[k, 0]), float(m.costs[k, 0]), float(m.raw_costs[k]))
                assert seg_len == tuple(m.seg_len[0, po[k]:po[k + 1]].tolist())
                if entry >= 0 and cost - raw <= 1.0 * G:
                    rows = [int(so[k]) + LO.row_of(q - int(po[k]) + n, n, 3) for q, n, _ in m.segments(po, k)]
                    assert text == words[entry]
                    assert np.array_equal(where, spans.boxes[rows].reshape(-1, 4)) and np.array_equal(pr, probs[rows])
                    assert len(rows) + int(m.n_ins[k, 0]) == len(text)
                    taken += 1
                else:
                    assert text == wd0[0] and np.array_equal(pr, wd0[1]) and np.array_equal(where, wd0[2])
                k += 1
        assert k == m.n_words and 0 < taken < k
        print(f"\nread_words with a lattice lexicon: {k} words, {pieces.n_glyphs} pieces, {spans.n_glyphs} spans, {len(words)} entries, "
              f"{taken} words took an entry")
    finally:
        det.close()
