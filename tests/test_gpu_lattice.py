"""The segmentation lattice's decode on the MI355X (ocr_lattice_decode; csrc/lattice.hip) against tests/lattice_oracle.py: labels,
segment lengths, counts and flags equal, every cost bit-equal (compared as uint64), for words of 0..33 pieces at max_span 1, 2, 4 and
top_k 1, 2, 8, batches either side of the words of a workgroup, ties, extreme span costs, max_span 1 against ocr_lm_decode from the
device, both memory kinds and every OCR_ERR_INVALID case; read_words composed with a lattice against the calls made by hand."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import char_lm_oracle as CL
from tests import lattice_oracle as LO

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
    assert got.labels.shape == want["labels"].shape and got.costs.shape == want["costs"].shape
    assert np.array_equal(got.word_flags, want["word_flags"])
    assert np.array_equal(_u64(got.raw_costs), _u64(want["raw_costs"]))
    assert np.array_equal(_u64(got.costs), _u64(want["costs"]))
    assert np.array_equal(got.labels, want["labels"]) and np.array_equal(got.seg_len, want["seg_len"])
    assert np.array_equal(got.n_chars, want["n_chars"])


def _check(rec, cost, so, po, T, M, top_k, sc=None, lm=None):
    from ocr_rs_amd import capi
    want = LO.decode(cost, so, po, T, M, top_k, sc)
    prm = dict(max_span=M, top_k=top_k, span_cost=list(sc) if sc is not None else [])
    if lm is not None:
        got = rec.lattice_decode(lm, cost, so, po, prm)
    else:
        with capi.CharLm(rec, T) as m:
            got = rec.lattice_decode(m, cost, so, po, prm)
    _same(got, want)
    return got, want


def test_constants_match_the_kernel():
    from ocr_rs_amd import capi
    assert capi.LATTICE_WORDS == 4 and capi.LATTICE_MAX_PIECES == LO.MAX_PIECES == 32 and capi.LATTICE_MAX_SPAN == LO.MAX_SPAN == 4


GS = [0, 1, 2, 3, 4, 5, 31, 32, 33]


@functools.lru_cache(maxsize=None)
def _shapes(M):
    return LO.make_case(np.random.default_rng(40 + M), GS, M)


@pytest.mark.parametrize("top_k", [1, 2, 8])
@pytest.mark.parametrize("M", [1, 2, 4])
def test_word_shapes(rec, M, top_k):
    cost, so, po, T = _shapes(M)
    got, want = _check(rec, cost, so, po, T, M, top_k, [0.5, 0.25, 0.0, 1.0])
    assert want["word_flags"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 2]
    assert np.all(np.isinf(got.costs[[0, 8]])) and np.all(np.isfinite(got.costs[1:8])) and np.all(got.labels[:, po[8]:] == -1)
    assert np.all(got.costs[1:8, 0] <= got.raw_costs[1:8]) and got.raw_costs[0] == 0.0 and got.raw_costs[8] > 0
    if M > 1:
        assert got.seg_len.max() > 1   # some hypothesis does merge pieces


@pytest.mark.parametrize("integer", [False, True], ids=["floats", "whole"])
def test_against_every_pair(rec, integer):
    """G = 1, 2, 3 at M = 1..3 against the enumeration of every (segmentation, classes) pair: the 8 smallest costs, bit for bit, from
    the device's output; every reported pair's own cost is its reported cost, and the pairs are distinct."""
    for M in (1, 2, 3):
        rng = np.random.default_rng(50 + M + 10 * integer)
        cost, so, po, T = LO.make_case(rng, [1, 2, 3], M, integer=integer)
        sc = [0.0, 1.0, 2.0] if integer else [0.25, 0.0, 1.5]
        got, _ = _check(rec, cost, so, po, T, M, 8, sc)
        res = dict(labels=got.labels, seg_len=got.seg_len)
        for w in range(3):
            rows = cost[so[w]:so[w + 1]]
            all_cost, _ = LO.enumerate_paths(rows, T, w + 1, M, sc)
            assert np.array_equal(_u64(got.costs[w]), _u64(np.sort(all_cost)[:8]))
            pairs = [LO.hypothesis(res, po, w, k) for k in range(8)]
            assert len(set(pairs)) == 8
            for k, (seg, cls) in enumerate(pairs):
                assert _u64(LO.path_cost(rows, T, M, seg, cls, sc)) == _u64(got.costs[w, k])


# capi.LATTICE_WORDS words share a workgroup: 3, 4, 5 are one either side of it, 7..9 of two workgroups
@pytest.mark.parametrize("n_words", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_word_counts_around_a_workgroup(rec, n_words):
    rng = np.random.default_rng(60 + n_words)
    cost, so, po, T = LO.make_case(rng, rng.integers(0, 7, n_words).tolist(), 3, integer=bool(n_words % 2))
    _check(rec, cost, so, po, T, 3, 8, [0.0, 1.0, 0.0])


@pytest.mark.parametrize("M,top_k", [(1, 8), (2, 1), (4, 8)])
def test_257_words(rec, M, top_k):
    rng = np.random.default_rng(70 + M)
    cost, so, po, T = LO.make_case(rng, rng.integers(0, 7, 257).tolist(), M, integer=(M == 2))
    _check(rec, cost, so, po, T, M, top_k)


def test_a_word_does_not_see_its_neighbours(rec):
    from ocr_rs_amd import capi
    rng = np.random.default_rng(81)
    gs = [3, 5, 0, 7, 2, 6]
    cost, so, po, T = LO.make_case(rng, gs, 4)
    with capi.CharLm(rec, T) as lm:
        batch, _ = _check(rec, cost, so, po, T, 4, 8, None, lm)
        for w, g in enumerate(gs):
            alone, _ = _check(rec, cost[so[w]:so[w + 1]], LO.span_offsets([0, g], 4), [0, g], T, 4, 8, None, lm)
            assert np.array_equal(_u64(alone.costs[0]), _u64(batch.costs[w]))
            assert np.array_equal(alone.labels, batch.labels[:, po[w]:po[w + 1]])
            assert np.array_equal(alone.seg_len, batch.seg_len[:, po[w]:po[w + 1]])


def test_no_words(rec):
    from ocr_rs_amd import capi
    with capi.CharLm(rec, CL.zero_model()) as lm:
        got = rec.lattice_decode(lm, np.zeros((0, 62), np.float32), [0], [0])
        assert got.n_words == 0 and got.labels.shape == (1, 0)
        got = rec.lattice_decode(lm, np.zeros((0, 62), np.float32), [0, 0, 0], [0, 0, 0], dict(top_k=3))
        assert got.word_flags.tolist() == [1, 1] and np.all(np.isinf(got.costs)) and got.costs.shape == (2, 3)


def test_ties_go_by_the_written_order(rec):
    cost, so, po, T, M = LO.tie_case()
    got, want = _check(rec, cost, so, po, T, M, 8)
    assert want["ties"] >= 20
    cost, so, po, T, M = LO.hand_tie_case()
    got, _ = _check(rec, cost, so, po, T, M, 8)
    assert got.costs[0].tolist() == [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    assert got.segments(po, 0, 0) == [(0, 1, 0), (1, 1, 0)] and got.segments(po, 0, 1) == [(0, 2, 0)] and got.segments(po, 0, 2) == [(0, 2, 1)]
    assert got.text(po, 0, 0) == "AA" and got.text(po, 0, 1) == "A" and got.text(po, 0, 2) == "B" and got.text(po, 0, 3) == "BA"


def test_span_costs_zero_huge_and_subnormal(rec):
    rng = np.random.default_rng(90)
    cost, so, po, T = LO.make_case(rng, [1, 2, 4, 6], 4)
    tiny = float(np.nextafter(0.0, 1.0))
    for sc in ([0.0, 0.0, 0.0, 0.0], [1e30, 0.0, 0.0, 0.0], [0.0, 1e30, 1e30, 1e30], [tiny, 0.0, tiny, 0.0], [tiny, 1e30, 0.0, tiny]):
        got, _ = _check(rec, cost, so, po, T, 4, 8, sc)
    assert np.all(got.costs[:, 0] <= got.raw_costs)
    got, _ = _check(rec, cost, so, po, T, 4, 1, [0.0, 1e30, 1e30, 1e30])
    assert np.all(got.seg_len[0] == 1)                                   # merging costs 1e30: the cut stays
    got, _ = _check(rec, np.zeros_like(cost), so, po, CL.zero_model(), 4, 2, [tiny, 0.0, 0.0, 0.0])
    assert got.costs[0].tolist() == [tiny, tiny] and got.costs[1].tolist() == [0.0, 0.0]   # two pieces: the merge is free, the cut is not
    assert got.seg_len[:, po[1]].tolist() == [2, 2] and got.labels[:, po[1]].tolist() == [0, 1]


@pytest.mark.parametrize("top_k", [1, 2, 8])
def test_max_span_1_is_lm_decode_from_the_device(rec, top_k):
    from ocr_rs_amd import capi
    rng = np.random.default_rng(95)
    off = CL.offsets([0, 1, 2, 3, 9, 31, 32, 33] + rng.integers(0, 12, 40).tolist())
    cost, T = CL.make_costs(rng, int(off[-1])), CL.make_model(rng)
    with capi.CharLm(rec, T) as lm:
        a = rec.lm_decode(lm, cost, off, dict(top_k=top_k))
        b = rec.lattice_decode(lm, cost, off, off, dict(max_span=1, top_k=top_k))
    assert np.array_equal(_u64(a.costs), _u64(b.costs)) and np.array_equal(_u64(a.raw_costs), _u64(b.raw_costs))
    assert np.array_equal(a.labels, b.labels) and np.array_equal(a.word_flags, b.word_flags)
    decoded = np.repeat(a.word_flags == 0, np.diff(off))
    assert np.all(b.seg_len[:, decoded] == 1) and np.all(b.seg_len[:, ~decoded] == 0)


def test_memory_kinds(rec):
    import torch
    from ocr_rs_amd import capi
    cost, so, po, T = _shapes(2)
    want = LO.decode(cost, so, po, T, 2, 8)
    d = torch.from_numpy(cost).cuda()
    torch.cuda.synchronize()
    with capi.CharLm(rec, T) as lm:
        _same(rec.lattice_decode_device(lm, d.data_ptr(), cost.shape[0], so, po, dict(max_span=2, top_k=8)), want)
        _same(rec.lattice_decode(lm, cost, so, po, dict(max_span=2, top_k=8)), want)      # the same handle and workspace, host memory
        _same(rec.lattice_decode_device(lm, d.data_ptr(), cost.shape[0], so, po, capi.lattice_params(max_span=2, top_k=8)), want)


# ---- errors: bad arguments only, and the handle is used again after each

def _invalid(fn, *needles):
    from ocr_rs_amd import capi
    with pytest.raises(capi.OcrError) as e:
        fn()
    assert e.value.code == INVALID, e.value
    for n in needles:
        assert n in str(e.value), e.value


def test_invalid_decode(rec):
    from ocr_rs_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(99)
    po = np.array([0, 5, 8], np.int32)
    so = LO.span_offsets(po, 2)                      # [0, 9, 14]
    cost = CL.make_costs(rng, int(so[-1]))
    T = CL.make_model(rng)
    want = LO.decode(cost, so, po, T, 2, 2)
    prm = dict(max_span=2, top_k=2)
    with capi.CharLm(rec, T) as lm:
        good = lambda: _same(rec.lattice_decode(lm, cost, so, po, prm), want)
        out = C.POINTER(capi.LatticePathsBlock)()
        p = capi.lattice_params(**prm)
        raw = lambda *a: capi.check(L.ocr_lattice_decode(*a))
        ok = (rec._h, lm.handle, cost.ctypes.data, 14, capi.MEM_HOST, so.ctypes.data, po.ctypes.data, 2, C.byref(p), C.byref(out))
        for k in (0, 1, 2, 5, 6, 9):      # rec, lm, costs, span_offsets, piece_offsets, out
            args = list(ok)
            args[k] = None
            _invalid(lambda: raw(*args), "null")
            good()
        _invalid(lambda: raw(*ok[:4], 5, *ok[5:]), "mem_kind")
        _invalid(lambda: rec.lattice_decode(lm, cost, [1, 9, 14], po, prm), "start at 1")
        _invalid(lambda: rec.lattice_decode(lm, cost, so, [1, 5, 8], prm), "start at")
        _invalid(lambda: rec.lattice_decode(lm, cost, so, [0, 5, 4], prm), "decrease at word 1")
        _invalid(lambda: rec.lattice_decode(lm, cost, [0, 9, 13], po, prm), "word 1", "holds 4 spans")      # a wrong span count
        _invalid(lambda: rec.lattice_decode(lm, cost, [0, 8, 14], po, prm), "word 0", "holds 8 spans")
        _invalid(lambda: rec.lattice_decode(lm, cost, so, po, dict(max_span=3, top_k=2)), "holds 9 spans", "gives 12")   # counted for M = 2
        _invalid(lambda: rec.lattice_decode(lm, cost[:13], so, po, prm), "end at 14")
        _invalid(lambda: rec.lattice_decode(lm, np.concatenate([cost, cost[:1]]), so, po, prm), "end at 14")
        good()
        for bad in (dict(top_k=0), dict(top_k=9), dict(max_span=0), dict(max_span=5), dict(max_span=-1), dict(reserved=(1, 0)),
                    dict(reserved=(0, 5))):
            _invalid(lambda: rec.lattice_decode(lm, cost, so, po, bad), "params")
        for bad in (np.nan, np.inf, -np.inf, -1.0, -1e-300):
            for slot in range(4):
                sc = [0.0] * 4
                sc[slot] = bad
                _invalid(lambda: rec.lattice_decode(lm, cost, so, po, dict(prm, span_cost=sc)), f"span_cost[{slot}]")
        good()
        for bad in (np.nan, np.inf, -np.inf, -1.0):
            c = cost.copy()
            c[12, 61] = bad
            _invalid(lambda: rec.lattice_decode(lm, c, so, po, dict(max_span=2, top_k=8)), "word 1")
            c[2, 0] = bad                              # a merged span's row (e = 2, m = 2) of word 0
            _invalid(lambda: rec.lattice_decode(lm, c, so, po, dict(max_span=2)), "word 0")
            good()
        po3 = np.array([0, 5, 8, 41], np.int32)          # ... also in a word that is too long to be decoded
        so3 = LO.span_offsets(po3, 2)
        c = np.concatenate([cost, CL.make_costs(rng, int(so3[-1] - so3[2]))])
        c[40, 3] = np.nan
        _invalid(lambda: rec.lattice_decode(lm, c, so3, po3, prm), "word 2")
        good()
        with pytest.raises(ValueError):
            rec.lattice_decode(lm, cost, so, [0, 8], prm)
    L.ocr_lattice_paths_free(None)
    L.ocr_span_table_free(None)
    with pytest.raises(TypeError):
        capi.lattice_params(beam=3)


# ---- read_words composed

def _plain(pages):
    return [[(t, p.tolist(), np.asarray(b).tolist()) for t, p, b in pg] for pg in pages]


def test_read_words_with_a_lattice(rec):
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    from tests.test_gpu_glyphs import _synthetic_pages
    det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    try:
        frames, polys = _synthetic_pages(2, 320, 320, 25, seed=33)
        adj = np.ones((2, 2))
        before = reading.read_words(det, rec, frames, polys, adj)
        assert _plain(reading.read_words(det, rec, frames, polys, adj, lattice=None, split=None)) == _plain(before)
        split = dict(aspect_pct=60, max_pieces=3)
        lat = dict(max_span=3, top_k=2, span_cost=[0.5, 0.0, 0.0])
        table = capi.char_lm_table(["code", "node", "mode", "home", "come"], weight=2.0)
        with capi.CharLm(rec, table) as lm:
            got = reading.read_words(det, rec, frames, polys, adj, lm=lm, lattice=lat, split=split)
            zero = reading.read_words(det, rec, frames, polys, adj, lattice={})
            # the calls by hand
            glyphs = det.segment_glyphs(frames, polys, adj)
            pieces, pmap = det.split_glyphs(frames, glyphs, split)
            spans, tab = capi.glyph_spans(pieces, 3)
            crops = det.extract_glyph_crops(frames, spans)
            logits = rec.forward_host(crops)
            costs = rec.glyph_costs(logits)
            labels, probs = rec.classify_host(crops)
            p = rec.lattice_decode(lm, costs, tab.span_offsets, tab.piece_offsets, lat)
            with pytest.raises(capi.OcrError):
                reading.read_words(det, rec, frames, polys, adj, cc={}, mask=True, lattice={})
            with capi.Lexicon(rec, ["code"]) as lex, pytest.raises(capi.OcrError):
                reading.read_words(det, rec, frames, polys, adj, lexicon=lex, lattice={})
        _same(p, LO.decode(costs, tab.span_offsets, tab.piece_offsets, table, 3, 2, lat["span_cost"]))
        assert pieces.n_glyphs > glyphs.n_glyphs and len(pmap) == pieces.n_glyphs
        po, so = tab.piece_offsets, tab.span_offsets
        k = merged = 0
        for pg, pg0 in zip(got, before):
            assert len(pg) == len(pg0)
            for text, pr, where, (cost, raw, raw_text, seg_len) in pg:
                segs = p.segments(po, k) if p.word_flags[k] == 0 else [(q, 1, -1) for q in range(po[k], po[k + 1])]
                rows = [int(so[k]) + LO.row_of(q - int(po[k]) + m, m, 3) for q, m, _ in segs]
                assert (cost, raw) == (float(p.costs[k, 0]), float(p.raw_costs[k])) and seg_len == tuple(m for _, m, _ in segs)
                assert raw_text == "".join(capi._ALPHABET[int(labels[int(so[k]) + LO.row_of(e, 1, 3)])] for e in range(1, int(po[k + 1] - po[k]) + 1))
                if p.word_flags[k] == 0:
                    assert text == p.text(po, k) and len(text) == len(seg_len)
                assert np.array_equal(where, spans.boxes[rows].reshape(-1, 4)) and np.array_equal(pr, probs[rows])
                merged += any(m > 1 for m in seg_len)
                k += 1
        assert k == p.n_words and merged > 0
        assert sum(len(pg) for pg in zero) == k and all(len(wd) == 4 and len(wd[3]) == 4 for pg in zero for wd in pg)
        print(f"\nread_words with a lattice: {k} words, {glyphs.n_glyphs} glyphs -> {pieces.n_glyphs} pieces -> {spans.n_glyphs} spans, "
              f"{merged} words read with a merged segment")
    finally:
        det.close()
