"""The character language model on the MI355X (ocr_char_lm_create, ocr_lm_decode; csrc/char_lm.hip) against tests/char_lm_oracle.py:
labels and flags equal, every cost bit-equal (compared as uint64), for words of 0..33 glyphs, batches either side of the words of a
workgroup, ties, extreme model values, permuted batches, both memory kinds, model lifetimes and every OCR_ERR_INVALID case; the zero
model against ocr_lexicon_match's raw costs; read_words composed with a model, and with a model and a lexicon."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import char_lm_oracle as LM
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
    assert got.labels.shape == want["labels"].shape and got.costs.shape == want["costs"].shape
    assert np.array_equal(got.word_flags, want["word_flags"])
    assert np.array_equal(_u64(got.raw_costs), _u64(want["raw_costs"]))
    assert np.array_equal(_u64(got.costs), _u64(want["costs"]))
    assert np.array_equal(got.labels, want["labels"])


def _check(rec, cost, off, T, top_k, lm=None):
    from ocr_rs_amd import capi
    want = LM.decode(cost, off, T, top_k=top_k)
    if lm is not None:
        got = rec.lm_decode(lm, cost, off, dict(top_k=top_k))
    else:
        with capi.CharLm(rec, T) as m:
            got = rec.lm_decode(m, cost, off, dict(top_k=top_k))
    _same(got, want)
    return got, want


def test_constants_match_the_kernel():
    from ocr_rs_amd import capi
    assert capi.LM_WORDS == 4 and capi.LM_MAX_LEN == LM.MAX_LEN == 32 and capi.LM_BEGIN == LM.BEGIN == 62 and capi.LM_END == LM.END == 62


@functools.lru_cache(maxsize=None)
def _shapes():
    rng = np.random.default_rng(11)
    off = LM.offsets([0, 1, 2, 3, 31, 32, 33])
    return LM.make_costs(rng, int(off[-1])), off, LM.make_model(rng)


@pytest.mark.parametrize("top_k", [1, 2, 8])
def test_word_shapes(rec, top_k):
    cost, off, T = _shapes()
    got, want = _check(rec, cost, off, T, top_k)
    assert want["word_flags"].tolist() == [1, 0, 0, 0, 0, 0, 2]
    assert np.all(np.isinf(got.costs[[0, 6]])) and np.all(np.isfinite(got.costs[1:6])) and np.all(got.labels[:, 69:] == -1)
    assert np.all(got.costs[1:6, 0] <= got.raw_costs[1:6]) and got.raw_costs[0] == 0.0 and got.raw_costs[6] > 0


@pytest.mark.parametrize("integer", [False, True], ids=["floats", "whole"])
def test_against_every_path(rec, integer):
    """G = 1, 2, 3 against the enumeration of all 62^G paths: the 8 smallest costs, bit for bit."""
    rng = np.random.default_rng(12 + integer)
    off = LM.offsets([1, 2, 3])
    cost, T = LM.make_costs(rng, 6, integer=integer), LM.make_model(rng, integer=integer)
    got, _ = _check(rec, cost, off, T, 8)
    for w in range(3):
        all_cost, _ = LM.enumerate_paths(cost[off[w]:off[w + 1]], T)
        assert np.array_equal(_u64(got.costs[w]), _u64(np.sort(all_cost)[:8]))


# capi.LM_WORDS words share a workgroup: 3, 4, 5 are one either side of it, 7..9 of two workgroups
@pytest.mark.parametrize("n_words", [1, 3, 4, 5, 7, 8, 9])
def test_word_counts_around_a_workgroup(rec, n_words):
    from ocr_rs_amd import capi
    assert capi.LM_WORDS == 4
    rng = np.random.default_rng(20 + n_words)
    off = LM.offsets(rng.integers(1, 7, n_words).tolist())
    cost, T = LM.make_costs(rng, int(off[-1])), LM.make_model(rng)
    for k in (1, 8):
        _check(rec, cost, off, T, k)


@pytest.mark.parametrize("top_k", [1, 8])
def test_257_words(rec, top_k):
    rng = np.random.default_rng(30)
    off = LM.offsets(rng.integers(1, 13, 257).tolist())
    _check(rec, LM.make_costs(rng, int(off[-1])), off, LM.make_model(rng), top_k)


def test_a_word_does_not_see_its_neighbours(rec):
    from ocr_rs_amd import capi
    rng = np.random.default_rng(31)
    off = LM.offsets([4, 6, 1, 9, 3, 6, 12, 2])
    cost, T = LM.make_costs(rng, int(off[-1])), LM.make_model(rng)
    probe = LM.make_costs(rng, 6)
    with capi.CharLm(rec, T) as lm:
        alone, _ = _check(rec, probe, [0, 6], T, 8, lm)
        for pos in (0, 3, 8):
            gl = np.diff(off).tolist()
            gl.insert(pos, 6)
            g0 = int(off[pos])
            got = rec.lm_decode(lm, np.concatenate([cost[:g0], probe, cost[g0:]]), LM.offsets(gl), dict(top_k=8))
            assert np.array_equal(_u64(got.costs[pos]), _u64(alone.costs[0])) and got.raw_costs[pos] == alone.raw_costs[0]
            assert np.array_equal(got.labels[:, g0:g0 + 6], alone.labels)


def test_no_words_and_words_without_glyphs(rec):
    from ocr_rs_amd import capi
    with capi.CharLm(rec, LM.zero_model()) as lm:
        got = rec.lm_decode(lm, np.zeros((0, 62), np.float32), [0], None)              # no word: an empty block
        assert got.costs.shape == (0, 1) and got.raw_costs.shape == (0,) and got.labels.shape == (1, 0)
        got = rec.lm_decode(lm, np.zeros((0, 62), np.float32), [0, 0, 0], dict(top_k=2))   # words without glyphs only
        assert got.word_flags.tolist() == [1, 1] and np.all(np.isinf(got.costs)) and got.costs.shape == (2, 2)
        assert got.raw_costs.tolist() == [0.0, 0.0] and got.labels.shape == (2, 0)


def test_ties_go_by_class_and_rank(rec):
    cost, off, T = LM.tie_case()
    for k in (1, 2, 8):
        _, want = _check(rec, cost, off, T, k)
        assert want["ties"] > 0
    cost, off, T = LM.hand_tie_case()
    got, _ = _check(rec, cost, off, T, 8)
    assert [got.text(off, 0, k) for k in range(8)] == ["AA", "BA", "BB", "CA", "DA", "EA", "FA", "GA"]


def test_model_values_zero_huge_and_subnormal(rec):
    rng = np.random.default_rng(40)
    off = LM.offsets([1, 2, 5, 32, 7])
    cost = LM.make_costs(rng, int(off[-1]))
    tiny = np.float32(np.finfo(np.float32).smallest_subnormal)
    T = LM.zero_model()
    pick = rng.integers(0, 3, size=(63, 63))
    T[:63, :63] = np.choose(pick, [np.float32(0.0), np.float32(1e30), tiny])
    T[LM.BEGIN, LM.END] = 0.0
    assert (T == np.float32(1e30)).sum() > 100 and (T == tiny).sum() > 100
    for k in (1, 8):
        got, _ = _check(rec, cost, off, T, k)
        assert np.all(np.isfinite(got.costs))
    huge = LM.zero_model()
    huge[:63, :63] = np.float32(1e30)                     # every path pays 1e30 per transition: the sums stay finite and exact to f64
    huge[LM.BEGIN, LM.END] = 0.0
    _check(rec, cost, off, huge, 8)
    sub = LM.zero_model()
    sub[:63, :63] = tiny
    sub[LM.BEGIN, LM.END] = 0.0
    _check(rec, cost, off, sub, 8)


def test_layout_independence(rec):
    """A model whose rows are all equal, and the words of a batch permuted: every word keeps its result."""
    from ocr_rs_amd import capi
    rng = np.random.default_rng(50)
    gs = rng.integers(1, 10, 23).tolist()
    off = LM.offsets(gs)
    cost = LM.make_costs(rng, int(off[-1]))
    T = LM.zero_model()
    T[:63, :63] = rng.uniform(0, 5, 63).astype(np.float32)[None, :]
    T[LM.BEGIN, LM.END] = 0.0
    with capi.CharLm(rec, T) as lm:
        got, _ = _check(rec, cost, off, T, 8, lm)
        perm = rng.permutation(len(gs))
        pcost = np.concatenate([cost[off[w]:off[w + 1]] for w in perm])
        poff = LM.offsets([gs[w] for w in perm])
        again, _ = _check(rec, pcost, poff, T, 8, lm)
    for n, w in enumerate(perm):
        assert np.array_equal(_u64(again.costs[n]), _u64(got.costs[w])) and again.raw_costs[n] == got.raw_costs[w]
        assert np.array_equal(again.labels[:, poff[n]:poff[n + 1]], got.labels[:, off[w]:off[w + 1]])


def test_zero_model_against_the_lexicon_call(rec):
    """Under an all-zero model the cheapest path is the greedy reading, and its cost equals ocr_lexicon_match's raw cost from the
    device bit for bit: x + 0.0 is exact."""
    from ocr_rs_amd import capi
    rng = np.random.default_rng(60)
    off = LM.offsets([1, 2, 0, 5, 12, 32, 40, 3])
    cost = LX.make_costs(rng, int(off[-1]))
    with capi.CharLm(rec, LM.zero_model()) as lm, capi.Lexicon(rec, ["A"]) as lex:
        got, _ = _check(rec, cost, off, LM.zero_model(), 1, lm)
        m = rec.lexicon_match(lex, cost, off)
    assert np.array_equal(_u64(got.raw_costs), _u64(m.raw_costs))
    dec = got.word_flags == 0
    assert np.array_equal(_u64(got.costs[dec, 0]), _u64(m.raw_costs[dec]))
    first = cost.argmin(axis=1)
    rows = np.repeat(dec, np.diff(off))
    assert np.array_equal(got.labels[0][rows], first[rows])


def test_memory_kinds_and_model_lifetimes(rec):
    import torch
    from ocr_rs_amd import capi
    rng = np.random.default_rng(70)
    off = LM.offsets([3, 5, 0, 8, 33, 2])
    cost, T, T2 = LM.make_costs(rng, int(off[-1])), LM.make_model(rng), LM.make_model(rng)
    lm = capi.CharLm(rec, T)
    host, _ = _check(rec, cost, off, T, 8, lm)
    d = torch.from_numpy(cost).cuda()
    torch.cuda.synchronize()
    dev = rec.lm_decode_device(lm, d.data_ptr(), cost.shape[0], off, dict(top_k=8))       # the same handle, a second call
    _same(dev, {"labels": host.labels, "costs": host.costs, "raw_costs": host.raw_costs, "word_flags": host.word_flags})
    _check(rec, cost, off, T, 1, lm)
    lm.close()
    with pytest.raises(capi.OcrError):
        lm.handle
    lm = capi.CharLm(rec, T2)                                                             # destroyed and created again
    try:
        _check(rec, cost, off, T2, 8, lm)
    finally:
        lm.close()
    with capi.CharLm.from_words(rec, ["code", "node"], alpha=0.25, weight=2.0) as lw:
        assert np.array_equal(lw.table, capi.char_lm_table(["code", "node"], alpha=0.25, weight=2.0))
        _check(rec, cost, off, lw.table, 2, lw)


# ---- errors: bad arguments only, and the handle is used again after each

def _invalid(fn, *needles):
    from ocr_rs_amd import capi
    with pytest.raises(capi.OcrError) as e:
        fn()
    assert e.value.code == INVALID, e.value
    for n in needles:
        assert n in str(e.value), e.value


def test_invalid_model(rec):
    from ocr_rs_amd import capi
    L = capi.lib()
    T = LM.zero_model()
    out = C.c_void_p()
    call = lambda *a: capi.check(L.ocr_char_lm_create(*a))
    _invalid(lambda: call(None, T.ctypes.data, C.byref(out)), "null")
    _invalid(lambda: call(rec._h, None, C.byref(out)), "null")
    _invalid(lambda: call(rec._h, T.ctypes.data, None), "null")
    for bad in (np.nan, np.inf, -np.inf, -1.0):
        Tb = T.copy()
        Tb[5, 17] = bad
        Tb[40, 2] = bad
        _invalid(lambda: capi.CharLm(rec, Tb), "[5][17]")
    for cell in ((63, 4), (4, 63), (62, 62), (63, 63)):
        Tb = T.copy()
        Tb[cell] = 1.0
        _invalid(lambda: capi.CharLm(rec, Tb), f"[{cell[0]}][{cell[1]}]", "unused")
    _invalid(lambda: capi.CharLm(rec, np.zeros((62, 62), np.float32)), "64 x 64")
    Tb = T.copy()
    Tb[62, 3] = Tb[3, 62] = 2.0                                    # begin and end costs are used cells
    cost = LM.make_costs(np.random.default_rng(1), 3)
    _check(rec, cost, [0, 3], Tb, 2)                               # the handle still works
    L.ocr_char_lm_destroy(None)


def test_invalid_decode(rec):
    from ocr_rs_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(80)
    cost = LM.make_costs(rng, 8)
    off = np.array([0, 5, 8], np.int32)
    T = LM.make_model(rng)
    want = LM.decode(cost, off, T, top_k=2)
    with capi.CharLm(rec, T) as lm:
        good = lambda: _same(rec.lm_decode(lm, cost, off, dict(top_k=2)), want)
        out = C.POINTER(capi.LmPathsBlock)()
        raw = lambda r, m, c, ng, mk, o, nw, p, ou: capi.check(L.ocr_lm_decode(r, m, c, ng, mk, o, nw, p, ou))
        ok = (rec._h, lm.handle, cost.ctypes.data, 8, capi.MEM_HOST, off.ctypes.data, 2, None, C.byref(out))
        for k in (0, 1, 2, 5, 8):      # rec, lm, costs, word_offsets, out
            args = list(ok)
            args[k] = None
            _invalid(lambda: raw(*args), "null")
            good()
        _invalid(lambda: raw(*ok[:4], 5, *ok[5:]), "mem_kind")
        _invalid(lambda: rec.lm_decode(lm, cost, [1, 5, 8]), "start at 1")
        _invalid(lambda: rec.lm_decode(lm, cost, [0, 6, 5, 8]), "decrease at word 1")
        _invalid(lambda: rec.lm_decode(lm, cost, [0, 5, 7]), "end at 7")
        _invalid(lambda: rec.lm_decode(lm, cost, [0, 5, 9]), "end at 9")
        good()
        for bad in (dict(top_k=0), dict(top_k=9), dict(top_k=-1), dict(reserved=(1, 0, 0)), dict(reserved=(0, 0, 5))):
            _invalid(lambda: rec.lm_decode(lm, cost, off, bad), "params")
        good()
        for bad in (np.nan, np.inf, -np.inf, -1.0):
            c = cost.copy()
            c[6, 61] = bad
            _invalid(lambda: rec.lm_decode(lm, c, off, dict(top_k=8)), "word 1")
            c[0, 0] = bad
            _invalid(lambda: rec.lm_decode(lm, c, off), "word 0")
            good()
        c = np.concatenate([cost, LM.make_costs(rng, 33)])          # ... also in a word that is too long to be decoded
        c[20, 3] = np.nan
        _invalid(lambda: rec.lm_decode(lm, c, [0, 5, 8, 41]), "word 2")
        good()
        if L.ocr_device_count() > 1:
            from ocr_rs_amd import weights as W
            other = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 1)
            try:
                _invalid(lambda: other.lm_decode(lm, cost, off), "device")
            finally:
                other.close()
    L.ocr_lm_paths_free(None)
    with pytest.raises(TypeError):
        capi.lm_params(beam=3)


# ---- read_words composed

def _plain(pages):
    return [[(t, p.tolist(), np.asarray(b).tolist()) for t, p, b in pg] for pg in pages]


def test_read_words_with_a_model_and_with_a_lexicon(rec):
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    from tests.test_gpu_glyphs import _synthetic_pages
    det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    try:
        frames, polys = _synthetic_pages(2, 320, 320, 25, seed=33)
        adj = np.ones((2, 2))
        before = reading.read_words(det, rec, frames, polys, adj)
        raw_texts = [t for pg in before for t, _, _ in pg]
        assert all(len(wd) == 3 for pg in before for wd in pg)
        known = sorted({t for t in raw_texts[::2] if 1 <= len(t) <= 32})
        words = known + LX.random_words(np.random.default_rng(4), 100, 1, 12)
        lparams = dict(top_k=1, max_len_diff=1, fold_case=0)
        table = capi.char_lm_table(LX.random_words(np.random.default_rng(6), 400, 1, 9), weight=3.0)
        with capi.CharLm(rec, table) as lm, capi.Lexicon(rec, words) as lex:
            got = reading.read_words(det, rec, frames, polys, adj, lm=lm, lm_params=dict(top_k=2))
            both = reading.read_words(det, rec, frames, polys, adj, lexicon=lex, lexicon_params=lparams, lm=lm)
            rect = reading.read_words_rectified(det, rec, frames, polys, adj, lm=lm)
            lines = reading.read_lines(det, rec, frames, polys, adj, lm=lm)
            assert _plain(reading.read_words(det, rec, frames, polys, adj, lm=None)) == _plain(before)
            # the calls by hand: crops -> logits -> costs -> decode, match
            glyphs, crops = reading.glyph_crops(det, frames, polys, adj)
            costs = rec.glyph_costs(rec.forward_host(crops))
            p = rec.lm_decode(lm, costs, glyphs.word_offsets, dict(top_k=2))
            m = rec.lexicon_match(lex, costs, glyphs.word_offsets, lparams)
        _same(p, LM.decode(costs, glyphs.word_offsets, table, top_k=2))
        assert sum(len(pg) for pg in got) == len(raw_texts) == p.n_words and len(rect) == len(lines) == 2
        k = changed = by_lex = 0
        for pg, pgb, pg0 in zip(got, both, before):
            for (text, pr, boxes, (lc, lr, raw)), wb, (t0, p0, b0) in zip(pg, pgb, pg0):
                assert raw == t0 and np.array_equal(pr, p0) and np.array_equal(boxes, b0)
                assert (lc, lr) == (float(p.costs[k, 0]), float(p.raw_costs[k]))
                decoded = int(p.word_flags[k]) == 0
                assert lc <= lr or not decoded
                assert text == (p.text(glyphs.word_offsets, k) if decoded else raw) and len(text) == len(raw)
                changed += text != raw
                # with both: the lexicon's element first, its accepted words keep the entry's string
                tb, _, _, (e, c, r, raw_b), (lc_b, lr_b, raw_b2) = wb
                assert (e, c, r) == (int(m.entries[k, 0]), float(m.costs[k, 0]), float(m.raw_costs[k])) and raw_b == raw_b2 == raw
                assert (lc_b, lr_b) == (lc, lr)
                take = e >= 0 and c - r <= 1.5 * len(raw)
                assert tb == (words[e] if take else text)
                by_lex += bool(take)
                k += 1
        assert by_lex > 0
        print(f"\nread_words with a model: {k} words, {changed} texts changed by the model, {by_lex} taken by the lexicon")
        for pg in rect:
            for wd in pg:
                assert len(wd) == 4 and len(wd[3]) == 3
    finally:
        det.close()
