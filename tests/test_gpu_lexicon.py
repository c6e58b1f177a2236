"""Lexicon matching on the MI355X (ocr_rec_glyph_costs, ocr_lexicon_create, ocr_lexicon_match; csrc/lexicon.hip) against
tests/lexicon_oracle.py: entries, candidate counts and flags equal, every cost bit-equal (compared as uint64), at the lexicon sizes
where the grid changes, for words of 0..33 glyphs, batches of 1..257 words, ties, permuted layouts, both memory kinds and every
OCR_ERR_INVALID case; the glyph costs against their f64 restatement; read_words composed with a lexicon."""
import ctypes as C
import functools

import numpy as np
import pytest

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


def _same(got, want):
    assert got.entries.shape == want["entries"].shape
    assert np.array_equal(got.entries, want["entries"])
    assert np.array_equal(got.costs.view(np.uint64), want["costs"].view(np.uint64))
    assert np.array_equal(got.raw_costs.view(np.uint64), want["raw_costs"].view(np.uint64))
    assert np.array_equal(got.n_candidates, want["n_candidates"])
    assert np.array_equal(got.word_flags, want["word_flags"])


def _check(rec, cost, off, words, params, lex=None):
    from ocr_rs_amd import capi
    want = LX.match(cost, off, words, **params)
    if lex is not None:
        got = rec.lexicon_match(lex, cost, off, params)
    else:
        with capi.Lexicon(rec, words) as lx:
            assert len(lx) == len(words)
            got = rec.lexicon_match(lx, cost, off, params)
    _same(got, want)
    return got, want


@pytest.mark.parametrize("name", sorted(LX.hand_cases()))
def test_hand_cases(rec, name):
    cost, off, words, params = LX.hand_cases()[name]
    _check(rec, cost, off, words, params)


def test_chunk_constant_matches_the_kernel():
    from ocr_rs_amd import capi
    assert capi.LEX_CHUNK == 256 and capi.LEX_MAX_LEN == LX.MAX_LEN == 32 and capi.LEX_MAX_ENTRIES == 1 << 22


# 255, 256 and 257 are one entry either side of capi.LEX_CHUNK, the entries of one pass of a workgroup; 511..513 of two passes' worth
@pytest.mark.parametrize("n_entries", [1, 63, 64, 65, 255, 256, 257, 511, 512, 513])
def test_lexicon_sizes(rec, n_entries):
    from ocr_rs_amd import capi
    assert capi.LEX_CHUNK == 256
    # every entry is a candidate of every word (lengths 1..8, max_len_diff 8), then the default window
    cost, off, words = LX.fuzz(100 + n_entries, n_entries, [1, 2, 3, 5, 8, 4], 1, 8)
    with capi.Lexicon(rec, words) as lex:
        for params in (dict(max_len_diff=8, top_k=1), dict(max_len_diff=8, top_k=8), dict(top_k=8, ins_cost=1.5, del_cost=0.0),
                       dict(top_k=1, ins_cost=0.0, del_cost=2.25, fold_case=0)):
            got, want = _check(rec, cost, off, words, params, lex)
            if params.get("max_len_diff") == 8:
                assert want["n_candidates"].tolist() == [n_entries] * 6


@functools.lru_cache(maxsize=None)
def _mixed():
    """about 5 000 entries of 1..32 characters, words of 0, 1, 2, 31, 32 and 33 glyphs among 64"""
    rng = np.random.default_rng(5)
    gs = [0, 1, 2, 31, 32, 33] + rng.integers(1, 33, 58).tolist()
    return LX.fuzz(6, 5000, gs)


@pytest.mark.parametrize("params", [dict(top_k=1), dict(top_k=8, ins_cost=2.5, del_cost=3.5, max_len_diff=3)], ids=["k1", "k8"])
def test_mixed_lengths_and_word_shapes(rec, params):
    cost, off, words = _mixed()
    got, want = _check(rec, cost, off, words, params)
    assert want["word_flags"][:6].tolist() == [1, 0, 0, 0, 0, 2] and np.all(want["n_candidates"][1:5] > 0)


def test_many_words_take_several_passes_per_workgroup(rec):
    """257 words against 5 000 entries that are all candidates: 20 chunks x 257 words is above the 4 096 workgroups the launch aims
    at, so every workgroup makes two passes."""
    from ocr_rs_amd import capi
    rng = np.random.default_rng(9)
    cost, off, words = LX.fuzz(10, 5000, rng.integers(1, 13, 257).tolist(), 1, 12)
    assert -(-len(words) // capi.LEX_CHUNK) * 257 > 4096
    _check(rec, cost, off, words, dict(top_k=8, max_len_diff=8))


def test_batches_of_one_and_two_words(rec):
    from ocr_rs_amd import capi
    cost, off, words = LX.fuzz(21, 300, [5, 7], 3, 9)
    with capi.Lexicon(rec, words) as lex:
        _check(rec, cost, off, words, dict(top_k=8), lex)
        _check(rec, cost[:5], off[:2], words, dict(top_k=8), lex)
        got = rec.lexicon_match(lex, np.zeros((0, 62), np.float32), [0], None)        # no word: an empty block
        assert got.entries.shape == (0, 1) and got.raw_costs.shape == (0,)
        got = rec.lexicon_match(lex, np.zeros((0, 62), np.float32), [0, 0, 0], None)  # words without glyphs only
        assert got.word_flags.tolist() == [1, 1] and got.entries.tolist() == [[-1], [-1]]


def test_ties_go_to_the_smaller_index(rec):
    fa, params, _ = LX.TIE_CASES["integer_ties"]
    cost, off, words = LX.fuzz(**fa)
    _, want = _check(rec, cost, off, words, params)
    assert want["ties"] > 0


@pytest.mark.parametrize("top_k", [1, 8])
def test_equal_costs_in_every_wave_of_three_chunks_go_to_the_smaller_index(rec, top_k):
    """One word of 3 glyphs whose cost rows are constant against 600 distinct entries of 3 characters (behind four of other lengths):
    every one of them costs the same, in all four waves of three chunks, so the wave's butterfly, the read-back of the waves' slots
    and the merge over the chunks all see equal costs and the index alone decides."""
    words = ["a", "bc", "defg", "hijkl"] + ["".join(LX.ALPHABET[37 * n // d % 62] for d in (3844, 62, 1)) for n in range(600)]
    assert len(set(words)) == 604
    got, want = _check(rec, np.full((3, 62), 1.5, np.float32), [0, 3], words, dict(top_k=top_k))
    assert want["n_candidates"].tolist() == [604] and got.entries.tolist() == [list(range(4, 4 + top_k))] and np.all(got.costs == 4.5)


def test_layout_independence(rec):
    """The same lexicon permuted: the same costs, and the same entries through the permutation (no cost ties, so the index decides
    nothing)."""
    fa, params, _ = LX.TIE_CASES["layout_no_ties"]
    cost, off, words = LX.fuzz(**fa)
    got, want = _check(rec, cost, off, words, params)
    assert want["ties"] == 0
    perm = np.random.default_rng(3).permutation(len(words))
    from ocr_rs_amd import capi
    with capi.Lexicon(rec, [words[k] for k in perm]) as lex:
        again = rec.lexicon_match(lex, cost, off, params)
    assert np.array_equal(again.costs.view(np.uint64), got.costs.view(np.uint64))
    assert np.array_equal(perm[again.entries], got.entries)


def test_a_word_does_not_see_its_neighbours(rec):
    from ocr_rs_amd import capi
    cost, off, words = LX.fuzz(31, 700, [4, 6, 1, 9, 3, 6, 12, 2], 1, 14)
    probe = LX.make_costs(np.random.default_rng(32), 6)
    params = dict(top_k=8)
    with capi.Lexicon(rec, words) as lex:
        alone = rec.lexicon_match(lex, probe, [0, 6], params)
        _same(alone, LX.match(probe, [0, 6], words, **params))
        for pos in (0, 3, 8):
            gl = np.diff(off).tolist()
            gl.insert(pos, 6)
            g0 = int(off[pos])
            batch = np.concatenate([cost[:g0], probe, cost[g0:]])
            got = rec.lexicon_match(lex, batch, np.concatenate([[0], np.cumsum(gl)]), params)
            assert np.array_equal(got.entries[pos], alone.entries[0])
            assert np.array_equal(got.costs[pos].view(np.uint64), alone.costs[0].view(np.uint64))
            assert got.raw_costs[pos] == alone.raw_costs[0] and got.n_candidates[pos] == alone.n_candidates[0]


def test_host_and_device_memory_agree(rec):
    import torch
    from ocr_rs_amd import capi
    cost, off, words = LX.fuzz(41, 400, [3, 5, 0, 8, 33], 1, 10)
    with capi.Lexicon(rec, words) as lex:
        host = rec.lexicon_match(lex, cost, off, dict(top_k=8))
        d = torch.from_numpy(cost).cuda()
        torch.cuda.synchronize()
        dev = rec.lexicon_match_device(lex, d.data_ptr(), cost.shape[0], off, dict(top_k=8))
    for a in ("entries", "n_candidates", "word_flags"):
        assert np.array_equal(getattr(host, a), getattr(dev, a))
    assert np.array_equal(host.costs.view(np.uint64), dev.costs.view(np.uint64))
    assert np.array_equal(host.raw_costs.view(np.uint64), dev.raw_costs.view(np.uint64))


# ---- errors: bad arguments only, and the handle is used again after each

def _invalid(fn, *needles):
    from ocr_rs_amd import capi
    with pytest.raises(capi.OcrError) as e:
        fn()
    assert e.value.code == INVALID, e.value
    for n in needles:
        assert n in str(e.value), e.value


def test_invalid_glyph_costs(rec):
    from ocr_rs_amd import capi
    L = capi.lib()
    x = np.zeros((4, 62), np.float32)
    out = np.empty_like(x)
    h = rec._h
    call = lambda *a: capi.check(L.ocr_rec_glyph_costs(*a))
    _invalid(lambda: call(None, x.ctypes.data, 4, out.ctypes.data, capi.MEM_HOST))
    _invalid(lambda: call(h, None, 4, out.ctypes.data, capi.MEM_HOST))
    _invalid(lambda: call(h, x.ctypes.data, 4, None, capi.MEM_HOST))
    _invalid(lambda: call(h, x.ctypes.data, 4, out.ctypes.data, 7), "mem_kind")
    _invalid(lambda: call(h, x.ctypes.data, -1, out.ctypes.data, capi.MEM_HOST))
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[2, 5] = bad
        y[3, 0] = bad
        _invalid(lambda: rec.glyph_costs(y), "row 2")
    call(h, x.ctypes.data, 0, out.ctypes.data, capi.MEM_HOST)     # n = 0 does nothing
    _costs_within_bar(rec.glyph_costs(x), x)                      # the handle still works


def test_invalid_lexicon_create(rec):
    from ocr_rs_amd import capi
    L = capi.lib()
    blob = np.frombuffer(b"HELLOWORLD", np.uint8)
    off = np.array([0, 5, 10], np.int32)
    out = C.c_void_p()
    call = lambda *a: capi.check(L.ocr_lexicon_create(*a))
    _invalid(lambda: call(None, blob.ctypes.data, off.ctypes.data, 2, C.byref(out)))
    _invalid(lambda: call(rec._h, None, off.ctypes.data, 2, C.byref(out)))
    _invalid(lambda: call(rec._h, blob.ctypes.data, None, 2, C.byref(out)))
    _invalid(lambda: call(rec._h, blob.ctypes.data, off.ctypes.data, 2, None))
    _invalid(lambda: call(rec._h, blob.ctypes.data, off.ctypes.data, 0, C.byref(out)), "0 entries")
    _invalid(lambda: call(rec._h, blob.ctypes.data, off.ctypes.data, capi.LEX_MAX_ENTRIES + 1, C.byref(out)), "entries")
    _invalid(lambda: capi.Lexicon.from_bytes(rec, b"HELLOWORLD", [1, 5, 10]), "start at 1")
    _invalid(lambda: capi.Lexicon.from_bytes(rec, b"HELLOWORLD", [0, 5, 3, 10]), "entry 1")
    _invalid(lambda: capi.Lexicon.from_bytes(rec, b"HELLOWORLD", [0, 5, 5, 10]), "entry 1")     # an empty entry
    _invalid(lambda: capi.Lexicon.from_bytes(rec, b"A" * 40, [0, 3, 36, 40]), "entry 1")        # 33 characters
    _invalid(lambda: capi.Lexicon(rec, ["HELLO", "WOR-D", "A B"]), "entry 1", "0x2d")
    _invalid(lambda: capi.Lexicon(rec, []))
    _invalid(lambda: capi.check(L.ocr_lexicon_size(None, C.byref(C.c_int32()))))
    with capi.Lexicon(rec, ["HELLO", "HELLO", "A" * 32]) as lex:      # duplicates and the longest entry are legal
        assert len(lex) == 3
        got = rec.lexicon_match(lex, LX.costs_for_text("HELLO"), [0, 5], dict(top_k=3))
        assert got.entries.tolist() == [[0, 1, -1]]
    L.ocr_lexicon_destroy(None)


def test_invalid_lexicon_match(rec):
    from ocr_rs_amd import capi
    L = capi.lib()
    cost = LX.costs_for_text("HELLOYOU")
    off = np.array([0, 5, 8], np.int32)
    words = ["HELLO", "YOU", "YOUR"]
    with capi.Lexicon(rec, words) as lex:
        good = lambda: _same(rec.lexicon_match(lex, cost, off, dict(top_k=2)), LX.match(cost, off, words, top_k=2))
        out = C.POINTER(capi.LexiconMatchesBlock)()
        raw = lambda r, lx, c, ng, mk, o, nw, p, ou: capi.check(L.ocr_lexicon_match(r, lx, c, ng, mk, o, nw, p, ou))
        ok = (rec._h, lex.handle, cost.ctypes.data, 8, capi.MEM_HOST, off.ctypes.data, 2, None, C.byref(out))
        for k in (0, 1, 2, 5, 8):      # rec, lex, costs, word_offsets, out
            args = list(ok)
            args[k] = None
            _invalid(lambda: raw(*args), "null")
            good()
        _invalid(lambda: raw(*ok[:4], 5, *ok[5:]), "mem_kind")
        _invalid(lambda: rec.lexicon_match(lex, cost, [1, 5, 8]), "start at 1")
        _invalid(lambda: rec.lexicon_match(lex, cost, [0, 6, 5, 8]), "decrease at word 1")
        _invalid(lambda: rec.lexicon_match(lex, cost, [0, 5, 7]), "end at 7")
        _invalid(lambda: rec.lexicon_match(lex, cost, [0, 5, 9]), "end at 9")
        good()
        for bad in (dict(ins_cost=-1.0), dict(ins_cost=np.nan), dict(ins_cost=np.inf), dict(del_cost=-0.5), dict(del_cost=np.nan),
                    dict(del_cost=np.inf), dict(max_len_diff=-1), dict(max_len_diff=9), dict(fold_case=2), dict(fold_case=-1), dict(top_k=0),
                    dict(top_k=9), dict(reserved=(1, 0, 0)), dict(reserved=(0, 0, 5))):
            _invalid(lambda: rec.lexicon_match(lex, cost, off, bad), "params")
        good()
        for bad in (np.nan, np.inf, -np.inf, -1.0):
            c = cost.copy()
            c[6, 61] = bad
            _invalid(lambda: rec.lexicon_match(lex, c, off), "word 1")
            c[0, 0] = bad
            _invalid(lambda: rec.lexicon_match(lex, c, off), "word 0")
            good()
        c = np.concatenate([cost, LX.costs_for_text("A" * 33)])      # ... also in a word that is too long to be matched
        c[20, 3] = np.nan
        _invalid(lambda: rec.lexicon_match(lex, c, [0, 5, 8, 41]), "word 2")
        good()
        if L.ocr_device_count() > 1:
            from ocr_rs_amd import weights as W
            other = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 1)
            try:
                _invalid(lambda: other.lexicon_match(lex, cost, off), "device")
            finally:
                other.close()
    L.ocr_lexicon_matches_free(None)


# ---- ocr_rec_glyph_costs against the f64 restatement.  Bar per row: |got - want| <= 2^-23 want + 2^-40 max(1, max|x|).  The device's
# f64 exp and log are within a few ulp of f64, so lse is off by far less than 2^-40 max(1, |lse|); the rounding to f32 can then land
# on the neighbouring value, one f32 ulp.

def _costs_within_bar(got, logits):
    want = LX.glyph_costs(logits).astype(np.float64)
    bar = 2.0 ** -23 * want + 2.0 ** -40 * np.maximum(1.0, np.abs(logits.astype(np.float64)).max(axis=1, keepdims=True))
    err = np.abs(got.astype(np.float64) - want)
    print(f"\nglyph costs: {got.shape[0]} rows, max err / bar {float((err / bar).max()):.3f}, rows not bit-equal "
          f"{int((got != want.astype(np.float32)).any(axis=1).sum())}")
    assert got.dtype == np.float32 and np.all(got >= 0) and np.all(err <= bar)


def test_glyph_costs(rec):
    import torch
    from ocr_rs_amd import weights as W
    logits = rec.forward_host(W.synth_crops(3, 300))
    _costs_within_bar(rec.glyph_costs(logits), logits)
    wide = (np.random.default_rng(8).standard_normal((1025, 62)) * 8).astype(np.float32)
    got = rec.glyph_costs(wide)
    _costs_within_bar(got, wide)
    d_in = torch.from_numpy(wide).cuda()
    d_out = torch.empty_like(d_in)
    torch.cuda.synchronize()
    rec.glyph_costs_device(d_in.data_ptr(), wide.shape[0], d_out.data_ptr())
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), got.view(np.uint32))
    peak = np.zeros((3, 62), np.float32)
    peak[1, 17] = 60.0          # exp(-60) * 61 is below half an ulp of 1: lse == 60 and the clamp holds exactly 0.0
    got = rec.glyph_costs(peak)
    assert got[1, 17] == 0.0 and np.all(got[1, :17] == 60.0) and np.all(got >= 0)


# ---- read_words composed

def _plain(pages):
    return [[(t, p.tolist(), np.asarray(b).tolist()) for t, p, b in pg] for pg in pages]


def test_read_words_with_a_lexicon(rec):
    import torch
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    from tests.test_gpu_glyphs import _synthetic_pages
    det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    try:
        frames, polys = _synthetic_pages(4, 320, 320, 25, seed=33)
        adj = np.ones((4, 2))
        before = reading.read_words(det, rec, frames, polys, adj)
        raw_texts = [t for pg in before for t, _, _ in pg]
        known = sorted({t for t in raw_texts[::2] if 1 <= len(t) <= 32})      # half of the readings, plus decoys
        words = known + LX.random_words(np.random.default_rng(4), 300, 1, 12)
        params = dict(top_k=1, max_len_diff=1, fold_case=0)
        with capi.Lexicon(rec, words) as lex:
            got = reading.read_words(det, rec, frames, polys, adj, lexicon=lex, lexicon_params=params)
            rect = reading.read_words_rectified(det, rec, frames, polys, adj, lexicon=lex, lexicon_params=params)
            lines = reading.read_lines(det, rec, frames, polys, adj, lexicon=lex, lexicon_params=params)
            assert _plain(reading.read_words(det, rec, frames, polys, adj, lexicon=None)) == _plain(before)
            # the three calls by hand: crops -> logits -> costs -> match
            glyphs, crops = reading.glyph_crops(det, frames, polys, adj)
            logits = rec.forward_host(crops)
            costs = rec.glyph_costs(logits)
            m = rec.lexicon_match(lex, costs, glyphs.word_offsets, params)
        assert sum(len(pg) for pg in got) == len(raw_texts) == m.n_words and len(rect) == len(lines) == 4
        k = kept = swapped = 0
        for pg, pg0 in zip(got, before):
            for (text, pr, boxes, (e, c, r, raw)), (t0, p0, b0) in zip(pg, pg0):
                assert raw == t0 and np.array_equal(pr, p0) and np.array_equal(boxes, b0)
                assert (e, c, r) == (int(m.entries[k, 0]), float(m.costs[k, 0]), float(m.raw_costs[k]))
                take = e >= 0 and c - r <= 1.5 * len(raw)
                assert text == (words[e] if take else raw)
                if raw in known:        # the greedy reading is in the list: nothing is cheaper, and it keeps its text
                    assert c == r and text == raw
                    kept += 1
                swapped += text != raw
                k += 1
        assert kept > 0
        print(f"\nread_words with a lexicon: {k} words, {kept} with their raw reading in the list, {swapped} texts replaced")
        for pg in rect:
            for wd in pg:
                assert len(wd) == 4 and len(wd[3]) == 4
        x = torch.from_numpy(frames).cuda()
        with capi.Lexicon(rec, words) as lex:
            again = reading.read_words(det, rec, x, polys, adj, lexicon=lex, lexicon_params=params)
        assert [[(t, m4) for t, _, _, m4 in pg] for pg in again] == [[(t, m4) for t, _, _, m4 in pg] for pg in got]
    finally:
        det.close()
