"""Column-aware reading order on the MI355X (ocr_group_columns, csrc/columns.hip) against tests/column_oracle.py: every array of
ocr_columns_t equal, the f64 ones bit for bit (compared as uint64), on every hand case of tests/test_column_oracle.py, pages of the
two-column generator, seeded fuzz at the sizes where the kernels change path (one word, the wave and tile sizes, more than one LDS
tile, the 4 096-word cap), integer-grid fuzz that really has ties in every stage, pages that must not see their batch neighbours,
every parameter at both ends of its range, every OCR_ERR_INVALID case, and read_columns / page_text over the real reading chain."""
import ctypes as C

import numpy as np
import pytest

from tests import column_oracle as CO
from tests import line_oracle as LO
from tests.test_column_oracle import cases, flat, reading

pytestmark = pytest.mark.gpu

CASES = cases()


@pytest.fixture(scope="module")
def det():
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    yield d
    d.close()


def _same(got, want):
    for name in CO.ARRAYS:
        g, w = getattr(got, name).reshape(-1), want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if w.dtype == np.float64:
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), name
        else:
            assert g.tolist() == w.tolist(), name


def _check(det, quads, offsets, params=None):
    """the device result of one batch against the oracle; returns the oracle's result"""
    want = CO.group(quads, offsets, params)
    _same(det.group_columns(quads, offsets, params), want)
    return want


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_cases_equal_the_oracle(det, name):
    _check(det, *CASES[name])


@pytest.mark.parametrize("gutter", [2, 3, 5])
@pytest.mark.parametrize("angle", [0.0, 0.6])
def test_generated_pages_equal_the_oracle_and_read_in_order(det, gutter, angle):
    q, labels = CO.columns_page(gutter, angle, (8, 5), 2, seed=2)
    want = _check(det, q, [0, len(q)])
    assert flat(reading(want, labels)) == sorted(labels) and want["block_levels"].tolist() == [0, 1, 2, 3]


def _fuzz_with_a_page(n, seed):
    """LO.fuzz with two rings from 64 words on (as tests/test_gpu_lines.py has them), and from 255 words on a two-column page beside it"""
    q = LO.fuzz(n, seed)
    if n >= 64:
        span = float(np.abs(q).max())
        q[7:31] = LO.ring(24, 150.0, (span + 400.0, 300.0))
        q[40:56] = LO.ring(16, 80.0, (span + 400.0, 700.0), w=20.0)[::-1]
    if n >= 255:
        page = CO.columns_page(2, 0.1, (8, 8), 2, seed, origin=(float(np.abs(q).max()) + 1400.0, 500.0))[0]
        q[100:100 + len(page)] = page
    return q


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_fuzz_at_the_sizes_where_the_kernels_change_path(det, n):
    want = _check(det, _fuzz_with_a_page(n, seed=100 + n), [0, n])
    if n >= 64:
        assert (want["word_flags"] & 2).sum() >= 2
    if n >= 255:
        assert (want["word_flags"] & 4).sum() >= 8 and len(want["block_levels"]) < len(want["line_flags"]) < n
    if n == 1025:
        assert want["block_levels"].max() == 63, "the level cap of 64 is not reached: the case would not exercise it"
    if n == 1:
        assert want["order"].tolist() == [0] and want["block_offsets"].tolist() == [0, 1] and want["img_offsets"].tolist() == [0, 1]


def test_4096_words_with_four_levels(det):
    want = _check(det, _fuzz_with_a_page(4096, seed=5), [0, 4096], dict(max_levels=4))
    assert want["block_levels"].max() == 3 and sorted(want["order"].tolist()) == list(range(4096))


@pytest.mark.parametrize("n,seed", [(257, 7), (1025, 8)])
def test_integer_grid_fuzz_exercises_the_tie_breaks(det, n, seed):
    want = _check(det, CO.grid_fuzz(n, seed), [0, n])
    assert all(t > 0 for t in want["ties"]), "a stage without two equal projections in the oracle's run: the case would pass vacuously"
    assert (want["word_flags"] & 4).any()


def test_a_page_does_not_see_its_batch_neighbours(det):
    page = CO.columns_page(3, 0.1, (8, 5), 2, seed=3)[0]
    others = [_fuzz_with_a_page(257, seed=32), LO.ring(), CO.grid_fuzz(90, seed=33) + 1000.0, np.zeros((0, 8))]
    alone = det.group_columns(page, [0, len(page)])
    assert alone.n_blocks == 4 and alone.n_lines == 15
    for at in range(3):
        batch = [others[(at + k) % 4] for k in range(3)]
        batch.insert(at, page)
        off = np.concatenate([[0], np.cumsum([len(b) for b in batch])])
        _check(det, np.concatenate(batch), off)
        got = det.group_columns(np.concatenate(batch), off)
        w0, w1 = int(off[at]), int(off[at + 1])
        b0, b1 = int(got.img_offsets[at]), int(got.img_offsets[at + 1])
        l0, l1 = int(got.block_offsets[b0]), int(got.block_offsets[b1])
        assert (got.order[w0:w1] - w0).tolist() == alone.order.tolist()
        assert (got.block_offsets[b0:b1 + 1] - l0).tolist() == alone.block_offsets.tolist()
        assert (got.line_offsets[l0:l1 + 1] - w0).tolist() == alone.line_offsets.tolist()
        assert got.word_flags[w0:w1].tolist() == alone.word_flags.tolist() and got.line_flags[l0:l1].tolist() == alone.line_flags.tolist()
        assert got.block_levels[b0:b1].tolist() == alone.block_levels.tolist()
        assert np.array_equal(got.gaps[w0:w1].view(np.uint64), alone.gaps.view(np.uint64))
        assert np.array_equal(got.block_quads[b0:b1].view(np.uint64), alone.block_quads.view(np.uint64))


# both ends of every range; an open end is approached (0.05), and max_gap = 64 takes row_gap with it (row_gap >= max_gap)
ENDS = [dict(line_tol=0.05), dict(line_tol=4.0), dict(height_ratio=1.0), dict(height_ratio=16.0), dict(min_cos=0.0), dict(min_cos=1.0),
        dict(max_gap=0.0), dict(max_gap=64.0, row_gap=64.0), dict(row_gap=3.0), dict(row_gap=64.0), dict(min_gutter=0.0),
        dict(min_gutter=64.0), dict(gutter_reach=0.05), dict(gutter_reach=16.0), dict(min_rows=1), dict(min_rows=4096),
        dict(min_overlap=0.0), dict(min_overlap=1.0), dict(block_reach=0.05), dict(block_reach=16.0), dict(max_levels=1),
        dict(max_levels=256)]


@pytest.mark.parametrize("params", ENDS, ids=lambda p: ",".join("%s=%g" % kv for kv in p.items()))
def test_every_parameter_at_both_ends_of_its_range(det, params):
    q = _fuzz_with_a_page(300, seed=41)
    # three rows of two words 360 px = 22.5 heights apart, away from the rest: links (and a gutter of three) only beyond row_gap = 16
    q[250:256] = [LO.quad(x, -2000.0 + 30.0 * r, 40.0, 16.0) for r in range(3) for x in (0.0, 400.0)]
    base = CO.group(q, [0, 300])
    want = _check(det, q, [0, 300], params)
    assert any(want[k].tolist() != base[k].tolist() for k in CO.ARRAYS), "the parameter changes nothing on this input"


def test_every_invalid_call_is_refused_and_the_handle_stays_usable(det):
    from ocr_rs_amd import capi
    L = capi.lib()
    q, off, _ = CASES["narrow_gutter"]
    q = np.ascontiguousarray(q, np.float64)
    off32 = np.array(off, np.int32)
    out = C.POINTER(capi.ColumnsBlock)()
    ok = lambda: _check(det, q, off)
    ok()
    for args in [(None, q.ctypes.data, off32.ctypes.data, 1, None, C.byref(out)),          # null handle
                 (det._h, None, off32.ctypes.data, 1, None, C.byref(out)),                 # null quads with words
                 (det._h, q.ctypes.data, None, 1, None, C.byref(out)),                     # null offsets
                 (det._h, q.ctypes.data, off32.ctypes.data, 1, None, None),                # null out
                 (det._h, q.ctypes.data, off32.ctypes.data, 0, None, C.byref(out)),        # n_images < 1
                 (det._h, q.ctypes.data, off32.ctypes.data, -3, None, C.byref(out))]:
        assert L.ocr_group_columns(*args) == 1, args
        ok()

    def refused(quads, offsets, params=None):
        with pytest.raises(capi.OcrError) as e:
            det.group_columns(quads, offsets, params)
        assert e.value.code == 1, e.value
        ok()
    refused(q, [1, 16])                                  # offsets do not start at 0
    refused(np.concatenate([q, q]), [0, 16, 4, 32])      # offsets decrease
    nan, inf = float("nan"), float("inf")
    for field, bad in [("line_tol", 0.0), ("line_tol", 4.5), ("line_tol", nan), ("height_ratio", 0.99), ("height_ratio", 16.5),
                       ("min_cos", -0.01), ("min_cos", 1.01), ("max_gap", -1.0), ("max_gap", 64.5), ("max_gap", inf),
                       ("row_gap", 2.99), ("row_gap", 64.5), ("row_gap", nan), ("min_gutter", -0.01), ("min_gutter", 64.5),
                       ("min_gutter", nan), ("gutter_reach", 0.0), ("gutter_reach", 16.5), ("gutter_reach", nan), ("min_rows", 0),
                       ("min_rows", 4097), ("min_overlap", -0.01), ("min_overlap", 1.01), ("min_overlap", nan), ("block_reach", 0.0),
                       ("block_reach", 16.5), ("block_reach", inf), ("max_levels", 0), ("max_levels", 257)]:
        refused(q, off, {field: bad})
    refused(q, off, {"max_gap": 20.0})                   # row_gap (16) below max_gap
    for field in ("reserved", "line_reserved"):
        refused(q, off, {field: (0, 1)})
        refused(q, off, {field: (1, 0)})
    for bad in (np.nan, np.inf, -np.inf):
        qq = q.copy()
        qq[4, 5] = bad
        refused(qq, off)
    # one word over the cap in the second image: refused on the host, nothing is launched; exactly the cap is taken
    big = np.tile(np.array(LO.quad(50, 50, 40, 16)), (4097 + 16, 1))
    big[:16] = q
    refused(big, [0, 16, 16 + 4097])
    got = det.group_columns(big[:4096 + 16], [0, 16, 16 + 4096])
    assert got.n_lines == 8 + 4096 and got.n_blocks == 2 + 4096      # (coinciding words: nobody is right of, below or before anybody)


def _two_column_frame(rows, cols, gutter, angle, h, w):
    """a frame of striped dark words on a light page turned by `angle`: two columns of rows x cols words, the columns `gutter` px
    apart, and their quads as integer polygons in shuffled order with (column, row, k) of every polygon"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    frame = np.full((h, w), 215.0)
    c, s = np.cos(angle), np.sin(angle)
    polys, where = [], []
    col_w = (cols - 1) * 62.0 + 46.0
    for col in range(2):
        for r in range(rows):
            for k in range(cols):
                x = (col - 0.5) * (col_w + gutter) + (k - (cols - 1) / 2) * 62.0
                y = (r - (rows - 1) / 2) * 44.0
                cx, cy = w / 2 + x * c - y * s, h / 2 + x * s + y * c
                lx, ly = (xx + 0.5 - cx) * c + (yy + 0.5 - cy) * s, -(xx + 0.5 - cx) * s + (yy + 0.5 - cy) * c
                frame[(np.abs(lx) < 20) & (np.abs(ly) < 8) & (np.floor((lx + 20) / 5) % 2 == 0)] = 35.0
                polys.append([(int(round(px)), int(round(py))) for px, py in np.reshape(LO.quad(cx, cy, 46, 22, angle), (4, 2))])
                where.append((col, r, k))
    perm = np.random.default_rng(6).permutation(len(polys))
    return frame.astype(np.float32), [polys[i] for i in perm], [where[i] for i in perm]


def test_read_columns_on_a_two_column_page(det):
    from ocr_rs_amd import capi, reading as R
    from ocr_rs_amd import weights as W
    rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    try:
        # gutters of 50 px (2.3 word heights: found as a stack of four gaps) and of 90 px (4.1: beyond max_gap as well)
        f0, p0, w0 = _two_column_frame(4, 3, 50.0, 0.1, 320, 480)
        f1, p1, w1 = _two_column_frame(4, 3, 90.0, -0.15, 320, 480)
        frames = np.stack([f0, f1, np.full((320, 480), 200.0, np.float32)])[:, None]
        polys, adj = [p0, p1, []], [[1.0, 1.0]] * 3
        lines = R.read_lines(det, rec, frames, polys, adj, cc={})
        cols = R.read_columns(det, rec, frames, polys, adj, cc={})
        assert len(cols) == 3 and cols[2] == [] and R.page_text(cols[2], columns=True) == ""
        for b, where in enumerate([w0, w1]):
            # two blocks: the left column's rows top to bottom, then the right column's, each left to right
            assert [[[where[int(k)] for k in ks] for _, ks, _ in block] for block in cols[b]] == \
                [[[(col, r, k) for k in range(3)] for r in range(4)] for col in range(2)]
            for block in cols[b]:
                for text, ks, gaps in block:
                    assert ks.dtype == np.int32 and gaps[0] == 0.0 and np.all(gaps[1:] > 0) and len(gaps) == len(ks)
            text = R.page_text(cols[b], columns=True)
            assert text == "\n\n".join("\n".join(t for t, _, _ in block) for block in cols[b]) and text.count("\n\n") == 1
            assert text.replace("\n\n", "\n").count("\n") == 7 and any(t for block in cols[b] for t, _, _ in block)
            # without the keyword page_text is what it was: the lines of read_lines joined by "\n"
            assert R.page_text(lines[b]) == "\n".join(t for t, _, _ in lines[b])
        assert len(lines[0]) == 4 and len(lines[1]) == 8       # the line rule: merged at 50 px, interleaved at 90 px
        # at 90 px both rules find the same eight lines, in another order: the same words give the same texts
        key = lambda pg: sorted((ks.tolist(), t) for t, ks, _ in pg)
        assert key(lines[1]) == key([ln for block in cols[1] for ln in block])
        # parameters through to the call, with the unrectified reader: at min_rows = 5 nothing finds the 50 px gutter of four rows
        merged = R.read_columns(det, rec, frames, polys, adj, column_params=dict(min_rows=5), rectified=False)
        assert [len(blk) for blk in merged[0]] == [4] and [len(ks) for _, ks, _ in merged[0][0]] == [6] * 4
        with pytest.raises(TypeError):
            R.read_columns(det, rec, frames, polys, adj, rectified=False, curved=True)
    finally:
        rec.close()
