"""Line grouping on the MI355X (ocr_group_lines, csrc/lines.hip) against tests/line_oracle.py: order, line_offsets, img_offsets and
word_flags equal, gaps bit-equal (compared as uint64), on every hand case of tests/test_line_oracle.py, seeded fuzz at the sizes
where the kernels change path (one word, the wave and block sizes, more than one LDS tile, the 4 096-word cap), integer-grid fuzz
that really has ties, pages that must not see their batch neighbours, non-default parameters, every OCR_ERR_INVALID case, and
read_lines composed over the real reading chain."""
import ctypes as C

import numpy as np
import pytest

from tests import line_oracle as LO
from tests.test_line_oracle import cases

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


def _check(det, quads, offsets, params=None):
    """the device result of one batch against the oracle; returns the oracle's result"""
    want = LO.group(quads, offsets, params)
    got = det.group_lines(quads, offsets, params)
    assert got.img_offsets.tolist() == want["img_offsets"].tolist()
    assert got.line_offsets.tolist() == want["line_offsets"].tolist()
    assert got.order.tolist() == want["order"].tolist()
    assert got.word_flags.tolist() == want["word_flags"].tolist()
    assert got.gaps.dtype == np.float64 and np.array_equal(got.gaps.view(np.uint64), want["gaps"].view(np.uint64))
    return want


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_cases_equal_the_oracle(det, name):
    _check(det, *CASES[name])


def _fuzz_with_rings(n, seed, grid=False):
    """LO.fuzz, and from 64 words on two rings beside the page (a seal of 24 words and one of 16): cycles that no other word disturbs"""
    q = LO.fuzz(n, seed, grid)
    if n >= 64:
        span = float(np.abs(q).max())
        q[7:31] = LO.ring(24, 150.0, (span + 400.0, 300.0))
        q[40:56] = LO.ring(16, 80.0, (span + 400.0, 700.0), w=20.0)[::-1]     # (the smallest index is not the first word clockwise)
    return q


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025, 4096])
def test_fuzz_at_the_sizes_where_the_kernels_change_path(det, n):
    want = _check(det, _fuzz_with_rings(n, seed=100 + n), [0, n])
    if n >= 64:
        assert (want["word_flags"] == 2).sum() >= 2                       # both rings were cut (and whatever cycles the page has)
        assert len(want["line_offsets"]) - 1 < n                           # ... and the page has links
    if n == 1:
        assert want["order"].tolist() == [0] and want["line_offsets"].tolist() == [0, 1]


@pytest.mark.parametrize("n,seed", [(257, 11), (1025, 12)])
def test_integer_grid_fuzz_exercises_the_tie_breaks(det, n, seed):
    want = _check(det, _fuzz_with_rings(n, seed, grid=True), [0, n])
    assert want["ties"] > 0, "no two equal projections in the oracle's run: the case would pass vacuously"


def test_a_page_does_not_see_its_batch_neighbours(det):
    page = LO.page(5, 7, 0.2, seed=31)[0]
    others = [_fuzz_with_rings(257, seed=32), LO.ring(), LO.fuzz(90, seed=33) + 1000.0, np.zeros((0, 8))]
    alone = det.group_lines(page, [0, len(page)])
    assert alone.n_lines == 5
    for at in range(3):
        batch = [others[(at + k) % 4] for k in range(3)]
        batch.insert(at, page)
        off = np.concatenate([[0], np.cumsum([len(b) for b in batch])])
        got = det.group_lines(np.concatenate(batch), off)
        _check(det, np.concatenate(batch), off)
        w0, w1 = int(off[at]), int(off[at + 1])
        l0, l1 = int(got.img_offsets[at]), int(got.img_offsets[at + 1])
        assert (got.order[w0:w1] - w0).tolist() == alone.order.tolist()
        assert (got.line_offsets[l0:l1 + 1] - w0).tolist() == alone.line_offsets.tolist()
        assert got.word_flags[w0:w1].tolist() == alone.word_flags.tolist()
        assert np.array_equal(got.gaps[w0:w1].view(np.uint64), alone.gaps.view(np.uint64))


@pytest.mark.parametrize("params", [dict(line_tol=0.05), dict(line_tol=4.0), dict(height_ratio=1.0), dict(height_ratio=16.0),
                                    dict(min_cos=0.0), dict(min_cos=1.0), dict(max_gap=0.0), dict(max_gap=64.0)],
                         ids=lambda p: "%s=%g" % next(iter(p.items())))
def test_non_default_parameters_one_at_a_time(det, params):
    q = _fuzz_with_rings(300, seed=41)
    base = LO.group(q, [0, 300])
    want = _check(det, q, [0, 300], params)
    assert want["order"].tolist() != base["order"].tolist() or want["line_offsets"].tolist() != base["line_offsets"].tolist()


def test_every_invalid_call_is_refused_and_the_handle_stays_usable(det):
    from ocr_rs_amd import capi
    L = capi.lib()
    q, off = CASES["two_lines"]
    q = np.ascontiguousarray(q, np.float64)
    off32 = np.array(off, np.int32)
    out = C.POINTER(capi.LinesBlock)()

    def raw(h, qp, op, n, prm, outp):
        return L.ocr_group_lines(h, qp, op, n, prm, outp)
    ok = lambda: _check(det, q, off)
    ok()
    for args in [(None, q.ctypes.data, off32.ctypes.data, 1, None, C.byref(out)),          # null handle
                 (det._h, None, off32.ctypes.data, 1, None, C.byref(out)),                 # null quads with words
                 (det._h, q.ctypes.data, None, 1, None, C.byref(out)),                     # null offsets
                 (det._h, q.ctypes.data, off32.ctypes.data, 1, None, None),                # null out
                 (det._h, q.ctypes.data, off32.ctypes.data, 0, None, C.byref(out)),        # n_images < 1
                 (det._h, q.ctypes.data, off32.ctypes.data, -3, None, C.byref(out))]:
        assert raw(*args) == 1, args
        ok()

    def refused(quads, offsets, params=None):
        with pytest.raises(capi.OcrError) as e:
            det.group_lines(quads, offsets, params)
        assert e.value.code == 1, e.value
        ok()
    refused(q, [1, 6])                                   # offsets do not start at 0
    refused(np.concatenate([q, q]), [0, 6, 4, 12])       # offsets decrease
    for field, bad in [("line_tol", 0.0), ("line_tol", 4.5), ("line_tol", float("nan")), ("height_ratio", 0.99), ("height_ratio", 16.5),
                       ("min_cos", -0.01), ("min_cos", 1.01), ("max_gap", -1.0), ("max_gap", 64.5), ("max_gap", float("inf"))]:
        refused(q, off, {field: bad})
    refused(q, off, {"reserved": (0, 1)})
    refused(q, off, {"reserved": (1, 0)})
    for bad in (np.nan, np.inf, -np.inf):
        qq = q.copy()
        qq[4, 5] = bad
        refused(qq, off)
    # one word over the cap in the second image: refused on the host, nothing is launched; exactly the cap is taken
    big = np.tile(np.array(LO.quad(50, 50, 40, 16)), (4097 + 6, 1))
    refused(big, [0, 6, 6 + 4097])
    assert det.group_lines(big[:4096 + 6], [0, 6, 6 + 4096]).n_lines == 6 + 4096      # (coinciding words: nobody is right of anybody)


def _tilted_page(rows, cols, angle, h, w):
    """a frame of striped dark words on a light page turned by `angle`, and their quads as integer polygons in shuffled order"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    frame = np.full((h, w), 215.0)
    c, s = np.cos(angle), np.sin(angle)
    polys, where = [], []
    for r in range(rows):
        for k in range(cols):
            x, y = (k - (cols - 1) / 2) * 62.0, (r - (rows - 1) / 2) * 44.0
            cx, cy = w / 2 + x * c - y * s, h / 2 + x * s + y * c
            lx, ly = (xx + 0.5 - cx) * c + (yy + 0.5 - cy) * s, -(xx + 0.5 - cx) * s + (yy + 0.5 - cy) * c
            inside = (np.abs(lx) < 20) & (np.abs(ly) < 8) & (np.floor((lx + 20) / 5) % 2 == 0)
            frame[inside] = 35.0
            polys.append([(int(round(px)), int(round(py))) for px, py in np.reshape(LO.quad(cx, cy, 46, 22, angle), (4, 2))])
            where.append((r, k))
    perm = np.random.default_rng(5).permutation(len(polys))
    return frame.astype(np.float32), [polys[i] for i in perm], [where[i] for i in perm]


def test_read_lines_on_a_tilted_page(det):
    import torch
    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    try:
        f0, p0, w0 = _tilted_page(4, 5, 0.25, 320, 400)
        f1, p1, w1 = _tilted_page(3, 4, -0.3, 320, 400)
        frames = np.stack([f0, f1, np.full((320, 400), 200.0, np.float32)])[:, None]
        polys, adj = [p0, p1, []], [[1.0, 1.0]] * 3
        words = reading.read_words_rectified(det, rec, frames, polys, adj, cc={})
        lines = reading.read_lines(det, rec, frames, polys, adj, cc={})
        assert len(lines) == 3 and lines[2] == [] and reading.page_text(lines[2]) == ""
        for b, (where, rows, cols) in enumerate([(w0, 4, 5), (w1, 3, 4)]):
            idx = [int(k) for _, ks, _ in lines[b] for k in ks]
            assert sorted(idx) == list(range(rows * cols))                                   # a permutation of the polygons
            # the rows top to bottom, each left to right
            assert [[where[int(k)] for k in ks] for _, ks, _ in lines[b]] == [[(r, k) for k in range(cols)] for r in range(rows)]
            for text, ks, gaps in lines[b]:
                assert text == " ".join(t for t in (words[b][int(k)][0] for k in ks) if t)
                assert ks.dtype == np.int32 and gaps[0] == 0.0 and np.all(gaps[1:] > 0) and len(gaps) == len(ks)
            assert reading.page_text(lines[b]) == "\n".join(t for t, _, _ in lines[b]) and reading.page_text(lines[b]).count("\n") == rows - 1
            assert any(t for t, _, _ in lines[b])
        # the same through the unrectified reader and device frames, with non-default line parameters through to the call
        plain = reading.read_lines(det, rec, torch.from_numpy(frames).cuda(), polys, adj, rectified=False)
        assert [[ks.tolist() for _, ks, _ in pg] for pg in plain] == [[ks.tolist() for _, ks, _ in pg] for pg in lines]
        tight = reading.read_lines(det, rec, frames, polys, adj, line_params=dict(max_gap=0.0))
        assert [len(pg) for pg in tight] == [20, 12, 0]
        with pytest.raises(TypeError):
            reading.read_lines(det, rec, frames, polys, adj, rectified=False, curved=True)
    finally:
        rec.close()
