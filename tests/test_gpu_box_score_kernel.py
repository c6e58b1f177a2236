"""box_score.hip at kernel level: the rasteriser (scanline fill + Bresenham outline in closed form per pixel, banded LDS mask) and both of
its launches, held to the oracle's draw_polygon on the same map.  Pixel counts EQUAL, f64 sums within 1e-13 relative (the kernel adds in
another order), count == 0 and sum == 0 where the oracle's mask is empty.  The polygons come from tests/box_score_cases.py, which the CPU
test tests/test_box_score_cases.py holds to the oracle; its pinned list makes a contracted FMA, a round-half-even, an f64 intersection
or a moved outline tie fail here on at least 24 polygons each."""
import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from ocr_rs_amd import weights as W
from tests import box_score_cases as BC

pytestmark = pytest.mark.gpu
REL = 1e-13
GRIDS = ("1", "3", "64", "jobs", "jobs+7")
SLACK = 9


@pytest.fixture(scope="module")
def det():
    d = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    yield d
    d.close()


def _pred(shape, seed):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def _hold_to_oracle(pred, polys, got, names=None, want=None):
    """got = (sums, counts, boxes, ...) of the hook for polys on pred (H x W); want: oracle_sum_count per polygon if already known"""
    sums, counts, boxes = got[0], got[1], got[2]
    assert len(sums) == len(counts) == len(boxes) == len(polys)
    for k, p in enumerate(polys):
        ws, wc, wbox = want[k] if want is not None else BC.oracle_sum_count(pred, p)
        tag = (k, names[k] if names else p)
        assert boxes[k] == wbox, tag
        assert counts[k] == wc, (tag, counts[k], wc)
        if wc == 0:
            assert sums[k] == 0.0 and counts[k] == 0.0, tag     # the host turns 0 / 0 into the reference's NaN score
        else:
            assert abs(sums[k] - ws) <= REL * abs(ws), (tag, sums[k], ws)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def fuzz():
    """per fuzz map: (pred, polygons, the oracle's (sum, count, box) of each) - computed once, never changed"""
    cases = BC.fuzz_polys()
    out = []
    for mi, shape in enumerate(BC.FUZZ_MAPS):
        pred = _pred(shape, 40 + mi)
        polys = [p for m, p in cases if m == mi]
        out.append((pred, polys, [BC.oracle_sum_count(pred, p) for p in polys]))
    return out


def test_pinned_rule_sensitive_polygons(det):
    """each on its own map, just large enough: a wrong intersection or tie rule changes at least 24 of these results"""
    assert len(BC.PINNED) >= 24
    for k, p in enumerate(BC.PINNED):
        pred, p = BC.pinned_pred(k), BC.as_poly(p)
        _hold_to_oracle(pred, [p], det.debug_box_scores_batch(pred, [p]))


def test_octants_and_ties(det):
    pred, polys = _pred(BC.OCTANT_MAP, 11), BC.octant_polys()
    _hold_to_oracle(pred, polys, det.debug_box_scores_batch(pred, polys))


def test_scanline_rules(det):
    pred = _pred(BC.SCANLINE_MAP, 12)
    names, polys = zip(*BC.scanline_polys())
    _hold_to_oracle(pred, list(polys), det.debug_box_scores_batch(pred, list(polys)), names=names)


def test_random_fuzz_on_square_and_non_square_maps(det, fuzz):
    tot = {"empty": 0, "clipped": 0, "unclipped": 0}
    for pred, polys, want in fuzz:
        h, w = pred.shape
        _hold_to_oracle(pred, polys, det.debug_box_scores_batch(pred, polys), want=want)
        if h != w:
            for p, (_, c, _) in zip(polys, want):
                tot[BC.clip_class(p, h, w, c)] += 1
    n = sum(tot.values())
    assert sum(len(f[1]) for f in fuzz) >= 1400
    assert tot["clipped"] >= 0.25 * n and tot["unclipped"] >= 0.25 * n and tot["empty"] > 0, tot


def test_many_vertices_up_to_the_limit(det):
    pred = _pred(BC.MANY_MAP, 13)
    polys = [BC.many_vertex_poly(2048), BC.many_vertex_poly(2047)]
    _hold_to_oracle(pred, polys, det.debug_box_scores_batch(pred, polys), names=["2048 points", "2047 points"])
    with pytest.raises(capi.OcrError) as e:
        det.debug_box_scores_batch(pred, [BC.many_vertex_poly(2049)])
    assert e.value.code == 1   # OCR_ERR_INVALID


def test_row_bands(det):
    pred = _pred(BC.BAND_MAP, 14)
    names, polys = zip(*BC.band_polys())
    _hold_to_oracle(pred, list(polys), det.debug_box_scores_batch(pred, list(polys)), names=names)


def test_row_bands_of_narrow_canvases_taller_than_one_band(det):
    pred = _pred(BC.TALL_MAP, 15)
    names, polys = zip(*BC.tall_band_polys())
    _hold_to_oracle(pred, list(polys), det.debug_box_scores_batch(pred, list(polys)), names=names)


@pytest.fixture(scope="module")
def counted_lists(det, fuzz):
    """the job lists of the counted launch with their plain-launch results: each fuzz map with its own polygons, and the 96 x 96 map with
    ALL fuzz polygons (about 1 500 jobs: on a square map any coordinates are allowed)"""
    lists = [(pred, polys) for pred, polys, _ in fuzz]
    lists.append((fuzz[0][0], [p for _, polys, _ in fuzz for p in polys]))
    assert len(lists[-1][1]) >= 1400
    out = []
    for pred, polys in lists:
        plain = det.debug_box_scores_batch(pred, polys, slack=SLACK)
        assert (plain[3] == det.BOX_SCORE_SENTINEL).all() and (plain[4] == det.BOX_SCORE_SENTINEL).all()
        out.append((pred, polys, plain))
    _hold_to_oracle(lists[-1][0], lists[-1][1], out[-1][2])   # the long list is new on this map; the others are held to the oracle above
    return out


@pytest.mark.parametrize("grid", GRIDS)
def test_counted_launch_equals_the_plain_one(det, counted_lists, grid):
    """a fixed grid walking a list whose length is in device memory: workgroups take many jobs each (LDS reused from job to job), or
    none (grid > jobs); bit for bit the plain launch's results, and nothing written behind the count"""
    for pred, polys, plain in counted_lists:
        g = {"jobs": len(polys), "jobs+7": len(polys) + 7}.get(grid) or int(grid)
        got = det.debug_box_scores_batch(pred, polys, grid=g, slack=SLACK)
        assert np.array_equal(_bits(got[0]), _bits(plain[0])) and np.array_equal(_bits(got[1]), _bits(plain[1])), (pred.shape, g)
        assert got[2] == plain[2]
        assert (got[3] == det.BOX_SCORE_SENTINEL).all() and (got[4] == det.BOX_SCORE_SENTINEL).all(), (pred.shape, g)


@pytest.mark.parametrize("grid", [1, 64])
def test_counted_launch_stops_at_the_device_count(det, counted_lists, grid):
    """a device count of 0 writes nothing at all; a count in the middle of the list writes exactly that many results"""
    pred, polys, plain = counted_lists[1]
    for cnt in (0, 1, len(polys) // 2):
        got = det.debug_box_scores_batch(pred, polys, grid=grid, dev_count=cnt, slack=SLACK)
        for a, b, tail in ((got[0], plain[0], got[3]), (got[1], plain[1], got[4])):
            assert np.array_equal(_bits(a[:cnt]), _bits(b[:cnt])), (grid, cnt)
            assert (a[cnt:] == det.BOX_SCORE_SENTINEL).all() and (tail == det.BOX_SCORE_SENTINEL).all(), (grid, cnt)


@pytest.mark.parametrize("grid", [0, 5])
def test_batch_of_non_square_maps(det, fuzz, grid):
    """three 48 x 160 maps with different contents: a polygon scored on image i gives image i's oracle value (pmap = prob + image * H * W)"""
    _, polys, _ = fuzz[1]
    polys = polys[:120]
    preds = np.stack([_pred((48, 160), 60 + i) for i in range(3)])
    jobs = [(p, (k + j) % 3) for k, p in enumerate(polys) for j in range(3)]   # every polygon on every image, the images interleaved
    got = det.debug_box_scores_batch(preds, [p for p, _ in jobs], images=[i for _, i in jobs], grid=grid)
    want = {}
    for k, (p, i) in enumerate(jobs):
        key = (i, tuple(p))
        if key not in want:
            want[key] = BC.oracle_sum_count(preds[i], p)
        _hold_to_oracle(preds[i], [p], tuple(g[k:k + 1] for g in got[:3]), want=[want[key]])
    assert sum(len({got[0][3 * k + j] for j in range(3)}) == 3 for k in range(len(polys))) > len(polys) // 2   # the images really differ
