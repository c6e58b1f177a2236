"""The cases of tests/crop_cases.py on the CPU, against oracle/crop_oracle.py alone (no GPU): every case reaches what it was written for
- counted from the rule's own intermediates -, the counting restatement equals the oracle bit for bit, the oracle stays within a
derived bar of an independent f64 restatement, and the properties that need no second implementation hold (constant frames, ramps,
independent images, permutations, non-finite adjust values).  tests/test_gpu_crops.py then holds the kernel to the oracle bit for bit
on the same cases.

    case                 must reach
    borders              sx / sy clamped at 0 and at W - 1 / H - 1; ix1 == ix0 at the last column, iy1 == iy0 at the last row
    one pixel            the x0 + 1 / y0 + 1 widening; x1 clamped to W after x0 was clamped to W - 1
    outside              both clamps of crop_boxes, at either end
    fractional           boxes that are not f32 numbers; boxes under and over 28 px
    tiny frames          every tap clamped (1 x 1)
    wide and tall        positions in the thousands
    batch                two frames of four used, empty images between them
    counts               1, 255, 256, 257, 1025 boxes
    constant and ramp    the value / 255 bit for bit; monotone along the ramp's axis"""
import numpy as np
import pytest

from oracle import crop_oracle as CR
from tests import crop_cases as CC

NAMES = CC.case_names()
GROUPS = list(dict.fromkeys(CC.group(n) for n in NAMES))
_TRACED = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _traced(name):
    if name not in _TRACED:
        _, fr, polys, adj = CC.case(name)
        _TRACED[name] = CC.extract_crops_traced(fr, polys, adj)
    return _TRACED[name]


def test_the_cases_are_the_issue_s_and_stay_small():
    assert GROUPS == ["borders", "one pixel", "outside", "fractional", "tiny frames", "wide and tall", "batch", "counts", "constant and ramp"]
    shapes = {n: CC.case(n)[1].shape for n in NAMES}
    assert shapes["borders/37x53"] == (1, 1, 37, 53)
    assert [shapes[n][2:] for n in NAMES if CC.group(n) == "tiny frames"] == [(1, 1), (1, 40), (40, 1), (2, 2)]
    assert [shapes[n][2:] for n in NAMES if CC.group(n) == "wide and tall"] == [(8, 2048), (1024, 8)]
    assert [sum(map(len, CC.case(n)[2])) for n in NAMES if CC.group(n) == "counts"] == [1, 255, 256, 257, 1025]
    assert all(shapes[n][2:] == (64, 96) for n in NAMES if CC.group(n) == "counts")
    _, fr, polys, adj = CC.case("batch/4 x 24x32")
    assert fr.shape[0] == 4 and polys[0] == [] and polys[2] == [] and polys[3] == polys[1] and len(polys[1]) > 0
    assert not np.array_equal(fr[1], fr[3]) and not np.array_equal(fr[0], fr[1])
    assert sorted(map(tuple, CC.case("fractional/120x160")[3].tolist())) == sorted([(800 / 300, 533 / 200), (0.37, 1.9), (1.0, 1.0)])
    total = 0
    for n in NAMES:
        _, fr, polys, adj = CC.case(n)
        assert fr.dtype == np.float32 and fr.flags["C_CONTIGUOUS"] and fr.shape[1] == 1 and fr.size <= 1 << 16, n
        assert adj.shape == (fr.shape[0], 2) and adj.dtype == np.float64 and len(polys) == fr.shape[0], n
        assert np.array_equal(fr, np.rint(fr)) and fr.min() >= 0 and fr.max() <= 255, n
        total += sum(map(len, polys))
    assert total < 2500, total


@pytest.mark.parametrize("name", NAMES)
def test_traced_restatement_equals_the_oracle_bit_for_bit(name):
    """... boxes and crops: what the hit counts are read from IS the oracle's computation; no tap leaves the frame"""
    _, fr, polys, adj = CC.case(name)
    n, _, h, w = fr.shape
    want_boxes = CR.crop_boxes(polys, adj, h, w)
    got_boxes = [r["box"] for r in CC.trace_boxes(polys, adj, h, w)]
    assert [(b, *map(lambda v: _bits(v).item(), bx)) for b, *bx in got_boxes] == [(b, *map(lambda v: _bits(v).item(), bx)) for b, *bx in want_boxes]
    crops, hits = _traced(name)
    assert np.array_equal(_bits(crops), _bits(CC.oracle_crops(name)))
    assert hits["taps_outside"] == 0 and not np.isnan(crops).any()
    assert all(0 <= x0 <= w - 1 and x0 + 1 <= x1 <= w and 0 <= y0 <= h - 1 and y0 + 1 <= y1 <= h for _, x0, y0, x1, y1 in want_boxes)


def test_every_case_reaches_what_it_names():
    print()
    keys = [k for k in _traced(NAMES[0])[1]]
    total = {g: dict.fromkeys(keys, 0) for g in GROUPS}
    for n in NAMES:
        for k, v in _traced(n)[1].items():
            total[CC.group(n)][k] += v
    for g in GROUPS:
        print(f"  {g:18s} " + " ".join(f"{k}={v}" for k, v in total[g].items() if v))
    for g in GROUPS:
        for k in CC.REQUIRED[g]:
            assert total[g][k] > 0, (g, k)
    # the rows of the table, each from its own case
    t = _traced("tiny frames/1x1")[1]
    assert t["all_taps_same"] == t["boxes"] and t["ix_same"] == t["iy_same"] == 28 * t["boxes"]      # 1 x 1: every tap is the one pixel
    assert _traced("batch/4 x 24x32")[1]["frames_used"] == 2
    b = _traced("borders/37x53")[1]
    assert b["widened"] == 0 and b["box_low"] == 0 and b["box0_high"] == 0 and b["box1_high"] == 0     # inside the frame: no box clamp acts
    o = _traced("outside/29x41")[1]
    assert o["box_low"] >= 4 and o["box0_high"] >= 4 and o["widened"] >= 4


def test_oracle_within_the_derived_bar_of_the_f64_restatement():
    print()
    worst = (0.0, "")
    for n in NAMES:
        _, fr, polys, adj = CC.case(n)
        boxes = CR.crop_boxes(polys, adj, fr.shape[2], fr.shape[3])
        if not boxes:
            continue
        ref = CC.extract_crops_f64(fr, boxes)
        err = np.abs(CC.oracle_crops(n).astype(np.float64) - ref).max(axis=1)
        bar = np.array([CC.f64_bar(fr[b, 0]) for b, *_ in boxes])
        ratio = float((err / bar).max())
        print(f"  {n:32s} max |oracle - f64| = {err.max():.3e}   bar {bar.max():.3e}   largest error / bar = {ratio:.3f}")
        worst = max(worst, (ratio, n))
        assert (err <= bar).all(), (n, err.max(), bar.max())
    print(f"  largest error / bar over all cases: {worst[0]:.3f} ({worst[1]})")


def test_constant_frames_and_ramps():
    _, fr, polys, adj = CC.case("constant and ramp/constant 137")
    want = np.float32(137.0) / np.float32(255.0)
    got = CC.oracle_crops("constant and ramp/constant 137")
    assert (_bits(got) == _bits(want)).all()
    x = CC.oracle_crops("constant and ramp/v = x").reshape(-1, 28, 28)
    assert (np.diff(x, axis=2) >= 0).all() and (x == x[:, :1, :]).all() and (np.diff(x, axis=2) > 0).any()
    y = CC.oracle_crops("constant and ramp/v = y").reshape(-1, 28, 28)
    assert (np.diff(y, axis=1) >= 0).all() and (y == y[:, :, :1]).all() and (np.diff(y, axis=1) > 0).any()


def test_images_are_independent_and_polygons_permute():
    name = "batch/4 x 24x32"
    _, fr, polys, adj = CC.case(name)
    want = CC.oracle_crops(name)
    k = len(polys[1])
    assert want.shape[0] == 2 * k
    for img, rows in ((1, slice(0, k)), (3, slice(k, 2 * k))):     # each image alone, as a batch of one
        alone = CR.extract_crops(fr[img:img + 1], [polys[img]], adj[img:img + 1])
        assert np.array_equal(_bits(alone), _bits(want[rows])), img
    assert not np.array_equal(want[:k], want[k:])                    # the same polygons on another frame: other crops
    perm = [2, 0, 3, 1]
    got = CR.extract_crops(fr, [[], [polys[1][i] for i in perm], [], polys[3]], adj)
    assert np.array_equal(_bits(got[:k]), _bits(want[:k][perm])) and np.array_equal(_bits(got[k:]), _bits(want[k:]))


def test_non_finite_adjust_values_keep_the_box_inside_the_frame():
    for name, fr, polys, adj, boxes in CC.nonfinite_cases():
        n, _, h, w = fr.shape
        got = CR.crop_boxes(polys, adj, h, w)
        assert [tuple(map(float, b)) for b in got] == [tuple(map(float, b)) for b in boxes], name
        # a NaN takes no part wherever it stands in the vertex list (Python's own min() / max() depend on its place)
        for shift in range(1, 4):
            rolled = [[p[shift:] + p[:shift] for p in polys[0]]]
            assert [tuple(map(float, b)) for b in CR.crop_boxes(rolled, adj, h, w)] == [tuple(map(float, b)) for b in boxes], (name, shift)
        crops = CR.extract_crops(fr, polys, adj)
        assert np.isfinite(crops).all() and crops.min() >= 0 and crops.max() <= 1
    # the sentinel path on a finite adjust value: a vertex at 0 under adj = NaN is NaN too, under adj = inf as well (0 * inf)
    assert CR.crop_boxes([[CC.point(0, 0)]], [[float("inf"), float("inf")]], 5, 7) == [(0, 6.0, 4.0, 7.0, 5.0)]
