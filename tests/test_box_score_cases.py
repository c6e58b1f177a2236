"""tests/box_score_cases.py on the CPU: the switchable copy of draw_polygon equals the oracle on every polygon the GPU test uses, the
pinned rule-sensitive polygons really are sensitive (>= 24 changed masks per wrong rule), and the non-square fuzz holds enough clipped
and unclipped polygons.  No GPU."""
import numpy as np
import pytest

from oracle import postproc_oracle as O
from tests import box_score_cases as BC

MIN_PER_RULE = 24


def _same_as_oracle(pts, h, w):
    box, got = BC.mask_on_map(pts, h, w)
    box2, want = BC.mask_on_map(pts, h, w, draw=O.draw_polygon)
    return box == box2 and np.array_equal(got, want)


@pytest.mark.parametrize("name", ["pinned", "octants", "scanline", "fuzz", "many", "bands", "tall"])
def test_switchable_copy_as_specified_is_the_oracle(name):
    if name == "pinned":
        cases = [(BC.pinned_map(p), BC.as_poly(p)) for p in BC.PINNED]
    elif name == "octants":
        cases = [(BC.OCTANT_MAP, p) for p in BC.octant_polys()]
    elif name == "scanline":
        cases = [(BC.SCANLINE_MAP, p) for _, p in BC.scanline_polys()]
    elif name == "fuzz":
        cases = [(BC.FUZZ_MAPS[mi], p) for mi, p in BC.fuzz_polys()]
    elif name == "many":
        cases = [(BC.MANY_MAP, BC.many_vertex_poly(n)) for n in (2047, 2048)]
    elif name == "bands":
        cases = [(BC.BAND_MAP, p) for _, p in BC.band_polys()]
    else:
        cases = [(BC.TALL_MAP, p) for _, p in BC.tall_band_polys()]
    assert cases
    for (h, w), p in cases:
        assert BC.fits(p, h, w), (name, p)
        assert _same_as_oracle(p, h, w), (name, p)


def test_generated_polygons_are_what_they_claim():
    assert len(BC.octant_polys()) >= 2 * (19 * 19 - 1)
    for p in BC.octant_polys():
        assert BC.job_box(p, *BC.OCTANT_MAP) == BC.extent(p)
    assert [len(BC.many_vertex_poly(n)) for n in (2047, 2048, 2049)] == [2047, 2048, 2049]
    x0, y0, bw, bh = BC.extent(BC.many_vertex_poly(2048))
    assert 190 <= bw <= 210 and 30 <= bh <= 50 and bw * bh * 2048 <= 2.2e7
    boxes = {n: BC.job_box(p, *BC.BAND_MAP) for n, p in BC.band_polys()}
    assert sorted(b[2] for b in boxes.values() if b[3] == 1024) == [33, 260, 330, 1024, 1024, 1024]   # canvases of the full height
    assert boxes["bw 97, few points"][2] == 97 and boxes["bw 1"][2] == 1 and boxes["bh 1"][3] == 1
    assert sum(b[2:] == (1, 1) for b in boxes.values()) == 4
    for (n, p), bw in zip(BC.tall_band_polys(), (33, 97)):
        b = BC.job_box(p, *BC.TALL_MAP)
        assert b[2] == bw and b[3] > 8192 // ((bw + 31) // 32), n   # taller than one band


def test_oracle_sum_count_is_box_score_fast():
    rng = np.random.default_rng(3)
    for mi, (h, w) in enumerate(BC.FUZZ_MAPS):
        pred = rng.random((h, w), dtype=np.float32)
        for _, p in [c for c in BC.fuzz_polys() if c[0] == mi][:60]:
            s, c, box = BC.oracle_sum_count(pred, p)
            want = O.box_score_fast(pred, p)
            assert box == BC.job_box(p, h, w)
            assert (c == 0 and s == 0.0 and np.isnan(want)) or s / c == want


def test_every_wrong_rule_changes_at_least_24_pinned_masks():
    """the condition that makes the GPU test fail on a kernel with one of these defects - on every run"""
    changed = {mu: 0 for mu in BC.MUTANTS}
    caught = {mu: 0 for mu in BC.MUTANTS}
    for k, p in enumerate(BC.PINNED):
        p = BC.as_poly(p)
        assert BC.job_box(p, *BC.pinned_map(p)) == BC.extent(p)   # the map is just large enough, and the mask is whole
        ch = BC.mutants_changing(p)
        assert ch, p                                            # nothing listed that no rule needs
        pred = BC.pinned_pred(k)
        s, c, _ = BC.oracle_sum_count(pred, p)
        for mu in ch:
            changed[mu] += 1
            ms, mc = BC.sum_count_under(pred, p, *mu)
            caught[mu] += mc != c or abs(ms - s) > 1e-13 * abs(s)   # what the GPU test asserts, on the map it uses
    print("pinned polygons:", len(BC.PINNED), "masks changed per wrong rule:", changed, "caught by count or sum:", caught)
    assert all(v >= MIN_PER_RULE for v in changed.values()), changed
    assert caught == changed


def test_pinned_list_comes_from_the_seeded_search():
    """the search code stays honest: stopped at one polygon per rule it keeps a subsequence of what the full search keeps (a polygon
    that changes a rule nobody has changed yet is kept whatever the quota), so its result must be found, in order, in the committed list"""
    polys, hits, _ = BC.search_rule_sensitive(per_rule=1, seconds=60.0)
    assert min(hits.values()) >= 1
    at = [BC.PINNED.index(p) for p in polys]
    assert at == sorted(at) and len(set(at)) == len(at)


def test_non_square_fuzz_has_clipped_and_unclipped_polygons():
    """at least a quarter of the polygons on the 48 x 160 and 160 x 48 maps have a non-empty mask on a canvas smaller than their extent,
    at least a quarter an unclipped one; some are wholly outside.  From the oracle alone."""
    fuzz = BC.fuzz_polys()
    assert 1400 <= len(fuzz) <= 1600
    share = {}
    for mi, (h, w) in enumerate(BC.FUZZ_MAPS):
        cls = {"empty": 0, "clipped": 0, "unclipped": 0}
        ps = [p for m, p in fuzz if m == mi]
        for p in ps:
            _, m = BC.mask_on_map(p, h, w, draw=O.draw_polygon)
            cls[BC.clip_class(p, h, w, int(m.sum()))] += 1
        share[(h, w)] = {k: v / len(ps) for k, v in cls.items()}
        print(f"fuzz {h}x{w}: {len(ps)} polygons", cls)
    for hw in ((48, 160), (160, 48)):
        assert share[hw]["clipped"] >= 0.25 and share[hw]["unclipped"] >= 0.25 and share[hw]["empty"] >= 0.05, (hw, share[hw])
