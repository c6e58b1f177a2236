"""candidates.hip alone (dp_kernel, cand_count_kernel, cand_fill_kernel) on the batches of tests/candidates_cases.py, through the raw
hook capi.device_candidates_batch: tot, totals, every job field and every point equal expected_chain() exactly; the words behind
jobs[max_jobs] and pts_xy[2 * max_pts] - and, on a batch that fits, every list word beyond the totals - still hold the poison the hook
wrote.  Integer comparisons, no tolerances; nothing here goes through the product's host fallback, which would hide a chain that gives up
or miscounts.  tests/test_candidates_cases.py shows on the CPU that the cases reach the paths they are named for and that a kernel with
any of the pinned defects (tie rule inside a lane or between lanes, distance to the segment, arc length without its closing segment, a
repeated end point kept) fails the "pinned" group."""
import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from tests import candidates_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def groups():
    return CC.named_groups()


_expected = {}


def _want(c):
    k = c["key"]
    if k not in _expected:   # the fills of one case share its expected values
        _expected[k] = CC.expected_chain(c["images"], c["h"], c["w"], c["max_jobs"], c["max_pts"])
    return _expected[k]


def _check(c):
    name = (c["name"], hex(c["scratch_fill"]))
    e = _want(c)
    mj, mp = c["max_jobs"], c["max_pts"]
    tot, totals, jobs, pts = capi.device_candidates_batch(c["images"], c["h"], c["w"], c["cap"], c["maxc"], mj, mp, c["scratch_fill"], c["guard"], CC.POISON)
    assert jobs.shape == (mj + c["guard"], 7) and pts.shape == (mp + c["guard"], 2)
    assert [tuple(t) for t in tot.tolist()] == e["tot"], name
    assert tuple(totals.tolist()) == e["totals"], name
    assert np.all(jobs[mj:] == CC.POISON_I32), name     # the guard behind jobs[max_jobs]
    assert np.all(pts[mp:] == CC.POISON_I32), name      # the guard behind pts_xy[2 * max_pts]
    if e["totals"][2]:
        return 0
    nj, npt = e["totals"][0], e["totals"][1]
    assert [tuple(j) for j in jobs[:nj].tolist()] == e["jobs"], name
    assert [tuple(p) for p in pts[:npt].tolist()] == e["points"], name
    assert np.all(jobs[nj:] == CC.POISON_I32) and np.all(pts[npt:] == CC.POISON_I32), name   # nothing written beyond the totals
    return nj


@pytest.mark.parametrize("group", CC.GROUPS)
def test_candidates_chain_equals_the_oracle(groups, group):
    cases = groups[group]
    assert cases
    jobs = sum(_check(c) for c in cases)
    assert jobs > 0


def test_the_hook_refuses_what_it_cannot_lay_out():
    sq = CC.square(3, 3)
    ok = dict(h=32, w=32, cap=64, maxc=2, max_jobs=4, max_pts=64)
    tot, totals, _, _ = capi.device_candidates_batch([(0, [sq, sq])], **ok)
    assert tot.tolist() == [[2, 8]] and totals.tolist() == [2, 8, 0]
    with pytest.raises(capi.OcrError):
        capi.device_candidates_batch([(0, [sq, sq, sq])], **ok)                          # nc > maxc
    with pytest.raises(capi.OcrError):
        capi.device_candidates_batch([(0, [sq]), (0, [CC.blob(65, 1)])], **ok)           # an image's points above cap
    with pytest.raises(capi.OcrError):
        capi.device_candidates_batch([(0, [[(0, 0), (65536, 0), (3, 3), (0, 3)]])], **ok)
    with pytest.raises(capi.OcrError):
        capi.device_candidates_batch([(0, [[(0, 0), (5, -1), (3, 3), (0, 3)]])], **ok)
