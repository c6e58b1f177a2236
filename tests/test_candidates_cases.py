"""tests/candidates_cases.py held to the oracle on the CPU: the iterative Douglas-Peucker is O.approximate_polygon_dp, the switchable
copy at its spec settings is the iterative oracle, every observable wrong rule changes at least 8 pinned contours, and the named
cases reach the paths they are named for (ties 64 apart and not, three scan chunks, every group non-empty)."""
import os

import numpy as np
import pytest
from PIL import Image

from oracle import postproc_oracle as O
from tests import candidates_cases as CC
from tests.test_gpu_device_chain import FIXTURES, _box, _oracle_candidates


def _eps(c):
    eps = 0.01 * O.arc_length(c, True)
    return 0.01 if eps == 0.0 else eps


@pytest.fixture(scope="module")
def groups():
    return CC.named_groups()


@pytest.fixture(scope="module")
def contours():
    return CC.all_contours()


@pytest.fixture(scope="module")
def fixture_contours(golden_dir):
    out = {}
    for name in FIXTURES:
        bm = (np.array(Image.open(os.path.join(golden_dir, name)).convert("L")) > 0).astype(np.uint8)
        out[name] = (bm.shape, [[(int(x), int(y)) for x, y in c] for c in O.find_contours(bm * 255)])
    return out


def test_iterative_douglas_peucker_is_the_oracles(contours, fixture_contours):
    """kept indices of dp_indices == the points of O.approximate_polygon_dp, closed and open, on every contour of at most 4000 points
    of every named case and of PINNED, and on the contours of the four reference fixtures"""
    cs = [c for c in contours if 1 <= len(c) <= 4000] + [c for _, v in fixture_contours.values() for c in v]
    assert len(cs) > 300 and max(len(c) for c in cs) == 2080
    for c in cs:
        eps = _eps(c)
        idx = CC.dp_indices(c, eps)
        assert idx == sorted(idx) and (len(c) == 1 or len(set(idx)) == len(idx))
        assert [tuple(c[i]) for i in idx] == [tuple(p) for p in O.approximate_polygon_dp(c, eps, False)]
        assert [tuple(c[i]) for i in idx[:-1]] == [tuple(p) for p in O.approximate_polygon_dp(c, eps, True)]
    for c in cs:
        if len(c) >= 4:
            assert ([CC.candidate(c)] if CC.candidate(c) else []) == _oracle_candidates([c])


def test_switchable_copy_at_spec_is_the_iterative_oracle(contours):
    """... on every contour, the 32768-point ones included"""
    assert max(len(c) for c in contours) == CC.K_KEEP_CAP + 1
    for c in contours:
        assert CC.candidate_rules(c) == CC.candidate(c)


def test_every_observable_mutant_changes_at_least_8_pinned_contours():
    pinned = [CC.expand(p) for p in CC.PINNED]
    assert all(CC.compress(c) == p for c, p in zip(pinned, CC.PINNED))
    assert all(0 <= x < 512 and 0 <= y < 512 for c in pinned for x, y in c)
    hits = {mu: 0 for mu in CC.MUTANTS}
    for c in pinned:
        ch = CC.mutants_changing(c)
        assert ch, "a pinned contour no mutant changes"
        for mu in ch:
            hits[mu] += 1
    assert len(CC.MUTANTS) == 7 and set(CC.EQUIVALENT_MUTANTS) == {("eps0", "zero")}
    for mu in CC.MUTANTS:
        if mu not in CC.EQUIVALENT_MUTANTS:
            assert hits[mu] >= 8, (mu, hits)
    # the tie rules are pinned across strides and across lanes: contours longer than 128 points where "lane" differs from "last"
    long_ties = [c for c in pinned if len(c) > 128 and CC.candidate_rules(c, tie="lane") != CC.candidate_rules(c)]
    assert len(long_ties) >= 8


def test_the_epsilon_substitution_cannot_be_observed(contours):
    """eps0 = "zero" changes no contour at all (the module docstring says why); the all-identical contours do reach the substitution"""
    zero = [c for c in contours if len(c) >= 4 and O.arc_length(c, True) == 0.0]
    assert sorted(len(c) for c in zero) == [4, 70]
    for c in contours + [CC.expand(p) for p in CC.PINNED]:
        assert CC.candidate_rules(c, eps0="zero") == CC.candidate_rules(c)


def test_pinned_reproduces_from_its_seed():
    cs, hits, _, most = CC.search_rule_sensitive()
    assert tuple(CC.compress(c) for c in cs) == CC.PINNED
    assert min(hits.values()) >= 8 and most == 14


def test_every_named_group_is_there(groups):
    assert tuple(groups) == CC.GROUPS
    for g, cases in groups.items():
        assert cases, g
        fills = {c["scratch_fill"] for c in cases}
        assert fills == ({0x00, 0xA5, 0xFF} if g == "batches" else {0x00, 0xA5}), g
        for c in cases:
            tots = [sum(len(q) for q in cs) for _, cs in c["images"]]
            assert c["cap"] >= max(64, max(tots)) and c["maxc"] >= max(len(cs) for _, cs in c["images"])
            assert all(0 <= x <= 65535 and 0 <= y <= 65535 for _, cs in c["images"] for q in cs for x, y in q)
    lens = [[len(q) for q in c["images"][0][1]] for c in groups["lengths"]]
    assert all(tuple(v) == CC.LENGTHS for v in lens)
    e = [CC.expected_chain(c["images"], c["h"], c["w"], c["max_jobs"], c["max_pts"]) for c in groups["lengths"][::2]]
    assert all(x["totals"][0] >= 14 for x in e)          # most lengths give a candidate (none below 5 points can)
    assert e[0]["points"] != e[1]["points"]              # the rotated contours start elsewhere
    assert any(j[3:] != CC.job_box(x["points"][j[1]:j[1] + j[2]], 1 << 16, 1 << 16) for x in e for j in x["jobs"])   # the clamp by H does something
    assert [len(c["images"][0][1][0]) for c in groups["long"][:-2:2]] == list(CC.LONG_LENGTHS)
    e = CC.expected_chain(groups["long"][-1]["images"], 16384, 16384, 99, 9999)
    assert e["tot"][1] == (-1, -1) and e["tot"][0][0] == 2 and e["tot"][2][0] == 1 and e["totals"][0] == 3
    for c in groups["long"][:-2:2]:
        assert CC.expected_chain(c["images"], c["h"], c["w"], 9, 999)["totals"][0] == 1, c["name"]


def test_tie_cases_repeat_the_maximum_across_strides_and_across_lanes(groups):
    """per rectangle with a side above 64 points: a decisive scan whose maximum is attained again 64 k further on (one lane, a later
    stride), and one whose maximum is attained again elsewhere (another lane)"""
    cases = [c for c in groups["ties"] if c["scratch_fill"] == 0]
    rects = [c for c in cases if c["name"].startswith("rectangle")]
    assert len(rects) == len(CC.RECTS)
    for c in rects:
        cs = c["images"][0][1]
        assert len(cs) == 5 and len({tuple(q[0]) for q in cs}) == 5 and len({tuple(sorted(q)) for q in cs}) == 1
        same_lane = other_lane = 0
        for q in cs:
            st = []
            assert CC.candidate_rules(q, stats=st) is not None
            same_lane += sum(1 for s in st if s[0] != "kept" and s[3])
            other_lane += sum(1 for s in st if s[0] != "kept" and s[4])
        assert same_lane >= 1 and other_lane >= 1, c["name"]
    line = [c for c in cases if c["name"].startswith("line")][0]["images"][0][1]
    assert len(line[0]) == 298 and all(CC.candidate(q) is None for q in line)
    # a wrong tie rule inside a lane or between lanes changes a job of this group (>= everywhere only swaps a side's two corners)
    for tie in ("stride", "lane"):
        assert any(CC.candidate_rules(q, tie=tie) != CC.candidate(q) for c in cases for q in c["images"][0][1]), tie


def test_degenerate_cases_reach_their_paths(groups):
    cs = groups["degenerate"][0]["images"][0][1]
    same4, same70, closed, inner, repeat, tri, quad, tri2, quad2 = cs[:9]
    assert len(set(same4)) == 1 and len(set(same70)) == 1 and CC.candidate(same4) is None and CC.candidate(same70) is None
    assert closed[0] == closed[-1] and CC.candidate(closed) is None          # every distance of the first range is NaN
    assert inner[20] == inner[0] and inner[0] in CC.candidate(inner)[1:]      # P[0]'s twin is kept: ranges with coinciding ends below it
    assert [len(q) for q in [repeat] + cs[9:]] == list(CC.REPEAT_LENGTHS)
    for q in [repeat] + cs[9:]:      # the repeated end point is kept by Douglas-Peucker and dropped behind it: one point fewer than with "keep_repeat"
        assert q[-2] == q[0] and len(CC.candidate_rules(q, close="keep_repeat")) == len(CC.candidate(q)) + 1, len(q)
    for t, q in ((tri, quad), (tri2, quad2)):
        st = []
        assert CC.candidate_rules(t, stats=st) is None and st[-1] == ("kept", 3)
        assert len(CC.candidate(q)) == 4


def test_striding_cases_fill_three_scan_chunks(groups):
    """700 contours: candidates in all three chunks of 256, non-candidates on both sides of the chunk borders"""
    by_nc = {}
    for c in groups["striding"]:
        if c["scratch_fill"] == 0:
            by_nc.setdefault(len(c["images"][0][1]), set()).add(c["maxc"])
    assert by_nc == {nc: {nc, 4096} for nc in CC.STRIDE_NCS}
    has = [CC.candidate(q) is not None for q in CC.stride_contours(700)]
    for lo in (0, 256, 512):
        assert any(has[lo:lo + 256]) and not all(has[lo:lo + 256])
    for border in (256, 512):
        assert not all(has[border - 3:border]) and not all(has[border:border + 3])
    kinds = {len(q) for q, h in zip(CC.stride_contours(700), has) if not h}
    assert kinds == {3, 6}                                                  # too short, and collapsing


def test_batches_cover_the_second_stride_of_the_prefix_and_every_status_pattern(groups):
    ns = {len(c["images"]) for c in groups["batches"]}
    assert ns == set(CC.BATCH_NS)
    names = {c["name"] for c in groups["batches"]}
    for k in (255, 256, 257):
        assert f"300 images, given up at {k}" in names
    assert "257 images, given up at 256" in names and "257 images, given up last" in names
    for c in groups["batches"] + groups["batches_empty"]:
        if c["scratch_fill"] != 0:
            continue
        e = CC.expected_chain(c["images"], c["h"], c["w"], c["max_jobs"], c["max_pts"])
        live = [t for t in e["tot"] if t[0] > 0]
        assert e["totals"] == (sum(t[0] for t in live), sum(t[1] for t in live), 0) and live
        if "given up last" in c["name"]:
            assert e["tot"][-1] == (-1, -1) and e["totals"][0] > 0
    zero = [c for c in groups["batches_empty"] if "all collapse" in c["name"] or "no contours" in c["name"]]
    for where, pos in (("first", 0), ("last", -1)):
        assert any(CC.expected_chain(c["images"], 64, 48, 1 << 20, 1 << 20)["tot"][pos] == (0, 0) for c in zero if where in c["name"])


def test_capacity_cases_sit_on_both_sides_of_the_limits(groups):
    cases = [c for c in groups["capacities"] if c["scratch_fill"] == 0]
    full = CC.expected_chain(cases[0]["images"], 64, 48, 1 << 20, 1 << 20)
    J, P = full["totals"][:2]
    want = {(J, P): 0, (J + 3, P + 3): 0, (J - 1, P): 1, (J, P - 1): 1, (0, P): 1, (J, 0): 1}
    got = {(c["max_jobs"], c["max_pts"]): CC.expected_chain(c["images"], 64, 48, c["max_jobs"], c["max_pts"])["totals"] for c in cases}
    for k, over in want.items():
        assert got[k] == ((0, 0, 1) if over else (J, P, 0)), k
    assert all(c["guard"] == 4096 for c in cases)


def test_expected_chain_is_the_single_image_oracle(fixture_contours):
    """expected_chain == _oracle_candidates + _box of tests/test_gpu_device_chain.py on single-image maps: the four reference fixtures,
    noise (wide and tall: the clamp acts), rings and lines"""
    rng = np.random.default_rng(17)
    maps = [(shape, cs) for shape, cs in fixture_contours.values()]
    for h, w, p in ((96, 96, 0.5), (128, 160, 0.35), (64, 224, 0.65), (224, 64, 0.6)):
        bm = (rng.random((h, w)) < p).astype(np.uint8)
        maps.append(((h, w), [[(int(x), int(y)) for x, y in c] for c in O.find_contours(bm * 255)]))
    ring = np.zeros((96, 128), np.uint8)
    ring[10:40, 10:50] = 1; ring[11:39, 11:49] = 0; ring[50:90, 20:100] = 1; ring[55:85, 25:95] = 0; ring[5, 60:120] = 1; ring[5:45, 120] = 1
    maps.append(((96, 128), [[(int(x), int(y)) for x, y in c] for c in O.find_contours(ring * 255)]))
    total = 0
    for (h, w), cs in maps:
        want = _oracle_candidates(cs)
        e = CC.expected_chain([(0, cs)], h, w, len(cs), sum(len(c) for c in cs))
        assert e["tot"] == [(len(want), sum(len(p) for p in want))] and e["totals"] == (len(want), sum(len(p) for p in want), 0)
        assert [e["points"][j[1]:j[1] + j[2]] for j in e["jobs"]] == want
        assert [j[3:] for j in e["jobs"]] == [_box(p, h, w) for p in want] and all(j[0] == 0 for j in e["jobs"])
        total += len(want)
    assert total > 100
