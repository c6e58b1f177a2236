"""The split oracle (tests/glyph_split_oracle.py) on its drawn frames, with every expected number written out by hand, and the fuzz
generators' coverage.  Then a numpy model of split_kernel as written (csrc/glyph_split.hip: lanes that step over columns by 64, the
packed key, butterfly reductions) held to the oracle on every case, six wrong variants of it that the wide cases must tell from the
oracle (and four of which the narrow fuzz cannot), and the reach() counters of the wide fuzz.  No GPU."""
import functools

import numpy as np
import pytest

from tests import glyph_cc_oracle as GC
from tests import glyph_oracle as GO
from tests import glyph_split_oracle as SO

CASES = {c[0]: c for c in SO.drawn_cases()}
WIDE = {c[0]: c for c in SO.wide_drawn_cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_drawn_case(name):
    _, frames, blk, prm, want, bits = CASES[name]
    got = SO.split(frames, blk, prm)
    assert got["boxes"].tolist() == want and got["word_info"][:, 3].tolist() == bits
    assert np.array_equal(got["word_info"][:, :3], blk["word_info"][:, :3]) and np.array_equal(got["img_offsets"], blk["img_offsets"])
    assert got["word_offsets"][-1] == len(want) == len(got["map"])


def test_the_bridge_is_one_component_and_is_cut_at_column_13():
    _, frames, blk, _, want, _ = CASES["bridge"]
    cc = GC.segment_cc(frames, [[[(0, 0), (39, 23)]]], np.ones((1, 2)))
    assert cc["boxes"].tolist() == blk["boxes"].tolist() == [[4, 6, 22, 18]] and cc["word_info"][0, 2] == 1
    got = SO.split(frames, cc)
    assert got["boxes"].tolist() == want and got["boxes"][0, 2] == 13 and got["map"].tolist() == [[0, 0], [0, 1]]
    # the tie rule: all five columns of the window [11, 15] hold one ink pixel; the distance to c = 13 decides, then the smaller x
    assert SO.cuts_of(np.ones(18, np.int64), 4, 22, 2) == [13]
    cnt = np.ones(18, np.int64)
    cnt[13 - 4] = 2
    assert SO.cuts_of(cnt, 4, 22, 2) == [12]   # 12 and 14 tie in count and distance: the smaller x


def test_pass_through_and_asked_counts():
    _, frames, blk, prm, _, _ = CASES["clip"]
    got = SO.split(frames, blk, prm)
    assert got["asked"].tolist() == [4, 1]
    assert SO.split(frames, blk, dict(aspect_pct=25, max_pieces=1))["boxes"].tolist() == blk["boxes"].tolist()


def test_window_clamps_of_the_rule():
    """With min_piece_w >= 3 no window reaches x0 + 1 or x1 - 1 (c_1 - r >= x0 + 2, c_(n-1) + r <= x1 - 2), so the clamps cannot be met
    through the call; cuts_of applies them all the same, and this holds them on widths the call never passes."""
    assert SO.cuts_of(np.array([0, 5, 1]), 10, 13, 2) == [12]    # c = 11, r = 1: [10, 12] clipped to [11, 12]
    assert SO.cuts_of(np.array([5, 1]), 10, 12, 2) == [11]       # c = 11, r = 1: [10, 12] clipped to [11, 11]
    for gw in range(3, 200):
        for n in range(2, min(4, gw // 3) + 1):
            r = max(1, gw // (4 * n))
            assert (gw // n) - r >= 2 and ((n - 1) * gw) // n + r <= gw - 2


@functools.lru_cache(maxsize=None)
def _narrow():
    """the narrow fuzz and its two input blocks (column rule, component rule)"""
    frames, polys, adj = SO.fuzz_case()
    return frames, GO.segment(frames, polys, adj, dict(polarity=1)), GC.segment_cc(frames, polys, adj, dict(polarity=1))


NARROW_PARAMS = (dict(max_pieces=1), dict(max_pieces=2), dict(max_pieces=3), dict(max_pieces=4),
                 dict(max_pieces=4, max_word_pieces=2, aspect_pct=50, min_piece_w=4))     # the sets of tests/test_gpu_glyph_split.py


def test_the_fuzz_generator_covers_every_piece_count():
    frames, col, cc = _narrow()
    assert len(col["word_offsets"]) - 1 == 64 and frames.shape == (2, 1, 96, 160)
    widths = np.concatenate([b["boxes"][:, 2] - b["boxes"][:, 0] for b in (col, cc)])
    assert widths.min() <= 3 and widths.max() == 60
    for blk in (col, cc):
        asked = SO.split(frames, blk, dict(max_pieces=4))["asked"]
        assert set(asked.tolist()) == {1, 2, 3, 4}
    assert SO.split(frames, col, dict(max_pieces=1))["boxes"].tolist() == col["boxes"].tolist()


def test_what_the_narrow_fuzz_does_not_reach():
    """Why the wide cases exist: at widths up to 60 no window and no piece has 64 columns, nothing is dropped; ties in the count it has."""
    frames, col, cc = _narrow()
    ties = 0
    for blk in (col, cc):
        for prm in NARROW_PARAMS:
            r = SO.reach(frames, blk, prm)
            assert [r[k] for k in ("win_gt64", "cut_ge64", "piece_gt64", "dropped", "far_rows")] == [0] * 5, (prm, r)
            ties += r["count_ties"]
    assert ties > 0
    assert set(col["word_info"][:, 2].tolist()) | set(cc["word_info"][:, 2].tolist()) == {1}


# ---- the wide cases ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(WIDE))
def test_wide_drawn_case(name):
    _, frames, blk, prm, want, bits = WIDE[name]
    got = SO.split(frames, blk, prm)
    assert got["boxes"].tolist() == want and got["word_info"][:, 3].tolist() == bits
    assert set(blk["word_info"][:, 2].tolist()) == {int(name[-1])}                  # the polarity its name says
    assert got["word_offsets"][-1] == len(want) == len(got["map"])


def test_wide_drawn_cases_come_in_both_polarities_and_reach_past_a_wave():
    assert len(WIDE) == 14 and {n[:-3] for n in WIDE} == {"far_min", "far_tie", "far_rows", "far_only", "far_only3", "at_threshold", "tall_wide"}
    for name in WIDE:
        if name.startswith("at_threshold"):
            continue
        a, b = WIDE[name[:-1] + "1"], WIDE[name[:-1] + "2"]
        assert np.array_equal(a[1] + b[1], np.full_like(a[1], SO.PAPER + SO.INK)) and a[4] == b[4]      # the same drawing, inverted
    r = {n: SO.reach(c[1], c[2], c[3]) for n, c in WIDE.items()}
    for pol in "12":
        assert r["far_min-p" + pol]["cut_ge128"] == 1 and r["tall_wide-p" + pol]["cut_ge128"] == 1
        assert r["far_tie-p" + pol]["dist_ties"] == 1 and r["far_tie-p" + pol]["count_ties"] == 2
        assert r["far_rows-p" + pol]["far_rows"] == 1 and r["far_only-p" + pol]["far_rows"] == 1
        assert r["far_only3-p" + pol]["dropped"] == 1 and r["far_only3-p" + pol]["asked"] == {3: 1}
    f1, f2 = WIDE["at_threshold-p1"][1], WIDE["at_threshold-p2"][1]
    at = (f1 >= 120) & (f1 <= 121)
    assert at.sum() == 10 and np.array_equal(f1[at], f2[at]) and sorted(set(GO.quantise(f1[at]).tolist())) == [120, 121]
    f = WIDE["tall_wide-p1"][1]
    assert int((GO.quantise(f[0, 0, 3:1003]) <= SO.T_HAND).sum(axis=0).max()) == 1000                      # four digits in the key


@functools.lru_cache(maxsize=None)
def _wide(pol):
    return SO.wide_fuzz_case(polarity=pol)


@functools.lru_cache(maxsize=None)
def _wide_want(pol, i):
    frames, blk = _wide(pol)
    return SO.split(frames, blk, SO.WIDE_PARAMS[i])


def test_the_wide_fuzz_is_what_it_says():
    for pol in (1, 2):
        frames, blk = _wide(pol)
        assert frames.shape == (2, 1, SO.WIDE_H, SO.WIDE_W) and SO.WIDE_W % 2 == 1 and frames.dtype == np.float32
        b = blk["boxes"]
        assert b[:, 0].min() == 0 and b[:, 1].min() == 0 and b[:, 2].max() == SO.WIDE_W and b[:, 3].max() == SO.WIDE_H
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 0).all() and (b[:, 0] < b[:, 2]).all() and (b[:, 1] < b[:, 3]).all()
        w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        assert {3, 65, 129, 257, 513, SO.WIDE_W} <= set(w.tolist()) and h.min() == 3 and h.max() == 6
        assert set(blk["word_info"][:, 2].tolist()) == {pol} and set(blk["word_info"][:, 0].tolist()) == {0, 1}
        per_word = np.diff(blk["word_offsets"])
        assert per_word.min() == 1 and per_word.max() >= 6
        # hw comes from a neighbour: a glyph lower than its word's tallest
        hw = np.repeat([h[a:e].max() for a, e in zip(blk["word_offsets"][:-1], blk["word_offsets"][1:])], per_word)
        assert (h < hw).sum() >= 10
        q = GO.quantise(frames)
        ink = (q <= SO.T_HAND) if pol == 1 else (q > SO.T_HAND)
        assert 0.08 < ink.mean() < 0.16 and (q == SO.T_HAND).any()
        # waves that return at once beside waves that cut, inside one workgroup of four glyphs; and max_word_pieces on both sides
        for i, prm in enumerate(SO.WIDE_PARAMS):
            asked = _wide_want(pol, i)["asked"]
            if prm["max_pieces"] > 1:
                groups = [set((asked[a:a + 4] > 1).tolist()) for a in range(0, len(asked), 4)]
                assert sum(g == {False, True} for g in groups) >= 4
        bit4 = _wide_want(pol, len(SO.WIDE_PARAMS) - 1)["word_info"][:, 3] & 4
        assert "max_word_pieces" in SO.WIDE_PARAMS[-1] and bit4.any() and not bit4.all() and (bit4[per_word > 1] == 0).any()


def test_reach_of_the_wide_fuzz():
    """Every counter is met in each polarity over the parameter sets the GPU test runs, and a cut at window index >= 128 at max_pieces 2."""
    for pol in (1, 2):
        frames, blk = _wide(pol)
        total = None
        for prm in SO.WIDE_PARAMS:
            r = SO.reach(frames, blk, prm)
            if prm == dict(max_pieces=2):
                assert r["cut_ge128"] >= 1 and r["win_gt128"] >= 1
            if prm["max_pieces"] == 1:
                assert r["asked"] == {1: len(blk["boxes"])} and all(r[k] == 0 for k in SO.REACH_KEYS)
            total = r if total is None else SO.add_reach(total, r)
        assert all(total[k] >= 1 for k in SO.REACH_KEYS), total
        assert set(total["asked"]) == {1, 2, 3, 4} and all(v >= 1 for v in total["asked"].values())


# ---- split_kernel as written, in numpy ---------------------------------------------------------------------------------------------

LANES = np.arange(64)
WRONG = ("window_first_64",    # 1  the window scan stops after its first 64 columns
         "rows_first_64",      # 2  a piece's rows come from its first 64 columns only
         "lane_keeps_last",    # 3  a lane keeps the last column of its stride, not its smallest key
         "pol2_ge",            # 4  polarity 2 inks q >= t
         "no_distance",        # 5  the key leaves |x - c| out
         "larger_x")           # 6  a tie in count and distance goes to the larger x


def _butterfly(v, op):
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v, v[LANES ^ o])
    assert (v == v[0]).all()
    return v[0]


def _wave(img, x0, y0, x1, y1, t, pol, n, wrong):
    """one wave of split_kernel on one glyph -> its kept boxes.  cnt[x] and the first / last ink row of column x are what the lane that
    holds x finds in its loop over y; everything across columns is done lane by lane as the kernel does it."""
    if n <= 1:
        return [(x0, y0, x1, y1)]
    q = GO.quantise(img[y0:y1])
    ink = (q <= t) if pol == 1 else ((q >= t) if wrong == "pol2_ge" else (q > t))
    cnt = ink.sum(axis=0).astype(np.uint64)
    rows = np.arange(y0, y1)[:, None]
    col_lo = np.where(ink, rows, np.iinfo(np.int32).max).min(axis=0)
    col_hi = np.where(ink, rows, -1).max(axis=0)
    gw = x1 - x0
    r = max(gw // (4 * n), 1)
    cut = [x0, x1, x1, x1]
    for j in range(1, n):
        c = x0 + (j * gw) // n
        lo, hi = max(c - r, x0 + 1), min(c + r, x1 - 1)
        key = np.full(64, 2 ** 64 - 1, np.uint64)
        for step, base in enumerate(range(lo, hi + 1, 64)):                 # for (x = lo + lane; x <= hi; x += 64)
            if wrong == "window_first_64" and step:
                break
            x = (base + LANES)[base + LANES <= hi]
            live = LANES[:len(x)]
            d = np.zeros_like(x) if wrong == "no_distance" else np.abs(x - c)
            low = (0xFFFFF - x) if wrong == "larger_x" else x
            k = (cnt[x] << np.uint64(40)) | (d.astype(np.uint64) << np.uint64(20)) | low.astype(np.uint64)
            key[live] = k if wrong == "lane_keeps_last" else np.minimum(key[live], k)
        best = int(_butterfly(key, np.minimum)) & 0xFFFFF
        cut[j] = 0xFFFFF - best if wrong == "larger_x" else best
    out = []
    for i in range(n):
        xa, xb = cut[i], (cut[i + 1] if i + 1 < n else x1)
        lo = np.full(64, np.iinfo(np.int32).max, np.int64)
        hi = np.full(64, -1, np.int64)
        for step, base in enumerate(range(xa, xb, 64)):                     # for (x = xa + lane; x < xb; x += 64)
            if wrong == "rows_first_64" and step:
                break
            x = (base + LANES)[base + LANES < xb]
            live = LANES[:len(x)]
            lo[live] = np.minimum(lo[live], col_lo[x])
            hi[live] = np.maximum(hi[live], col_hi[x])
        lo, hi = int(_butterfly(lo, np.minimum)), int(_butterfly(hi, np.maximum))
        if hi >= 0:
            out.append((xa, lo, xb, hi + 1))
    return out


def kernel_model(frames, glyphs, params=None, wrong=None) -> dict:
    """ocr_split_glyphs as csrc/glyph_split.hip does it: the host's n per glyph, one _wave per glyph, the host's scan of the records
    into the block (max_word_pieces, bit 4) -> boxes, word_offsets, word_info, map as tests/glyph_split_oracle.py's split gives them."""
    p = SO.params_with(params)
    off = np.asarray(glyphs["word_offsets"], np.int64)
    info = np.array(glyphs["word_info"], np.int32).reshape(-1, 4)
    boxes = np.asarray(glyphs["boxes"], np.int32).reshape(-1, 4)
    out_boxes, out_map, woff = [], [], [0]
    for k in range(len(off) - 1):
        g0, g1 = int(off[k]), int(off[k + 1])
        recs = []
        if g1 > g0:
            hw = max(int(b[3] - b[1]) for b in boxes[g0:g1])
        for g in range(g0, g1):
            x0, y0, x1, y1 = (int(v) for v in boxes[g])
            gw, den = x1 - x0, 2 * hw * p["aspect_pct"]
            n = max(1, min((200 * gw + hw * p["aspect_pct"]) // den, p["max_pieces"], gw // p["min_piece_w"]))
            recs.append(_wave(frames[int(info[k, 0]), 0], x0, y0, x1, y1, int(info[k, 1]), int(info[k, 2]), n, wrong))
        if sum(len(r) for r in recs) > p["max_word_pieces"]:
            info[k, 3] |= 4
            recs = [[tuple(int(v) for v in boxes[g])] for g in range(g0, g1)]
        for g, r in zip(range(g0, g1), recs):
            out_boxes += r
            out_map += [(g, i) for i in range(len(r))]
        woff.append(len(out_boxes))
    return dict(word_offsets=np.asarray(woff, np.int32), word_info=info, boxes=np.asarray(out_boxes, np.int32).reshape(-1, 4),
                map=np.asarray(out_map, np.int32).reshape(-1, 2))


def _agree(got, want):
    return all(np.array_equal(got[k], want[k]) for k in ("boxes", "word_offsets", "word_info", "map"))


def _narrow_agrees(wrong=None):
    frames, col, cc = _narrow()
    return all(_agree(kernel_model(frames, blk, prm, wrong), SO.split(frames, blk, prm)) for blk in (col, cc) for prm in NARROW_PARAMS)


def _wide_fuzz_disagreements(wrong, pol):
    """the indices into SO.WIDE_PARAMS at which the model disagrees with the oracle"""
    frames, blk = _wide(pol)
    return [i for i, prm in enumerate(SO.WIDE_PARAMS) if not _agree(kernel_model(frames, blk, prm, wrong), _wide_want(pol, i))]


def test_the_kernel_model_equals_the_oracle_on_every_case():
    for name, frames, blk, prm, want, _ in list(CASES.values()) + list(WIDE.values()):
        got = kernel_model(frames, blk, prm)
        assert _agree(got, SO.split(frames, blk, prm)) and got["boxes"].tolist() == want, name
    assert _narrow_agrees()
    for pol in (1, 2):
        assert _wide_fuzz_disagreements(None, pol) == []


CUTTING = [i for i, prm in enumerate(SO.WIDE_PARAMS) if prm["max_pieces"] > 1]
# the drawn cases (without their polarity suffix) that each wrong model must miss
CAUGHT_BY = dict(window_first_64={"far_min", "tall_wide"}, rows_first_64={"far_rows", "far_only", "far_only3", "at_threshold"},
                 lane_keeps_last={"far_tie"}, pol2_ge={"at_threshold"}, no_distance={"far_tie"}, larger_x={"far_tie"})


@pytest.mark.parametrize("wrong", WRONG)
def test_a_wrong_model_is_told_from_the_oracle(wrong):
    missed = {name for name, (_, frames, blk, prm, want, _) in WIDE.items() if kernel_model(frames, blk, prm, wrong)["boxes"].tolist() != want}
    if wrong == "pol2_ge":
        assert missed == {"at_threshold-p2"}
    else:
        assert {n + "-p1" for n in CAUGHT_BY[wrong]} | {n + "-p2" for n in CAUGHT_BY[wrong]} <= missed, missed
    if wrong in WRONG[:3]:          # the wide fuzz alone tells these apart, at every parameter set that cuts, in both polarities
        assert _wide_fuzz_disagreements(wrong, 1) == CUTTING and _wide_fuzz_disagreements(wrong, 2) == CUTTING
    if wrong == "pol2_ge":          # ... and this one through its pixels at q = t, at polarity 2 only
        assert _wide_fuzz_disagreements(wrong, 1) == [] and _wide_fuzz_disagreements(wrong, 2) != []
    if wrong in WRONG[:4]:          # which the narrow fuzz cannot: it has no second step of 64 and no polarity 2
        assert _narrow_agrees(wrong)
    else:                           # the two that the narrow fuzz does tell apart already
        assert not _narrow_agrees(wrong)
