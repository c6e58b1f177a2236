"""Which form of the device contour tracer a map gets (contour_trace_form, contours.hip: needs no GPU), and the large maps that
tests/test_gpu_large_maps.py feeds it: that they reach what they are meant to reach - every edge of the map, every band edge, a
plausible-start count on each side of the LDS cache and of kMaxStarts - and that the restated plausible starts hold every start
the host tracer takes."""
import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from tests import contour_maps as CM

LWS = (14336, 22528, 35840)   # the parallel form's instantiations (contours.hip launch_contour_trace)
LDS_WORDS = 39808             # contours.hip kLdsWords: the one-wave form's bit image and two label planes


def _expected_form(h, w, sequential=False, have_spec=True):
    shape_ok = h > 0 and w > 0 and w % 32 == 0 and w <= 2048 and h <= 32767
    seq_fits = shape_ok and 3 * ((h * w + 31) // 32) + 1 <= LDS_WORDS
    par_fits = shape_ok and h <= 1024 and CM.parallel_words(h, w) <= LWS[-1]
    if have_spec and par_fits and not (sequential and seq_fits):
        return next(lw for lw in LWS if CM.parallel_words(h, w) <= lw)
    return 1 if seq_fits else 0


@pytest.mark.parametrize("h,w,form", [
    (652, 640, 14336), (653, 640, 22528), (837, 800, 22528), (838, 800, 35840), (896, 896, 35840), (1024, 1024, 35840),
    (1024, 800, 35840), (495, 2048, 35840), (1025, 32, 1), (1105, 384, 1), (496, 2048, 0), (1106, 384, 0), (1024, 1088, 0),
    (640, 640, 14336), (800, 800, 22528), (64, 2048, 14336), (1024, 32, 14336)])
def test_form_at_the_size_limits(h, w, form):
    assert capi.contour_trace_form(h, w) == form
    assert _expected_form(h, w) == form


def test_form_table_against_its_restatement():
    """Every height of the widths the tests and the product use, asked for either form, with and without the parallel form's
    scratch: the smallest instantiation that holds the map, the one-wave form where only it fits or it was asked for."""
    for w in (32, 64, 384, 640, 800, 896, 1024, 1088, 2048):
        for h in list(range(1, 1200, 7)) + [652, 653, 837, 838, 1024, 1025, 1105, 1106]:
            for seq in (False, True):
                for spec in (False, True):
                    assert capi.contour_trace_form(h, w, seq, spec) == _expected_form(h, w, seq, spec), (h, w, seq, spec)
    assert capi.contour_trace_form(64, 48) == 0 and capi.contour_trace_form(0, 64) == 0   # (width not a multiple of 32, empty map)
    # the parallel form asked for the one-wave form where that does not fit: the parallel form still runs (the product has no third choice)
    assert capi.contour_trace_form(1024, 1024, True) == 35840 and capi.contour_trace_form(1024, 1024, True, False) == 0


LARGE = [(652, 640), (653, 640), (837, 800), (838, 800), (896, 896), (1024, 1024), (1024, 800), (495, 2048), (1025, 32), (1105, 384)]


@pytest.mark.parametrize("h,w", LARGE)
def test_text_pages_reach_every_edge(h, w):
    bm = CM.text_page(h, w, 1)
    assert bm.shape == (h, w) and not bm[:, 0].any()
    assert bm[h - 1].sum() >= 20 and bm[h - 1, w - 1] and bm[:, w - 1].sum() >= h // 11
    tail = bm[h - CM.BAND_ROWS:]                                              # the last 64 rows (row h-1: phase A's last thread)
    assert tail.any(axis=1).mean() >= 0.5 and tail.sum() >= 200
    for b in range(CM.BAND_ROWS, h, CM.BAND_ROWS):                             # something crosses every band edge
        assert (bm[b - 1] & bm[b]).any(), b
    # one-pixel runs in column w-1 (W neighbour clear), hole borders (a background pixel enclosed by foreground in its row and column)
    assert (bm[:, w - 1] & ~bm[:, w - 2] & 1).sum() >= 5
    inner = (bm[1:-1, 1:-1] == 0) & (bm[:-2, 1:-1] == 1) & (bm[1:-1, :-2] == 1)
    assert inner.sum() >= 3
    hc = capi.host_contours(bm)
    assert 100 <= len(hc) and sum(len(c) for c in hc) < 65_000              # half the parallel form's pool of walked points (131 072)


def test_the_restated_plausible_starts_hold_every_host_start():
    """Every contour the host tracer starts at x > 0 starts at a restated plausible start (the device's claim: a start outside the
    list exists only for a component whose first pixel sits in column 0), and the list is in raster order."""
    for bm in (CM.text_page(1024, 1024, 3), CM.text_page(495, 2048, 4), CM.text_page(200, 96, 5, fill=0.9, hollow=0.8)):
        keys = CM.plausible_starts(bm)
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        ks = set(keys)
        w = bm.shape[1]
        for c in capi.host_contours(bm):
            x, y = c[0]
            assert 2 * (y * w + x) in ks or 2 * (y * w + x) + 1 in ks, (x, y)


def test_the_matrix_maps_keep_their_walks_in_the_pool():
    """Every map tests/test_gpu_large_maps.py expects status 0 from: K within kMaxStarts and the speculative walks within the pool."""
    from tests import test_gpu_large_maps as G
    for (h, w), form, seeds in G.MATRIX:
        for seed in seeds:
            bm = CM.text_page(h, w, seed)
            assert len(CM.plausible_starts(bm)) <= CM.MAX_STARTS and CM.walked_points(bm) <= CM.POOL * 3 // 4, (h, w, seed)


def test_walk_lengths_are_the_host_tracers_borders():
    """The restated walk from a start the host tracer takes is as long as the contour it traces from there."""
    bm = CM.text_page(200, 96, 5, fill=0.9, hollow=0.8)
    w = bm.shape[1]
    ks = set(CM.plausible_starts(bm))
    for c in capi.host_contours(bm):
        x, y = c[0]
        key = 2 * (y * w + x) + (0 if 2 * (y * w + x) in ks else 1)
        assert CM.walk_length(bm, key) == len(c), (x, y)


def test_start_counts_of_the_fallback_maps():
    """The 1024 x 1024 maps of the outcomes: K past the LDS cache within kMaxStarts and the pool; K within kMaxStarts but walks past
    the pool; K past kMaxStarts; and the pages of the batched post-processing call fit the product's per-image buffers
    (ContourBuffers: 32 768 points, 4 096 contours)."""
    from tests import test_gpu_large_maps as G
    bm = G._k_mid()
    assert CM.KEY_CACHE < len(CM.plausible_starts(bm)) <= CM.MAX_STARTS and CM.walked_points(bm) <= CM.POOL * 3 // 4
    bm = G._pool_overflow()
    assert CM.KEY_CACHE < len(CM.plausible_starts(bm)) <= CM.MAX_STARTS and CM.walked_points(bm) > CM.POOL
    assert len(CM.plausible_starts(CM.dot_field(1024, 1024, 8, 12))) > CM.MAX_STARTS
    for seed in (21, 22):
        bm = CM.text_page(1024, 1024, seed, fill=0.08)
        hc = capi.host_contours(bm)
        assert len(hc) < 4096 and sum(len(c) for c in hc) < 24_000 and CM.walked_points(bm) <= CM.POOL // 2
    bm = G._gives_up(31)
    assert bm[:, 0].any() and CM.walked_points(bm) <= CM.POOL // 2
