"""The device contour tracer (contours.hip) at every form the dispatcher picks and at its limits: the parallel form's three LDS sizes
(14336, 22528 and 35840 words: up to 1024 x 1024), the one-wave form where only it takes the map (h > 1024), the shapes just inside
and just outside each limit, and at 1024 x 1024 the three ways an image can end - plausible starts past the scan's LDS cache, past
kMaxStarts or walks past the pool (status 1), a start outside the list (status 3) - alone, in a batched ocr_det_postprocess call and
in the pipelined calls.  Contours are compared point for point, in order, with the host tracer and the oracle; the hook says which
form ran and its K, and K must be the count tests/contour_maps.py restates (which also says that every map here but the status-1
ones keeps its walks inside the pool: tests/test_contour_forms.py)."""
import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from ocr_rs_amd import weights as W
from oracle import postproc_oracle as O
from tests import contour_maps as CM

pytestmark = pytest.mark.gpu

# (h, w), the form the dispatcher must pick, the seeds of the text pages traced at that shape
MATRIX = [
    ((652, 640), 14336, (1,)),             # the largest map of the 56 KB form
    ((653, 640), 22528, (1,)),
    ((837, 800), 22528, (1,)),             # the largest map of the 88 KB form
    ((838, 800), 35840, (1, 2)),
    ((896, 896), 35840, (1, 3)),
    ((1024, 1024), 35840, (1, 2, 3)),
    ((1024, 800), 35840, (1, 2)),
    ((495, 2048), 35840, (1, 2)),          # the widest map that fits: 35 777 of 35 840 words
    ((1025, 32), 1, (1,)),                 # the parallel form refuses h > 1024: the one-wave form runs although it was not asked for
    ((1105, 384), 1, (1,)),                # the one-wave form's last height at this width (3 x 13 260 + 1 of 39 808 words)
]


def _same_contours(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{what}: contour {k} differs"


def _oracle(bm):
    return [[(int(x), int(y)) for x, y in c] for c in O.find_contours(bm * 255)]


def _trace(bm, form, want_status=0):
    got, status, ran, k = capi.device_contours(bm, report=True)
    assert ran == form
    assert status == want_status, (status, k)
    assert k == (len(CM.plausible_starts(bm)) if form != 1 else 0)
    return got, k


@pytest.mark.parametrize("shape,form,seeds", MATRIX, ids=[f"{h}x{w}" for (h, w), _, _ in MATRIX])
def test_large_maps_trace_like_the_host_and_the_oracle(shape, form, seeds):
    h, w = shape
    for seed in seeds:
        bm = CM.text_page(h, w, seed)
        got, _ = _trace(bm, form)
        _same_contours(got, capi.host_contours(bm), f"{h}x{w} seed {seed} vs host")
        _same_contours(got, _oracle(bm), f"{h}x{w} seed {seed} vs oracle")


@pytest.mark.parametrize("shape", [(496, 2048), (1106, 384), (1024, 1088)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_maps_past_the_limits_are_refused(shape):
    assert capi.contour_trace_form(*shape) == 0
    with pytest.raises(capi.OcrError):
        capi.device_contours(np.zeros(shape, np.uint8), report=True)


def _k_mid():
    """a text page above, dots below: about 5 600 plausible starts, most of them past the scan's LDS cache"""
    bm = CM.text_page(1024, 1024, 7)
    bm[512:] = CM.dot_field(512, 1024, 8, 12)
    return bm


def _pool_overflow():
    """dots on words: each dot that touches a word from above is a plausible start of the word's border, walked again - 2 800 starts
    within kMaxStarts, but 346 000 walked points, past the pool of 131 072"""
    return np.maximum(CM.text_page(1024, 1024, 7, fill=0.15), CM.dot_field(1024, 1024, 16, 24))


def _gives_up(seed):
    """a text page plus a block whose first pixel in raster order sits in column 0"""
    bm = CM.text_page(1024, 1024, seed, fill=0.08)
    bm[495:530, 0:48] = 0
    bm[500:520, 0:40] = 1
    return bm


def test_starts_past_the_lds_cache():
    """K between kKeyCache and kMaxStarts: the scan reads the later starts' keys, lengths and offsets from global memory"""
    bm = _k_mid()
    got, k = _trace(bm, 35840)
    assert CM.KEY_CACHE < k <= CM.MAX_STARTS
    _same_contours(got, capi.host_contours(bm), "K past the cache vs host")
    _same_contours(got, _oracle(bm), "K past the cache vs oracle")


def test_more_starts_than_the_list_holds_report_status_1():
    bm = CM.dot_field(1024, 1024, 8, 12)
    got, k = _trace(bm, 35840, want_status=1)
    assert k > CM.MAX_STARTS and got == []


def test_walks_past_the_pool_report_status_1():
    got, k = _trace(_pool_overflow(), 35840, want_status=1)
    assert CM.KEY_CACHE < k <= CM.MAX_STARTS and got == []


def test_a_start_in_column_0_gives_the_image_up():
    bm = _gives_up(31)
    got, _ = _trace(bm, 35840, want_status=3)
    assert got == []


def _probs(bms, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([np.where(b, 0.8 + 0.2 * rng.random(b.shape), 0.1 * rng.random(b.shape)) for b in bms])[:, None]
                                .astype(np.float32))


@pytest.mark.parametrize("options", ["device_contours=1", "device_contours=1;device_unclip=2", "device_contours=1;device_polygons=0"],
                         ids=["device", "device-chain", "device-trace-only"])
def test_postprocess_batch_of_1024_maps_with_one_given_up(options):
    """Two good 1024 x 1024 pages and one the parallel form gives up, in ONE ocr_det_postprocess call: the same polygons and scores as
    the host tracer and the oracle; two images traced on the device, one on the host."""
    maps = _probs([CM.text_page(1024, 1024, 21, fill=0.08), _gives_up(32), CM.text_page(1024, 1024, 22, fill=0.08)], 5)
    adj = np.array([[1.0, 1.0], [1.25, 0.8], [800 / 1024, 600 / 1024]])
    p = capi.default_params(skip_degenerate=True)
    blob = W.pack_blob(W.make_det_weights(0))
    host = capi.Detector(blob, 0, options="device_contours=0")
    dev = capi.Detector(blob, 0, options=options)
    want = host.postprocess(maps, 3, 1024, 1024, adj, capi.MEM_HOST, p)
    got = dev.postprocess(maps, 3, 1024, 1024, adj, capi.MEM_HOST, p)
    st = dev.post_stats()
    host.close()
    dev.close()
    assert got[0] == want[0]
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got[1], want[1]))
    want_p, want_s = O.get_boxes_and_box_scores(maps, adj, skip_degenerate=True)
    assert got[0] == want_p
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got[1], want_s))
    assert all(len(q) >= 10 for q in got[0])   # there was something to compare on every page
    assert st["images_device_traced"] == 2 and st["images_host_traced"] == 1, st


def test_pipelined_calls_at_1024():
    """detect_pipelined_host on 1024 x 1024 pages: the 35840-word tracer on the trace stream beside the next forward, as the product
    runs it - the same polygons and scores as the host tracer, batch after batch, every image traced on the device."""
    blob = W.pack_blob(W.make_det_weights_text())
    params = capi.default_params(skip_degenerate=True)
    pages = [W.synth_text_pages(700 + i, n, 1024, 1024)[0] for i, n in enumerate((2, 3, 1))]
    results, stats = {}, {}
    for dc in (0, 1):
        det = capi.Detector(blob, 0, options=f"device_contours={dc};post_threads=2")
        got = []
        for x in pages:
            r = det.detect_pipelined_host(x, adjust_values=np.ones((x.shape[0], 2)), params=params)
            if r is not None:
                got.append(r)
        got.append(det.detect_pipelined_host(None))
        stats[dc] = det.post_stats()
        det.close()
        results[dc] = got
    assert len(results[0]) == len(results[1]) == len(pages)
    for k, (a, b) in enumerate(zip(results[0], results[1])):
        assert a[0] == b[0], k
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a[1], b[1])), k
    assert sum(len(p) for r in results[0] for p in r[0]) > 50   # there was something to compare
    assert stats[1]["images_device_traced"] == 6 and stats[1]["images_host_traced"] == 0, stats[1]
