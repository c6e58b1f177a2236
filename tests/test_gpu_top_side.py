"""Engine option top_side: behind layer3, layer4's shortcut conv and in4 run on the side stream, the top-down add
up2(in5) + in4 is made by out4's input transform on load, and out5's three launches run beside out4's on a scratch of their own.

Nothing is composed and no sum re-associated: every map must be BIT-identical to the top_side=0 engine's - for every move alone and all
together, back to back without a host synchronise (one call's scratch, sum or shortcut under the other's), and under the pipelined calls."""
import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from ocr_rs_amd import weights as W

pytestmark = pytest.mark.gpu

ALL = 7                                   # layer4's shortcut | in4 | out5
SIZES = ((64, 96), (160, 128))            # H/16 = 4 x 6, 10 x 8 and H/32 = 2 x 3, 5 x 4: whole and ragged 4 x 4 tiles on both grids


@pytest.fixture(scope="module")
def blob():
    return W.pack_blob(W.make_det_weights(0))


@pytest.fixture(scope="module")
def engines(blob):
    """Detectors by option string, made on first use and shared by the cases of this module."""
    made = {}

    def get(options):
        if options not in made:
            made[options] = capi.Detector(blob, 0, options=options)
        return made[options]

    yield get
    for d in made.values():
        d.close()


def run(det, x):
    """forward_device on a device batch; (prob, bitmap) as numpy.  The outputs start out poisoned."""
    import torch
    n, _, h, w = x.shape
    prob = torch.full(x.shape, float("nan"), dtype=torch.float32, device="cuda")
    bm = torch.full(x.shape, 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    det.forward_device(x.data_ptr(), n, h, w, prob.data_ptr(), bm.data_ptr(), 0.6)
    det.synchronize()
    return prob.cpu().numpy(), bm.cpu().numpy()


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_maps_are_bit_identical_and_the_default_takes_the_new_order(engines, size, n):
    import torch
    h, w = size
    x = torch.from_numpy(W.synth_image_batch(31 + n + h, n, h, w)).cuda()
    ref = engines("top_side=0")
    want_prob, want_bm = run(ref, x)
    assert ref.last_top_side() == 0
    assert np.isfinite(want_prob).all() and want_bm.max() <= 1
    for opt, moves in ((None, ALL), ("top_side=1", 1), ("top_side=2", 2), ("top_side=4", 4)):
        det = engines(opt)
        prob, bm = run(det, x)
        assert det.last_top_side() == moves, (opt, size, n)         # the forward really ran in the new order
        assert np.array_equal(prob, want_prob), (opt, size, n)
        assert np.array_equal(bm, want_bm), (opt, size, n)


def test_back_to_back_calls_without_host_sync(engines):
    """Three calls on one handle with different frames and batch sizes, separate outputs, ONE synchronise at the end: in4 and the shortcut
    of call j + 1 (side stream) must not overwrite sum_[2] / d_[3] under call j's readers, nor out5's scratch or in5 under its chain."""
    import torch
    h, w = 160, 128
    xs = [torch.from_numpy(W.synth_image_batch(41 + j, n, h, w)).cuda() for j, n in enumerate((3, 2, 3))]
    want = [run(engines("top_side=0"), x) for x in xs]
    det = engines(None)
    probs = [torch.full(x.shape, float("nan"), dtype=torch.float32, device="cuda") for x in xs]
    bms = [torch.full(x.shape, 7, dtype=torch.uint8, device="cuda") for x in xs]
    torch.cuda.synchronize()
    for x, p, b in zip(xs, probs, bms):
        det.forward_device(x.data_ptr(), x.shape[0], h, w, p.data_ptr(), b.data_ptr(), 0.6)
        assert det.last_top_side() == ALL
    det.synchronize()
    for j, (p, b) in enumerate(zip(probs, bms)):
        assert np.array_equal(p.cpu().numpy(), want[j][0]), j
        assert np.array_equal(b.cpu().numpy(), want[j][1]), j


def test_pipelined_calls_keep_the_old_order_beside_a_pending_batch_and_give_the_same_maps():
    """detect_pipelined: the first call of a sequence has nothing beside it and takes the new order under auto; a call whose previous batch
    is pending (its post-processing runs beside this part of the forward) keeps the old one; a forced mask applies to both.  Maps and
    polygons are the top_side=0 engine's whichever schedule a call got."""
    import torch
    n, S = 3, 160
    blob = W.pack_blob(W.make_det_weights_text())
    params = capi.default_params(skip_degenerate=True)
    xs = [torch.from_numpy(W.synth_text_pages(960 + b, n, S, S)[0]).cuda() for b in range(2)]
    results, maps = [], []
    for opt, first, beside in (("top_side=0", 0, 0), (None, ALL, 0), ("top_side=7", ALL, ALL)):
        det = capi.Detector(blob, 0, options=opt)
        try:
            probs = [torch.full(x.shape, float("nan"), dtype=torch.float32, device="cuda") for x in xs]
            torch.cuda.synchronize()
            got = []
            for j, (x, p) in enumerate(zip(xs, probs)):
                got.append(det.detect_pipelined(x.data_ptr(), n, S, S, p.data_ptr(), np.ones((n, 2)), params))
                assert det.last_top_side() == (first if j == 0 else beside), (opt, j)
            got.append(det.detect_pipelined(0, 0, 0, 0, 0))
            assert got[0] is None
            results.append(got[1:])
            maps.append([p.cpu().numpy() for p in probs])
        finally:
            det.close()
    for k in (1, 2):
        assert results[k] == results[0]
        assert all(np.array_equal(a, b) for a, b in zip(maps[k], maps[0]))
    assert all(np.isfinite(m).all() for m in maps[0])


def test_other_schedules_keep_their_order_and_their_maps(engines):
    """overlap=0|1, fpn_unfused=1, the bf16 precision and ocr_det_forward_profile keep today's order launch for launch: no move is taken
    whatever top_side says, and the maps are those of top_side=0 under the same option."""
    import torch
    n, h, w = 3, 160, 128
    x = torch.from_numpy(W.synth_image_batch(51, n, h, w)).cuda()
    for base in ("overlap=0", "overlap=1", "fpn_unfused=1", "precision=bf16"):
        want_prob, want_bm = run(engines(base + ";top_side=0"), x)
        det = engines(base + ";top_side=7")
        prob, bm = run(det, x)
        assert det.last_top_side() == 0, base
        assert np.array_equal(prob, want_prob) and np.array_equal(bm, want_bm), base
    # the profiled forward: one stream, the old launches under their old names, the same map
    ref, det = engines("top_side=0"), engines(None)
    pa = torch.full(x.shape, float("nan"), dtype=torch.float32, device="cuda")
    pb = torch.full(x.shape, float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    names_ref = [e[0] for e in ref.forward_profile(x.data_ptr(), n, h, w, pa.data_ptr())]
    names = [e[0] for e in det.forward_profile(x.data_ptr(), n, h, w, pb.data_ptr())]
    assert det.last_top_side() == 0 and names == names_ref and len(names) > 20
    assert np.array_equal(pa.cpu().numpy(), pb.cpu().numpy()) and np.isfinite(pb.cpu().numpy()).all()


def test_bad_values(blob):
    for bad in ("top_side=-1", "top_side=8", "top_side=on", "top_side="):
        with pytest.raises(capi.OcrError) as e:
            capi.Detector(blob, 0, options=bad)
        assert e.value.code == 1, bad
