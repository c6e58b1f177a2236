"""Engine option front_split: stem .. layer2 as two frame groups on the detector's two streams.

No kernel computes anything that depends on the batch it was launched with, so every map must be BIT-identical to the
front_split=0 engine's - whatever the group sizes, back to back without a host synchronise, and under the pipelined calls."""
import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from ocr_rs_amd import weights as W

pytestmark = pytest.mark.gpu

# ragged 16 x 16 blocks at H/4 (24 x 40, 56 x 88), odd grids at H/32 (3 x 5, 7 x 11), one-frame and uneven groups, and a batch whose
# groups' launches really co-run (8 x 320 x 320: 100 + 100 blocks per fused Winograd launch at k = 4)
SHAPES = ((2, 64, 64), (3, 96, 160), (5, 224, 352), (8, 320, 320))


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


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_split_front_is_bit_identical(engines, shape, precision):
    import torch
    n, h, w = shape
    pre = f"precision={precision};"
    x = torch.from_numpy(W.synth_image_batch(61 + n, n, h, w)).cuda()
    ref = engines(pre + "front_split=0")
    want_prob, want_bm = run(ref, x)
    assert ref.last_front_split() == 0
    assert np.isfinite(want_prob).all() and want_bm.max() <= 1
    for k in sorted({1, n - 1, n // 2}):
        det = engines(pre + f"front_split={k}")
        prob, bm = run(det, x)
        assert det.last_front_split() == k, (shape, precision, k)      # the forward really ran as two groups
        assert np.array_equal(prob, want_prob), (shape, precision, k)
        assert np.array_equal(bm, want_bm), (shape, precision, k)


def test_no_split_cases_and_bad_values(engines, blob):
    import torch
    x3 = torch.from_numpy(W.synth_image_batch(71, 3, 96, 160)).cuda()
    want_prob, want_bm = run(engines("front_split=0"), x3)
    for opt in ("front_split=3", "front_split=100", "front_split=auto", None):     # k >= n; the default engine
        prob, bm = run(engines(opt), x3)
        assert engines(opt).last_front_split() == 0, opt
        assert np.array_equal(prob, want_prob) and np.array_equal(bm, want_bm), opt
    x1 = x3[1:2].contiguous()
    for opt in ("front_split=1", "front_split=auto"):                               # n = 1
        prob, bm = run(engines(opt), x1)
        assert engines(opt).last_front_split() == 0, opt
        assert np.array_equal(prob, want_prob[1:2]) and np.array_equal(bm, want_bm[1:2]), opt
    for bad in ("front_split=-1", "front_split=half", "front_split=", "front_split=2.5"):
        with pytest.raises(capi.OcrError) as e:
            capi.Detector(blob, 0, options=bad)
        assert e.value.code == 1, bad


def test_back_to_back_calls_without_host_sync(engines):
    """Three calls on one handle, batch sizes 3, 2, 3, different frames, separate outputs, ONE synchronise at the end: the side
    stream's first launch of call j + 1 must sit behind everything of call j (which still reads the shared workspace)."""
    import torch
    h, w = 224, 352
    xs = [torch.from_numpy(W.synth_image_batch(81 + j, n, h, w)).cuda() for j, n in enumerate((3, 2, 3))]
    want = [run(engines("front_split=0"), x) for x in xs]
    det = engines("front_split=1")
    probs = [torch.full(x.shape, float("nan"), dtype=torch.float32, device="cuda") for x in xs]
    bms = [torch.full(x.shape, 7, dtype=torch.uint8, device="cuda") for x in xs]
    torch.cuda.synchronize()
    for x, p, b in zip(xs, probs, bms):
        det.forward_device(x.data_ptr(), x.shape[0], h, w, p.data_ptr(), b.data_ptr(), 0.6)
        assert det.last_front_split() == 1
    det.synchronize()
    for j, (p, b) in enumerate(zip(probs, bms)):
        assert np.array_equal(p.cpu().numpy(), want[j][0]), j
        assert np.array_equal(b.cpu().numpy(), want[j][1]), j


def test_pipelined_calls_return_the_same_polygons():
    """detect_pipelined (the forward of batch k + 1 beside the polygon chain of batch k) with a forced split and without."""
    import torch
    S = 320
    blob = W.pack_blob(W.make_det_weights_text())
    params = capi.default_params(skip_degenerate=True)
    xs = [torch.from_numpy(W.synth_text_pages(930 + b, 4, S, S)[0]).cuda() for b in range(2)]
    results = []
    for opt in ("front_split=0", "front_split=2"):
        det = capi.Detector(blob, 0, options=opt)
        try:
            probs = [torch.empty_like(x) for x in xs]
            torch.cuda.synchronize()
            got = []
            for x, p in zip(xs, probs):
                got.append(det.detect_pipelined(x.data_ptr(), 4, S, S, p.data_ptr(), np.ones((4, 2)), params))
                assert det.last_front_split() == (2 if opt == "front_split=2" else 0)
            got.append(det.detect_pipelined(0, 0, 0, 0, 0))
            assert got[0] is None
            results.append(got[1:])
        finally:
            det.close()
    assert results[0] == results[1]
    assert all(sum(len(p) for p in polys) > 0 for polys, _ in results[0])


def test_auto_rule(engines):
    """front_split=auto (the default): two halves where a half fills the resident slots of layer1's persistent grids once - 100 blocks of
    16 x 16 per 640 x 640 frame at H/4 against two workgroups per CU - in the f32 precision, and not while a pipelined batch is pending."""
    import torch
    slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    n_split = 2 * -(-slots // 100)          # the smallest even batch whose half holds `slots` blocks (12 frames on 256 CUs)
    x = torch.from_numpy(W.synth_image_batch(91, n_split, 640, 640)).cuda()
    want_prob, want_bm = run(engines("front_split=0"), x)
    det = engines(None)
    prob, bm = run(det, x)
    assert det.last_front_split() == n_split // 2
    assert np.array_equal(prob, want_prob) and np.array_equal(bm, want_bm)
    run(det, x[:n_split - 2])               # a half of 5 frames: 500 blocks on 512 slots
    assert det.last_front_split() == 0
    bf = engines("precision=bf16")
    run(bf, x)
    assert bf.last_front_split() == 0


def test_auto_leaves_calls_beside_a_pending_batch_unsplit():
    """A pipelined call whose previous batch is pending (its post-processing runs beside this forward) stays unsplit under auto; the
    first call of a sequence has nothing beside it and splits.  The maps are the unsplit engine's either way."""
    import torch
    n, S = 12, 640
    blob = W.pack_blob(W.make_det_weights_text())
    params = capi.default_params(skip_degenerate=True)
    x = torch.from_numpy(W.synth_text_pages(950, n, S, S)[0]).cuda()
    ref, det = capi.Detector(blob, 0, options="front_split=0"), capi.Detector(blob, 0)
    try:
        want_prob, _ = run(ref, x)
        p1, p2 = torch.empty_like(x), torch.empty_like(x)
        torch.cuda.synchronize()
        slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count
        assert det.detect_pipelined(x.data_ptr(), n, S, S, p1.data_ptr(), np.ones((n, 2)), params) is None
        assert det.last_front_split() == (n // 2 if (n // 2) * 100 >= slots else 0)
        first = det.detect_pipelined(x.data_ptr(), n, S, S, p2.data_ptr(), np.ones((n, 2)), params)
        assert det.last_front_split() == 0
        second = det.detect_pipelined(0, 0, 0, 0, 0)
        assert first == second and sum(len(p) for p in first[0]) > 0
        assert np.array_equal(p1.cpu().numpy(), want_prob) and np.array_equal(p2.cpu().numpy(), want_prob)
    finally:
        ref.close()
        det.close()
