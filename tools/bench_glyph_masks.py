"""Time the label planes and the masked glyph crops beside the calls they extend, in one run: the inputs and protocol of
tools/bench_segment_cc.py (device-resident 640 x 640 frames with about 100 block words per page, 1 page and 32 pages; every call is
blocking, so a host clock around a call is its time, host-side preparation, launch, copies and sync included).  Each pair is
alternated call by call after a warm-up - A, B, A, B, ... - so drift of the clocks or the machine lands on both sides, and the whole
measurement is repeated `--repeats` times to show the spread between repeats:

    ocr_segment_glyphs_cc      against  ocr_segment_glyphs_cc_labelled (+ ocr_glyph_labels_free: the planes' one allocation per call)
    ocr_extract_glyph_crops    against  ocr_extract_glyph_crops_masked at halo 0 and 1
    read_words(cc={})          against  read_words(cc={}, mask=True), 32 pages

Results are checked against tests/glyph_mask_oracle.py outside the timed region.  Prints one JSON line.

    timeout -k 10 900 python tools/bench_glyph_masks.py [--iters 20] [--repeats 3]

Kernel time: a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/bench_glyph_masks.py`
(segment_cc_labelled_kernel, glyph_crop_masked_kernel).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _alternate_ms(fns, warmup, iters):
    """Median and minimum milliseconds of every function of `fns`, called in turn."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(iters):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    return [(round(1e3 * float(np.median(t)), 4), round(1e3 * min(t), 4)) for t in ts]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch

    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    from tests import glyph_cc_oracle as CC
    from tests import glyph_mask_oracle as M
    from tests.test_gpu_glyphs import _synthetic_pages

    if not torch.cuda.is_available():
        raise SystemExit("bench_glyph_masks needs a GPU")
    det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    cc = capi.cc_params()
    rows = []
    for pages in (1, 32):
        frames, polys = _synthetic_pages(pages, 640, 640, 100, seed=pages)
        adj = np.ones((pages, 2))
        x = torch.from_numpy(frames).cuda()
        block, keep = capi.python_to_polygons(polys, [[0.0] * len(p) for p in polys])
        torch.cuda.synchronize()
        n, _, h, w = frames.shape
        ptr = x.data_ptr()
        g, lab = det.segment_glyphs_cc_labelled_device(ptr, n, h, w, block, adj, cc=cc)
        crops = torch.empty((g.n_glyphs, 784), dtype=torch.float32, device="cuda")
        halo = [capi.mask_params(halo=0), capi.mask_params(halo=1)]

        def labelled():
            det.segment_glyphs_cc_labelled_device(ptr, n, h, w, block, adj, cc=cc)[1].free()
        seg_fns = [lambda: det.segment_glyphs_device(ptr, n, h, w, block, adj, cc=cc), labelled]
        crop_fns = [lambda: det.extract_glyph_crops_device(ptr, n, h, w, g, crops.data_ptr()),
                    lambda: det.extract_glyph_crops_masked_device(ptr, n, h, w, g, lab, crops.data_ptr(), None, halo[0]),
                    lambda: det.extract_glyph_crops_masked_device(ptr, n, h, w, g, lab, crops.data_ptr(), None, halo[1])]
        read_fns = [lambda: reading.read_words(det, rec, x, polys, adj, cc=cc), lambda: reading.read_words(det, rec, x, polys, adj, cc=cc, mask=True)]
        reps = []
        for _ in range(a.repeats):
            rep = {}
            (rep["segment_cc_ms"], rep["labelled_ms"]) = _alternate_ms(seg_fns, a.warmup, a.iters)
            (rep["crops_ms"], rep["masked_halo0_ms"], rep["masked_halo1_ms"]) = _alternate_ms(crop_fns, a.warmup, a.iters)
            if pages == 32:
                (rep["read_words_ms"], rep["read_words_masked_ms"]) = _alternate_ms(read_fns, 1, max(3, a.iters // 4))
            reps.append(rep)
        # outside the timed region: the planes and the crops of the last call against the oracle
        want = CC.segment_cc(frames, polys, adj)
        planes = M.label_planes(frames, polys, adj)
        match = bool(np.array_equal(g.boxes, want["boxes"]) and np.array_equal(lab.read(), planes["planes"]) and
                     np.array_equal(crops.cpu().numpy().view(np.uint32), M.masked_glyph_crops(frames, want, planes).view(np.uint32)))
        ink = int(np.count_nonzero(planes["planes"]))
        rows.append({"pages": pages, "h": h, "w": w, "words": g.n_words, "glyphs": g.n_glyphs, "plane_elements": int(lab.plane_offsets[-1]),
                     "ink_pixels": ink, "ink_of_no_glyph": int(np.count_nonzero(planes["planes"] == M.NO_GLYPH)),
                     "repeats_median_min_ms": reps, "oracle_match": match})
        lab.free()
    rec.close()
    det.close()
    print(json.dumps({"bench": "glyph_masks", "device": torch.cuda.get_device_name(0), "iters": a.iters, "rows": rows}))
    if not all(r["oracle_match"] for r in rows):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
