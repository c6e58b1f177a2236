"""Time the word strips on device-resident 640 x 640 frames with about 110 words per page (block words, about a fifth of them slanted,
plus ten rotated rectangles per page): 1 page and 32 pages.
  plan       ocr_plan_word_strips (host geometry, no GPU)
  atlas      ocr_extract_word_strips (blocking: host clock around the call; the map upload, launch and sync included)
  rectified  reading.read_words_rectified against reading.read_words (whole calls, numpy in -> text out; synthetic recogniser weights)
The atlas is checked against tests/strip_oracle.py outside the timed region.  Prints one JSON line.  The kernel's own duration comes
from a kernel trace of the same command (rocprofv3 --kernel-trace --stats -- python tools/bench_word_strips.py).

    timeout -k 10 600 python tools/bench_word_strips.py [--iters 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * min(ts)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch

    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    from tests import strip_oracle as S
    from tests.test_gpu_strips import _rotated_pages

    if not torch.cuda.is_available():
        raise SystemExit("bench_word_strips needs a GPU")
    det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    rows = []
    for pages in (1, 32):
        frames, polys = _rotated_pages(pages, 640, 640, seed=100 + pages)
        adj = np.ones((pages, 2))
        n, _, h, w = frames.shape
        x = torch.from_numpy(frames).cuda()
        block, keep = capi.python_to_polygons(polys, [[0.0] * len(p) for p in polys])
        torch.cuda.synchronize()
        st = capi.plan_word_strips(block, adj, h, w)
        atlas = torch.empty((st.height, st.total_width), dtype=torch.float32, device="cuda")
        plan_ms, plan_min = _median_ms(lambda: capi.plan_word_strips(block, adj, h, w), a.warmup, a.iters)
        atlas_ms, atlas_min = _median_ms(lambda: det.extract_word_strips_device(x.data_ptr(), n, h, w, st, atlas.data_ptr()), a.warmup, a.iters)
        got = atlas.cpu().numpy()
        match = bool(np.array_equal(got.view(np.uint32), S.extract(frames, S.plan(polys, adj)).view(np.uint32)))
        rect_ms, _ = _median_ms(lambda: reading.read_words_rectified(det, rec, frames, polys, adj), 1, max(3, a.iters // 4))
        axis_ms, _ = _median_ms(lambda: reading.read_words(det, rec, frames, polys, adj), 1, max(3, a.iters // 4))
        samples = st.height * st.total_width
        rows.append({"pages": pages, "h": h, "w": w, "words": st.n_words, "atlas": [st.height, st.total_width],
                     "plan_ms_median": round(plan_ms, 4), "plan_ms_min": round(plan_min, 4),
                     "atlas_ms_median": round(atlas_ms, 4), "atlas_ms_min": round(atlas_min, 4),
                     "samples_per_s_call": round(samples / (atlas_ms / 1e3)),
                     "read_words_rectified_ms": round(rect_ms, 3), "read_words_ms": round(axis_ms, 3),
                     "oracle_match": match})
    rec.close()
    det.close()
    print(json.dumps({"bench": "word_strips", "device": torch.cuda.get_device_name(0), "iters": a.iters, "rows": rows}))
    if not all(r["oracle_match"] for r in rows):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
