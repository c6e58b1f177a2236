"""Time glyph segmentation (ocr_segment_glyphs) and glyph crops (ocr_extract_glyph_crops) on device-resident 640 x 640 frames with about
100 block words per page: 1 page and 32 pages.  Both calls are blocking (they end in a stream synchronise), so a host clock around a
call is its time, host-side box preparation, launch, copies and sync included.  Results are checked against tests/glyph_oracle.py
outside the timed region.  Prints one JSON line.

    timeout -k 10 600 python tools/bench_read_words.py [--iters 20]
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
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    from tests import glyph_oracle as G
    from tests.test_gpu_glyphs import _synthetic_pages

    if not torch.cuda.is_available():
        raise SystemExit("bench_read_words needs a GPU")
    det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    rows = []
    for pages in (1, 32):
        frames, polys = _synthetic_pages(pages, 640, 640, 100, seed=pages)
        adj = np.ones((pages, 2))
        x = torch.from_numpy(frames).cuda()
        block, keep = capi.python_to_polygons(polys, [[0.0] * len(p) for p in polys])
        torch.cuda.synchronize()
        n, _, h, w = frames.shape
        g = det.segment_glyphs_device(x.data_ptr(), n, h, w, block, adj)
        crops = torch.empty((g.n_glyphs, 784), dtype=torch.float32, device="cuda")
        seg_ms, seg_min = _median_ms(lambda: det.segment_glyphs_device(x.data_ptr(), n, h, w, block, adj), a.warmup, a.iters)
        crop_ms, crop_min = _median_ms(lambda: det.extract_glyph_crops_device(x.data_ptr(), n, h, w, g, crops.data_ptr()), a.warmup, a.iters)
        want = G.segment(frames, polys, adj)
        wc = G.glyph_crops(frames, want)
        match = bool(np.array_equal(g.word_info, want["word_info"]) and np.array_equal(g.boxes, want["boxes"])
                     and np.array_equal(g.word_levels.view(np.uint32), want["word_levels"].view(np.uint32))
                     and np.array_equal(crops.cpu().numpy().view(np.uint32), wc.view(np.uint32)))
        rows.append({"pages": pages, "h": h, "w": w, "words": g.n_words, "glyphs": g.n_glyphs,
                     "segment_ms_median": round(seg_ms, 4), "segment_ms_min": round(seg_min, 4),
                     "segment_words_per_s": round(g.n_words / (seg_ms / 1e3)), "segment_glyphs_per_s": round(g.n_glyphs / (seg_ms / 1e3)),
                     "crops_ms_median": round(crop_ms, 4), "crops_ms_min": round(crop_min, 4),
                     "crops_words_per_s": round(g.n_words / (crop_ms / 1e3)), "crops_glyphs_per_s": round(g.n_glyphs / (crop_ms / 1e3)),
                     "oracle_match": match})
    det.close()
    print(json.dumps({"bench": "read_words", "device": torch.cuda.get_device_name(0), "iters": a.iters, "rows": rows}))
    if not all(r["oracle_match"] for r in rows):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
