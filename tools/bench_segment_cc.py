"""Time glyph segmentation by connected components (ocr_segment_glyphs_cc) beside the unchanged column call (ocr_segment_glyphs) in
one run: the inputs and protocol of tools/bench_read_words.py (device-resident 640 x 640 frames with about 100 block words per page,
1 page and 32 pages; both calls are blocking, so a host clock around a call is its time, host-side box preparation, launch, copies and
sync included).  Results are checked against tests/glyph_cc_oracle.py and tests/glyph_oracle.py outside the timed region.  Prints one
JSON line.

    timeout -k 10 600 python tools/bench_segment_cc.py [--iters 20]

Kernel time: a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/bench_segment_cc.py` (segment_cc_kernel).
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


def _same(g, want):
    return bool(np.array_equal(g.word_offsets, want["word_offsets"]) and np.array_equal(g.word_info, want["word_info"])
                and np.array_equal(g.boxes, want["boxes"]) and np.array_equal(g.word_levels.view(np.uint32), want["word_levels"].view(np.uint32)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch

    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    from tests import glyph_cc_oracle as CC
    from tests import glyph_oracle as G
    from tests.test_gpu_glyphs import _synthetic_pages

    if not torch.cuda.is_available():
        raise SystemExit("bench_segment_cc needs a GPU")
    det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    cc = capi.cc_params()
    rows = []
    for pages in (1, 32):
        frames, polys = _synthetic_pages(pages, 640, 640, 100, seed=pages)
        adj = np.ones((pages, 2))
        x = torch.from_numpy(frames).cuda()
        block, keep = capi.python_to_polygons(polys, [[0.0] * len(p) for p in polys])
        torch.cuda.synchronize()
        n, _, h, w = frames.shape
        g_col = det.segment_glyphs_device(x.data_ptr(), n, h, w, block, adj)
        g_cc = det.segment_glyphs_device(x.data_ptr(), n, h, w, block, adj, cc=cc)
        col_ms, col_min = _median_ms(lambda: det.segment_glyphs_device(x.data_ptr(), n, h, w, block, adj), a.warmup, a.iters)
        cc_ms, cc_min = _median_ms(lambda: det.segment_glyphs_device(x.data_ptr(), n, h, w, block, adj, cc=cc), a.warmup, a.iters)
        st = []
        match = _same(g_col, G.segment(frames, polys, adj)) and _same(g_cc, CC.segment_cc(frames, polys, adj, stats=st))
        rows.append({"pages": pages, "h": h, "w": w, "words": g_cc.n_words, "glyphs_columns": g_col.n_glyphs, "glyphs_components": g_cc.n_glyphs,
                     "most_runs": max(s.get("runs", 0) for s in st), "most_components": max(s.get("components", 0) for s in st),
                     "fallback_words": int(np.count_nonzero(g_cc.word_info[:, 3] & 2)),
                     "columns_ms_median": round(col_ms, 4), "columns_ms_min": round(col_min, 4),
                     "components_ms_median": round(cc_ms, 4), "components_ms_min": round(cc_min, 4),
                     "components_words_per_s": round(g_cc.n_words / (cc_ms / 1e3)), "ratio": round(cc_ms / col_ms, 2),
                     "oracle_match": match})
    det.close()
    print(json.dumps({"bench": "segment_cc", "device": torch.cuda.get_device_name(0), "iters": a.iters, "rows": rows}))
    if not all(r["oracle_match"] for r in rows):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
