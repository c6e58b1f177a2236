"""Time ocr_extract_curved_strips beside ocr_extract_word_strips on the same polygons, in one run: the workload of
tools/bench_glyph_masks.py (32 device-resident pages of 640 x 640 with about 100 block words each).  Both calls are blocking, so a
host clock around a call is its time: host-side preparation of the word table, the copies of the tables, the launch and the sync
included.  The two are alternated call by call after a warm-up - straight, curved, straight, curved, ... - so drift of the clocks or
the machine lands on both sides, and the whole measurement is repeated `--repeats` times to show the spread between repeats.  The two
planners (host code, no GPU work) are timed the same way.

The curved atlas is checked against tests/curved_strip_oracle.py and the straight one against tests/strip_oracle.py outside the
timed region.  Prints one JSON line.

    timeout -k 10 600 python tools/bench_curved_strips.py [--iters 200] [--repeats 3]

Kernel time: a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/bench_curved_strips.py`
(strip_kernel, curved_strip_kernel).
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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pages", type=int, default=32)
    a = ap.parse_args()
    import torch

    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    from tests import curved_strip_oracle as CS
    from tests import strip_oracle as S
    from tests.test_gpu_glyphs import _synthetic_pages

    if not torch.cuda.is_available():
        raise SystemExit("bench_curved_strips needs a GPU")
    det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    frames, polys = _synthetic_pages(a.pages, 640, 640, 100, seed=a.pages)
    adj = np.ones((a.pages, 2))
    x = torch.from_numpy(frames).cuda()
    block, keep = capi.python_to_polygons(polys, [[0.0] * len(p) for p in polys])
    n, _, h, w = frames.shape
    ptr = x.data_ptr()
    straight = det.plan_word_strips(block, adj, h, w)
    curved = det.plan_curved_strips(block, adj, h, w)
    sat = torch.empty((straight.height, straight.total_width), dtype=torch.float32, device="cuda")
    cat = torch.empty((curved.height, curved.total_width), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ext_fns = [lambda: det.extract_word_strips_device(ptr, n, h, w, straight, sat.data_ptr()),
               lambda: det.extract_curved_strips_device(ptr, n, h, w, curved, cat.data_ptr())]
    plan_fns = [lambda: det.plan_word_strips(block, adj, h, w), lambda: det.plan_curved_strips(block, adj, h, w)]
    reps = []
    for _ in range(a.repeats):
        rep = {}
        (rep["extract_word_strips_ms"], rep["extract_curved_strips_ms"]) = _alternate_ms(ext_fns, a.warmup, a.iters)
        (rep["plan_word_strips_ms"], rep["plan_curved_strips_ms"]) = _alternate_ms(plan_fns, 2, max(5, a.iters // 10))
        reps.append(rep)
    # outside the timed region: both atlases of the last calls against their oracles
    cwant = CS.plan(polys, adj)
    swant = S.plan(polys, adj)
    match = bool(np.array_equal(cat.cpu().numpy().view(np.uint32), CS.extract(frames, cwant).view(np.uint32)) and
                 np.array_equal(sat.cpu().numpy().view(np.uint32), S.extract(frames, swant).view(np.uint32)))
    row = {"pages": a.pages, "h": h, "w": w, "words": curved.n_words, "strip_height": curved.height,
           "straight_columns": straight.total_width, "curved_columns": curved.total_width,
           "curved_flags": {str(k): int(v) for k, v in zip(*np.unique(curved.word_info[:, 1], return_counts=True))},
           "repeats_median_min_ms": reps, "oracle_match": match}
    det.close()
    print(json.dumps({"bench": "curved_strips", "device": torch.cuda.get_device_name(0), "iters": a.iters, "row": row}))
    if not match:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
