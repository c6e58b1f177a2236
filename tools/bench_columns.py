"""Time ocr_group_columns (csrc/columns.hip) against ocr_group_lines (csrc/lines.hip) in one run, call by call in turn:
  (a) both on the workload of tools/bench_lines.py: 32 pages of 640 x 640 with about 100 block words each, the quads of
      ocr_plan_word_strips
  (b) both on one image of 4 096 words (the cap)
  (c) the worst case of stage E alone: 4 096 single-word blocks on a lattice of 256 rows x 16 columns at max_levels = 256 (a block is
      preceded by the blocks above it and left of it, so the levels climb to the cap round by round: all 255 rounds run)
Both calls are blocking: a host clock around a call is its time (checks, uploads, launches, downloads, sync, CSR assembly).  The two
calls alternate after a warm-up so drift lands on both; every measurement is repeated `--repeats` times to show the spread.  The
results of (a) and (b) are checked against tests/column_oracle.py outside the timed region.  Prints one JSON line.

    timeout -k 10 600 python tools/bench_columns.py [--iters 200] [--repeats 3]

Kernel time: a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/bench_columns.py --iters 50 --repeats 1`
(the three kernels of lines.hip, column_gap_kernel, pair_link_kernel<Gap>, column_line_kernel, pair_link_kernel<Line>,
column_block_kernel).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _med_min(ts):
    return (round(1e3 * float(np.median(ts)), 4), round(1e3 * min(ts), 4))


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
    return [_med_min(t) for t in ts]


def lattice(rows=256, cols=16, pitch_x=80.0, pitch_y=60.0):
    """rows x cols words of 30 x 14, further apart than every reach (a gap of 3.6 heights is beyond row_gap = 3, a pitch of 4.3
    heights beyond block_reach): every word is a line and a block of its own, preceded by the blocks left of it in its row and above
    it in its column, so its level is row + column and the last rows sit at the cap of 255"""
    from tests import line_oracle as LO
    return np.array([LO.quad(100.0 + pitch_x * k, 100.0 + pitch_y * r, 30.0, 14.0) for r in range(rows) for k in range(cols)])


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
    from tests import column_oracle as CO
    from tests import line_oracle as LO
    from tests.test_gpu_glyphs import _synthetic_pages

    if not torch.cuda.is_available():
        raise SystemExit("bench_columns needs a GPU")
    det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    _, polys = _synthetic_pages(a.pages, 640, 640, 100, seed=a.pages)
    strips = det.plan_word_strips(polys, np.ones((a.pages, 2)), 640, 640)
    big = LO.fuzz(capi.LINE_MAX_WORDS, seed=5)
    worst = lattice()
    worst_params = capi.column_params(max_levels=256, row_gap=3.0)

    reps = []
    for _ in range(a.repeats):
        rep = {}
        rep["pages_lines_ms"], rep["pages_columns_ms"] = _alternate_ms(
            [lambda: det.group_lines(strips.quads, strips.img_offsets), lambda: det.group_columns(strips.quads, strips.img_offsets)],
            a.warmup, a.iters)
        rep["one_image_lines_ms"], rep["one_image_columns_ms"] = _alternate_ms(
            [lambda: det.group_lines(big, [0, len(big)]), lambda: det.group_columns(big, [0, len(big)])], a.warmup, max(20, a.iters // 4))
        rep["lattice_256_levels_ms"] = _alternate_ms([lambda: det.group_columns(worst, [0, len(worst)], worst_params)], 2, 5)[0]
        reps.append(rep)

    # outside the timed region: both results against the oracle
    def same(got, want):
        return all(np.array_equal(getattr(got, k).reshape(-1).view(np.uint64 if want[k].dtype == np.float64 else np.int32),
                                  want[k].view(np.uint64 if want[k].dtype == np.float64 else np.int32)) for k in CO.ARRAYS)
    got_pages, got_big = det.group_columns(strips.quads, strips.img_offsets), det.group_columns(big, [0, len(big)])
    got_worst = det.group_columns(worst, [0, len(worst)], worst_params)
    match = same(got_pages, CO.group(strips.quads, strips.img_offsets)) and same(got_big, CO.group(big, [0, len(big)]))
    row = {"pages": a.pages, "words": strips.n_words, "lines": got_pages.n_lines, "blocks": got_pages.n_blocks,
           "one_image_words": len(big), "one_image_lines": got_big.n_lines, "one_image_blocks": got_big.n_blocks,
           "one_image_top_level": int(got_big.block_levels.max()), "lattice_blocks": got_worst.n_blocks,
           "lattice_top_level": int(got_worst.block_levels.max()), "repeats_median_min_ms": reps, "oracle_match": match}
    det.close()
    print(json.dumps({"bench": "columns", "device": torch.cuda.get_device_name(0), "iters": a.iters, "row": row}))
    if not match:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
