"""Time ocr_group_lines (csrc/lines.hip) and what read_lines costs over read_words_rectified, in one run:
  (a) group_lines on the workload of tools/bench_curved_strips.py: 32 pages of 640 x 640 with about 100 block words each, the quads of
      ocr_plan_word_strips
  (b) group_lines on one image of 4 096 words (the cap: 16.7 M oriented pair tests, twice)
  (c) reading.read_lines against reading.read_words_rectified on the pages of (a): the difference is the cost of the feature (the
      second ocr_plan_word_strips on the host, the group call, the Python loop over the lines)
The group call is blocking: a host clock around it is its time (checks, uploads, three launches, downloads, sync, CSR assembly), and
HIP events on the handle's stream around it give the span on the device side of the same call.  (c) alternates the two readers call
by call after a warm-up so drift lands on both; every measurement is repeated `--repeats` times to show the spread.  The results of
(a) and (b) are checked against tests/line_oracle.py outside the timed region.  Prints one JSON line.

    timeout -k 10 600 python tools/bench_lines.py [--iters 200] [--repeats 3]

Kernel time: a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/bench_lines.py --iters 50 --repeats 1`
(line_feature_kernel, line_link_kernel, line_chain_kernel).
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pages", type=int, default=32)
    a = ap.parse_args()
    import torch

    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    from tests import line_oracle as LO
    from tests.test_gpu_glyphs import _synthetic_pages

    if not torch.cuda.is_available():
        raise SystemExit("bench_lines needs a GPU")
    det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    frames, polys = _synthetic_pages(a.pages, 640, 640, 100, seed=a.pages)
    adj = np.ones((a.pages, 2))
    x = torch.from_numpy(frames).cuda()
    n, _, h, w = frames.shape
    strips = det.plan_word_strips(polys, adj, h, w)
    big = LO.fuzz(capi.LINE_MAX_WORDS, seed=5)
    stream = torch.cuda.Stream()
    det.set_stream(stream.cuda_stream)

    def group_timed(quads, offsets, iters):
        """host clock around the blocking call and events on the handle's stream around the same call"""
        host, dev = [], []
        for k in range(a.warmup + iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record()
                t0 = time.perf_counter()
                det.group_lines(quads, offsets)
                t1 = time.perf_counter()
                e1.record()
            e1.synchronize()
            if k >= a.warmup:
                host.append(t1 - t0)
                dev.append(e0.elapsed_time(e1) / 1e3)
        return {"host_ms": _med_min(host), "events_ms": _med_min(dev)}

    reps = []
    for _ in range(a.repeats):
        rep = {"pages": group_timed(strips.quads, strips.img_offsets, a.iters), "one_image_4096": group_timed(big, [0, len(big)], max(20, a.iters // 4))}
        det.set_stream(None)
        torch.cuda.synchronize()
        rep["read_words_rectified_ms"], rep["read_lines_ms"] = _alternate_ms(
            [lambda: reading.read_words_rectified(det, rec, x, polys, adj), lambda: reading.read_lines(det, rec, x, polys, adj)],
            3, max(10, a.iters // 10))
        rep["plan_word_strips_ms"] = _alternate_ms([lambda: det.plan_word_strips(polys, adj, h, w)], 2, max(10, a.iters // 10))[0]
        det.set_stream(stream.cuda_stream)
        reps.append(rep)
    det.set_stream(None)

    # outside the timed region: both results against the oracle
    def same(got, want):
        return bool(got.img_offsets.tolist() == want["img_offsets"].tolist() and got.line_offsets.tolist() == want["line_offsets"].tolist() and
                    got.order.tolist() == want["order"].tolist() and got.word_flags.tolist() == want["word_flags"].tolist() and
                    np.array_equal(got.gaps.view(np.uint64), want["gaps"].view(np.uint64)))
    got_pages, got_big = det.group_lines(strips.quads, strips.img_offsets), det.group_lines(big, [0, len(big)])
    match = same(got_pages, LO.group(strips.quads, strips.img_offsets)) and same(got_big, LO.group(big, [0, len(big)]))
    row = {"pages": a.pages, "h": h, "w": w, "words": strips.n_words, "lines": got_pages.n_lines, "max_words_per_page": int(np.diff(strips.img_offsets).max()),
           "one_image_words": len(big), "one_image_lines": got_big.n_lines, "repeats_median_min_ms": reps, "oracle_match": match}
    rec.close()
    det.close()
    print(json.dumps({"bench": "line_grouping", "device": torch.cuda.get_device_name(0), "iters": a.iters, "row": row}))
    if not match:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
