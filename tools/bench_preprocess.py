"""Time the step in front of the detector: 32 decoded pages to 32 frames of 640 x 640 f32 on the device.
  single   n calls of ocr_preprocess_image, one image each (two kernels, six table uploads and two stream synchronisations per call)
  batch    one ocr_preprocess_batch (blocking), or one ocr_preprocess_batch_async + ocr_det_synchronize
for device-resident sources (device -> device) and for pinned host sources (host -> device; the single-image call has one memory kind
for both sides, so its leg writes pinned host frames and uploads them in one copy at the end).  Both legs run in one process, after a
warm-up of every shape, alternating; a host clock around work that ends in a device synchronise; median, min and max of each side.
The frames of the two legs are compared bit for bit outside the timed region.  Also the device time of the batch launch (events on the
handle's stream around plan upload + kernel) and the compulsory bytes - every source read once, every frame written once - over it:
a figure for one HBM-bound kernel, not for the pipeline.  Decoding and the transport of the RGBA pixels to where the call finds
them are outside what is timed.  Prints a table and one JSON line.

    timeout -k 10 600 python tools/bench_preprocess.py [--reps 7] [--n 32]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29   # HBM3E peak and the measured float4-copy rate of the MI355X


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(ts.min()), 3), "max_ms": round(float(ts.max()), 3)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--target", type=int, default=640)
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("at least five alternations")
    import torch

    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W

    if not torch.cuda.is_available():
        raise SystemExit("bench_preprocess needs a GPU")
    L = capi.lib()
    det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    n, T = a.n, a.target
    px = T * T
    rows = []
    for w, h in ((1600, 1200), (1240, 1754)):
        rng = np.random.RandomState(w)
        pinned = [capi.HostBuffer((h, w, 4), np.uint8) for _ in range(n)]
        for b in pinned:
            b.array[:] = rng.randint(0, 256, (h, w, 4), dtype=np.uint8)
        dev = [torch.from_numpy(b.array).cuda() for b in pinned]
        out_single = torch.empty((n, 1, T, T), dtype=torch.float32, device="cuda")
        out_batch = torch.empty_like(out_single)
        host_frames = capi.HostBuffer((n, 1, T, T), np.float32)
        host_frames_t = torch.from_numpy(host_frames.array)
        adj1, adjn = (C.c_double * 2)(), np.zeros((n, 2))
        adjn_p = adjn.ctypes.data_as(C.POINTER(C.c_double))
        d_dev, _, _ = capi.Detector._image_descs(dev)
        d_host, _, _ = capi.Detector._image_descs([b.array for b in pinned])
        torch.cuda.synchronize()

        def single_dev():
            for i in range(n):
                capi.check(L.ocr_preprocess_image(det._h, dev[i].data_ptr(), w, h, T, T, None, out_single.data_ptr() + 4 * px * i, adj1, capi.MEM_DEVICE))

        def batch_dev():
            capi.check(L.ocr_preprocess_batch(det._h, d_dev, n, capi.MEM_DEVICE, T, T, None, out_batch.data_ptr(), capi.MEM_DEVICE, adjn_p))

        def batch_dev_async():
            capi.check(L.ocr_preprocess_batch_async(det._h, d_dev, n, T, T, None, out_batch.data_ptr(), adjn_p))
            det.synchronize()

        def single_host():
            for i in range(n):
                capi.check(L.ocr_preprocess_image(det._h, pinned[i].array.ctypes.data, w, h, T, T, None, host_frames.array.ctypes.data + 4 * px * i, adj1,
                                                  capi.MEM_HOST))
            out_single.copy_(host_frames_t, non_blocking=True)
            torch.cuda.synchronize()

        def batch_host():
            capi.check(L.ocr_preprocess_batch(det._h, d_host, n, capi.MEM_HOST, T, T, None, out_batch.data_ptr(), capi.MEM_DEVICE, adjn_p))

        legs = {"single_dev": single_dev, "batch_dev": batch_dev, "batch_dev_async": batch_dev_async, "single_host": single_host, "batch_host": batch_host}
        times = {k: [] for k in legs}
        for fn in legs.values():      # warm-up of every shape and path
            fn()
        for pair in (("single_dev", "batch_dev", "batch_dev_async"), ("single_host", "batch_host")):
            for k in pair[1:]:        # the same frames, outside the timed region
                out_single.zero_()
                out_batch.fill_(-1.0)
                torch.cuda.synchronize()
                legs[pair[0]]()
                legs[k]()
                if not torch.equal(out_single, out_batch):
                    raise SystemExit(f"{k}: frames differ from {pair[0]}")
            for _ in range(a.reps):   # alternating
                for k in pair:
                    t0 = time.perf_counter()
                    legs[k]()
                    times[k].append(time.perf_counter() - t0)
        # device time of the batch launch: events on the handle's stream around the plan upload and the kernel
        stream = torch.cuda.Stream()
        det.set_stream(stream.cuda_stream)
        ev = []
        for _ in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record()
                capi.check(L.ocr_preprocess_batch_async(det._h, d_dev, n, T, T, None, out_batch.data_ptr(), adjn_p))
                e1.record()
            det.synchronize()
            ev.append(e0.elapsed_time(e1) / 1e3)
        det.set_stream(None)
        ev = ev[1:]
        nbytes = n * (4 * w * h + 4 * px)
        launch_s = float(np.median(ev))
        row = {"w": w, "h": h, "n": n, "target": T, "source_bytes": n * 4 * w * h, "compulsory_bytes": nbytes,
               **{k: stats(v) for k, v in times.items()}, "batch_launch_device": stats(ev),
               "compulsory_TBps": round(nbytes / launch_s / 1e12, 3),
               "share_of_hbm_spec": round(nbytes / launch_s / 1e12 / HBM_SPEC_TBS, 3), "share_of_hbm_copy_rate": round(nbytes / launch_s / 1e12 / HBM_COPY_TBS, 3)}
        sd, bd = row["single_dev"], row["batch_dev"]
        row["dev_margin_ms"] = round(sd["median_ms"] - bd["median_ms"], 3)
        row["single_dev_spread_ms"] = round(sd["max_ms"] - sd["min_ms"], 3)
        row["accepted"] = bool(bd["median_ms"] < sd["median_ms"] and row["dev_margin_ms"] > row["single_dev_spread_ms"])
        rows.append(row)
        print(f"{n} pages of {w} x {h} -> {T} x {T} f32 frames on the device, {a.reps} alternations, ms median (min .. max)")
        for k in legs:
            s = row[k]
            print(f"  {k:16s} {s['median_ms']:9.3f}  ({s['min_ms']:.3f} .. {s['max_ms']:.3f})")
        s = row["batch_launch_device"]
        print(f"  batch launch on the device (plan upload + kernel, events) {s['median_ms']:.3f} ({s['min_ms']:.3f} .. {s['max_ms']:.3f}); compulsory "
              f"{nbytes / 1e6:.1f} MB -> {row['compulsory_TBps']:.3f} TB/s = {100 * row['share_of_hbm_spec']:.1f} % of the {HBM_SPEC_TBS} TB/s HBM peak "
              f"({100 * row['share_of_hbm_copy_rate']:.1f} % of the measured {HBM_COPY_TBS} TB/s copy rate): one HBM-bound kernel")
        print(f"  device -> device: batch ahead by {row['dev_margin_ms']:.3f} ms, spread of the single-call leg {row['single_dev_spread_ms']:.3f} ms: "
              f"{'accepted' if row['accepted'] else 'NOT accepted'}")
        del dev, out_single, out_batch
        for b in pinned:
            b.close()
        host_frames_t = None
        host_frames.close()
    det.close()
    print(json.dumps({"bench": "preprocess_batch", "device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows}))
    if not all(r["accepted"] for r in rows):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
