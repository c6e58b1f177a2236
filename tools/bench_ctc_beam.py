"""Time ocr_ctc_beam_decode on device memory: 256 x 32 x 63 (the recognition config's batch; a 32 x 128 crop at stride 4 over the
62-symbol alphabet plus the blank) for B in {1, 4, 8, 16, 32}, and 65 536 crops at B = 8.  A call is blocking (it ends in a stream
synchronise), so a host clock around it is the call's time, launch and sync included.  Results are checked against
tests/ctc_beam_oracle.py outside the timed region (the first 256 crops of the large batch).  Prints one JSON line.

    timeout -k 10 600 python tools/bench_ctc_beam.py [--iters 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch

    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    from tests import ctc_beam_oracle as O

    if not torch.cuda.is_available():
        raise SystemExit("bench_ctc_beam needs a GPU")
    rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    rng = np.random.default_rng(0)
    t, c, blank = 32, 63, 62
    rows = []
    for n, b in [(256, 1), (256, 4), (256, 8), (256, 16), (256, 32), (65536, 8)]:
        x = rng.standard_normal((n, t, c)).astype(np.float32)
        x[:, :, blank] += 1.5
        xd = torch.from_numpy(x).cuda()
        lab = torch.empty((n, b, t), dtype=torch.int32, device="cuda")
        ln = torch.empty((n, b), dtype=torch.int32, device="cuda")
        sc = torch.empty((n, b), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def call():
            rec.ctc_beam_decode_device(xd.data_ptr(), n, t, c, blank, b, lab.data_ptr(), ln.data_ptr(), sc.data_ptr())

        for _ in range(a.warmup):
            call()
        ts = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        ms = 1e3 * float(np.median(ts))
        k = min(n, 256)
        wl, wn, ws, wm = O.ctc_beam_decode(x[:k], blank, b)
        ok = wm > 1e-6
        gl, gn, gs = lab[:k].cpu().numpy(), ln[:k].cpu().numpy(), sc[:k].cpu().numpy()
        match = bool(np.array_equal(gl[ok], wl[ok]) and np.array_equal(gn[ok], wn[ok])
                     and np.all(np.abs(gs[ok] - ws[ok]) <= 1e-9 * np.maximum(1.0, np.abs(ws[ok]))))
        rows.append({"n": n, "t": t, "c": c, "beam_width": b, "ms_median": round(ms, 4), "ms_min": round(1e3 * min(ts), 4),
                     "crops_per_s": round(n / (ms / 1e3)), "oracle_match": match, "oracle_crops_checked": int(ok.sum())})
    rec.close()
    print(json.dumps({"bench": "ctc_beam_decode", "device": torch.cuda.get_device_name(0), "iters": a.iters, "rows": rows}))
    if not all(r["oracle_match"] for r in rows):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
