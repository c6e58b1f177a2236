#!/usr/bin/env python3
"""Back-to-back forward time under engine option sets, alternating over rounds (run on the GPU box).
  tools/bench_front_split.py <n> <size> <rounds> <options> [<options> ...]     ("none" = the default engine)
Every round makes one handle per option set in turn (one handle alive at a time: which hardware queue a stream gets depends
on the streams made before it), warms it up and keeps the best of three timings of 20 calls behind one synchronise.
Prints the min and the median over the rounds."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import ocr_rs_amd  # noqa: E402,F401
from ocr_rs_amd import capi, weights as W  # noqa: E402

n, size, rounds = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
opts = [None if o == "none" else o for o in sys.argv[4:]]
x = torch.from_numpy(W.synth_image_batch(1, n, size, size)).cuda()
prob = torch.empty_like(x)
blob = W.pack_blob(W.make_det_weights(0))
ms = [[] for _ in opts]
for r in range(rounds):
    for i, o in enumerate(opts):
        det = capi.Detector(blob, 0, options=o)
        for _ in range(10):
            det.forward_device(x.data_ptr(), n, size, size, prob.data_ptr(), 0, 0.6)
        det.synchronize()
        best = 1e9
        for rep in range(3):
            t = time.perf_counter()
            for _ in range(20):
                det.forward_device(x.data_ptr(), n, size, size, prob.data_ptr(), 0, 0.6)
            det.synchronize()
            best = min(best, (time.perf_counter() - t) / 20 * 1e3)
        ms[i].append(best)
        det.close()
for o, m in zip(opts, ms):
    print(f"n={n} {size}x{size} {str(o):36s} min {min(m):.4f} median {statistics.median(m):.4f} ms", flush=True)
