#!/usr/bin/env python3
"""Front of the detector graph in `rocprofv3 --kernel-trace` runs of bench.py (rocpd SQLite databases):
  tools/front_span.py <dir with *_results.db> [<dir> ...]
Per forward step (the launches up to a tail kernel) the span from the start of the first stem launch to the end of the last
layer2 launch, and the summed duration of the kernels that start inside it.  Co-running launches stretch individually, so
only the span compares two schedules.  layer2's launches are the step's fused-Winograd <c128> launches except the last one
by start time (p3's lateral term, which every schedule queues behind layer2).  Steps are grouped by their number of stem
launches (1: one frame group, 2: the split front) and reported as medians in ms."""
import glob
import os
import sqlite3
import statistics
import sys

for d in sys.argv[1:]:
    db = glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
    s_col = "start" if "start" in cols else "start_time"
    e_col = "end" if "end" in cols else "end_time"
    rows = c.execute(f'select name, "{s_col}", "{e_col}" from kernels order by "{s_col}"').fetchall()
    steps, cur = [], []
    for name, s, e in rows:
        cur.append((name, s, e))
        if "tail" in name:
            steps.append(cur)
            cur = []
    groups = {}
    for st in steps:
        stems = [k for k in st if "stem" in k[0]]
        c128 = [k for k in st if "winograd43_fused_kernel<8>" in k[0]]
        if not stems or len(c128) < 2:
            continue
        t0 = min(k[1] for k in stems)
        t1 = max(k[2] for k in c128[:-1])
        busy = sum(k[2] - k[1] for k in st if t0 <= k[1] < t1)
        whole = st[-1][2] - t0
        groups.setdefault((len(stems), len(st)), []).append((t1 - t0, busy, whole))
    for (nstem, nk), v in sorted(groups.items()):
        med = [statistics.median(x[i] for x in v) / 1e6 for i in range(3)]
        print(f"{d}: {len(v):4d} steps of {nk} launches, {nstem} stem launch(es): front span {med[0]:.3f} ms, kernel time inside {med[1]:.3f} ms, "
              f"stem start to tail end {med[2]:.3f} ms")
