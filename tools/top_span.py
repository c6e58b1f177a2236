#!/usr/bin/env python3
"""Top of the detector graph in `rocprofv3 --kernel-trace` runs of bench.py (rocpd SQLite databases), the sibling of tools/front_span.py:
  tools/top_span.py <dir with *_results.db> [<dir> ...]
Per forward step (the launches up to a tail kernel) the span from the start of layer4's first launch to the start of bin_conv1.pyramid, and
the summed duration of the kernels that start inside it.  Co-running launches stretch individually, so only the span compares two schedules
(option top_side).  layer4's first launch is the step's last 3x3 stride-2 split-bf16 conv by start time
(conv_igemm<.., 3, 2, 0, 0, true>: layer2, layer3 and layer4 open with one, in that order on the main stream); bin_conv1.pyramid is the step's
first PYR4 launch (conv_igemm<.., 3, 1, 3, 2, true>).  Steps are grouped by their number of launches and reported as medians in ms."""
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
        s2 = [k for k in st if "conv_igemm<" in k[0] and ", 3, 2, 0, 0, true>" in k[0]]
        pyr = [k for k in st if "conv_igemm<" in k[0] and ", 3, 1, 3, 2, true>" in k[0]]
        if len(s2) < 3 or not pyr:
            continue
        t0 = s2[-1][1]
        t1 = min(k[1] for k in pyr)
        inside = [k for k in st if t0 <= k[1] < t1]
        busy = sum(k[2] - k[1] for k in inside)
        groups.setdefault(len(st), []).append((t1 - t0, busy, len(inside)))
    for nk, v in sorted(groups.items()):
        med = [statistics.median(x[i] for x in v) / 1e6 for i in range(2)]
        print(f"{d}: {len(v):4d} steps of {nk} launches: layer4 start to bin_conv1.pyramid start {med[0]:.3f} ms, kernel time inside {med[1]:.3f} ms "
              f"({statistics.median(x[2] for x in v):.0f} launches start inside)")
