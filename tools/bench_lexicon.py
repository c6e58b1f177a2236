"""Time lexicon matching (csrc/lexicon.hip) and what a lexicon costs in read_words, in one run:
  (a) ocr_lexicon_match alone on device-resident costs: 1 word, 256 words and the whole reading batch (32 pages of 640 x 640 with
      about 100 block words each, the glyph costs of the recogniser's own logits), each against 1 000, 50 000 and 1 000 000 synthetic
      entries of 2..12 characters; per case the time and the DP cells per second (cells = sum over words and candidates of G x M)
  (b) ocr_rec_glyph_costs on 7 300 rows (the reading batch's size) and 65 536 rows, device to device
  (c) reading.read_words without and with the 50 000-entry lexicon on the same pages, alternating call by call
The calls are blocking: a host clock around each is its time (checks, uploads of the offsets and jobs, launches, downloads, sync).
Every measurement is repeated `--repeats` times to show the spread.  The smallest case of (a) is checked against
tests/lexicon_oracle.py outside the timed region.  Prints one JSON line.

    timeout -k 10 900 python tools/bench_lexicon.py [--iters 20] [--repeats 3]

Kernel time: a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/bench_lexicon.py --iters 5 --repeats 1`
(glyph_cost_kernel, lex_raw_kernel, lex_match_kernel, lex_merge_kernel).
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


def _time(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def _cells(gs, lens, max_len_diff=2):
    """DP cells of a match: for every word of G glyphs (1..32) the entries of length M with |M - G| <= max_len_diff, G x M each."""
    count = np.bincount(lens, minlength=34)
    total = 0
    for g, n in zip(*np.unique(gs, return_counts=True)):
        if 1 <= g <= 32:
            total += int(n) * sum(int(count[m]) * int(g) * m for m in range(max(1, g - max_len_diff), min(32, g + max_len_diff) + 1))
    return total


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 50000, 1000000])
    a = ap.parse_args()
    import torch

    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    from tests import lexicon_oracle as LX
    from tests.test_gpu_glyphs import _synthetic_pages

    if not torch.cuda.is_available():
        raise SystemExit("bench_lexicon needs a GPU")
    det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    frames, polys = _synthetic_pages(a.pages, 640, 640, 100, seed=a.pages)
    adj = np.ones((a.pages, 2))
    x = torch.from_numpy(frames).cuda()
    glyphs, crops = reading.glyph_crops(det, frames, polys, adj)
    off = glyphs.word_offsets
    ng = glyphs.n_glyphs
    logits = torch.from_numpy(rec.forward_host(crops)).cuda()
    costs = torch.empty_like(logits)
    torch.cuda.synchronize()
    rec.glyph_costs_device(logits.data_ptr(), ng, costs.data_ptr())
    # one word of 6 glyphs, the first 256 words, the batch
    six = int(np.flatnonzero(np.diff(off) == 6)[0]) if np.any(np.diff(off) == 6) else 0
    batches = {"1_word": (costs[int(off[six]):int(off[six + 1])], np.array([0, off[six + 1] - off[six]], np.int32)),
               "256_words": (costs[:int(off[256])], off[:257]), "batch": (costs, off)}

    rng = np.random.default_rng(1)
    match_rows, lex50k, ok = [], None, True
    for size in a.sizes:
        words = LX.random_words(rng, size, 2, 12)
        lens = np.array([len(w) for w in words])
        lex = capi.Lexicon(rec, words)
        for name, (c, o) in batches.items():
            gs = np.diff(o)
            cells = _cells(gs, lens)
            iters = max(3, a.iters // 4) if cells > 2e10 else a.iters
            reps = []
            for _ in range(a.repeats):
                med, mn = _med_min(_time(lambda: rec.lexicon_match_device(lex, c.data_ptr(), int(o[-1]), o), a.warmup, iters))
                reps.append({"ms": (med, mn), "gcells_per_s": round(cells / (med * 1e-3) / 1e9, 2)})
            match_rows.append({"entries": size, "words": len(o) - 1, "glyphs": int(o[-1]), "case": name, "dp_cells": cells, "iters": iters, "repeats": reps})
        if size == a.sizes[0]:      # outside the timed region: the smallest list against the oracle, bit for bit
            c, o = batches["256_words"]
            got = rec.lexicon_match_device(lex, c.data_ptr(), int(o[-1]), o, {"top_k": 8})
            want = LX.match(c.cpu().numpy(), o, words, top_k=8)
            ok = bool(np.array_equal(got.entries, want["entries"]) and np.array_equal(got.costs.view(np.uint64), want["costs"].view(np.uint64)) and
                      np.array_equal(got.raw_costs.view(np.uint64), want["raw_costs"].view(np.uint64)))
        if size == 50000:
            lex50k = lex
        else:
            lex.close()

    cost_rows = []
    for n in (ng, 65536):
        lg = (torch.randn((n, 62), device="cuda") * 4).contiguous()
        out = torch.empty_like(lg)
        torch.cuda.synchronize()
        cost_rows.append({"rows": n, "repeats_median_min_ms": [_med_min(_time(lambda: rec.glyph_costs_device(lg.data_ptr(), n, out.data_ptr()), a.warmup, a.iters))
                                                               for _ in range(a.repeats)]})

    reading_rows = []
    if lex50k is not None:
        fns = [lambda: reading.read_words(det, rec, x, polys, adj), lambda: reading.read_words(det, rec, x, polys, adj, lexicon=lex50k)]
        for _ in range(a.repeats):
            for fn in fns:
                fn()
            ts = [[], []]
            for _ in range(max(5, a.iters // 2)):
                for k, fn in enumerate(fns):
                    t0 = time.perf_counter()
                    fn()
                    ts[k].append(time.perf_counter() - t0)
            reading_rows.append({"read_words_ms": _med_min(ts[0]), "read_words_lexicon_50000_ms": _med_min(ts[1])})
        lex50k.close()
    rec.close()
    det.close()
    print(json.dumps({"bench": "lexicon", "device": torch.cuda.get_device_name(0), "iters": a.iters, "pages": a.pages, "words": glyphs.n_words,
                      "glyphs": ng, "match": match_rows, "glyph_costs": cost_rows, "read_words": reading_rows, "oracle_match": ok}))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
