"""Time ocr_lexicon_phrase_match (csrc/lexicon_phrase.hip) and what the `phrases` option costs the reading calls, in one run:
  (a) the phrase match on the glyph costs of the usual reading batch (32 pages of 640 x 640 with about 100 block words each, every
      polygon a line) against a lexicon of 50 000 entries, with ocr_lexicon_match on the same costs beside it, call by call in turn:
      that call is the yardstick, the phrase match does about G times the table reads per polygon;
  (b) one line of 256 glyphs against 50 000 and against 1 000 000 entries;
  (c) read_words with and without phrases=, alternated call by call.
(a) and (b) are timed twice per call: a host clock around the blocking call and events on the handle's stream around it.
--kernel-only runs (a) and (b) a few times without timing, for a kernel trace (rocprofv3 --kernel-trace --stats -- python
tools/bench_phrase.py --kernel-only).  Every measurement is repeated `--repeats` times to show the spread.  Outside the timed region
the result of (a) on its first lines and of (b) against the small lexicon are compared with tests/phrase_oracle.py.  Prints one JSON
line, with the table reads (cells: one per start, entry and character) a second of the match.

    timeout -k 10 900 python tools/bench_phrase.py [--iters 100] [--repeats 3]
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
    """the calls in turn, `iters` rounds: (median, min) ms of a host clock around each"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    ts = [[] for _ in fns]
    for _ in range(iters):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    return [_med_min(t) for t in ts]


def cells(line_lengths, entry_lengths):
    """table reads of the match: for every line of G glyphs and every entry of M <= G characters, (G - M + 1) starts x M characters"""
    g = np.asarray(line_lengths, np.int64)
    g = g[(g >= 1) & (g <= 256)]
    hist = np.bincount(np.asarray(entry_lengths, np.int64), minlength=33)
    total = 0
    for m in range(1, 33):
        if hist[m]:
            total += int(hist[m]) * m * int(np.maximum(g - m + 1, 0).sum())
    return total


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--entries", type=int, default=50000)
    ap.add_argument("--big-entries", type=int, default=1000000)
    ap.add_argument("--check-lines", type=int, default=64)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    import torch

    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    from tests import lexicon_oracle as LX
    from tests import phrase_oracle as PO
    from tests.test_gpu_glyphs import _synthetic_pages

    if not torch.cuda.is_available():
        raise SystemExit("bench_phrase needs a GPU")
    det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    frames, polys = _synthetic_pages(a.pages, 640, 640, 100, seed=a.pages)
    adj = np.ones((a.pages, 2))
    n, _, h, w = frames.shape
    glyphs, crops = reading.glyph_crops(det, frames, polys, adj)
    costs = rec.glyph_costs(rec.forward_host(crops))
    off = glyphs.word_offsets
    dcosts = torch.from_numpy(costs).cuda()
    rng = np.random.default_rng(3)
    line = torch.from_numpy(LX.make_costs(rng, 256)).cuda()
    line_off = np.array([0, 256], np.int32)
    words = LX.random_words(np.random.default_rng(1), a.entries, 2, 12)
    big_words = LX.random_words(np.random.default_rng(2), a.big_entries, 2, 12)
    stream = torch.cuda.Stream()

    def timed(fn, iters):
        """host clock around the blocking call and events on the handle's stream around the same call"""
        host, dev = [], []
        for k in range(a.warmup + iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record()
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                e1.record()
            e1.synchronize()
            if k >= a.warmup:
                host.append(t1 - t0)
                dev.append(e0.elapsed_time(e1) / 1e3)
        return {"host_ms": _med_min(host), "events_ms": _med_min(dev)}

    def alternate_timed(fns, iters):
        """timed() over several calls in turn, call by call"""
        out = [{"host": [], "dev": []} for _ in fns]
        for k in range(a.warmup + iters):
            for j, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(stream):
                    e0.record()
                    t0 = time.perf_counter()
                    fn()
                    t1 = time.perf_counter()
                    e1.record()
                e1.synchronize()
                if k >= a.warmup:
                    out[j]["host"].append(t1 - t0)
                    out[j]["dev"].append(e0.elapsed_time(e1) / 1e3)
        return [{"host_ms": _med_min(o["host"]), "events_ms": _med_min(o["dev"])} for o in out]

    reps = []
    with capi.Lexicon(rec, words) as lex, capi.Lexicon(rec, big_words) as big:
        phrase_pages = lambda: rec.phrase_match_device(lex, dcosts.data_ptr(), costs.shape[0], off)
        match_pages = lambda: rec.lexicon_match_device(lex, dcosts.data_ptr(), costs.shape[0], off)
        phrase_line = lambda: rec.phrase_match_device(lex, line.data_ptr(), 256, line_off)
        phrase_line_big = lambda: rec.phrase_match_device(big, line.data_ptr(), 256, line_off)
        if a.kernel_only:
            for _ in range(5):
                phrase_pages()
                match_pages()
                phrase_line()
                phrase_line_big()
        x = torch.from_numpy(frames).cuda()
        for _ in range(0 if a.kernel_only else a.repeats):
            rec.set_stream(stream.cuda_stream)
            pp, mp = alternate_timed([phrase_pages, match_pages], a.iters)
            rep = {"phrase_match_pages": pp, "lexicon_match_pages": mp, "phrase_match_line256": timed(phrase_line, a.iters),
                   "phrase_match_line256_big": timed(phrase_line_big, max(5, a.iters // 5))}
            rec.set_stream(None)
            torch.cuda.synchronize()
            it = max(5, a.iters // 10)
            without, with_, spaced = _alternate_ms([lambda: reading.read_words(det, rec, x, polys, adj),
                                                    lambda: reading.read_words(det, rec, x, polys, adj, phrases={"lexicon": lex}),
                                                    lambda: reading.read_words(det, rec, x, polys, adj, spaces={}, phrases={"lexicon": lex})], 2, it)
            rep["read_words_ms"] = {"without_phrases": without, "with_phrases": with_, "with_spaces_and_phrases": spaced}
            reps.append(rep)

        # outside the timed region: against the oracle
        def same(got, want):
            return bool(all(np.array_equal(getattr(got, k).view(np.uint8), want[k].view(np.uint8)) for k in want))
        nchk = 0 if a.kernel_only else min(a.check_lines, len(off) - 1)
        g1 = int(off[nchk])
        match = same(rec.phrase_match(lex, costs[:g1], off[:nchk + 1]), PO.phrase_match(costs[:g1], off[:nchk + 1], words))
        lc = line.cpu().numpy()
        match_line = same(rec.phrase_match(lex, lc, line_off), PO.phrase_match(lc, line_off, words))
        got = phrase_pages()
    if a.kernel_only:
        rec.close()
        det.close()
        return
    lens = np.diff(off)
    elens, blens = [len(x_) for x_ in words], [len(x_) for x_ in big_words]
    row = {"pages": a.pages, "h": h, "w": w, "lines": len(off) - 1, "glyphs": int(costs.shape[0]), "words_found": got.n_words,
           "lexicon_words_found": int(np.count_nonzero(got.entries >= 0)), "longest_line": int(lens.max()) if len(lens) else 0,
           "lexicon_entries": len(words), "big_entries": len(big_words), "cells_pages": cells(lens, elens),
           "cells_line256": cells([256], elens), "cells_line256_big": cells([256], blens), "repeats_median_min_ms": reps,
           "oracle_match_pages_first_lines": match, "lines_checked": nchk, "oracle_match_line256": match_line}
    rec.close()
    det.close()
    print(json.dumps({"bench": "phrase", "device": torch.cuda.get_device_name(0), "iters": a.iters, "row": row}))
    if not (match and match_line):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
