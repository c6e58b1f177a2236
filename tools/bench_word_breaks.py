"""Time ocr_break_words (csrc/word_breaks.hip) and what the `spaces` option costs the reading calls, in one run:
  (a) break_words on the glyph block of the usual reading batch (32 pages of 640 x 640 with about 100 block words each), with
      ocr_group_lines on the same pages beside it, call by call in turn: the yardstick for a small upload-launch-download call;
  (b) break_words on one block of 4 096 words of 256 glyphs each (a million glyphs: the call at its largest per word), and on a
      block of one word of two glyphs (what a call costs when there is nothing to do);
  (c) read_words with and without spaces, with a lexicon and with a language model: the call without spaces is the path the parent
      commit runs, measured in the same run, alternated call by call.
(a) and (b) are timed twice per call: a host clock around the blocking call (validation, copies, kernel, the host's scan into
offsets and the copy of the block) and events on the handle's stream around it (the copies and the kernel only).  --kernel-only
runs (a) and (b) a few times without timing, for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_word_breaks.py
--kernel-only).  Every measurement is repeated `--repeats` times to show the spread.  Outside the timed region the results of (a) and
of the first words of (b) are compared with tests/word_break_oracle.py.  Prints one JSON line.

    timeout -k 10 900 python tools/bench_word_breaks.py [--iters 100] [--repeats 3]
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


def big_block(n_words, G, seed):
    """n_words words of G glyphs: widths 1..12, heights 6..40, letter gaps 0..4 and a word gap of 12..24 after one glyph in seven"""
    rng = np.random.default_rng(seed)
    n = n_words * G
    w = rng.integers(1, 13, n)
    gap = np.where(rng.random(n) < 1 / 7, rng.integers(12, 25, n), rng.integers(0, 5, n))
    x0 = (np.cumsum(w + gap) - w).reshape(n_words, G)
    x0 = (x0 - x0[:, :1]).reshape(-1)
    y0 = rng.integers(0, 8, n)
    boxes = np.stack([x0, y0, x0 + w, y0 + rng.integers(6, 41, n)], axis=1).astype(np.int32)
    info = np.tile(np.array([0, 100, 1, 0], np.int32), (n_words, 1))
    return {"img_offsets": np.array([0, n_words], np.int32), "word_offsets": (np.arange(n_words + 1) * G).astype(np.int32),
            "word_info": info, "word_levels": np.zeros((n_words, 2), np.float32), "boxes": boxes}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--entries", type=int, default=50000)
    ap.add_argument("--check-words", type=int, default=64)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    import torch

    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    from tests import lexicon_oracle as LX
    from tests import word_break_oracle as WB
    from tests.test_gpu_glyphs import _synthetic_pages

    if not torch.cuda.is_available():
        raise SystemExit("bench_word_breaks needs a GPU")
    det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    frames, polys = _synthetic_pages(a.pages, 640, 640, 100, seed=a.pages)
    adj = np.ones((a.pages, 2))
    n, _, h, w = frames.shape
    glyphs = det.segment_glyphs(frames, polys, adj)
    strips = det.plan_word_strips(polys, adj, h, w)
    as_set = lambda b: capi.GlyphSet(b["img_offsets"], b["word_offsets"], b["word_info"], b["word_levels"], b["boxes"])
    big_d = big_block(4096, 256, 7)
    big, tiny = as_set(big_d), as_set(big_block(1, 2, 8))
    if a.kernel_only:
        for _ in range(5):
            det.break_words(glyphs)
            det.break_words(big)
            det.group_lines(strips.quads, strips.img_offsets)
        rec.close()
        det.close()
        return
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

    x = torch.from_numpy(frames).cuda()
    words = LX.random_words(np.random.default_rng(1), a.entries, 2, 12)
    table = capi.char_lm_table(LX.random_words(np.random.default_rng(6), 400, 1, 9), weight=3.0)
    reps = []
    with capi.Lexicon(rec, words) as lex, capi.CharLm(rec, table) as lm:
        for _ in range(a.repeats):
            det.set_stream(stream.cuda_stream)
            rep = {"break_words_pages": timed(lambda: det.break_words(glyphs), a.iters),
                   "group_lines_pages": timed(lambda: det.group_lines(strips.quads, strips.img_offsets), a.iters),
                   "break_words_one_word": timed(lambda: det.break_words(tiny), a.iters),
                   "break_words_4096x256": timed(lambda: det.break_words(big), max(5, a.iters // 10))}
            det.set_stream(None)
            torch.cuda.synchronize()
            it = max(5, a.iters // 10)
            for name, kw in (("plain", {}), ("lexicon", {"lexicon": lex}), ("lm", {"lm": lm})):
                without, with_ = _alternate_ms([lambda: reading.read_words(det, rec, x, polys, adj, **kw),
                                                lambda: reading.read_words(det, rec, x, polys, adj, spaces={}, **kw)], 2, it)
                rep[f"read_words_{name}_ms"] = {"without_spaces": without, "with_spaces": with_}
            reps.append(rep)

    # outside the timed region: against the oracle
    def same(got, want):
        gw, gb = got
        ww, wb = want
        return bool(all(np.array_equal(getattr(gw, k).reshape(-1), np.asarray(ww[k]).reshape(-1)) for k in ("img_offsets", "word_offsets", "word_info", "boxes"))
                    and all(np.array_equal(getattr(gb, k).reshape(-1), wb[k].reshape(-1)) for k in ("source", "sub_offsets", "gap_pct", "source_info")))
    got = det.break_words(glyphs)
    pages_d = dict(img_offsets=glyphs.img_offsets, word_offsets=glyphs.word_offsets, word_info=glyphs.word_info, word_levels=glyphs.word_levels,
                   boxes=glyphs.boxes)
    match = same(got, WB.break_words(pages_d))
    nchk = min(a.check_words, 4096)
    head = dict(big_d, img_offsets=np.array([0, nchk], np.int32), word_offsets=big_d["word_offsets"][:nchk + 1], word_info=big_d["word_info"][:nchk],
                word_levels=big_d["word_levels"][:nchk], boxes=big_d["boxes"][:nchk * 256])
    match_big = same(det.break_words(as_set(head)), WB.break_words(head))
    got_big = det.break_words(big)
    row = {"pages": a.pages, "h": h, "w": w, "words": glyphs.n_words, "glyphs": glyphs.n_glyphs, "sub_words": got[1].n_words,
           "rules_pages": np.bincount(got[1].source_info[:, 1], minlength=3).tolist(),
           "big_words": big.n_words, "big_glyphs": big.n_glyphs, "big_sub_words": got_big[1].n_words,
           "rules_big": np.bincount(got_big[1].source_info[:, 1], minlength=3).tolist(), "lexicon_entries": len(words),
           "repeats_median_min_ms": reps, "oracle_match_pages": match, "oracle_match_big_first_words": match_big, "big_words_checked": nchk}
    rec.close()
    det.close()
    print(json.dumps({"bench": "word_breaks", "device": torch.cuda.get_device_name(0), "iters": a.iters, "row": row}))
    if not (match and match_big):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
