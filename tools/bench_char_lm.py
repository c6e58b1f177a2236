"""Time the character language model (csrc/char_lm.hip) and what a model costs in read_words, in one run:
  (a) ocr_lm_decode alone on device-resident costs at top_k 1, 2 and 8: the whole reading batch (32 pages of 640 x 640 with about 100
      block words each, the glyph costs of the recogniser's own logits), one word of 32 glyphs, and 65 536 glyphs' worth of words (the
      batch's words repeated); per case the time and the DP transitions per second (transitions = sum over decoded words of
      (G - 1) x 62 x 62 x top_k candidate reads, an upper bound: the kernel leaves a list early)
  (b) ocr_lexicon_match against 50 000 entries on the same batch, for context
  (c) reading.read_words without and with the model on the same pages, alternating call by call
The calls are blocking: a host clock around each is its time (checks, uploads, one launch, downloads, sync).  Every measurement is
repeated `--repeats` times to show the spread.  The batch at top_k 8 is checked against tests/char_lm_oracle.py outside the timed
region.  Prints one JSON line.

    timeout -k 10 600 python tools/bench_char_lm.py [--iters 12] [--repeats 2]

Kernel time: a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/bench_char_lm.py --iters 5 --repeats 1`
(lm_decode_kernel).
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


def _transitions(gs, k):
    g = np.asarray(gs, np.int64)
    g = g[(g >= 1) & (g <= 32)]
    return int(((g - 1) * 62 * 62 * k).sum())


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--pages", type=int, default=32)
    a = ap.parse_args()
    import torch

    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    from tests import char_lm_oracle as LM
    from tests import lexicon_oracle as LX
    from tests.test_gpu_glyphs import _synthetic_pages

    if not torch.cuda.is_available():
        raise SystemExit("bench_char_lm needs a GPU")
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
    rng = np.random.default_rng(1)
    table = capi.char_lm_table(LX.random_words(rng, 20000, 2, 12), weight=2.0)
    lm = capi.CharLm(rec, table)

    # one word of 32 glyphs (the batch's first 32 rows), and the batch repeated up to 65 536 glyphs
    reps_needed = -(-65536 // max(ng, 1))
    big_costs = costs.repeat(reps_needed, 1).contiguous()
    big_off = np.concatenate([[0]] + [off[1:].astype(np.int64) + r * ng for r in range(reps_needed)])
    cut = int(np.searchsorted(big_off, 65536, side="right")) - 1
    big_off = big_off[:cut + 1].astype(np.int32)
    batches = {"batch": (costs, off), "1_word_of_32": (costs[:32].contiguous(), np.array([0, 32], np.int32)),
               "65536_glyphs": (big_costs[:int(big_off[-1])], big_off)}
    torch.cuda.synchronize()

    rows = []
    for name, (c, o) in batches.items():
        for k in (1, 2, 8):
            tr = _transitions(np.diff(o), k)
            reps = []
            for _ in range(a.repeats):
                med, mn = _med_min(_time(lambda: rec.lm_decode_device(lm, c.data_ptr(), int(o[-1]), o, {"top_k": k}), a.warmup, a.iters))
                reps.append({"ms": (med, mn), "gtransitions_per_s": round(tr / (med * 1e-3) / 1e9, 2)})
            rows.append({"case": name, "top_k": k, "words": len(o) - 1, "glyphs": int(o[-1]), "transitions": tr, "repeats": reps})
    # outside the timed region: the batch at top_k 8 against the oracle, bit for bit
    got = rec.lm_decode_device(lm, costs.data_ptr(), ng, off, {"top_k": 8})
    want = LM.decode(costs.cpu().numpy(), off, table, top_k=8)
    ok = bool(np.array_equal(got.labels, want["labels"]) and np.array_equal(got.costs.view(np.uint64), want["costs"].view(np.uint64)) and
              np.array_equal(got.raw_costs.view(np.uint64), want["raw_costs"].view(np.uint64)))
    changed = int(sum(got.text(off, w) != "".join(LM.ALPHABET[int(v)] for v in np.argmin(costs[int(off[w]):int(off[w + 1])].cpu().numpy(), axis=1))
                      for w in range(len(off) - 1) if got.word_flags[w] == 0))

    lex = capi.Lexicon(rec, LX.random_words(rng, 50000, 2, 12))
    lex_rows = [_med_min(_time(lambda: rec.lexicon_match_device(lex, costs.data_ptr(), ng, off), a.warmup, a.iters)) for _ in range(a.repeats)]
    lex.close()

    reading_rows = []
    fns = [lambda: reading.read_words(det, rec, x, polys, adj), lambda: reading.read_words(det, rec, x, polys, adj, lm=lm),
           lambda: reading.read_words(det, rec, x, polys, adj, lm=lm, lm_params={"top_k": 8})]
    for _ in range(a.repeats):
        for fn in fns:
            fn()
        ts = [[] for _ in fns]
        for _ in range(max(5, a.iters // 2)):
            for k, fn in enumerate(fns):
                t0 = time.perf_counter()
                fn()
                ts[k].append(time.perf_counter() - t0)
        reading_rows.append({"read_words_ms": _med_min(ts[0]), "read_words_lm_ms": _med_min(ts[1]), "read_words_lm_top8_ms": _med_min(ts[2])})
    lm.close()
    rec.close()
    det.close()
    print(json.dumps({"bench": "char_lm", "device": torch.cuda.get_device_name(0), "iters": a.iters, "pages": a.pages, "words": glyphs.n_words,
                      "glyphs": ng, "decode": rows, "lexicon_match_50000_ms": lex_rows, "read_words": reading_rows,
                      "words_changed_by_the_model": changed, "oracle_match": ok}))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
