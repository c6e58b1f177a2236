"""Time the segmentation lattice (csrc/lattice.hip, csrc/glyph_split.hip) and what it costs in read_words, in one run, on the reading
batch of tools/bench_char_lm.py (32 pages of 640 x 640 with about 100 block words each):
  (a) ocr_lattice_decode on device-resident costs at max_span 1, 2, 4 and top_k 1, 8, and beside each ocr_lm_decode on the same words
      (its kernel is the parent commit's, instruction for instruction: docs/vmcnt_audit.md).  max_span 1 runs on the glyph block itself,
      so both calls see the same costs and offsets and their outputs are compared bit for bit outside the timed region; max_span 2 and 4
      run on the spans of the split pieces (the split parameters of --aspect-pct / --max-pieces), whose costs are the recogniser's on
      the span crops.  Per case the candidate reads: relax reads (G - 1) x 62 x 62 x top_k and merge reads sum_e min(M, e) x 62 x top_k
      over the decoded words (an upper bound on the relax side: the kernel leaves a list early)
  (b) ocr_split_glyphs on the same pages (device frames), with the default parameters and with the bench's, and how many glyphs each cut
  (c) reading.read_words without and with lattice={...}, alternating call by call, and the factor in crops seen by the recogniser
The calls are blocking: a host clock around each is its time.  Every measurement is repeated `--repeats` times to show the spread.  The
lattice at max_span 4, top_k 8 is checked against tests/lattice_oracle.py outside the timed region.  Prints one JSON line.

    timeout -k 10 900 python tools/bench_lattice.py [--iters 12] [--repeats 2]
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


def _reads(gs, M, k):
    g = np.asarray(gs, np.int64)
    g = g[(g >= 1) & (g <= 32)]
    relax = int(((g - 1) * 62 * 62 * k).sum())
    merge = int(sum(sum(min(M, e) for e in range(1, int(n) + 1)) for n in g) * 62 * k)
    return relax, merge


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--aspect-pct", type=int, default=60)
    ap.add_argument("--max-pieces", type=int, default=3)
    ap.add_argument("--check-words", type=int, default=400)
    a = ap.parse_args()
    import torch

    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi, reading
    from ocr_rs_amd import weights as W
    from tests import lattice_oracle as LO
    from tests import lexicon_oracle as LX
    from tests.test_gpu_glyphs import _synthetic_pages

    if not torch.cuda.is_available():
        raise SystemExit("bench_lattice needs a GPU")
    det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    frames, polys = _synthetic_pages(a.pages, 640, 640, 100, seed=a.pages)
    adj = np.ones((a.pages, 2))
    x = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    n, _, h, w = frames.shape
    glyphs = det.segment_glyphs(frames, polys, adj)
    split = {"aspect_pct": a.aspect_pct, "max_pieces": a.max_pieces}
    table = capi.char_lm_table(LX.random_words(np.random.default_rng(1), 20000, 2, 12), weight=2.0)
    lm = capi.CharLm(rec, table)

    def device_costs(block):
        crops = det.extract_glyph_crops(frames, block)
        logits = torch.from_numpy(rec.forward_host(crops)).cuda()
        costs = torch.empty_like(logits)
        torch.cuda.synchronize()
        rec.glyph_costs_device(logits.data_ptr(), block.n_glyphs, costs.data_ptr())
        return costs

    # (b) the split call
    split_rows = []
    for name, prm in (("defaults", None), ("bench", split)):
        pieces, pmap = det.split_glyphs(frames, glyphs, prm)
        cut = int(np.count_nonzero(np.bincount(pmap[:, 0], minlength=glyphs.n_glyphs) > 1))
        reps = [_med_min(_time(lambda: det.split_glyphs_device(x.data_ptr(), n, h, w, glyphs, prm), a.warmup, a.iters)) for _ in range(a.repeats)]
        split_rows.append({"params": name, "glyphs": glyphs.n_glyphs, "glyphs_cut": cut, "pieces": pieces.n_glyphs,
                           "flagged_words": int(np.count_nonzero(pieces.word_info[:, 3] & 4)), "ms": reps})
    pieces, _ = det.split_glyphs(frames, glyphs, split)

    # (a) the decode
    glyph_costs = device_costs(glyphs)
    rows, same_as_lm = [], True
    for M in (1, 2, 4):
        if M == 1:
            po, so, costs = glyphs.word_offsets, glyphs.word_offsets, glyph_costs
        else:
            spans, tab = capi.glyph_spans(pieces, M)
            po, so, costs = tab.piece_offsets, tab.span_offsets, device_costs(spans)
        for k in (1, 8):
            relax, merge = _reads(np.diff(po), M, k)
            prm = capi.lattice_params(max_span=M, top_k=k)
            lat = lambda: rec.lattice_decode_device(lm, costs.data_ptr(), int(so[-1]), so, po, prm)
            # beside it the character model's call on the same words: the glyph block's at M = 1, else the pieces one by one
            single = costs if M == 1 else costs[torch.from_numpy(np.flatnonzero(tab.span_len == 1)).cuda()].contiguous()
            ref = lambda: rec.lm_decode_device(lm, single.data_ptr(), int(po[-1]), po, {"top_k": k})
            torch.cuda.synchronize()
            reps = []
            for _ in range(a.repeats):
                for fn in (lat, ref):
                    for _ in range(a.warmup):
                        fn()
                ts = ([], [])
                for _ in range(a.iters):           # alternated call by call
                    for i, fn in enumerate((lat, ref)):
                        t0 = time.perf_counter()
                        fn()
                        ts[i].append(time.perf_counter() - t0)
                l, r = _med_min(ts[0]), _med_min(ts[1])
                reps.append({"lattice_ms": l, "lm_decode_ms": r, "ratio": round(l[0] / r[0], 3),
                             "greads_per_s": round((relax + merge) / (l[0] * 1e-3) / 1e9, 2)})
            rows.append({"max_span": M, "top_k": k, "words": len(po) - 1, "pieces": int(po[-1]), "spans": int(so[-1]), "relax_reads": relax,
                         "merge_reads": merge, "repeats": reps})
            if M == 1:
                g1, g2 = lat(), ref()
                same_as_lm &= bool(np.array_equal(g1.costs.view(np.uint64), g2.costs.view(np.uint64)) and np.array_equal(g1.labels, g2.labels) and
                                   np.array_equal(g1.raw_costs.view(np.uint64), g2.raw_costs.view(np.uint64)))
    # outside the timed region: max_span 4, top_k 8 against the oracle, bit for bit
    got = rec.lattice_decode_device(lm, costs.data_ptr(), int(so[-1]), so, po, {"max_span": 4, "top_k": 8})
    nchk = min(a.check_words, len(po) - 1)   # the oracle is slow: the first words only
    want = LO.decode(costs[:int(so[nchk])].cpu().numpy(), so[:nchk + 1], po[:nchk + 1], table, 4, 8)
    merged = int(np.count_nonzero(got.seg_len[0] > 1))
    got = rec.lattice_decode_device(lm, costs.data_ptr(), int(so[nchk]), so[:nchk + 1], po[:nchk + 1], {"max_span": 4, "top_k": 8})
    ok = bool(np.array_equal(got.labels, want["labels"]) and np.array_equal(got.seg_len, want["seg_len"]) and
              np.array_equal(got.costs.view(np.uint64), want["costs"].view(np.uint64)) and
              np.array_equal(got.raw_costs.view(np.uint64), want["raw_costs"].view(np.uint64)))

    # (c) read_words
    reading_rows = []
    lat2 = {"max_span": 2}
    lat4 = {"max_span": 4, "top_k": 8}
    fns = [lambda: reading.read_words(det, rec, x, polys, adj), lambda: reading.read_words(det, rec, x, polys, adj, lm=lm),
           lambda: reading.read_words(det, rec, x, polys, adj, lm=lm, lattice=lat2),
           lambda: reading.read_words(det, rec, x, polys, adj, lm=lm, lattice=lat2, split=split),
           lambda: reading.read_words(det, rec, x, polys, adj, lm=lm, lattice=lat4, split=split)]
    names = ["read_words_ms", "read_words_lm_ms", "read_words_lattice2_default_split_ms", "read_words_lattice2_ms", "read_words_lattice4_top8_ms"]
    for _ in range(a.repeats):
        for fn in fns:
            fn()
        ts = [[] for _ in fns]
        for _ in range(max(5, a.iters // 2)):
            for i, fn in enumerate(fns):
                t0 = time.perf_counter()
                fn()
                ts[i].append(time.perf_counter() - t0)
        reading_rows.append({nm: _med_min(t) for nm, t in zip(names, ts)})
    d_pieces, _ = det.split_glyphs(frames, glyphs)
    crops_seen = {"glyphs": glyphs.n_glyphs, "spans_default_split_M2": capi.glyph_spans(d_pieces, 2)[0].n_glyphs,
                  "spans_bench_split_M2": capi.glyph_spans(pieces, 2)[0].n_glyphs, "spans_bench_split_M4": capi.glyph_spans(pieces, 4)[0].n_glyphs}
    lm.close()
    rec.close()
    det.close()
    print(json.dumps({"bench": "lattice", "device": torch.cuda.get_device_name(0), "iters": a.iters, "pages": a.pages, "words": glyphs.n_words,
                      "glyphs": glyphs.n_glyphs, "split_params": split, "split": split_rows, "decode": rows, "read_words": reading_rows,
                      "crops_seen": crops_seen, "segments_merged_at_M4": merged, "words_checked_against_the_oracle": nchk, "max_span_1_equals_lm_decode": same_as_lm, "oracle_match": ok}))
    if not (ok and same_as_lm):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
