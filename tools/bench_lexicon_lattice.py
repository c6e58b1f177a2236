"""Time the joint lexicon and lattice search (csrc/lexicon_lattice.hip) beside ocr_lexicon_match, in one run, on the reading batch of
tools/bench_lattice.py (32 pages of 640 x 640 with about 100 block words each) and a lexicon of 50 000 random entries of 2..12
characters:
  ocr_lexicon_lattice_match on device-resident costs at max_span 1, 2, 4 and top_k 1, 8, and beside each ocr_lexicon_match on the same
  piece block (its kernel is the parent commit's, instruction for instruction: docs/vmcnt_audit.md), alternated call by call.
  max_span 1 runs on the glyph block itself, so both calls see the same costs and offsets and every output is compared bit for bit
  outside the timed region; max_span 2 and 4 run on the spans of the split pieces (the split parameters of --aspect-pct /
  --max-pieces), and the call beside them matches the pieces one by one (the rows of the one-piece spans).  Per case the counted work:
  DP cells sum over (word, candidate) of G x L, and span terms sum of L x sum_e min(M, e) - a cell of the new kernel takes up to M span
  terms, a cell of ocr_lexicon_match one.  The candidate sets differ at M > 1 (the length rule starts at ceil(G / M)), so the cells of
  both calls are counted.
The calls are blocking: a host clock around each is its time.  Every measurement is repeated `--repeats` times to show the spread.  The
call at max_span 4, top_k 8 is checked against tests/lexicon_lattice_oracle.py on the first --check-words words outside the timed
region.  Prints one JSON line.

    timeout -k 10 900 python tools/bench_lexicon_lattice.py [--iters 12] [--repeats 2]
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


def _work(gs, len_count, M, d, joint):
    """-> (DP cells, span terms, candidates) over the matched words: the length rule of the joint call, or of ocr_lexicon_match"""
    cells = terms = cands = 0
    for G in np.asarray(gs, np.int64):
        G = int(G)
        if not 1 <= G <= 32:
            continue
        lo = max(1, (-(-G // M) if joint else G) - d)
        hi = min(32, G + d)
        n = int(len_count[lo:hi + 1].sum())
        chars = int((len_count[lo:hi + 1] * np.arange(lo, hi + 1)).sum())
        cands += n
        cells += G * chars
        terms += chars * sum(min(M, e) for e in range(1, G + 1))
    return cells, terms, cands


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--entries", type=int, default=50000)
    ap.add_argument("--aspect-pct", type=int, default=60)
    ap.add_argument("--max-pieces", type=int, default=3)
    ap.add_argument("--check-words", type=int, default=24)
    a = ap.parse_args()
    import torch

    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    from tests import lexicon_lattice_oracle as O
    from tests import lexicon_oracle as LX
    from tests.test_gpu_glyphs import _synthetic_pages

    if not torch.cuda.is_available():
        raise SystemExit("bench_lexicon_lattice needs a GPU")
    det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
    rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    frames, polys = _synthetic_pages(a.pages, 640, 640, 100, seed=a.pages)
    adj = np.ones((a.pages, 2))
    glyphs = det.segment_glyphs(frames, polys, adj)
    pieces, _ = det.split_glyphs(frames, glyphs, {"aspect_pct": a.aspect_pct, "max_pieces": a.max_pieces})
    words = LX.random_words(np.random.default_rng(1), a.entries, 2, 12)
    len_count = np.bincount([len(w) for w in words], minlength=34)
    lex = capi.Lexicon(rec, words)
    d = 2

    def device_costs(block):
        crops = det.extract_glyph_crops(frames, block)
        logits = torch.from_numpy(rec.forward_host(crops)).cuda()
        costs = torch.empty_like(logits)
        torch.cuda.synchronize()
        rec.glyph_costs_device(logits.data_ptr(), block.n_glyphs, costs.data_ptr())
        return costs

    glyph_costs = device_costs(glyphs)
    rows, same_as_lexicon = [], True
    for M in (1, 2, 4):
        if M == 1:
            po, so, costs = glyphs.word_offsets, glyphs.word_offsets, glyph_costs
        else:
            spans, tab = capi.glyph_spans(pieces, M)
            po, so, costs = tab.piece_offsets, tab.span_offsets, device_costs(spans)
        single = costs if M == 1 else costs[torch.from_numpy(np.flatnonzero(tab.span_len == 1)).cuda()].contiguous()
        for k in (1, 8):
            cells, terms, cands = _work(np.diff(po), len_count, M, d, True)
            ref_cells, _, ref_cands = _work(np.diff(po), len_count, 1, d, False)
            prm = capi.lexlat_params(max_span=M, top_k=k, max_len_diff=d)
            new = lambda: rec.lexicon_lattice_match_device(lex, costs.data_ptr(), int(so[-1]), so, po, prm)
            ref = lambda: rec.lexicon_match_device(lex, single.data_ptr(), int(po[-1]), po, {"top_k": k, "max_len_diff": d})
            torch.cuda.synchronize()
            reps = []
            for _ in range(a.repeats):
                for fn in (new, ref):
                    for _ in range(a.warmup):
                        fn()
                ts = ([], [])
                for _ in range(a.iters):           # alternated call by call
                    for i, fn in enumerate((new, ref)):
                        t0 = time.perf_counter()
                        fn()
                        ts[i].append(time.perf_counter() - t0)
                n, r = _med_min(ts[0]), _med_min(ts[1])
                reps.append({"lexicon_lattice_ms": n, "lexicon_match_ms": r, "ratio": round(n[0] / r[0], 3),
                             "gcells_per_s": round(cells / (n[0] * 1e-3) / 1e9, 2), "gterms_per_s": round(terms / (n[0] * 1e-3) / 1e9, 2),
                             "lexicon_match_gcells_per_s": round(ref_cells / (r[0] * 1e-3) / 1e9, 2)})
            rows.append({"max_span": M, "top_k": k, "words": len(po) - 1, "pieces": int(po[-1]), "spans": int(so[-1]), "candidates": cands,
                         "dp_cells": cells, "span_terms": terms, "lexicon_match_candidates": ref_cands, "lexicon_match_dp_cells": ref_cells,
                         "repeats": reps})
            if M == 1:
                g1, g2 = new(), ref()
                same_as_lexicon &= bool(np.array_equal(g1.entries, g2.entries) and np.array_equal(g1.costs.view(np.uint64), g2.costs.view(np.uint64)) and
                                        np.array_equal(g1.raw_costs.view(np.uint64), g2.raw_costs.view(np.uint64)) and
                                        np.array_equal(g1.n_candidates, g2.n_candidates) and np.array_equal(g1.word_flags, g2.word_flags))
    # outside the timed region: max_span 4, top_k 8 against the oracle, every array (the oracle is slow: the first words only)
    got = rec.lexicon_lattice_match_device(lex, costs.data_ptr(), int(so[-1]), so, po, {"max_span": 4, "top_k": 8})
    merged = int(np.count_nonzero(got.seg_len[0] > 1))
    nchk = min(a.check_words, len(po) - 1)
    got = rec.lexicon_lattice_match_device(lex, costs.data_ptr(), int(so[nchk]), so[:nchk + 1], po[:nchk + 1], {"max_span": 4, "top_k": 8})
    want = O.match(costs[:int(so[nchk])].cpu().numpy(), so[:nchk + 1], po[:nchk + 1], words, max_span=4, top_k=8)
    ok = bool(all(np.array_equal(getattr(got, nm), want[nm]) for nm in O.ARRAYS) and
              all(np.array_equal(getattr(got, nm).view(np.uint64), want[nm].view(np.uint64)) for nm in O.F64_ARRAYS))
    lex.close()
    rec.close()
    det.close()
    print(json.dumps({"bench": "lexicon_lattice", "device": torch.cuda.get_device_name(0), "iters": a.iters, "pages": a.pages,
                      "words": glyphs.n_words, "glyphs": glyphs.n_glyphs, "pieces": pieces.n_glyphs, "entries": len(words), "max_len_diff": d,
                      "match": rows, "segments_merged_at_M4": merged, "words_checked_against_the_oracle": nchk,
                      "max_span_1_equals_lexicon_match": same_as_lexicon, "oracle_match": ok}))
    if not (ok and same_as_lexicon):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
