"""Numpy f64 restatement of the segmentation lattice's decode rule and of the span table (ocr_lattice_decode and ocr_glyph_spans,
include/ocr_amd.h; kernel csrc/lattice.hip, host csrc/lattice_host.cpp).  BUILD-DEFINED: the reference has no counterpart, nothing here
is read from it.

The rule.  Word w has G pieces; its spans are [e-m, e) for e = 1..G, m = 1..min(M, e), ordered by (e, m), and row(e, m) is the span's
row in cost (n_spans x 62 f32).  T is the 64 x 64 model of tests/char_lm_oracle.py.  f64 on the f32 values widened, every operation
rounded on its own, adds and mins only:
    A_0[c]  = the one-element list {T[62][c]}, link (p = 62, r = 0)
    A_j[c]  = the first K of L_j[p][r] + T[p][c] over p < 62 and r, by (value, p, r)                          (j >= 1)
    L_e[c]  = the first K by (value, m, a) of (A_(e-m)[c][a] + span_cost[m-1]) + cost[row(e, m)][c], m = 1..min(M, e)
    outputs = the first K of L_G[c][r] + T[c][62] by (value, c, r); segments and classes are read back along the links.
raw_costs[w] is the all-singletons path with the first-minimum class of every piece's own row, in the same association (span_cost[0]
included), for a word of any length; word_flags[w] is 1 for G = 0 and 2 for G > 32, and such a word has costs +inf, labels -1.

Candidates are laid out in key order ((m, a) and (p, r)) and sorted with a stable argsort, which is the key.
"""
from __future__ import annotations

import itertools

import numpy as np

from tests import char_lm_oracle as CL

MAX_SPAN = 4
MAX_PIECES = 32
BEGIN, END = CL.BEGIN, CL.END


def span_count(G: int, M: int) -> int:
    """sum over e = 1..G of min(M, e)"""
    return sum(min(M, e) for e in range(1, G + 1))


def row_of(e: int, m: int, M: int) -> int:
    """the row of span [e-m, e) inside its word"""
    return span_count(e - 1, M) + (m - 1)


def span_offsets(piece_offsets, M: int) -> np.ndarray:
    gs = np.diff(np.asarray(piece_offsets, np.int64))
    return np.concatenate([[0], np.cumsum([span_count(int(g), M) for g in gs])]).astype(np.int32)


def spans(piece_offsets, boxes, M: int) -> dict:
    """ocr_glyph_spans: -> span_offsets, boxes (unions), span_word, span_end, span_len."""
    off = np.asarray(piece_offsets, np.int64)
    bx = np.asarray(boxes, np.int32).reshape(-1, 4)
    out_b, sw, se, sl, so = [], [], [], [], [0]
    for w in range(len(off) - 1):
        p0, G = int(off[w]), int(off[w + 1] - off[w])
        for e in range(1, G + 1):
            for m in range(1, min(M, e) + 1):
                part = bx[p0 + e - m:p0 + e]
                out_b.append([part[:, 0].min(), part[:, 1].min(), part[:, 2].max(), part[:, 3].max()])
                sw.append(w)
                se.append(e)
                sl.append(m)
        so.append(len(sw))
    i32 = lambda a: np.asarray(a, np.int32)
    return {"span_offsets": i32(so), "boxes": i32(out_b).reshape(-1, 4), "span_word": i32(sw), "span_end": i32(se), "span_len": i32(sl)}


def _sc(span_cost) -> np.ndarray:
    sc = np.zeros(4, np.float64)
    if span_cost is not None:
        v = np.asarray(span_cost, np.float64).reshape(-1)
        sc[:len(v)] = v
    if not np.all(np.isfinite(sc)) or np.any(sc < 0):
        raise ValueError("span_cost")
    return sc


def path_cost(rows, T, M: int, seg_lens, classes, span_cost=None) -> np.float64:
    """The cost of one (segmentation, classes) pair of a word whose span rows are `rows`, summed left to right in the rule's
    association."""
    c64, t64, sc = np.asarray(rows, np.float32).astype(np.float64), np.asarray(T, np.float32).astype(np.float64), _sc(span_cost)
    acc, prev, e = None, BEGIN, 0
    for m, c in zip(seg_lens, classes):
        e += m
        acc = t64[prev, c] if acc is None else acc + t64[prev, c]
        acc = acc + sc[m - 1]
        acc = acc + c64[row_of(e, m, M), c]
        prev = c
    return acc + t64[prev, END]


def segmentations(G: int, M: int):
    """every way to write G as an ordered sum of parts in 1..M"""
    if G == 0:
        yield ()
        return
    for m in range(1, min(M, G) + 1):
        for rest in segmentations(G - m, M):
            yield (m,) + rest


def enumerate_paths(rows, T, G: int, M: int, span_cost=None, classes=None):
    """All (segmentation, classes) pairs of one word -> (costs f64 in the rule's association, [(seg_lens, classes)]).  `classes`
    restricts the classes tried (for G = 4: the rest is known to cost 1e30)."""
    c64, t64, sc = np.asarray(rows, np.float32).astype(np.float64), np.asarray(T, np.float32).astype(np.float64), _sc(span_cost)
    cl = np.arange(62) if classes is None else np.asarray(classes, np.int64)
    costs, pairs = [], []
    for seg in segmentations(G, M):
        paths = np.array(list(itertools.product(cl, repeat=len(seg))), np.int64)
        acc, e = None, 0
        for i, m in enumerate(seg):
            e += m
            tr = t64[BEGIN, paths[:, 0]] if i == 0 else t64[paths[:, i - 1], paths[:, i]]
            acc = tr if acc is None else acc + tr
            acc = acc + sc[m - 1]
            acc = acc + c64[row_of(e, m, M), paths[:, i]]
        costs.append(acc + t64[paths[:, -1], END])
        pairs += [(seg, tuple(int(c) for c in p)) for p in paths]
    return np.concatenate(costs), pairs


def raw_costs(cost, span_off, piece_off, T, M: int, span_cost=None) -> np.ndarray:
    c64 = np.asarray(cost, np.float32).reshape(-1, 62).astype(np.float64)
    t64, sc = np.asarray(T, np.float32).reshape(64, 64).astype(np.float64), _sc(span_cost)
    so, po = np.asarray(span_off, np.int64), np.asarray(piece_off, np.int64)
    out = np.zeros(len(po) - 1)
    for w in range(len(po) - 1):
        acc, prev, row = np.float64(0.0), BEGIN, int(so[w])
        for e in range(1, int(po[w + 1] - po[w]) + 1):
            c = int(c64[row].argmin())   # argmin takes the first minimum
            acc = acc + t64[prev, c]
            acc = acc + sc[0]
            acc = acc + c64[row, c]
            prev = c
            row += min(M, e)
        if po[w + 1] > po[w]:
            acc = acc + t64[prev, END]
        out[w] = acc
    return out


def decode(costs, span_off, piece_off, T, max_span: int = 2, top_k: int = 1, span_cost=None) -> dict:
    """-> labels, seg_len [top_k, n_pieces] int32, n_chars [n_words, top_k], costs [n_words, top_k] f64, raw_costs, word_flags, and
    `ties`: the number of (word, rank) pairs whose cost equals the next hypothesis' in sorted order (rank top_k + 1 included)."""
    cost = np.asarray(costs, np.float32).reshape(-1, 62)
    so, po = np.asarray(span_off, np.int64), np.asarray(piece_off, np.int64)
    nw, M, K, sc = len(po) - 1, int(max_span), int(top_k), _sc(span_cost)
    if not 1 <= M <= MAX_SPAN or not 1 <= K <= 8:
        raise ValueError("max_span / top_k")
    if len(so) != len(po) or so[0] != 0 or po[0] != 0 or np.any(np.diff(po) < 0) or so[-1] != cost.shape[0]:
        raise ValueError("offsets")
    if any(int(so[w + 1] - so[w]) != span_count(int(po[w + 1] - po[w]), M) for w in range(nw)):
        raise ValueError("span count")
    if not np.all(np.isfinite(cost)) or np.any(cost < 0):
        raise ValueError("cost")
    T = CL.check_model(T)
    c64, t64 = cost.astype(np.float64), T.astype(np.float64)
    tr = t64[:62, :62]
    n_pieces = int(po[-1])
    labels = np.full((K, n_pieces), -1, np.int32)
    seg_len = np.zeros((K, n_pieces), np.int32)
    n_chars = np.zeros((nw, K), np.int32)
    out_cost = np.full((nw, K), np.inf)
    flags = np.zeros(nw, np.int32)
    ties = 0
    for w in range(nw):
        p0, G, row = int(po[w]), int(po[w + 1] - po[w]), int(so[w])
        if G == 0 or G > MAX_PIECES:
            flags[w] = 1 if G == 0 else 2
            continue
        a_val = np.full((62, K), np.inf)
        a_val[:, 0] = t64[BEGIN, :62]
        A = {0: (a_val, np.full((62, K), BEGIN, np.int64), np.zeros((62, K), np.int64))}   # values, link p, link r
        Lm, La = {}, {}
        for e in range(1, G + 1):
            ms = min(M, e)
            # cand[c, (m - 1) * K + a] = (A_(e-m)[c][a] + span_cost[m-1]) + cost[row(e, m)][c]
            cand = np.concatenate([(A[e - m][0] + sc[m - 1]) + c64[row + m - 1][:, None] for m in range(1, ms + 1)], axis=1)
            order = np.argsort(cand, axis=1, kind="stable")[:, :K]
            l_val = np.take_along_axis(cand, order, axis=1)
            Lm[e], La[e] = order // K + 1, order % K
            row += ms
            if e < G:
                # cand2[c, p * K + r] = L_e[p][r] + T[p][c]
                cand2 = (l_val[None, :, :] + tr.T[:, :, None]).reshape(62, 62 * K)
                o2 = np.argsort(cand2, axis=1, kind="stable")[:, :K]
                A[e] = (np.take_along_axis(cand2, o2, axis=1), o2 // K, o2 % K)
        fin = (l_val + t64[:62, END][:, None]).reshape(62 * K)   # index c * K + r
        order = np.argsort(fin, kind="stable")
        s = fin[order[:K + 1]]
        ties += int(np.count_nonzero(s[1:] == s[:-1]))
        for k in range(K):
            out_cost[w, k] = fin[order[k]]
            c, r = int(order[k]) // K, int(order[k]) % K
            e, n = G, 0
            while e > 0:
                m, a = int(Lm[e][c, r]), int(La[e][c, r])
                labels[k, p0 + e - m] = c
                seg_len[k, p0 + e - m] = m
                c, r = int(A[e - m][1][c, a]), int(A[e - m][2][c, a])
                e -= m
                n += 1
            n_chars[w, k] = n
    return {"labels": labels, "seg_len": seg_len, "n_chars": n_chars, "costs": out_cost,
            "raw_costs": raw_costs(cost, so, po, T, M, sc), "word_flags": flags, "ties": ties}


def hypothesis(res: dict, piece_off, w: int, k: int = 0):
    """-> (seg_lens, classes) of hypothesis k of word w"""
    p0, p1 = int(piece_off[w]), int(piece_off[w + 1])
    at = [p for p in range(p0, p1) if res["seg_len"][k, p] > 0]
    return tuple(int(res["seg_len"][k, p]) for p in at), tuple(int(res["labels"][k, p]) for p in at)


def text(res: dict, piece_off, w: int, k: int = 0) -> str:
    return CL.text_of(hypothesis(res, piece_off, w, k)[1])


def offsets(gs) -> np.ndarray:
    return CL.offsets(gs)


def make_case(rng, gs, M: int, integer: bool = False, high: int = 4):
    """random span costs and a random model for words of gs pieces -> (costs, span_offsets, piece_offsets, T)"""
    po = offsets(gs)
    so = span_offsets(po, M)
    return CL.make_costs(rng, int(so[-1]), integer=integer, high=high), so, po, CL.make_model(rng, integer=integer, high=max(2, high - 1))


# The seeded whole-number case whose equal-cost hypotheses are part of the claim (tests/test_lattice_oracle.py counts its ties;
# tests/test_gpu_lattice.py runs it through the C ABI).
def tie_case(M: int = 3):
    rng = np.random.default_rng(4242)
    po = offsets([1, 2, 3, 4, 6, 9])
    so = span_offsets(po, M)
    return CL.make_costs(rng, int(so[-1]), integer=True, high=3), so, po, CL.make_model(rng, integer=True, high=2), M


def hand_tie_case():
    """Two pieces, M = 2, the zero model, span_cost 0.  Rows: (e=1, m=1) and (e=2, m=1) cost 1 everywhere but 0 at class A; the merged
    span (e=2, m=2) costs 0 at classes A and B and 1 elsewhere.  Cost 0: the pairs [A][A] (two segments) and [AA -> A], [AA -> B]
    (one segment).  Final key (value, c, r): class A first; inside L_2[A] the key (value, m, a) puts m = 1 (two segments) in front of
    m = 2; then class B.  So the order is (1, 1) AA, (2,) A, (2,) B, then the cost-1 pairs by class."""
    cost = np.ones((3, 62), np.float32)
    cost[0, 0] = cost[1, 0] = 0.0
    cost[2, 0] = cost[2, 1] = 0.0
    return cost, np.array([0, 3], np.int32), np.array([0, 2], np.int32), CL.zero_model(), 2


def rn_case():
    """Two pieces that read r and n, their merged span reads m.  -> (costs, span_offsets, piece_offsets), M = 2."""
    rows = np.full((3, 62), 6.0, np.float32)
    rows[0, CL.CLASS_OF["r"]] = 0.0   # (e=1, m=1)
    rows[1, CL.CLASS_OF["n"]] = 0.0   # (e=2, m=1)
    rows[2, CL.CLASS_OF["m"]] = 0.0   # (e=2, m=2)
    return rows, np.array([0, 3], np.int32), np.array([0, 2], np.int32)
