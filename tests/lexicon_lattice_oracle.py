"""Numpy f64 restatement of the joint lexicon and lattice search (ocr_lexicon_lattice_match, include/ocr_amd.h; kernels
csrc/lexicon_lattice.hip, host csrc/lexicon_lattice_host.cpp).  BUILD-DEFINED: the reference has no counterpart, nothing here is read
from it.

The rule.  Word w has G pieces, 1 <= G <= 32; its spans are [e-m, e) for e = 1..G, m = 1..min(M, e), ordered by (e, m), and
row(e, m) is the span's row in cost (n_spans x 62 f32).  An entry has classes c_0..c_(L-1).  f64 on the f32 values widened, every
operation rounded on its own, adds and mins only:
    s(row, c) = cost[row][c], with fold_case the min with the other-case twin of c (as in tests/lexicon_oracle.py)
    D[0][0] = 0;  D[i][0] = D[i-1][0] + del_cost;  D[0][j] = D[0][j-1] + ins_cost
    D[i][j] = min( min over m = 1..min(M, i) of ((D[i-m][j-1] + span_cost[m-1]) + s(row(i, m), c_(j-1))),
                   min(D[i-1][j] + del_cost, D[i][j-1] + ins_cost) )
    cost(w, entry) = D[G][L]
Candidates: the entries with max(1, ceil(G / M) - d) <= L <= min(32, G + d); the output is the first top_k by (cost, entry index),
slots past the candidates hold -1 and +inf.  word_flags: 1 for G = 0, 2 for G > 32, 4 when no entry has an admissible length.
raw_costs[w] = F[G] with F[0] = 0, F[e] = min over m = 1..min(M, e) of (F[e-m] + span_cost[m-1]) + min_c cost[row(e, m)][c], for a word
of any length.
The alignment of a returned (word, rank) is walked back from (G, L): at cell (i, j) with value v the first step whose recomputed value
equals v bit for bit, in the order segment of m = 1, 2, .., min(M, i) pieces (j >= 1), deletion (i >= 1), insertion (j >= 1).
seg_len is m at the first piece of a segment, 0 at its other pieces, -1 at a deleted piece; seg_char the entry position at the first
piece of a segment, -1 elsewhere; n_ins the entry characters that got no segment.

The costs are vectorised over (the words of one piece count) x (the entries of one length): every cell is one numpy operation, so each
add and each min is rounded separately.  The table of a winner is recomputed in Python floats (IEEE doubles, one rounding per
operation) and must end at the vectorised cost bit for bit.
"""
from __future__ import annotations

import struct

import numpy as np

from tests import lattice_oracle as LA
from tests import lexicon_oracle as LX

MAX_SPAN = LA.MAX_SPAN
MAX_PIECES = LA.MAX_PIECES
MAX_LEN = LX.MAX_LEN
CLASS_OF = LX.CLASS_OF
span_count, row_of, span_offsets, offsets = LA.span_count, LA.row_of, LA.span_offsets, LA.offsets

_bits = lambda x: struct.pack("<d", float(x))


def len_range(G: int, M: int, d: int):
    """the admissible entry lengths of a word of G pieces, inclusive"""
    return max(1, -(-G // M) - d), min(MAX_LEN, G + d)


def _fold(cost, fold_case):
    c64 = np.asarray(cost, np.float32).reshape(-1, 62).astype(np.float64)
    return np.minimum(c64, c64[:, LX.TWIN]) if fold_case else c64


def table(sub, classes, G, M, ins, dele, sc):
    """The full (G+1) x (L+1) table of one word of G pieces (sub: its span rows, folded, f64) against one entry, in Python floats."""
    L = len(classes)
    D = [[0.0] * (L + 1) for _ in range(G + 1)]
    for i in range(1, G + 1):
        D[i][0] = D[i - 1][0] + dele
    for j in range(1, L + 1):
        D[0][j] = D[0][j - 1] + ins
        c = int(classes[j - 1])
        for i in range(1, G + 1):
            v = min(D[i - 1][j] + dele, D[i][j - 1] + ins)
            for m in range(1, min(M, i) + 1):
                v = min(v, (D[i - m][j - 1] + sc[m - 1]) + float(sub[row_of(i, m, M)][c]))
            D[i][j] = v
    return D


def walk_back(D, sub, classes, M, ins, dele, sc):
    """-> (seg_len [G], seg_char [G], n_ins, trace_ties): trace_ties counts the cells of the walk at which more than one step
    recomputes to the cell's value, that is, where the order of the rule decided."""
    G, L = len(D) - 1, len(D[0]) - 1
    seg_len, seg_char, n_ins, ties = [0] * G, [-1] * G, 0, 0
    i, j = G, L
    while i > 0 or j > 0:
        v = _bits(D[i][j])
        steps = []
        if j >= 1:
            c = int(classes[j - 1])
            steps += [m for m in range(1, min(M, i) + 1) if _bits((D[i - m][j - 1] + sc[m - 1]) + float(sub[row_of(i, m, M)][c])) == v]
        if i >= 1 and _bits(D[i - 1][j] + dele) == v:
            steps.append(-1)
        if j >= 1 and _bits(D[i][j - 1] + ins) == v:
            steps.append(-2)
        assert steps, (i, j)
        ties += len(steps) > 1
        if steps[0] > 0:
            m = steps[0]
            seg_len[i - m], seg_char[i - m] = m, j - 1
            i, j = i - m, j - 1
        elif steps[0] == -1:
            seg_len[i - 1] = -1
            i -= 1
        else:
            n_ins += 1
            j -= 1
    return seg_len, seg_char, n_ins, ties


def brute_force(sub, classes, G, M, ins, dele, sc) -> float:
    """The minimum over ALL alignment paths from (0, 0) to (G, L) of the path's sum, taken left to right in the rule's association."""
    L = len(classes)
    best = [np.inf]

    def go(i, j, acc):
        if i == G and j == L:
            best[0] = min(best[0], acc)
            return
        if j < L:
            for m in range(1, min(M, G - i) + 1):
                go(i + m, j + 1, (acc + sc[m - 1]) + float(sub[row_of(i + m, m, M)][int(classes[j])]))
            go(i, j + 1, acc + ins)
        if i < G:
            go(i + 1, j, acc + dele)
    go(0, 0, 0.0)
    return best[0]


def raw_costs(cost, span_off, piece_off, M, sc) -> np.ndarray:
    c64 = np.asarray(cost, np.float32).reshape(-1, 62).astype(np.float64)
    rowmin = c64.min(axis=1) if c64.shape[0] else np.zeros(0)
    so, po = np.asarray(span_off, np.int64), np.asarray(piece_off, np.int64)
    out = np.zeros(len(po) - 1)
    for w in range(len(po) - 1):
        F, row = [np.float64(0.0)], int(so[w])
        for e in range(1, int(po[w + 1] - po[w]) + 1):
            ms = min(M, e)
            F.append(min((F[e - m] + sc[m - 1]) + rowmin[row + m - 1] for m in range(1, ms + 1)))
            row += ms
        out[w] = F[-1]
    return out


def match(costs, span_off, piece_off, words, max_span=2, ins_cost=4.0, del_cost=4.0, span_cost=None, max_len_diff=2, fold_case=1,
          top_k=1) -> dict:
    """-> entries [n_words, top_k] int32, costs [n_words, top_k] f64, raw_costs, n_candidates, word_flags, seg_len and seg_char
    [top_k, n_pieces] int32, n_ins [n_words, top_k] int32, `ties`: the (word, rank) pairs whose cost equals the next candidate's in
    sorted order (where the entry index decided), and `trace_ties` (walk_back) summed over the returned alignments."""
    cost = np.asarray(costs, np.float32).reshape(-1, 62)
    so, po = np.asarray(span_off, np.int64), np.asarray(piece_off, np.int64)
    nw, M, K, sc = len(po) - 1, int(max_span), int(top_k), LA._sc(span_cost)
    if not 1 <= M <= MAX_SPAN or not 1 <= K <= 8 or not 0 <= max_len_diff <= 8 or fold_case not in (0, 1):
        raise ValueError("parameters")
    if not (np.isfinite(ins_cost) and ins_cost >= 0 and np.isfinite(del_cost) and del_cost >= 0):
        raise ValueError("ins_cost / del_cost")
    if len(so) != len(po) or so[0] != 0 or po[0] != 0 or np.any(np.diff(po) < 0) or so[-1] != cost.shape[0]:
        raise ValueError("offsets")
    if any(int(so[w + 1] - so[w]) != span_count(int(po[w + 1] - po[w]), M) for w in range(nw)):
        raise ValueError("span count")
    if not np.all(np.isfinite(cost)) or np.any(cost < 0):
        raise ValueError("cost")
    sub = _fold(cost, fold_case)
    ins, dele = np.float64(ins_cost), np.float64(del_cost)
    lens = np.array([len(w) for w in words], np.int64)
    if np.any(lens < 1) or np.any(lens > MAX_LEN):
        raise ValueError("entry length")
    by_len = {}
    for L in range(1, MAX_LEN + 1):
        idx = np.flatnonzero(lens == L)
        if len(idx):
            by_len[L] = (idx, np.stack([LX.classes(words[k]) for k in idx]))
    G_of = np.diff(po)
    n_pieces = int(po[-1])
    entries = np.full((nw, K), -1, np.int32)
    out_cost = np.full((nw, K), np.inf)
    n_cand = np.zeros(nw, np.int32)
    flags = np.zeros(nw, np.int32)
    seg_len = np.zeros((K, n_pieces), np.int32)
    seg_char = np.full((K, n_pieces), -1, np.int32)
    n_ins = np.zeros((nw, K), np.int32)
    ties = trace_ties = 0
    flags[G_of == 0] = 1
    flags[G_of > MAX_PIECES] = 2
    for G in sorted(set(int(g) for g in G_of if 1 <= g <= MAX_PIECES)):
        ws = np.flatnonzero(G_of == G)
        S = np.stack([sub[so[w]:so[w + 1]] for w in ws])          # [words, span rows, 62]
        cand_idx, cand_cost = [], []
        lo, hi = len_range(G, M, max_len_diff)
        for L in range(lo, hi + 1):
            if L not in by_len:
                continue
            idx, codes = by_len[L]
            D = [np.zeros((len(ws), len(idx)))]
            for i in range(1, G + 1):
                D.append(D[i - 1] + dele)
            for j in range(L):
                old = D
                D = [old[0] + ins]
                for i in range(1, G + 1):
                    v = np.minimum(D[i - 1] + dele, old[i] + ins)
                    for m in range(1, min(M, i) + 1):
                        s = S[:, row_of(i, m, M), :][:, codes[:, j]]                # [words, entries]
                        v = np.minimum(v, (old[i - m] + sc[m - 1]) + s)
                    D.append(v)
            cand_idx.append(idx)
            cand_cost.append(D[G])
        if not cand_idx:
            flags[ws] = 4
            continue
        idx = np.concatenate(cand_idx)
        cc = np.concatenate(cand_cost, axis=1)
        n_cand[ws] = len(idx)
        for r, w in enumerate(ws):
            order = np.lexsort((idx, cc[r]))
            k = min(K, len(idx))
            entries[w, :k] = idx[order[:k]]
            out_cost[w, :k] = cc[r, order[:k]]
            s = cc[r, order[:k + 1]]
            ties += int(np.count_nonzero(s[1:] == s[:-1]))
            p0 = int(po[w])
            for t in range(k):
                cls = LX.classes(words[int(entries[w, t])])
                tab = table(S[r], cls, G, M, float(ins), float(dele), [float(x) for x in sc])
                assert _bits(tab[G][len(cls)]) == _bits(out_cost[w, t]), (w, t)
                sl, sch, ni, tt = walk_back(tab, S[r], cls, M, float(ins), float(dele), [float(x) for x in sc])
                seg_len[t, p0:p0 + G], seg_char[t, p0:p0 + G], n_ins[w, t] = sl, sch, ni
                trace_ties += tt
    return {"entries": entries, "costs": out_cost, "raw_costs": raw_costs(cost, so, po, M, sc), "n_candidates": n_cand,
            "word_flags": flags, "seg_len": seg_len, "seg_char": seg_char, "n_ins": n_ins, "ties": ties, "trace_ties": trace_ties}


ARRAYS = ("entries", "n_candidates", "word_flags", "seg_len", "seg_char", "n_ins")   # compared with array_equal
F64_ARRAYS = ("costs", "raw_costs")                                                  # compared as uint64


def segments(res: dict, piece_off, w: int, k: int = 0) -> list:
    """alignment k of word w as [(first piece inside the word, length, entry position)]"""
    p0, p1 = int(piece_off[w]), int(piece_off[w + 1])
    return [(p - p0, int(res["seg_len"][k, p]), int(res["seg_char"][k, p])) for p in range(p0, p1) if res["seg_len"][k, p] > 0]


def fuzz(seed: int, n_entries: int, gs, M: int, min_len: int = 1, max_len: int = MAX_LEN, integer: bool = False, high: int = 4):
    """A seeded case: n_entries random entries and one word per piece count of gs -> (costs, span_offsets, piece_offsets, words)."""
    rng = np.random.default_rng(seed)
    words = LX.random_words(rng, n_entries, min_len, max_len)
    po = offsets(gs)
    so = span_offsets(po, M)
    return LX.make_costs(rng, int(so[-1]), integer=integer, high=high), so, po, words


def span_rows(G: int, M: int, singles: str, merged=None, hit=0.0, miss=6.0) -> np.ndarray:
    """Hand cases: the span rows of one word of G pieces.  Piece i reads singles[i] at cost `hit` (a dict {char: cost} in a list is
    taken as given); merged maps (e, m) with m >= 2 to {char: cost}; everything else costs `miss`."""
    rows = np.full((span_count(G, M), 62), miss, np.float32)
    for i, ch in enumerate(singles):
        for c, v in (ch.items() if isinstance(ch, dict) else [(ch, hit)]):
            rows[row_of(i + 1, 1, M), CLASS_OF[c]] = v
    for (e, m), d in (merged or {}).items():
        for c, v in d.items():
            rows[row_of(e, m, M), CLASS_OF[c]] = v
    return rows


def hand_cases() -> dict:
    """name -> (costs, span_offsets, piece_offsets, words, params): the hand cases of tests/test_lexicon_lattice_oracle.py, which
    states what each must give, and of tests/test_gpu_lexicon_lattice.py, which runs each through the C ABI.  All costs are dyadic."""
    def one(G, M, singles, merged=None, **kw):
        return span_rows(G, M, singles, merged, **kw), span_offsets([0, G], M), np.array([0, G], np.int32)
    faint = ["c", "o", {"r": 1.0}, {"n": 1.0}]     # the halves of a cut m read r and n fairly, the merged span reads m well
    cases = {}
    cases["rn_span"] = (*one(4, 2, faint, {(4, 2): {"m": 0.5}}), ["corn", "com"], dict(max_span=2, top_k=2))
    cases["rn_span_cost"] = (*one(4, 2, faint, {(4, 2): {"m": 0.5}}), ["corn", "com"], dict(max_span=2, top_k=2, span_cost=[0.0, 3.0]))
    cases["rn_m1"] = (*one(4, 1, faint), ["corn", "com"], dict(max_span=1, top_k=2))
    cases["m_cut_m1"] = (*one(3, 1, "com"), ["corn", "com"], dict(max_span=1, top_k=2))
    cases["inserted"] = (*one(2, 1, "cm"), ["com"], dict(max_span=1))
    cases["fold_on"] = (*one(3, 2, "Com"), ["com", "Cam"], dict(max_span=2, fold_case=1, top_k=2))
    cases["fold_off"] = (*one(3, 2, "Com"), ["com", "Cam"], dict(max_span=2, fold_case=0, top_k=2))
    cases["trace_tie"] = (*one(2, 2, [{}, "a"], {(2, 2): {"a": 4.0}}), ["a"], dict(max_span=2))
    return cases


# The seeded whole-number case whose ties are part of the claim (tests/test_lexicon_lattice_oracle.py counts them without a GPU,
# tests/test_gpu_lexicon_lattice.py runs the case through the C ABI): at least 20 rank ties and at least one trace tie.
TIE_CASE = (dict(seed=83, n_entries=600, gs=[1, 2, 3, 4, 5, 6, 8, 3, 4], M=2, min_len=1, max_len=8, integer=True),
            dict(max_span=2, top_k=8))
