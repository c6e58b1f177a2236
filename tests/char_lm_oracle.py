"""Numpy f64 restatement of the character language model's rule (ocr_lm_decode, include/ocr_amd.h; kernel csrc/char_lm.hip).
BUILD-DEFINED: the reference has no counterpart, nothing here is read from it.

The rule.  cost is n_glyphs x 62 f32, T is 64 x 64 f32 with T[p, c] the cost of class c behind class p, row 62 begin-of-word, column 62
end-of-word.  All arithmetic is f64 on the f32 values widened, every operation rounded on its own, adds and mins only.  For a word
with glyph rows r_0 .. r_(G-1), 1 <= G <= 32:
    D_0[c]   = T[62][c] + cost[r_0][c]
    D_i[c]   = min_p (D_(i-1)[p] + T[p][c]) + cost[r_i][c]          (the transition first, the glyph cost second)
    total[c] = D_(G-1)[c] + T[c][62]
With top_k = K every state keeps a list; L_0[c] holds D_0[c] alone.  The candidates of state (i, c) are L_(i-1)[p][r] + T[p][c] over
all p < 62 and r < len(L_(i-1)[p]), ordered by (value, p, r) ascending and cut to the first K; then cost[r_i][c] is added to each.  The
outputs are the first K of L_(G-1)[c][r] + T[c][62] by (value, c, r); hypothesis k's classes are read back along the (p, r) links.
raw_costs[w] is the same association along the greedy reading (the first minimum class of every glyph), for a word of any length;
word_flags[w] is 1 for G = 0 and 2 for G > 32, and such a word has costs +inf and labels -1.

The lists are vectorised over (the words of one glyph count) x (class): the candidates of a step are one [words, 62, 62 * K] array in
(p, r) order, and a stable argsort of it is the key (value, p, r).
"""
from __future__ import annotations

import itertools

import numpy as np

ALPHABET = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789"
CLASS_OF = {ch: k for k, ch in enumerate(ALPHABET)}
MAX_LEN = 32
BEGIN = 62
END = 62


def check_model(T) -> np.ndarray:
    T = np.asarray(T, np.float32).reshape(64, 64)
    used = np.zeros((64, 64), bool)
    used[:63, :63] = True
    used[BEGIN, END] = False
    if not np.all(np.isfinite(T[used])) or np.any(T[used] < 0) or np.any(T[~used] != 0):
        raise ValueError("model")
    return T


def zero_model() -> np.ndarray:
    return np.zeros((64, 64), np.float32)


def text_of(labels) -> str:
    return "".join(ALPHABET[int(c)] for c in labels)


def path_cost(cost_rows, T, path) -> np.float64:
    """The cost of one path, summed left to right in the rule's association."""
    c64, t64 = np.asarray(cost_rows, np.float32).astype(np.float64), np.asarray(T, np.float32).astype(np.float64)
    acc = t64[BEGIN, path[0]] + c64[0, path[0]]
    for i in range(1, len(path)):
        acc = acc + t64[path[i - 1], path[i]]
        acc = acc + c64[i, path[i]]
    return acc + t64[path[-1], END]


def raw_costs(cost, word_offsets, T) -> np.ndarray:
    c64 = np.asarray(cost, np.float32).reshape(-1, 62).astype(np.float64)
    t64 = np.asarray(T, np.float32).reshape(64, 64).astype(np.float64)
    off = np.asarray(word_offsets, np.int64)
    first = c64.argmin(axis=1) if c64.shape[0] else np.zeros(0, np.int64)   # argmin takes the first minimum
    out = np.zeros(len(off) - 1)
    for w in range(len(off) - 1):
        acc, prev = np.float64(0.0), BEGIN
        for g in range(off[w], off[w + 1]):
            acc = acc + t64[prev, first[g]]
            acc = acc + c64[g, first[g]]
            prev = first[g]
        if off[w + 1] > off[w]:
            acc = acc + t64[prev, END]
        out[w] = acc
    return out


def decode(costs, word_offsets, T, top_k: int = 1) -> dict:
    """-> labels [top_k, n_glyphs] int32, costs [n_words, top_k] f64, raw_costs, word_flags, and `ties`: the number of (word, rank)
    pairs whose cost equals the next hypothesis' in sorted order (the rank below top_k + 1 included), that is, the places where
    (c, r) decided."""
    cost = np.asarray(costs, np.float32).reshape(-1, 62)
    off = np.asarray(word_offsets, np.int64)
    nw, ng, K = len(off) - 1, cost.shape[0], int(top_k)
    if off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] != ng:
        raise ValueError("word offsets")
    if not np.all(np.isfinite(cost)) or np.any(cost < 0):
        raise ValueError("cost")
    if not 1 <= K <= 8:
        raise ValueError("top_k")
    T = check_model(T)
    c64, t64 = cost.astype(np.float64), T.astype(np.float64)
    tr = t64[:62, :62]
    labels = np.full((K, ng), -1, np.int32)
    out_cost = np.full((nw, K), np.inf)
    flags = np.zeros(nw, np.int32)
    G_of = np.diff(off)
    flags[G_of == 0] = 1
    flags[G_of > MAX_LEN] = 2
    ties = 0
    groups = []                                                         # the words of one glyph count, 256 at a time
    for G in sorted(set(int(g) for g in G_of if 1 <= g <= MAX_LEN)):
        same = np.flatnonzero(G_of == G)
        groups += [(G, same[n:n + 256]) for n in range(0, len(same), 256)]
    for G, ws in groups:
        S = np.stack([c64[off[w]:off[w] + G] for w in ws])            # [words, G, 62]
        L = np.full((len(ws), 62, K), np.inf)                           # [words, class, rank]
        L[:, :, 0] = t64[BEGIN, :62][None, :] + S[:, 0, :]
        links = []
        for i in range(1, G):
            # cand[w, c, p * K + r] = L[w, p, r] + T[p, c]
            cand = (L[:, None, :, :] + tr.T[None, :, :, None]).reshape(len(ws), 62, 62 * K)
            order = np.argsort(cand, axis=2, kind="stable")[:, :, :K]
            L = np.take_along_axis(cand, order, axis=2) + S[:, i, :, None]
            links.append(order)                                         # p = order // K, r = order % K
        fin = (L + t64[:62, END][None, :, None]).reshape(len(ws), 62 * K)   # index c * K + r
        order = np.argsort(fin, axis=1, kind="stable")
        for n, w in enumerate(ws):
            sc = fin[n, order[n, :K + 1]]
            ties += int(np.count_nonzero(sc[1:] == sc[:-1]))
            for k in range(K):
                out_cost[w, k] = fin[n, order[n, k]]
                c, r = int(order[n, k]) // K, int(order[n, k]) % K
                for i in range(G - 1, -1, -1):
                    labels[k, off[w] + i] = c
                    if i > 0:
                        code = int(links[i - 1][n, c, r])
                        c, r = code // K, code % K
    return {"labels": labels, "costs": out_cost, "raw_costs": raw_costs(cost, off, T), "word_flags": flags, "ties": ties}


def enumerate_paths(cost_rows, T):
    """All 62^G paths of one word (G <= 3) -> (costs [62^G] f64 in the rule's association, paths [62^G, G])."""
    c64, t64 = np.asarray(cost_rows, np.float32).astype(np.float64), np.asarray(T, np.float32).astype(np.float64)
    G = c64.shape[0]
    paths = np.array(list(itertools.product(range(62), repeat=G)), np.int64)
    acc = t64[BEGIN, paths[:, 0]] + c64[0, paths[:, 0]]
    for i in range(1, G):
        acc = acc + t64[paths[:, i - 1], paths[:, i]]
        acc = acc + c64[i, paths[:, i]]
    return acc + t64[paths[:, -1], END], paths


def costs_for_text(text: str, hit: float = 0.0, miss: float = 6.0, confusions=None) -> np.ndarray:
    """Hand cases: one row per character, `hit` for its class and `miss` for every other one; confusions {position: {char: cost}}
    sets single cells."""
    c = np.full((len(text), 62), miss, np.float32)
    for i, ch in enumerate(text):
        c[i, CLASS_OF[ch]] = hit
    for i, row in (confusions or {}).items():
        for ch, v in row.items():
            c[i, CLASS_OF[ch]] = v
    return c


def make_costs(rng, n_glyphs: int, integer: bool = False, high: int = 4) -> np.ndarray:
    """n_glyphs x 62 f32: whole numbers in [0, high) (ties are real and every sum is exact), or positive floats with one favoured
    class per row."""
    if integer:
        return rng.integers(0, high, size=(n_glyphs, 62)).astype(np.float32)
    c = rng.uniform(0.5, 9.0, size=(n_glyphs, 62)).astype(np.float32)
    if n_glyphs:
        c[np.arange(n_glyphs), rng.integers(0, 62, n_glyphs)] *= np.float32(0.05)
    return c


def make_model(rng, integer: bool = False, high: int = 3) -> np.ndarray:
    """A random valid model: whole numbers in [0, high) or floats in [0, 6)."""
    T = np.zeros((64, 64), np.float32)
    v = rng.integers(0, high, size=(63, 63)).astype(np.float32) if integer else rng.uniform(0.0, 6.0, size=(63, 63)).astype(np.float32)
    T[:63, :63] = v
    T[BEGIN, END] = 0.0
    return T


def offsets(gs) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(np.asarray(gs, np.int64))]).astype(np.int32)


# The seeded whole-number case whose equal-cost hypotheses are part of the claim (tests/test_char_lm_oracle.py writes its tie order
# out by hand; tests/test_gpu_char_lm.py runs it through the C ABI).
def tie_case():
    rng = np.random.default_rng(2024)
    gs = [1, 2, 3, 4, 6, 9]
    off = offsets(gs)
    return make_costs(rng, int(off[-1]), integer=True, high=3), off, make_model(rng, integer=True, high=2)


def hand_tie_case():
    """Two glyphs, every glyph cost 1 except classes A and B at 0, an all-zero model but T[A][B] = 1: the paths AA, BA, BB cost 0 and
    AB costs 1, then every path through one other class costs 1."""
    cost = np.ones((2, 62), np.float32)
    cost[:, :2] = 0.0
    T = zero_model()
    T[0, 1] = 1.0
    return cost, np.array([0, 2], np.int32), T
