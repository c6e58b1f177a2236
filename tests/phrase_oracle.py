"""Numpy f64 restatement of the phrase-search rule of ocr_lexicon_phrase_match (include/ocr_amd.h; kernels
csrc/lexicon_phrase.hip).  BUILD-DEFINED: the reference has no counterpart, nothing here is read from it.

W(i, e) is vectorised over (the starts of a line) x (the entries of one length bucket): every character is one numpy add on a
[starts, entries] array, so each add is rounded separately and in the order of the rule.  The DP itself is plain Python: every
candidate is formed as (B + bnd) + T and the minimum is taken by the key (v, kind, M).  `enumerate_line` is the independent check: it
walks every composition of a short line with every entry of every part's length.
"""
from __future__ import annotations

import itertools

import numpy as np

from tests.lexicon_oracle import ALPHABET, CLASS_OF, MAX_LEN, TWIN, classes, costs_for_text, make_costs, random_words  # noqa: F401

MAX_GLYPHS = 256
INF = np.float64(np.inf)


def default_params() -> dict:
    return dict(word_cost=1.0, oov_word_cost=6.0, oov_glyph_cost=1.0, fold_case=1)


def _buckets(words):
    lens = np.array([len(w) for w in words], np.int64)
    if np.any(lens < 1) or np.any(lens > MAX_LEN):
        raise ValueError("entry length")
    out = {}
    for m in range(1, MAX_LEN + 1):
        idx = np.flatnonzero(lens == m)
        if len(idx):
            out[m] = (idx, np.stack([classes(words[k]) for k in idx]))
    return out


def _line_tables(sub, rowmin, join, buckets, prm):
    """L [G, 33] f64 with E [G, 33] (entry index or -1), U and J [G, 33] for one line; column M, row i; +inf where i + M > G."""
    G = sub.shape[0]
    L = np.full((G, MAX_LEN + 1), INF)
    E = np.full((G, MAX_LEN + 1), -1, np.int64)
    U = np.full((G, MAX_LEN + 1), INF)
    J = np.full((G, MAX_LEN + 1), INF)
    for M, (idx, codes) in buckets.items():
        n = G - M + 1
        if n <= 0:
            continue
        W = np.zeros((n, len(idx)))
        for k in range(M):
            W = W + sub[k:k + n][:, codes[:, k]]
        a = np.argmin(W, axis=1)          # the first minimum: idx ascends, so the lowest entry index among equal values
        L[:n, M] = W[np.arange(n), a]
        E[:n, M] = idx[a]
    oov_w, oov_g = np.float64(prm["oov_word_cost"]), np.float64(prm["oov_glyph_cost"])
    for i in range(G):
        u, j = oov_w, np.float64(0.0)
        for M in range(1, min(MAX_LEN, G - i) + 1):
            u = u + rowmin[i + M - 1]
            u = u + oov_g
            if M > 1:
                j = j + join[i + M - 1]
            U[i, M] = u
            J[i, M] = j
    return L, E, U, J


def _segment(L, E, U, J, bound, prm):
    """The DP of one line -> (word lengths, entries, word costs, B[G])."""
    G = L.shape[0]
    wc = np.float64(prm["word_cost"])
    B = [np.float64(0.0)]
    choice = [None]
    T = {}
    for j in range(1, G + 1):
        best = None
        for kind in (0, 1):
            for M in range(1, min(MAX_LEN, j) + 1):
                i = j - M
                t = (L[i, M] + wc) + J[i, M] if kind == 0 else U[i, M] + J[i, M]
                v = (B[i] + (bound[i] if i > 0 else np.float64(0.0))) + t
                if not np.isfinite(v):
                    continue
                key = (v, kind, M)
                if best is None or key < best:
                    best = key
                    T[j] = t
        B.append(best[0])
        choice.append((best[2], best[1]))
    lens, ents, costs = [], [], []
    j = G
    while j > 0:
        M, kind = choice[j]
        lens.append(M)
        ents.append(int(E[j - M, M]) if kind == 0 else -1)
        costs.append(T[j])
        j -= M
    return lens[::-1], ents[::-1], costs[::-1], B[G]


def phrase_match(costs, line_offsets, words, bound_cost=None, join_cost=None, **params) -> dict:
    """-> line_word_offsets, word_offsets, entries (int32), word_costs, line_costs, raw_costs (f64), line_flags (int32)."""
    prm = default_params()
    prm.update(params)
    cost = np.asarray(costs, np.float32).reshape(-1, 62)
    off = np.asarray(line_offsets, np.int64)
    nl = len(off) - 1
    if off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] != cost.shape[0]:
        raise ValueError("line offsets")
    if not np.all(np.isfinite(cost)) or np.any(cost < 0):
        raise ValueError("cost")
    for k in ("word_cost", "oov_word_cost", "oov_glyph_cost"):
        if not (np.isfinite(prm[k]) and prm[k] >= 0):
            raise ValueError(k)
    if (bound_cost is None) != (join_cost is None):
        raise ValueError("bound_cost and join_cost go together")
    ng = cost.shape[0]
    bound = np.zeros(ng) if bound_cost is None else np.asarray(bound_cost, np.float32).astype(np.float64)
    join = np.zeros(ng) if join_cost is None else np.asarray(join_cost, np.float32).astype(np.float64)
    if bound.shape != (ng,) or join.shape != (ng,) or not np.all(np.isfinite(bound)) or not np.all(np.isfinite(join)) or \
            np.any(bound < 0) or np.any(join < 0):
        raise ValueError("gap costs")
    c64 = cost.astype(np.float64)
    sub = np.minimum(c64, c64[:, TWIN]) if prm["fold_case"] else c64
    rowmin = c64.min(axis=1) if ng else np.zeros(0)
    buckets = _buckets(words)
    lwo, wo, ents, wcs = [0], [0], [], []
    lc, raw, flags = np.zeros(nl), np.zeros(nl), np.zeros(nl, np.int32)
    for l in range(nl):
        g0, g1 = int(off[l]), int(off[l + 1])
        G = g1 - g0
        acc = np.float64(0.0)
        for g in range(g0, g1):
            acc = acc + rowmin[g]
        raw[l] = acc
        if G == 0 or G > MAX_GLYPHS:
            flags[l] = 1 if G == 0 else 2
            lc[l] = 0.0 if G == 0 else np.inf
            wo.append(g1)
            ents.append(-1)
            wcs.append(lc[l])
        else:
            L, E, U, J = _line_tables(sub[g0:g1], rowmin[g0:g1], join[g0:g1], buckets, prm)
            lens, e, c, total = _segment(L, E, U, J, bound[g0:g1], prm)
            lc[l] = total
            for M in lens:
                wo.append(wo[-1] + M)
            ents += e
            wcs += c
        lwo.append(len(ents))
    return {"line_word_offsets": np.array(lwo, np.int32), "word_offsets": np.array(wo, np.int32), "entries": np.array(ents, np.int32),
            "word_costs": np.array(wcs, np.float64), "line_costs": lc, "raw_costs": raw, "line_flags": flags}


def enumerate_line(costs, words, bound_cost=None, join_cost=None, **params):
    """Every segmentation of ONE short line: each composition of G, each part read by every entry of its length or as an
    out-of-vocabulary word.  The value of a segmentation is summed exactly as the DP sums it - left to right,
    ((B + bnd) + T) - and the DP's tie order is a lexicographic one on the parts read from the right, which is restated here
    directly: compare the last parts' (value so far, kind, M), and on equality the rest.  -> (lens, entries, word costs, total)."""
    prm = default_params()
    prm.update(params)
    cost = np.asarray(costs, np.float32).reshape(-1, 62)
    G = cost.shape[0]
    c64 = cost.astype(np.float64)
    sub = np.minimum(c64, c64[:, TWIN]) if prm["fold_case"] else c64
    rowmin = c64.min(axis=1)
    bound = np.zeros(G) if bound_cost is None else np.asarray(bound_cost, np.float32).astype(np.float64)
    join = np.zeros(G) if join_cost is None else np.asarray(join_cost, np.float32).astype(np.float64)
    wc, ow, og = np.float64(prm["word_cost"]), np.float64(prm["oov_word_cost"]), np.float64(prm["oov_glyph_cost"])

    cache = {}

    def part_options(i, M):
        if (i, M) not in cache:
            cache[(i, M)] = _part_options(i, M)
        return cache[(i, M)]

    def _part_options(i, M):
        """[(T, kind, entry, W or U)] of the part [i, i + M): per kind only the best entry by (value, index) can win, but all are listed."""
        j = np.float64(0.0)
        for k in range(1, M):
            j = j + join[i + k]
        opts = []
        for e, w in enumerate(words):
            if len(w) == M:
                v = np.float64(0.0)
                for k, c in enumerate(classes(w)):
                    v = v + sub[i + k, c]
                opts.append(((v + wc) + j, 0, e, v))
        u = ow
        for k in range(M):
            u = u + rowmin[i + k]
            u = u + og
        opts.append((u + j, 1, -1, u))
        return opts

    best = None
    for cuts in itertools.product((0, 1), repeat=G - 1):
        lens, run = [], 1
        for c in cuts:
            if c:
                lens.append(run)
                run = 1
            else:
                run += 1
        lens.append(run)
        if max(lens) > MAX_LEN:
            continue
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int)
        for pick in itertools.product(*[part_options(int(i), M) for i, M in zip(starts, lens)]):
            b = np.float64(0.0)
            keys = []
            for (t, kind, e, w), i, M in zip(pick, starts, lens):
                b = (b + (bound[i] if i > 0 else np.float64(0.0))) + t
                keys.append((b, kind, M, w, e))
            # the DP compares, at the last part, (B[G], kind, M); among equal ones the prefix was chosen the same way at its own end,
            # and inside a part the entry by (W, index): the reversed list of (B, kind, M, W, entry) is that order
            key = tuple(reversed(keys))
            if best is None or key < best[0]:
                best = (key, lens, [p[2] for p in pick], [p[0] for p in pick], b)
    return best[1], best[2], best[3], best[4]


def costs_for_phrase(text: str, rng=None, hit: float = 0.0, miss: float = 6.0, noise: float = 0.0) -> np.ndarray:
    """One row per character of `text` (no spaces): `hit` for its class, `miss` for every other, plus |noise| * uniform f32 noise."""
    c = costs_for_text(text, hit=hit, miss=miss)
    if rng is not None and noise:
        c = (c + (rng.random(c.shape) * noise).astype(np.float32)).astype(np.float32)
    return c


def gap_costs(word_offsets, n_glyphs, break_penalty=2.0, join_penalty=2.0):
    """capi.phrase_gap_costs restated: word_offsets are the sub-words' glyph ranges (the block ocr_break_words returns)."""
    bound = np.full(n_glyphs, break_penalty, np.float32)
    join = np.zeros(n_glyphs, np.float32)
    starts = np.asarray(word_offsets, np.int64)[:-1]
    starts = starts[starts < n_glyphs]
    bound[starts] = 0.0
    join[starts] = join_penalty
    return bound, join


def fuzz(seed: int, n_entries: int, gs, min_len: int = 1, max_len: int = MAX_LEN, integer: bool = False, lens=None, gaps: bool = False):
    """A seeded case -> (costs, line_offsets, words, bound, join): one line per glyph count of `gs`; lens: the entry lengths allowed."""
    rng = np.random.default_rng(seed)
    if lens is None:
        words = random_words(rng, n_entries, min_len, max_len)
    else:
        words = []
        for m in rng.choice(np.asarray(lens), n_entries):
            words.append("".join(ALPHABET[c] for c in rng.integers(0, 62, int(m))))
    off = np.concatenate([[0], np.cumsum(np.asarray(gs, np.int64))]).astype(np.int32)
    ng = int(off[-1])
    cost = make_costs(rng, ng, integer=integer)
    if gaps:
        hi = 4 if integer else 3
        bound = rng.integers(0, hi, ng).astype(np.float32) if integer else (rng.random(ng) * hi).astype(np.float32)
        join = rng.integers(0, hi, ng).astype(np.float32) if integer else (rng.random(ng) * hi).astype(np.float32)
    else:
        bound = join = None
    return cost, off, words, bound, join
