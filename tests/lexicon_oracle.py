"""Numpy f64 restatement of the lexicon-matching rule of ocr_lexicon_match and of the glyph costs of ocr_rec_glyph_costs
(include/ocr_amd.h; kernels csrc/lexicon.hip).  BUILD-DEFINED: the reference has no counterpart, nothing here is read from it.

The DP is vectorised over (the words of one glyph count) x (the entries of one length bucket): every cell is one numpy operation on
a [words, entries] array, so each add and each min is rounded separately, exactly as the rule says.  The order of the two inner mins
follows the header: min(diagonal, min(up, left)).
"""
from __future__ import annotations

import numpy as np

ALPHABET = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789"
CLASS_OF = {ch: k for k, ch in enumerate(ALPHABET)}
MAX_LEN = 32
TWIN = np.array([c + 26 if c < 26 else c - 26 if c < 52 else c for c in range(62)])


def classes(word: str) -> np.ndarray:
    return np.array([CLASS_OF[ch] for ch in word], np.int64)


def glyph_costs(logits: np.ndarray) -> np.ndarray:
    """The negative log-softmax in f64, the sum in class order, clamped at 0, rounded to f32."""
    x = np.asarray(logits, np.float32).reshape(-1, 62).astype(np.float64)
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    s = np.zeros(x.shape[0])
    for c in range(62):
        s = s + e[:, c]
    lse = m[:, 0] + np.log(s)
    return np.maximum(lse[:, None] - x, 0.0).astype(np.float32)


def make_costs(rng, n_glyphs: int, integer: bool = False, high: int = 4) -> np.ndarray:
    """A cost table n_glyphs x 62 f32.  integer=True: whole numbers in [0, high), so that equal costs - ties - are real and every sum
    is exact; otherwise the glyph costs of random logits with one favoured class per row."""
    if integer:
        return rng.integers(0, high, size=(n_glyphs, 62)).astype(np.float32)
    lg = (rng.standard_normal((n_glyphs, 62)) * 3).astype(np.float32)
    if n_glyphs:
        lg[np.arange(n_glyphs), rng.integers(0, 62, n_glyphs)] += 6
    return glyph_costs(lg)


def costs_for_text(text: str, hit: float = 0.0, miss: float = 6.0) -> np.ndarray:
    """Hand cases: one row per character, `hit` for its class and `miss` for every other one (a miss is cheaper than an insertion
    plus a deletion at the default costs)."""
    c = np.full((len(text), 62), miss, np.float32)
    for i, ch in enumerate(text):
        c[i, CLASS_OF[ch]] = hit
    return c


def match(costs, word_offsets, words, ins_cost=4.0, del_cost=4.0, max_len_diff=2, fold_case=1, top_k=1) -> dict:
    """-> entries [n_words, top_k] int32, costs [n_words, top_k] f64, raw_costs, n_candidates, word_flags, and `ties`: the number of
    (word, rank) pairs whose cost equals the next candidate's in sorted order, that is, the places where the entry index decided."""
    cost = np.asarray(costs, np.float32).reshape(-1, 62)
    off = np.asarray(word_offsets, np.int64)
    nw = len(off) - 1
    if off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] != cost.shape[0]:
        raise ValueError("word offsets")
    if not np.all(np.isfinite(cost)) or np.any(cost < 0):
        raise ValueError("cost")
    c64 = cost.astype(np.float64)
    sub = np.minimum(c64, c64[:, TWIN]) if fold_case else c64
    ins, dele = np.float64(ins_cost), np.float64(del_cost)
    lens = np.array([len(w) for w in words], np.int64)
    if np.any(lens < 1) or np.any(lens > MAX_LEN):
        raise ValueError("entry length")
    by_len = {}
    for m in range(1, MAX_LEN + 1):
        idx = np.flatnonzero(lens == m)
        if len(idx):
            by_len[m] = (idx, np.stack([classes(words[k]) for k in idx]))
    G_of = np.diff(off)
    entries = np.full((nw, top_k), -1, np.int32)
    out_cost = np.full((nw, top_k), np.inf)
    raw = np.zeros(nw)
    n_cand = np.zeros(nw, np.int32)
    flags = np.zeros(nw, np.int32)
    ties = 0
    rowmin = c64.min(axis=1) if cost.shape[0] else np.zeros(0)
    for w in range(nw):
        acc = np.float64(0.0)
        for g in range(off[w], off[w + 1]):
            acc = acc + rowmin[g]
        raw[w] = acc
    flags[G_of == 0] = 1
    flags[G_of > MAX_LEN] = 2
    for G in sorted(set(int(g) for g in G_of if 1 <= g <= MAX_LEN)):
        ws = np.flatnonzero(G_of == G)
        S = np.stack([sub[off[w]:off[w] + G] for w in ws])          # [words, G, 62]
        cand_idx, cand_cost = [], []
        for M in range(max(1, G - max_len_diff), min(MAX_LEN, G + max_len_diff) + 1):
            if M not in by_len:
                continue
            idx, codes = by_len[M]
            D = [np.zeros((len(ws), len(idx)))]
            for i in range(1, G + 1):
                D.append(D[i - 1] + dele)
            for j in range(M):
                diag = D[0]
                D[0] = D[0] + ins
                for i in range(1, G + 1):
                    s = S[:, i - 1, :][:, codes[:, j]]                # [words, entries]
                    a = diag + s
                    diag = D[i]
                    D[i] = np.minimum(a, np.minimum(D[i - 1] + dele, diag + ins))
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
            k = min(top_k, len(idx))
            entries[w, :k] = idx[order[:k]]
            out_cost[w, :k] = cc[r, order[:k]]
            sc = cc[r, order[:k + 1]]
            ties += int(np.count_nonzero(sc[1:] == sc[:-1]))
    return {"entries": entries, "costs": out_cost, "raw_costs": raw, "n_candidates": n_cand, "word_flags": flags, "ties": ties}


def random_words(rng, n: int, min_len: int = 1, max_len: int = MAX_LEN) -> list:
    """n random entries over the alphabet, lengths uniform in [min_len, max_len]; duplicates may occur."""
    lens = rng.integers(min_len, max_len + 1, n)
    flat = rng.integers(0, 62, int(lens.sum()))
    out, p = [], 0
    for m in lens:
        out.append("".join(ALPHABET[c] for c in flat[p:p + m]))
        p += int(m)
    return out


def hand_cases() -> dict:
    """name -> (costs, word_offsets, words, params): the hand cases of tests/test_lexicon_oracle.py, which states what each must give,
    and of tests/test_gpu_lexicon.py, which runs each through the C ABI.  All costs are whole numbers."""
    def one(text, **kw):
        return costs_for_text(text, **kw), [0, len(text)]
    cases = {}
    cases["greedy_in_list"] = (*one("HELLO", hit=1.0), ["HELLO", "WORLD", "HELPS"], dict(fold_case=0, top_k=2))
    cases["missed_glyph"] = (*one("HELO"), ["HALO", "HELLO", "HELLOS"], dict(fold_case=0, top_k=3))
    cases["spurious_glyph"] = (*one("HELLLO"), ["HELLO", "JELLO"], dict(fold_case=0, del_cost=3.0, top_k=2))
    cases["fold_on"] = (*one("HELLo"), ["hello", "HELPS"], dict(fold_case=1, top_k=2))
    cases["fold_off"] = (*one("HELLo"), ["hello", "HELPS"], dict(fold_case=0, top_k=2))
    cases["len_diff_0"] = (*one("HELO"), ["HELLO", "HELLOS"], dict(max_len_diff=0))
    cases["len_diff_2"] = (*one("HELO"), ["HELLO", "HELLOS"], dict(max_len_diff=2))
    cases["duplicates"] = (*one("HELLO"), ["HELLO", "HELLO", "HELPS", "HELLO"], dict(top_k=3))
    cases["equal_costs"] = (*one("HELLO"), ["HELLB", "HELLA", "HELLO9"], dict(fold_case=0, top_k=3))
    cases["top_k_past_candidates"] = (*one("HELLO"), ["HELLO", "HELL"], dict(top_k=8))
    flag_costs = np.concatenate([costs_for_text("A" * 33), costs_for_text("HELLO")])
    cases["flags"] = (flag_costs, [0, 0, 33, 38, 38], ["A" * 20, "B" * 21], dict(top_k=2))
    return cases


def fuzz(seed: int, n_entries: int, gs, min_len: int = 1, max_len: int = MAX_LEN, integer: bool = False, unique: bool = False):
    """A seeded case: n_entries random entries (unique=True drops repeats, so there may be fewer) and one word per glyph count of
    `gs` -> (costs, word_offsets, words)."""
    rng = np.random.default_rng(seed)
    words = random_words(rng, n_entries, min_len, max_len)
    if unique:
        words = list(dict.fromkeys(words))
    off = np.concatenate([[0], np.cumsum(np.asarray(gs, np.int64))]).astype(np.int32)
    return make_costs(rng, int(off[-1]), integer=integer), off, words


# The seeded cases of tests/test_gpu_lexicon.py whose tie count is part of the claim: name -> (fuzz arguments, match parameters,
# whether the oracle must see ties).  tests/test_lexicon_oracle.py checks the counts without a GPU.
TIE_CASES = {
    "integer_ties": (dict(seed=71, n_entries=600, gs=[1, 2, 3, 4, 5, 6, 8, 3, 4], min_len=1, max_len=8, integer=True), dict(top_k=8), True),
    "layout_no_ties": (dict(seed=72, n_entries=900, gs=[2, 3, 4, 5, 6, 7, 9, 12], min_len=1, max_len=14, unique=True),
                       dict(top_k=8, ins_cost=9.25, del_cost=7.5, fold_case=0), False),
}
