"""Glyph blocks for tests/test_gpu_word_breaks.py.  Everything is seeded; a block is built once, shared and never written to.  The two
thread jobs differ in every shape (word counts 37 against 300, the longest word 256 against 40 glyphs), so two handles that run them
side by side never launch the same grid."""
import functools

import numpy as np

from tests.test_word_break_oracle import random_block, row

EDGE_LENGTHS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257]   # lane, slot and limit edges; 257 is flagged
BATCHES = [1, 3, 4, 5, 257]                                                   # workgroup edges (four words a workgroup)


def _frozen(blk):
    for a in blk.values():
        a.setflags(write=False)
    return blk


def block_of(word_boxes, n_images=1, cuts=None):
    """a glyph block from per-word box lists; cuts: the word index where every image but the first starts"""
    nw = len(word_boxes)
    off = np.concatenate([[0], np.cumsum([len(w) for w in word_boxes])]).astype(np.int32)
    img = np.asarray([0] + list(cuts or []) + [nw], np.int32)
    assert len(img) == n_images + 1
    boxes = np.asarray([b for w in word_boxes for b in w], np.int32).reshape(-1, 4)
    info = np.stack([np.searchsorted(img[1:], np.arange(nw), side="right"), np.full(nw, 100), np.ones(nw, np.int64), np.zeros(nw, np.int64)],
                    axis=1).astype(np.int32) if nw else np.zeros((0, 4), np.int32)
    levels = (np.arange(2 * nw, dtype=np.float32).reshape(nw, 2) + 0.5)
    return {"img_offsets": img, "word_offsets": off, "word_info": info, "word_levels": levels, "boxes": boxes}


@functools.lru_cache(maxsize=None)
def edges():
    return _frozen(random_block(np.random.default_rng(21), EDGE_LENGTHS, n_images=3))


@functools.lru_cache(maxsize=None)
def batch(nw: int):
    rng = np.random.default_rng(100 + nw)
    lengths = rng.choice([0, 1, 2, 3, 4, 5, 7, 12, 30, 64, 65, 100, 200, 256, 257], nw).tolist()
    return _frozen(random_block(rng, lengths, n_images=4))   # (random cuts: images without words occur)


@functools.lru_cache(maxsize=None)
def wide():
    """coordinates up to 2^22: heights and gaps whose products with the percentages pass 2^31"""
    rng = np.random.default_rng(31)
    top = 1 << 22
    words = []
    for G in (2, 4, 5, 64, 200, 256):
        xs = np.sort(rng.choice(top, 2 * G, replace=False))
        w = [[int(xs[2 * i]), 0, int(xs[2 * i + 1]), 0] for i in range(G)]
        for b in w:
            y0 = int(rng.integers(0, top - 1))
            b[1], b[3] = y0, int(rng.integers(y0 + 1, top + 1))
        words.append(w)
    words.append([[0, 0, 1, top], [top - 1, 0, top, top]])                 # one gap of 2^22 - 2 under a height of 2^22
    words.append([[0, 0, 1, 1], [2, 0, 3, 1], [4, 0, 5, 1], [top - 1, 0, top, 1]])   # T = 2^22 - 6 against L = 1
    return _frozen(block_of(words))


@functools.lru_cache(maxsize=None)
def ties():
    """gaps from two or three values, and arithmetic progressions of an odd count, whose two middle cuts score the same"""
    rng = np.random.default_rng(41)
    words = []
    for G in (4, 5, 6, 9, 33, 64, 65, 130, 256):
        words.append(row(rng.choice([2, 9], G - 1).tolist()))
        words.append(row(rng.choice([3, 4, 12], G - 1).tolist(), h=int(rng.integers(6, 30))))
        words.append(row([5] * (G - 1)))
    for n in (3, 5, 7, 63, 255):
        for a, d in ((0, 1), (3, 2)):
            words.append(row(rng.permutation(a + d * np.arange(n)).tolist(), h=4))
    # a palindrome of gaps: equal values at both ends of the word
    words.append(row([2, 7, 2, 11, 2, 7, 2]))
    return _frozen(block_of(words, n_images=2, cuts=[len(words) // 2]))


@functools.lru_cache(maxsize=None)
def job(k: int):
    rng = np.random.default_rng(500 + k)
    if k == 0:
        lengths = rng.choice([0, 3, 17, 64, 129, 256], 37).tolist()
        return _frozen(random_block(rng, lengths, n_images=2)), {"mode": 1}
    lengths = rng.integers(0, 41, 300).tolist()
    return _frozen(random_block(rng, lengths, n_images=5)), {"mode": 1, "sep_pct": 150, "min_gaps": 4}


def two_groups():
    """a 64 x 256 frame with two groups of three bars in one polygon: 3 px inside a group, 14 px between"""
    fr = np.full((1, 1, 64, 256), 210.0, np.float32)
    for x0 in (20, 31, 42, 64, 75, 86):
        fr[0, 0, 20:44, x0:x0 + 8] = 30.0
    return fr, [[[(4, 10), (120, 10), (120, 54), (4, 54)]]], np.ones((1, 2))


def forty_bars():
    """one polygon of 40 bars, 4 px wide and 2 px apart, with 16 px after the 20th"""
    fr = np.full((1, 1, 64, 320), 210.0, np.float32)
    x, xs = 10, []
    for i in range(40):
        xs.append(x)
        fr[0, 0, 16 + (i % 3):48 - (i % 5), x:x + 4] = 30.0
        x += 4 + (16 if i == 19 else 2)
    return fr, [[[(4, 8), (x + 4, 8), (x + 4, 56), (4, 56)]]], np.ones((1, 2))
