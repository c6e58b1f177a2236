"""CTC prefix beam search in f64 - the checker of ocr_ctc_beam_decode (include/ocr_amd.h states the rule; the kernel is
ocr-rs_amd/csrc/ctc_beam.hip).  A plain restatement: every extension of every beam is a candidate (no pre-selection), prefixes are
tuples and merges are found by dictionary lookup.  Besides the hypotheses it reports, per crop, the smallest score gap between
neighbours among the first B + 1 candidates of any column (the gaps that decided which candidates survive and in what order), so a
test can tell an exact tie (gap 0, decided by the key) from a near tie that rounding in a different log-softmax could flip."""
import math

import numpy as np

NEG_INF = -math.inf


def lse2(a: float, b: float) -> float:
    """a (+) b = M + log1p(exp(m - M)), exactly commutative, -inf (+) x = x."""
    M, m = (a, b) if a > b else (b, a)
    if m == NEG_INF:
        return M
    return M + math.log1p(math.exp(m - M))


def log_softmax(col: np.ndarray) -> np.ndarray:
    col = np.asarray(col, np.float64)
    mx = col.max()
    return (col - mx) - math.log(float(np.exp(col - mx).sum()))


def decode_one(x: np.ndarray, blank: int, beam_width: int, trace: bool = False):
    """x: T x C logits of one crop -> ([(prefix tuple, score)] in rank order, margin[, per-column beam prefixes])."""
    x = np.asarray(x)
    T, C = x.shape
    if not np.isfinite(x).all():
        raise ValueError("non-finite logit")
    beams = [((), 0.0, NEG_INF)]   # (prefix, lb, lnb) in rank order
    margin = math.inf
    steps = []
    classes = np.arange(C)
    for t in range(T):
        lp = log_softmax(x[t].astype(np.float64))
        index = {p: r for r, (p, _, _) in enumerate(beams)}
        tots = [lse2(lb, lnb) for _, lb, lnb in beams]
        stay_lb = [tots[r] + lp[blank] for r in range(len(beams))]
        stay_lnb = [lnb + lp[p[-1]] if p else NEG_INF for p, _, lnb in beams]
        merged = [set() for _ in beams]
        for j, (p, _, _) in enumerate(beams):
            r = index.get(p[:-1]) if p else None
            if r is not None:
                c = p[-1]
                lb_r, tot_r = beams[r][1], tots[r]
                e_r = beams[r][0][-1] if beams[r][0] else -1
                stay_lnb[j] = lse2(stay_lnb[j], (lb_r if c == e_r else tot_r) + lp[c])
                merged[r].add(c)
        sc, rr, cc = [], [], []
        for r, (p, lb, _) in enumerate(beams):
            sc.append(lse2(stay_lb[r], stay_lnb[r]))
            rr.append(r)
            cc.append(-1)
            ext = tots[r] + lp
            if p:
                ext[p[-1]] = lb + lp[p[-1]]
            keep = classes != blank
            for c in merged[r]:
                keep[c] = False
            sc.extend(ext[keep].tolist())
            rr.extend([r] * int(keep.sum()))
            cc.extend(classes[keep].tolist())
        sc = np.asarray(sc, np.float64)
        rr = np.asarray(rr)
        cc = np.asarray(cc)
        order = np.lexsort((cc, rr, -sc))[: beam_width + 1]
        top = sc[order]
        fin = top[:-1] > NEG_INF   # candidates of probability 0 (e.g. "aa" from a beam without a blank ending) tie exactly
        if fin.any():
            margin = min(margin, float(np.min(top[:-1][fin] - top[1:][fin])))
        nxt = []
        for i in order[:beam_width]:
            r, c = int(rr[i]), int(cc[i])
            p = beams[r][0]
            if c < 0:
                nxt.append((p, stay_lb[r], stay_lnb[r]))
            else:
                nxt.append((p + (c,), NEG_INF, float(sc[i])))
        beams = nxt
        if trace:
            steps.append([p for p, _, _ in beams])
    out = [(p, lse2(lb, lnb)) for p, lb, lnb in beams]
    return (out, margin, steps) if trace else (out, margin)


def ctc_beam_decode(logits: np.ndarray, blank: int, beam_width: int):
    """N x T x C -> (labels N x B x T int32 padded with -1, lengths N x B (-1: unused slot), scores N x B f64 (-inf: unused slot),
    margins N f64)."""
    x = np.asarray(logits)
    n, t, _ = x.shape
    labels = np.full((n, beam_width, t), -1, np.int32)
    lengths = np.full((n, beam_width), -1, np.int32)
    scores = np.full((n, beam_width), NEG_INF, np.float64)
    margins = np.empty(n, np.float64)
    for i in range(n):
        hyps, margins[i] = decode_one(x[i], blank, beam_width)
        for k, (p, s) in enumerate(hyps):
            lengths[i, k] = len(p)
            labels[i, k, : len(p)] = p
            scores[i, k] = s
    return labels, lengths, scores, margins


def brute_force(x: np.ndarray, blank: int) -> dict:
    """Exact CTC log P(l | x) of every label sequence l with P > 0 (the decoder also returns prefixes of probability 0, score -inf), by enumerating all C^T alignments of one T x C crop."""
    x = np.asarray(x)
    T, C = x.shape
    lp = np.stack([log_softmax(x[t].astype(np.float64)) for t in range(T)])
    terms = {}
    for a in np.ndindex(*([C] * T)):
        lab, prev = [], -1
        for k in a:
            if k != blank and k != prev:
                lab.append(int(k))
            prev = k
        terms.setdefault(tuple(lab), []).append(math.fsum(lp[t, a[t]] for t in range(T)))
    out = {}
    for lab, v in terms.items():
        m = max(v)
        out[lab] = m + math.log(math.fsum(math.exp(s - m) for s in v))
    return out
