"""fp64 restatement of espnet 202402 ``BeamSearchTimeSync`` (the reference's ``Speech2Text(time_sync=True)``), the yardstick of
tavsr/inference/timesync.py: a CTC prefix beam search walked frame by frame, every prefix that enters the beam rescored by
pluggable scorers.  Pure numpy, dictionaries keyed by token tuples, one utterance.

``timesync_search(lpz, K, sos, ...)`` -> ``Result``: the hypotheses ``[(list(h) + [sos], score)]`` best first, and what the tests ask
of the INPUTS: ``mingap`` (the smallest distance, over the frames, between the K-th and the (K+1)-th joint score and between the
C-th and the (C+1)-th frame value: below it a rounding error may change what is kept), ``reentries`` (a prefix that entered the
beam after it had dropped out of ``dp``) and ``merges`` (the fell-off-the-beam branch ran)."""
import math
from collections import namedtuple

import numpy as np

NEG = -math.inf
Result = namedtuple("Result", "hyps mingap reentries merges ncand_max")


def lae(a, b):
    m = max(a, b)
    if m == NEG:
        return NEG
    return m + math.log1p(math.exp(min(a, b) - m))


def timesync_search(lpz, K, sos, w_ctc=1.0, w_dec=0.0, w_lm=0.0, pen=0.0, dec_row=None, lm_row=None, pre_beam_ratio=1.5, blank=0,
                    C=None):
    """lpz [T, V] log-softmax of the CTC head.  ``dec_row`` / ``lm_row``: prefix tuple -> row [V] of log-probabilities of the next
    token (None or weight 0: the term is skipped)."""
    lpz = np.asarray(lpz, dtype=np.float64)
    T, V = lpz.shape
    C = int(pre_beam_ratio * K) if C is None else C
    if C > V:
        raise IndexError(f"pre-beam {C} > vocabulary {V}")
    use_dec = dec_row is not None and w_dec != 0.0
    use_lm = lm_row is not None and w_lm != 0.0
    rows = {}          # (which, prefix) -> row: pure functions of the prefix, cached as the reference caches them
    sums = {(sos,): (0.0, 0.0)}

    def row(which, fn, l):
        if (which, l) not in rows:
            rows[(which, l)] = np.asarray(fn(l), dtype=np.float64)
        return rows[(which, l)]

    def prefix_sums(h):
        if h not in sums:
            d, m = prefix_sums(h[:-1])
            if use_dec:
                d += float(row(0, dec_row, h[:-1])[h[-1]])
            if use_lm:
                m += float(row(1, lm_row, h[:-1])[h[-1]])
            sums[h] = (d, m)
        return sums[h]

    hyps = [(sos,)]
    dp = {(sos,): (NEG, 0.0)}
    score = {(sos,): 0.0}
    ever, mingap, reentries, merges, ncand_max = {(sos,)}, math.inf, 0, 0, 0
    for t in range(T):
        p = lpz[t]
        srt = np.sort(p)
        thr = srt[-C]
        cands = [c for c in range(V) if p[c] >= thr]
        ncand_max = max(ncand_max, len(cands))
        if C < V:
            mingap = min(mingap, float(srt[-C] - srt[-C - 1]))
        nxt, new = {}, []
        in_new = set()

        def add_new(h):
            if h not in in_new:
                in_new.add(h)
                new.append(h)

        hset = set(hyps)
        for l in hyps:
            l_nb, l_b = dp.get(l, (NEG, NEG))
            pl = lae(l_nb, l_b)
            for c in cands:
                if c == blank:
                    nb, b = nxt.get(l, (NEG, NEG))
                    nxt[l] = (nb, lae(b, p[c] + pl))
                    add_new(l)
                    continue
                lp = l + (c,)
                nb, b = nxt.get(lp, (NEG, NEG))
                if c == l[-1]:
                    nb = lae(nb, p[c] + l_b)
                    o_nb, o_b = nxt.get(l, (NEG, NEG))
                    nxt[l] = (lae(o_nb, p[c] + l_nb), o_b)
                else:
                    nb = lae(nb, p[c] + pl)
                if lp not in hset and lp in dp:
                    merges += 1
                    b = lae(b, p[blank] + lae(*dp[lp]))
                    nb = lae(nb, p[c] + dp[lp][0])
                nxt[lp] = (nb, b)
                add_new(lp)
        score = {}
        for h in new:
            s = w_ctc * lae(*nxt[h]) if w_ctc != 0.0 else 0.0
            if len(h) > 1:
                d, m = prefix_sums(h)
                if use_dec:
                    s += w_dec * d
                if use_lm:
                    s += w_lm * m
            s += pen * (len(h) - 1)
            score[h] = s
        ranked = sorted(new, key=lambda h: score[h], reverse=True)
        if len(ranked) > K and score[ranked[K - 1]] > NEG:
            mingap = min(mingap, score[ranked[K - 1]] - score[ranked[K]])
        for h in ranked[:K]:
            if h not in hset:
                if h in ever and h not in dp:
                    reentries += 1
                ever.add(h)
        hyps = ranked[:K]
        dp = nxt
    return Result([(list(h) + [sos], score.get(h, 0.0)) for h in hyps], mingap, reentries, merges, ncand_max)
