"""Host half of the batched beam search (inference/beam_search.py): espnet's ``post_process`` / ``end_detect`` for every utterance of
a batch at once, over the per-token records (token, back-pointer, score) the device leaves, or over the eager route's tensors.
CPU tensor code on [U] / [U * K]-sized operands: nothing here touches the device, so it runs (and is tested) without one."""
from __future__ import annotations

import math

import torch

D_END = math.log(1 * math.exp(-10))       # espnet end_detect: an ended hypothesis this far below the best one counts as hopeless


def max_tokens(maxlenratio: float, lens):
    """espnet BeamSearch.forward, per utterance of ``lens`` frames: maxlenratio == 0 -> up to T tokens (with end detection);
    < 0 -> -int(ratio) tokens; > 0 -> max(1, int(ratio * T)) tokens (both without end detection)"""
    if maxlenratio == 0.0:
        return list(lens)
    if maxlenratio < 0:
        return [-1 * int(maxlenratio)] * len(lens)
    return [max(1, int(maxlenratio * t)) for t in lens]


class HostSearch:
    """bookkeeping of one decode(): which utterances still search, the hypotheses that ended, the best ended score per length"""

    def __init__(self, maxlenratio: float, lens, K: int, sos: int, eos: int):
        self.maxlenratio, self.K, self.sos, self.eos = maxlenratio, K, sos, eos
        self.maxl = max_tokens(maxlenratio, lens)
        self.U, self.steps = len(lens), max(self.maxl)
        U = self.U
        self.lens_c = torch.tensor(self.maxl)                            # per-utterance maxlen: the last iteration closes every hypothesis
        self.active = torch.ones(U, dtype=torch.bool)
        self.n_host = torch.zeros(U, dtype=torch.int32)                  # tokens searched per utterance
        self.best = torch.full((U,), -float("inf"))                      # best ended score per utterance
        self.best_len = torch.full((U, self.steps + 4), -float("inf"))   # best ended score per (utterance, hypothesis length)
        self.ended = [[] for _ in range(U)]

    def step(self, i, tok_h, score_h, rows_of):
        """espnet post_process / end_detect for token i of every utterance: collects the hypotheses that end here
        (``rows_of(slot indices)`` -> their token lists incl. <sos>), returns the slots to retire."""
        U, K, best, best_len = self.U, self.K, self.best, self.best_len
        N = U * K
        self.n_host.add_(self.active.to(torch.int32))
        valid = torch.isfinite(score_h).view(U, K) & self.active.view(U, 1)
        last = (self.lens_c - 1 == i).view(U, 1)
        # espnet appends <eos> to EVERY hypothesis of the last iteration (also to the ones that just ended)
        take = valid & ((tok_h.view(U, K) == self.eos) | last)
        if bool(take.any()):
            idx = take.view(N).nonzero().view(-1)
            us = idx // K
            lns = torch.where(last.view(U)[us], torch.full_like(us, i + 3), torch.full_like(us, i + 2))
            scs = score_h[idx]
            for ys, u_, ln, sc in zip(rows_of(idx), us.tolist(), lns.tolist(), scs.tolist()):
                ys = (ys + [self.eos] * 2)[:ln]
                ys[ln - 1] = self.eos
                self.ended[u_].append((ys, sc))
            best.index_reduce_(0, us, scs, "amax")
            flat = us * best_len.shape[1] + lns
            best_len.view(-1).index_reduce_(0, flat, scs, "amax")
        running = (valid & ~take).sum(dim=1)
        count = torch.zeros(U, dtype=torch.int64)
        for m in range(3):                                     # end_detect: M = 3 most recent lengths
            if i - m >= 0:
                bl = best_len[:, i - m]
                count += (torch.isfinite(bl) & (bl - best < D_END)).to(torch.int64)
        if self.maxlenratio != 0.0:                            # end_detect runs only for maxlenratio == 0
            count.zero_()
        stop = (count == 3) | (running == 0) | last.view(U)
        self.active = self.active & ~stop
        return (take | ~self.active.view(U, 1)).view(N)

    def rows_from_records(self, rec, i):
        """``rows_of`` for ``step(i, ...)`` over the records rec[token][0: token, 1: slot it extended, 2: score bits][slot]"""
        def rows_of(idx):
            out_rows = []
            for n in idx.tolist():
                toks, cur = [], n
                for t in range(i, -1, -1):                  # back-track: token of slot `cur`, then the slot it extended
                    toks.append(int(rec[t, 0, cur]))
                    cur = int(rec[t, 1, cur])
                out_rows.append([self.sos] + toks[::-1])
            return out_rows
        return rows_of

    def step_from_records(self, rec, i):
        """``step`` for token i read from the records (int32 tensor [steps, 3, U * K]; the scores as float bits)"""
        return self.step(i, rec[i, 0].to(torch.int64), rec[i, 2].view(torch.float32), self.rows_from_records(rec.numpy(), i))

    def nbest(self, nbest=None):
        """per utterance the ended hypotheses (token list, score), best first"""
        out = []
        for hyps in self.ended:
            hyps = sorted(hyps, key=lambda h: h[1], reverse=True)
            out.append(hyps if nbest is None else hyps[:nbest])
        return out
