"""Restatements of espnet2 asr/transducer/beam_search_transducer.py ``align_length_sync_decoding`` (ALSD) and
``time_sync_decoding`` (TSD) for one utterance, over ``rnnt_ref.joint_logits`` and the LSTM step of ``rnnt_ref.greedy_search``
(CPU, plain torch; the dtype follows the inputs, so the same code is the float64 reference and the fp32 chain the GPU tests take
their score tolerance from).  espnet is not importable here; the two searches are restated from the published class.

Where ``torch.topk`` and ``sorted`` leave a choice, the rule is: among equal log-probabilities the lower token id comes first, and
every sort is stable in insertion order.

``alsd(...)`` and ``tsd(...)`` -> ``(hyps, merges, mingap)``: the FULL sorted result list ``[(yseq with the leading blank, score)]``
(``sort_nbest`` without the cut to ``nbest``), the number of ``logaddexp`` merges of equal prefixes, and the smallest margin of any
decision: at every cut (a label top-k, a beam cut) the difference between the last kept and the first dropped score, and the
difference between the first and the second sort key of the result.  An utterance is *binding* when ``mingap > 1e-4``.
(ALSD returns the beam itself, unsorted, where nothing reached the last frame: ``info["from_final"]`` tells.)"""
import math

import torch

import rnnt_ref as R

BINDING = 1e-4


class Net:
    """dec_out(y) and logp(t, y) of one utterance, each computed once per prefix"""

    def __init__(self, enc_out, embed_w, layers, P, blank=0):
        self.enc, self.embed_w, self.layers, self.P, self.blank = enc_out, embed_w, layers, P, blank
        self.states, self.rows = {}, {}

    def state(self, y):
        """(dec_out, h, c) after consuming every token of ``y`` from the zero state"""
        if y not in self.states:
            H = self.layers[0][1].shape[1]
            if len(y) == 1:
                h = [self.enc.new_zeros(1, H) for _ in self.layers]
                c = [self.enc.new_zeros(1, H) for _ in self.layers]
            else:
                _, h, c = self.state(y[:-1])
            x = self.embed_w[torch.tensor([y[-1]])]
            h2, c2 = [], []
            for li, (w_ih, w_hh, b_ih, b_hh) in enumerate(self.layers):
                g = x @ w_ih.T + b_ih + h[li] @ w_hh.T + b_hh
                i, f, gg, o = g.chunk(4, dim=1)
                cc = torch.sigmoid(f) * c[li] + torch.sigmoid(i) * torch.tanh(gg)
                x = torch.sigmoid(o) * torch.tanh(cc)
                h2.append(x)
                c2.append(cc)
            self.states[y] = (x[0], h2, c2)
        return self.states[y]

    def logp(self, t, y):
        if (t, y) not in self.rows:
            self.rows[(t, y)] = R.joint_logits(self.enc[t], self.state(y)[0], self.P).log_softmax(-1)
        return self.rows[(t, y)]


def topk_labels(logp, beam):
    """the ``beam`` best of logp[1:] with ids shifted by +1, the lower id first among equals -> (values, ids, margin of the cut)"""
    vals, idx = torch.sort(logp[1:], descending=True, stable=True)
    gap = float(vals[beam - 1] - vals[beam]) if vals.numel() > beam else math.inf
    return vals[:beam], [int(i) + 1 for i in idx[:beam]], gap


def best(hyps, beam):
    """sorted(hyps, key=score, reverse=True)[:beam], stable -> (kept, margin of the cut)"""
    order = sorted(range(len(hyps)), key=lambda j: -float(hyps[j][0]))
    gap = float(hyps[order[beam - 1]][0]) - float(hyps[order[beam]][0]) if len(order) > beam else math.inf
    return [hyps[j] for j in order[:beam]], gap


def recombine(hyps):
    """the first occurrence of a yseq keeps its place; a later equal yseq adds its score into it with logaddexp -> (list, merges)"""
    out, merges = [], 0
    for s, y in hyps:
        at = [j for j, (_, y2) in enumerate(out) if y2 == y]
        if at:
            out[at[0]] = (torch.logaddexp(out[at[0]][0], s), y)
            merges += 1
        else:
            out.append((s, y))
    return out, merges


def sort_nbest(hyps, score_norm=True, nbest=None):
    """descending by score / len(yseq) (len counts the leading blank) or by score, stable; the score returned is un-normalised
    -> (list cut to ``nbest``, margin between the first and the second key)"""
    key = [float(s) / len(y) if score_norm else float(s) for s, y in hyps]
    order = sorted(range(len(hyps)), key=lambda j: -key[j])
    gap = key[order[0]] - key[order[1]] if len(order) > 1 else math.inf
    out = [hyps[j] for j in order]
    return (out if nbest is None else out[:nbest]), gap


def sort_key(hyp, score_norm=True):
    ys, score = hyp
    return score / len(ys) if score_norm else score


def _result(hyps):
    return [(list(y), float(s)) for s, y in hyps]


@torch.no_grad()
def alsd(enc_out, embed_w, layers, P, beam_size, u_max=50, score_norm=True, blank=0, info=None):
    """``info`` (a dict) receives ``from_final``: False where no hypothesis reached the last frame and espnet returns the beam B
    as it stands - unfinished hypotheses in beam order, whose scores are those of partial alignments"""
    net = Net(enc_out, embed_w, layers, P, blank)
    T, V = enc_out.shape[0], P[3].shape[0]
    beam = min(beam_size, V)
    u_max = min(u_max, T - 1)
    B, final, merges, gap = [(enc_out.new_zeros(()), (blank,))], [], 0, math.inf
    for i in range(T + u_max):
        B_ = [(s, y) for s, y in B if i - (len(y) - 1) <= T - 1]
        if not B_:
            continue
        A = []
        for s, y in B_:
            t = i - (len(y) - 1)
            logp = net.logp(t, y)
            A.append((s + logp[0], y))
            if t == T - 1:
                final.append((s + logp[0], y))
            vals, ids, g = topk_labels(logp, beam)
            gap = min(gap, g)
            A += [(s + v, y + (k,)) for v, k in zip(vals, ids)]
        B, g = best(A, beam)
        gap = min(gap, g)
        B, m = recombine(B)
        merges += m
    if info is not None:
        info["from_final"] = bool(final)
    if not final:
        return _result(B), merges, gap
    out, g = sort_nbest(final, score_norm)
    return _result(out), merges, min(gap, g)


@torch.no_grad()
def tsd(enc_out, embed_w, layers, P, beam_size, max_sym_exp=2, score_norm=True, blank=0):
    net = Net(enc_out, embed_w, layers, P, blank)
    T, V = enc_out.shape[0], P[3].shape[0]
    beam = min(beam_size, V)
    B, merges, gap = [(enc_out.new_zeros(()), (blank,))], 0, math.inf
    for t in range(T):
        A, C = [], B
        for v in range(max_sym_exp):
            seen = [y for _, y in A]
            for s, y in C:
                sb = s + net.logp(t, y)[0]
                if y in seen:
                    at = seen.index(y)
                    A[at] = (torch.logaddexp(A[at][0], sb), y)
                    merges += 1
                else:
                    A.append((sb, y))
            if v < max_sym_exp - 1:
                D = []
                for s, y in C:
                    vals, ids, g = topk_labels(net.logp(t, y), beam)
                    gap = min(gap, g)
                    D += [(s + val, y + (k,)) for val, k in zip(vals, ids)]
                C, g = best(D, beam)
                gap = min(gap, g)
            else:
                C = []
        B, g = best(A, beam)
        gap = min(gap, g)
    out, g = sort_nbest(B, score_norm)
    return _result(out), merges, min(gap, g)


def nll_of(enc_out, embed_w, layers, P, yseq, blank=0):
    """-log p(labels of yseq | enc_out) over ALL alignments, on the same logits (rnnt_ref.rnnt_nll)"""
    labels = list(yseq[1:])
    dec = R.lstm_stack(embed_w, layers, torch.tensor([[blank] + labels]))[0]
    logits = R.joint_logits(enc_out[:, None, :], dec[None, :, :], P)
    return float(R.rnnt_nll(logits.detach(), labels, blank))


def parity_depth(hyps, score_norm=True, bar=BINDING):
    """how far down the result list a comparison runs: to the first neighbouring pair whose sort keys differ by less than
    ``bar`` (the best hypothesis is always compared)"""
    for j in range(len(hyps) - 1):
        if sort_key(hyps[j], score_norm) - sort_key(hyps[j + 1], score_norm) < bar:
            return max(1, j)      # the places of j and j + 1 may swap
    return len(hyps)
