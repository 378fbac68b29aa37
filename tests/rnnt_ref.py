"""Float64 restatements of the transducer leaves (CPU, plain torch; dtype follows the inputs, so the same code gives the fp32
chain the GPU tests take their tolerance from).  espnet and warp-transducer are not importable here: the loss convention
(warp-transducer RNNTLoss: logits in, log-softmax inside, blank = blank_id, reduction="mean" = sum over utterances / B,
fastemit_lambda = 0), the joint (espnet2 asr_transducer/joint_network.py), the decoder (espnet2 asr/decoder/transducer_decoder.py)
and the greedy search (espnet2 asr/transducer/beam_search_transducer.py greedy_search) are restated from the published classes."""
import itertools
import math

import torch


# ---------------------------------------------------------------------------------------------- lattice
def lattice(lp_blank, lp_label, T, U):
    """lp_blank, lp_label [>=T, >=U+1] -> (nll, alpha, beta) over T x (U + 1) nodes, differentiable"""
    ninf = lp_blank.new_tensor(-math.inf)
    alpha = [[None] * (U + 1) for _ in range(T)]
    for t in range(T):
        for u in range(U + 1):
            if t == 0 and u == 0:
                alpha[t][u] = lp_blank.new_tensor(0.0)
                continue
            up = alpha[t - 1][u] + lp_blank[t - 1, u] if t > 0 else ninf
            left = alpha[t][u - 1] + lp_label[t, u - 1] if u > 0 else ninf
            alpha[t][u] = torch.logaddexp(up, left)
    beta = [[None] * (U + 1) for _ in range(T)]
    for t in reversed(range(T)):
        for u in reversed(range(U + 1)):
            if t == T - 1 and u == U:
                beta[t][u] = lp_blank[t, u]
                continue
            down = beta[t + 1][u] + lp_blank[t, u] if t + 1 < T else ninf
            right = beta[t][u + 1] + lp_label[t, u] if u < U else ninf
            beta[t][u] = torch.logaddexp(down, right)
    ll = alpha[T - 1][U] + lp_blank[T - 1, U]
    return -ll, alpha, beta


def lattice_coefficients(lp_blank, lp_label, T, U):
    """-> (nll, occ, p_blank, p_label [T, U+1]): node occupancy and the posteriors of its blank / label transition"""
    nll, alpha, beta = lattice(lp_blank, lp_label, T, U)
    ll = -nll
    occ, pb, pl = (torch.zeros(T, U + 1, dtype=lp_blank.dtype) for _ in range(3))
    for t in range(T):
        for u in range(U + 1):
            occ[t, u] = torch.exp(alpha[t][u] + beta[t][u] - ll)
            if t + 1 < T:
                pb[t, u] = torch.exp(alpha[t][u] + lp_blank[t, u] + beta[t + 1][u] - ll)
            elif u == U:
                pb[t, u] = torch.exp(alpha[t][u] + lp_blank[t, u] - ll)
            if u < U:
                pl[t, u] = torch.exp(alpha[t][u] + lp_label[t, u] + beta[t][u + 1] - ll)
    return nll, occ, pb, pl


def node_logprobs(logits, labels, blank=0):
    """logits [T, U+1, V], labels [U] -> (lp_blank, lp_label [T, U+1]) (lp_label's last column is 0)"""
    lp = logits.log_softmax(-1)
    T, U1, _ = logits.shape
    lpb = lp[:, :, blank]
    if U1 > 1:
        idx = torch.as_tensor(labels, dtype=torch.int64)[: U1 - 1].view(1, U1 - 1, 1).expand(T, U1 - 1, 1)
        lpl = torch.cat([lp[:, : U1 - 1].gather(2, idx)[..., 0], lp.new_zeros(T, 1)], dim=1)
    else:
        lpl = lp.new_zeros(T, 1)
    return lpb, lpl


def rnnt_nll(logits, labels, blank=0):
    """one utterance: logits [T, U+1, V], labels [U] -> nll (differentiable)"""
    lpb, lpl = node_logprobs(logits, labels, blank)
    return lattice(lpb, lpl, logits.shape[0], logits.shape[1] - 1)[0]


def brute_force_nll(logits, labels, blank=0):
    """-log of the sum over ALL alignments: every order of T blanks and U labels that ends with a blank at (T-1, U)"""
    lp = logits.log_softmax(-1)
    T, U = logits.shape[0], logits.shape[1] - 1
    total = []
    for labs in itertools.combinations(range(T + U - 1), U):      # positions of the labels among the first T + U - 1 moves
        t = u = 0
        s = lp.new_tensor(0.0)
        for m in range(T + U - 1):
            if m in labs:
                s = s + lp[t, u, labels[u]]
                u += 1
            else:
                s = s + lp[t, u, blank]
                t += 1
        assert t == T - 1 and u == U
        total.append(s + lp[t, u, blank])
    return -torch.logsumexp(torch.stack(total), 0)


# ---------------------------------------------------------------------------------------------- joint + loss
def joint_logits(enc, dec, P):
    """enc [..., De], dec [..., Dd], P = (lin_enc.weight, lin_enc.bias, lin_dec.weight, lin_out.weight, lin_out.bias)"""
    w_enc, b_enc, w_dec, w_out, b_out = P
    z = torch.tanh(torch.nn.functional.linear(enc, w_enc, b_enc) + torch.nn.functional.linear(dec, w_dec))
    return torch.nn.functional.linear(z, w_out, b_out)


def joint_loss(enc, dec, t_len, u_len, target, P, blank=0):
    """enc [B, T, De], dec [B, U1, Dd] -> sum_b nll[b] / B; only the live rows of enc / dec are read"""
    B = enc.shape[0]
    total = 0.0
    for b in range(B):
        T, U = int(t_len[b]), int(u_len[b])
        logits = joint_logits(enc[b, :T, None, :], dec[b, None, : U + 1, :], P)
        total = total + rnnt_nll(logits, [int(v) for v in target[b][:U]], blank)
    return total / B


# ---------------------------------------------------------------------------------------------- decoder
def lstm_stack(embed_w, layers, labels, pad=0):
    """embed_w [V, H], layers = [(w_ih, w_hh, b_ih, b_hh)], labels [B, U1] -> dec_out [B, U1, H] (zero initial states, no dropout);
    ``pad``: the embedding's padding row (torch.nn.Embedding(padding_idx=...): read as it is, no gradient)"""
    x = torch.nn.functional.embedding(labels, embed_w, padding_idx=pad)
    for w_ih, w_hh, b_ih, b_hh in layers:
        B, L, _ = x.shape
        H = w_hh.shape[1]
        h, c = x.new_zeros(B, H), x.new_zeros(B, H)
        ys = []
        for t in range(L):
            g = x[:, t] @ w_ih.T + b_ih + h @ w_hh.T + b_hh
            i, f, gg, o = g.chunk(4, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
            h = torch.sigmoid(o) * torch.tanh(c)
            ys.append(h)
        x = torch.stack(ys, dim=1)
    return x


def decoder_params(dec, dtype=torch.float64):
    """(embed.weight, [(w_ih, w_hh, b_ih, b_hh)]) of a TransducerDecoder-shaped module as leaf tensors of ``dtype`` on the CPU"""
    sd = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in dec.state_dict().items()}
    n = len([k for k in sd if k.endswith("weight_ih_l0")])
    return sd, sd["embed.weight"], [tuple(sd[f"decoder.{l}.{s}_l0"] for s in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for l in range(n)]


def joint_params(jn, dtype=torch.float64):
    sd = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in jn.state_dict().items()}
    return sd, (sd["lin_enc.weight"], sd["lin_enc.bias"], sd["lin_dec.weight"], sd["lin_out.weight"], sd["lin_out.bias"])


# ---------------------------------------------------------------------------------------------- greedy search
@torch.no_grad()
def greedy_search(enc_out, embed_w, layers, P, blank=0):
    """espnet greedy_search for one utterance enc_out [T, De] -> (tokens, score, smallest top-2 gap over the decisions)"""
    n = len(layers)
    H = layers[0][1].shape[1]
    h = [enc_out.new_zeros(1, H) for _ in range(n)]
    c = [enc_out.new_zeros(1, H) for _ in range(n)]

    def step(tok, h, c):
        x = embed_w[torch.tensor([tok])]
        h2, c2 = [], []
        for li, (w_ih, w_hh, b_ih, b_hh) in enumerate(layers):
            g = x @ w_ih.T + b_ih + h[li] @ w_hh.T + b_hh
            i, f, gg, o = g.chunk(4, dim=1)
            cc = torch.sigmoid(f) * c[li] + torch.sigmoid(i) * torch.tanh(gg)
            x = torch.sigmoid(o) * torch.tanh(cc)
            h2.append(x)
            c2.append(cc)
        return x[0], h2, c2

    dec_out, h, c = step(blank, h, c)
    toks, score, gap = [], 0.0, math.inf
    for t in range(enc_out.shape[0]):
        logp = joint_logits(enc_out[t], dec_out, P).log_softmax(-1)
        top2 = logp.topk(2).values
        gap = min(gap, float(top2[0] - top2[1]))
        pred = int(logp.argmax())
        if pred != blank:
            toks.append(pred)
            score += float(logp[pred])
            dec_out, h, c = step(pred, h, c)
    return toks, score, gap
