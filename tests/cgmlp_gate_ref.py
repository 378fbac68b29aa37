"""The cgMLP gate of csrc/cgmlp.hip in plain torch on the CPU: the reference of tests/test_cgmlp_gate_host.py and
tests/test_gpu_cgmlp_gate.py.  The dtype follows the inputs: in float64 it is the reference, in fp32 it sets the error scale.

    conv[b,t,c] = bias[c] + sum_k w[c,k] * gn[b,t+k-pad,c]      pad = (K-1)//2, gn = 0 outside [0, T) of each utterance
    out         = r * conv

The convolution is an explicit shift-and-add over the K taps (no torch convolution: the host test compares it with one), the
gradients are autograd's."""
import torch


def dwconv(gn, w, bias):
    """gn [B, T, C], w [C, K] (K odd), bias [C] -> conv [B, T, C]"""
    B, T, C = gn.shape
    K = w.shape[1]
    assert K % 2 == 1 and w.shape[0] == C
    pad = (K - 1) // 2
    conv = bias.expand(B, T, C).clone()
    for k in range(K):
        s = k - pad                                   # conv[:, t] += w[:, k] * gn[:, t + s] for the t with 0 <= t + s < T
        lo, hi = max(0, -s), min(T, T - s)
        if lo < hi:
            shifted = torch.zeros_like(conv)
            shifted[:, lo:hi] = w[:, k] * gn[:, lo + s:hi + s]
            conv = conv + shifted
    return conv


def gate(r, gn, w, bias):
    """-> (out, conv)"""
    conv = dwconv(gn, w, bias)
    return r * conv, conv


def gate_with_grads(r, gn, w, bias, du, dtype):
    """(out, conv, dr, dgn, dw, dbias) of loss = <out, du>, everything evaluated in ``dtype``"""
    rr, gg, ww, bb = (t.to(dtype).clone().requires_grad_() for t in (r, gn, w, bias))
    out, conv = gate(rr, gg, ww, bb)
    grads = torch.autograd.grad(out, (rr, gg, ww, bb), du.to(dtype))
    return (out.detach(), conv.detach(), *grads)
