"""CPU: tests/cgmlp_gate_ref.py (the shift-and-add reference of the cgMLP gate kernels) in float64 against torch's grouped
convolution and against espnet's ConvolutionalSpatialGatingUnit as oracle/ restates it - values and all four gradients."""
import pytest
import torch
import torch.nn.functional as F

import cgmlp_gate_ref as R

# (B, T, C, K): K = 1 (no halo), the window wider than the utterance (T <= pad: 2 < 3, 5 < 15, 1 < 31), T = pad + 1, an odd C
CASES = [(3, 17, 10, 1), (2, 2, 6, 7), (3, 5, 7, 31), (1, 1, 4, 63), (2, 16, 5, 31), (3, 40, 6, 3), (2, 70, 3, 45)]


def _inputs(B, T, C, K):
    g = torch.Generator().manual_seed(100 * T + K)
    r, gn, du = (torch.randn(B, T, C, generator=g, dtype=torch.float64) for _ in range(3))
    w = torch.randn(C, K, generator=g, dtype=torch.float64) / K ** 0.5
    return r, gn, w, torch.randn(C, generator=g, dtype=torch.float64), du


def _same(got, want):
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()) + 1e-13


@pytest.mark.parametrize("B,T,C,K", CASES)
def test_reference_agrees_with_grouped_conv1d_in_float64(B, T, C, K):
    r, gn, w, bias, du = _inputs(B, T, C, K)
    got = R.gate_with_grads(r, gn, w, bias, du, torch.float64)
    rr, gg, ww, bb = (t.clone().requires_grad_() for t in (r, gn, w, bias))
    conv = F.conv1d(gg.transpose(1, 2), ww.view(C, 1, K), bb, padding=(K - 1) // 2, groups=C).transpose(1, 2)
    out = rr * conv
    want = (out.detach(), conv.detach(), *torch.autograd.grad(out, (rr, gg, ww, bb), du))
    for a, b in zip(got, want):
        _same(a, b)


@pytest.mark.parametrize("B,T,C,K", CASES)
def test_reference_agrees_with_the_spatial_gating_unit_in_float64(B, T, C, K):
    """ConvolutionalSpatialGatingUnit(x) = x_r * conv(LayerNorm(x_g)) with no dropout, identity gate activation: the reference
    behind the same LayerNorm gives its output, its input gradient and the convolution's parameter gradients"""
    from oracle import leaves as L
    from oracle.model import fill_parameters_
    r, g_, _, _, du = _inputs(B, T, C, K)
    m = L.ConvolutionalSpatialGatingUnit(2 * C, K, 0.0, False, "identity")
    fill_parameters_(m, seed=K)
    m = m.double().eval()
    x = torch.cat([r, g_], -1).requires_grad_()
    y = m(x)
    gx, gw, gb = torch.autograd.grad(y, (x, m.conv.weight, m.conv.bias), du)
    rr, gg = r.clone().requires_grad_(), g_.clone().requires_grad_()
    ww, bb = m.conv.weight.detach().view(C, K).clone().requires_grad_(), m.conv.bias.detach().clone().requires_grad_()
    out, _ = R.gate(rr, m.norm(gg), ww, bb)
    dr, dg, dw, db = torch.autograd.grad(out, (rr, gg, ww, bb), du)
    _same(out.detach(), y.detach())
    _same(torch.cat([dr, dg], -1), gx)
    _same(dw, gw.view(C, K))
    _same(db, gb)
