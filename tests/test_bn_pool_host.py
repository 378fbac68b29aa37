"""Host (no GPU): the restated BatchNorm / pooling formulas of tests/bn_pool_ref.py against torch's own routines in float64 under
autograd - the reference of tests/test_gpu_bn_pool_edges.py has to be right before a kernel is measured against it.  Tied maxima
(integer inputs in {-1, 0, 1}) included: torch's CPU max-pool keeps the first maximum in scan order, as the reference does."""
import pytest
import torch
import torch.nn.functional as F

import bn_pool_ref as R

TOL = 1e-12       # float64 against float64, other summation order


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, tol=TOL):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("M,C", [(2, 8), (9, 4), (513, 12)])
@pytest.mark.parametrize("act,with_res", [("swish", True), ("swish", False), (None, False)])
def test_batchnorm_training_matches_torch(M, C, act, with_res):
    g = _gen(M + C)
    x = (torch.randn(M, C, generator=g, dtype=torch.float64) * 2 + 0.7).requires_grad_(True)
    res = torch.randn(M, C, generator=g, dtype=torch.float64).requires_grad_(True) if with_res else None
    bn = torch.nn.BatchNorm1d(C, eps=1e-5, momentum=0.1).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g, dtype=torch.float64) * 0.3)
        bn.running_mean.copy_(torch.randn(C, generator=g, dtype=torch.float64))
        bn.running_var.copy_(torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
    rm0, rv0, nbt0 = bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()
    z = bn(x) + (res if with_res else 0)
    want = R.act_fwd(z, act)
    r = torch.randn(M, C, generator=g, dtype=torch.float64)
    (want * r).sum().backward()
    gamma, beta = bn.weight.detach(), bn.bias.detach()
    y, (mean, var, rstd), (rm, rv, nbt) = R.bn_train_fwd(x.detach(), gamma, beta, 1e-5, 0.1, rm0, rv0, nbt0,
                                                           None if res is None else res.detach(), act)
    assert _close(y, want)
    assert _close(mean, x.detach().mean(0)) and _close(var, x.detach().var(0, unbiased=False))
    assert _close(rstd, (x.detach().var(0, unbiased=False) + 1e-5).rsqrt())
    assert _close(rm, bn.running_mean) and _close(rv, bn.running_var) and int(nbt) == int(bn.num_batches_tracked) == int(nbt0) + 1
    dz, dx, dg, db = R.bn_bwd(r, x.detach(), mean, rstd, gamma, beta, None if res is None else res.detach(), act)
    assert _close(dx, x.grad, 1e-10) and _close(dg, bn.weight.grad, 1e-10) and _close(db, bn.bias.grad, 1e-10)
    if with_res:
        assert _close(dz, res.grad, 1e-10)


def test_batchnorm_of_one_row_is_the_formula():
    """torch refuses M = 1 in training mode, so this is the formula only: mean = x, var = 0, running_var blended with 0"""
    x = torch.tensor([[1.5, -2.0, 0.0, 7.0]], dtype=torch.float64)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        torch.nn.BatchNorm1d(4).double().train()(x)
    gamma, beta = torch.tensor([1.0, 2.0, 0.5, 1.5], dtype=torch.float64), torch.tensor([0.1, -0.2, 0.3, 0.0], dtype=torch.float64)
    rm0, rv0 = torch.full((4,), 0.25, dtype=torch.float64), torch.full((4,), 2.0, dtype=torch.float64)
    y, (mean, var, rstd), (rm, rv, nbt) = R.bn_train_fwd(x, gamma, beta, 1e-5, 0.1, rm0, rv0, torch.tensor(3))
    assert torch.equal(mean, x[0]) and torch.equal(var, torch.zeros(4, dtype=torch.float64))
    assert _close(rstd, torch.full((4,), 1e-5 ** -0.5, dtype=torch.float64))
    assert torch.equal(y, beta[None, :])
    assert _close(rm, 0.9 * rm0 + 0.1 * x[0]) and _close(rv, 0.9 * rv0) and int(nbt) == 4


@pytest.mark.parametrize("C", [4, 64])
def test_batchnorm_eval_matches_torch(C):
    g = _gen(C)
    bn = torch.nn.BatchNorm1d(C, eps=1e-5, momentum=0.1).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g, dtype=torch.float64) * 0.3)
    rm, rv, nbt = bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()
    for M in (37, 101):
        xb = torch.randn(M, C, generator=g, dtype=torch.float64) * 3 - 1
        bn(xb)
        _, _, (rm, rv, nbt) = R.bn_train_fwd(xb, bn.weight.detach(), bn.bias.detach(), 1e-5, 0.1, rm, rv, nbt)
    assert _close(rm, bn.running_mean) and _close(rv, bn.running_var) and int(nbt) == 2
    x = torch.randn(29, C, generator=g, dtype=torch.float64)
    assert _close(R.bn_eval_fwd(x, rm, rv, bn.weight.detach(), bn.bias.detach(), 1e-5), bn.eval()(x))


def _pool_input(kind, shape, g):
    if kind == "randn":
        return torch.randn(shape, generator=g, dtype=torch.float64)
    if kind == "ties":
        return torch.randint(-1, 2, shape, generator=g).double()
    assert kind == "relu"
    return torch.randn(shape, generator=g, dtype=torch.float64).clamp(min=0)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (2, 2), (2, 3), (3, 3), (5, 4), (7, 9), (12, 12)])
@pytest.mark.parametrize("kind", ["randn", "ties", "relu"])
def test_maxpool_matches_torch_ties_included(H, W, kind):
    N, C = 3, 4
    g = _gen(100 * H + W)
    x = _pool_input(kind, (N, H, W, C), g)
    xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    want, index = F.max_pool2d(xt, 3, 2, 1, return_indices=True)
    y, tap = R.maxpool3x3s2_fwd(x)
    assert y.shape == (N, R.pool_out(H), R.pool_out(W), C)
    assert torch.equal(y.permute(0, 3, 1, 2), want.detach())
    assert torch.equal(tap.permute(0, 3, 1, 2), R.tap_from_flat_index(index, H, W))
    assert int(tap.min()) >= 0 and int(tap.max()) <= 8
    if kind == "ties" and H * W >= 9:
        assert float((y == 1).double().mean()) > 0.5          # most windows do hold more than one maximum
    r = torch.randint(-3, 4, want.shape, generator=g).double()           # integer gradients: sums are exact in any order
    (want * r).sum().backward()
    dx = R.maxpool3x3s2_bwd(r.permute(0, 2, 3, 1).contiguous(), tap, H, W)
    assert torch.equal(dx.permute(0, 3, 1, 2), xt.grad)


def test_maxpool_nan_wins_its_window():
    x = torch.randn(1, 5, 5, 4, generator=_gen(7), dtype=torch.float64)
    x[0, 2, 3, 1] = float("nan")                  # window (1, 1): rows 1..3, columns 1..3 -> tap (2-1)*3 + (3-1) = 5; window (1, 2): tap 3
    y, tap = R.maxpool3x3s2_fwd(x)
    want, index = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    assert torch.isnan(y[0, 1, 1, 1]) and int(tap[0, 1, 1, 1]) == 5 and torch.isnan(y[0, 1, 2, 1]) and int(tap[0, 1, 2, 1]) == 3
    assert int(torch.isnan(y).sum()) == 2
    assert torch.equal(torch.isnan(y.permute(0, 3, 1, 2)), torch.isnan(want))
    assert torch.equal(tap.permute(0, 3, 1, 2), R.tap_from_flat_index(index, 5, 5))


@pytest.mark.parametrize("N,H,W,C", [(1, 1, 1, 4), (2, 2, 3, 8), (2, 9, 7, 4)])
def test_stem_tail_matches_autograd(N, H, W, C):
    """maxpool(swish(BN(x))) and its backward to dx, dgamma, dbeta against BatchNorm1d + max_pool2d under autograd"""
    g = _gen(N * H * W)
    x = (torch.randn(N, H, W, C, generator=g, dtype=torch.float64) * 1.5 + 0.3).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = (torch.randn(C, generator=g, dtype=torch.float64) * 0.2).requires_grad_(True)
    z = F.batch_norm(x.view(-1, C), None, None, gamma, beta, True, 0.1, 1e-5) if N * H * W > 1 else None
    mean, var, rstd = R.bn_stats(x.detach().view(-1, C), 1e-5)
    if z is None:                                  # one row: the formula (torch refuses it), still differentiated by autograd
        z = (x.view(-1, C) - x.view(-1, C).mean(0)) * rstd * gamma + beta
    a = (z * torch.sigmoid(z)).view(N, H, W, C).permute(0, 3, 1, 2)
    want = F.max_pool2d(a, 3, 2, 1).permute(0, 2, 3, 1)
    dp = torch.randn(want.shape, generator=g, dtype=torch.float64)
    (want * dp).sum().backward()
    y, tap, act_map = R.bn_act_maxpool_fwd(x.detach(), mean, rstd, gamma.detach(), beta.detach(), "swish")
    assert _close(y, want) and _close(act_map, a.permute(0, 2, 3, 1))
    dx, dg, db = R.bn_act_maxpool_bwd(dp, tap, x.detach(), mean, rstd, gamma.detach(), beta.detach(), "swish")
    assert _close(dx, x.grad, 1e-10) and _close(dg, gamma.grad, 1e-10) and _close(db, beta.grad, 1e-10)


@pytest.mark.parametrize("N,P,C", [(1, 1, 4), (3, 9, 16), (2, 36, 6)])
def test_avgpool_matches_torch(N, P, C):
    g = _gen(P)
    s = int(P ** 0.5)
    x = torch.randn(N, P, C, generator=g, dtype=torch.float64).requires_grad_(True)
    want = F.avg_pool2d(x.view(N, s, s, C).permute(0, 3, 1, 2), s).view(N, C)
    dy = torch.randn(N, C, generator=g, dtype=torch.float64)
    (want * dy).sum().backward()
    assert _close(R.avgpool_fwd(x.detach()), want) and _close(R.avgpool_bwd(dy, P), x.grad)
