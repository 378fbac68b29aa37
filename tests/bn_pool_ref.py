"""BatchNorm and the pools of the lip front-end in plain torch, written out by their formulas on channels-last data ([M, C] rows,
[N, H, W, C] maps, [N, P, C] frames): the reference of tests/test_bn_pool_host.py (which checks these functions against
torch.nn.BatchNorm1d / max_pool2d / avg_pool2d under autograd in float64) and of tests/test_gpu_bn_pool_edges.py (which checks
csrc/vision.hip against them).  The dtype and the device follow the inputs: called on ``.double()`` tensors it is the float64
reference.  Nothing here calls a batch-norm or pooling routine of torch.

Max-pool 3x3 / stride 2 / pad 1: the winning tap is k = kh*3 + kw in 0..8 of the window rows 2ho-1..2ho+1, columns 2wo-1..2wo+1;
the FIRST maximum in that (row-major) order wins, a NaN replaces whatever came before it (torch's scan: ``v > best or isnan(v)``).
The centre tap always lies inside the map, so every window has a valid tap."""
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------ activation
def act_fwd(z, act):
    if act == "swish":
        return z * torch.sigmoid(z)
    assert act is None, act
    return z


def act_grad(z, act):
    """d act(z) / dz"""
    if act == "swish":
        s = torch.sigmoid(z)
        return s * (1 + z * (1 - s))
    assert act is None, act
    return torch.ones_like(z)


# ------------------------------------------------------------------------------------------------ BatchNorm
def bn_stats(x, eps):
    """x [M, C] -> mean, biased variance, rstd = 1 / sqrt(var + eps)   (M = 1: mean = x, var = 0)"""
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def bn_running(mean, var, M, momentum, running_mean, running_var, nbt):
    """the buffers after one training step: the running variance takes the UNBIASED batch variance (M = 1: the biased one, 0)"""
    unb = var * (M / (M - 1)) if M > 1 else var
    return (1 - momentum) * running_mean + momentum * mean, (1 - momentum) * running_var + momentum * unb, nbt + 1


def bn_apply(x, mean, rstd, gamma, beta, res=None, act=None):
    """y = act((x - mean) * rstd * gamma + beta (+ res))"""
    z = (x - mean) * rstd * gamma + beta
    if res is not None:
        z = z + res
    return act_fwd(z, act)


def bn_train_fwd(x, gamma, beta, eps, momentum, running_mean, running_var, nbt, res=None, act=None):
    """-> y, (mean, var, rstd), (running_mean, running_var, num_batches_tracked) after the step; the inputs stay unchanged"""
    mean, var, rstd = bn_stats(x, eps)
    return (bn_apply(x, mean, rstd, gamma, beta, res, act), (mean, var, rstd),
            bn_running(mean, var, x.shape[0], momentum, running_mean, running_var, nbt))


def bn_eval_fwd(x, running_mean, running_var, gamma, beta, eps, res=None, act=None):
    return bn_apply(x, running_mean, 1.0 / torch.sqrt(running_var + eps), gamma, beta, res, act)


def bn_bwd(dy, x, mean, rstd, gamma, beta, res=None, act=None):
    """closed form of the training-mode backward: dz (gradient of the pre-activation, = the gradient of ``res``), dx, dgamma, dbeta
        dz = dy act'(z),  dbeta = sum dz,  dgamma = sum dz xhat,  dx = gamma rstd (dz - dbeta / M - xhat dgamma / M)"""
    M = x.shape[0]
    xhat = (x - mean) * rstd
    z = xhat * gamma + beta
    if res is not None:
        z = z + res
    dz = dy * act_grad(z, act)
    dbeta, dgamma = dz.sum(0), (dz * xhat).sum(0)
    dx = gamma * rstd * (dz - dbeta / M - xhat * dgamma / M)
    return dz, dx, dgamma, dbeta


# ------------------------------------------------------------------------------------------------ max-pool 3x3 / s2 / p1
def pool_out(n):
    return (n - 1) // 2 + 1


def maxpool3x3s2_fwd(x):
    """x [N, H, W, C] -> values [N, Ho, Wo, C], tap [N, Ho, Wo, C] (int64, 0..8)"""
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H), pool_out(W)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1), value=float("-inf"))                     # [N, H+2, W+2, C]: padded row 2ho + kh is row 2ho-1+kh
    best = torch.full((N, Ho, Wo, C), float("-inf"), dtype=x.dtype, device=x.device)
    tap = torch.zeros((N, Ho, Wo, C), dtype=torch.int64, device=x.device)
    for k in range(9):
        kh, kw = divmod(k, 3)
        v = xp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, :]
        take = (v > best) | torch.isnan(v)
        best = torch.where(take, v, best)
        tap = torch.where(take, torch.full_like(tap, k), tap)
    return best, tap


def maxpool3x3s2_bwd(dy, tap, H, W):
    """dx [N, H, W, C]: every pooled gradient goes to the pixel its window's tap names"""
    N, Ho, Wo, C = dy.shape
    dxp = torch.zeros((N, H + 2, W + 2, C), dtype=dy.dtype, device=dy.device)
    for k in range(9):
        kh, kw = divmod(k, 3)
        dxp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, :] += torch.where(tap == k, dy, torch.zeros_like(dy))
    return dxp[:, 1:H + 1, 1:W + 1, :].contiguous()


def tap_from_flat_index(index, H, W):
    """torch's max_pool2d index (h * W + w of the input map, any leading dims, last two [Ho, Wo]) -> tap 0..8"""
    Ho, Wo = index.shape[-2:]
    ho = torch.arange(Ho, device=index.device).view(Ho, 1)
    wo = torch.arange(Wo, device=index.device).view(1, Wo)
    return (index // W - (2 * ho - 1)) * 3 + (index % W - (2 * wo - 1))


# ------------------------------------------------------------------------------------------------ the stem's tail
def bn_act_maxpool_fwd(x, mean, rstd, gamma, beta, act):
    """maxpool(act(BN(x))), x [N, H, W, C] -> pooled values, tap, and the activation map itself"""
    a = bn_apply(x, mean, rstd, gamma, beta, None, act)
    y, tap = maxpool3x3s2_fwd(a)
    return y, tap, a


def bn_act_maxpool_bwd(dpool, tap, x, mean, rstd, gamma, beta, act):
    """gradient of the pooled output routed to ``tap``, then through the activation and the BatchNorm: -> dx [N,H,W,C], dgamma, dbeta"""
    N, H, W, C = x.shape
    da = maxpool3x3s2_bwd(dpool, tap, H, W)
    _, dx, dgamma, dbeta = bn_bwd(da.reshape(-1, C), x.reshape(-1, C), mean, rstd, gamma, beta, None, act)
    return dx.view(N, H, W, C), dgamma, dbeta


# ------------------------------------------------------------------------------------------------ average pool
def avgpool_fwd(x):
    """x [N, P, C] -> [N, C]"""
    return x.sum(1) / x.shape[1]


def avgpool_bwd(dy, P):
    """dy [N, C] -> dx [N, P, C]"""
    return (dy / P)[:, None, :].expand(dy.shape[0], P, dy.shape[1]).contiguous()
