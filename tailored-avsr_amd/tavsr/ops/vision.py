"""Lip front-end: Conv2dSubsampling's convolutions, im2col / col2im, the Conv3d stem, BatchNorm, pools and the 3x3 trunk
convolutions with their tap-skipping flags.
"""
from __future__ import annotations

import torch

from .. import ops
from .._lib import ACT, check, lib, ptr, require_cuda, stream
from .base import empty
from .matmul import gemm

__all__ = ["conv1_fwd", "conv1_bwd", "im2col3x3s2", "col2im3x3s2_relu", "conv_out", "im2col2d", "col2im2d", "stem_implicit_ok",
           "stem_pad16_ok", "stem_pad", "stem_weight_288", "stem_weight_grad_from_288", "stem_conv_fwd_pad16", "stem_conv_dw_pad16",
           "stem_conv_fwd", "stem_conv_dw", "im2col_stem", "bn_stats", "rsqrt_eps", "bn_apply_fwd", "bn_bwd", "bn_bwd_pooled",
           "maxpool3x3s2_fwd", "bn_act_maxpool3x3s2_fwd", "maxpool3x3s2_bwd", "avgpool_fwd", "avgpool_bwd", "conv_wflip", "conv_wsplit", "x6_takes", "x6_dw_takes", "_tapskip",
           "_tapskip2", "_tapskip_any", "conv3x3_fwd", "conv3x3_dx", "conv3x3_dw"]


# ---------------------------------------------------------------------------------------------- subsampling
def conv1_fwd(x, w, bias):
    B, T, F = x.shape
    Cn = w.shape[0]
    To, Fo = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    y = empty(B, To, Fo, Cn, like=x)
    require_cuda(x, w, bias)
    check(lib().tavsr_conv1_fwd(ptr(x), ptr(w), ptr(bias), ptr(y), B, T, F, Cn, stream()), "tavsr_conv1_fwd")
    return y


def conv1_bwd(dz, x, Cn):
    B, T, F = x.shape
    dw, db = empty(Cn, 9, like=x), empty(Cn, like=x)
    ws = empty(lib().tavsr_conv1_bwd_ws(B, T, F, Cn), like=x)
    check(lib().tavsr_conv1_bwd(ptr(dz), ptr(x), ptr(dw), ptr(db), 0, ptr(ws), B, T, F, Cn, stream()), "tavsr_conv1_bwd")
    return dw, db


def im2col3x3s2(y):
    B, Ti, Fi, Cn = y.shape
    To, Fo = (Ti - 3) // 2 + 1, (Fi - 3) // 2 + 1
    col = empty(B * To * Fo, 9 * Cn, like=y)
    check(lib().tavsr_im2col3x3s2(ptr(y), ptr(col), B, Ti, Fi, Cn, stream()), "tavsr_im2col3x3s2")
    return col, To, Fo


def col2im3x3s2_relu(dcol, yrelu):
    B, Ti, Fi, Cn = yrelu.shape
    dz = torch.empty_like(yrelu)
    check(lib().tavsr_col2im3x3s2_relu(ptr(dcol), ptr(yrelu), ptr(dz), B, Ti, Fi, Cn, stream()), "tavsr_col2im3x3s2_relu")
    return dz


# ---------------------------------------------------------------------------------------------- visual frontend
def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def im2col2d(x, N, H, W, Cn, KH, KW, stride, pad):
    """x [N*H*W, C] channels-last -> col [N*Ho*Wo, KH*KW*C]."""
    require_cuda(x)
    Ho, Wo = conv_out(H, KH, stride, pad), conv_out(W, KW, stride, pad)
    col = empty(N * Ho * Wo, KH * KW * Cn, like=x)
    check(lib().tavsr_im2col2d(ptr(x), ptr(col), N, H, W, Cn, KH, KW, stride, pad, stream()), "tavsr_im2col2d")
    return col, Ho, Wo


def col2im2d(dcol, N, H, W, Cn, KH, KW, stride, pad, extra=None):
    """``extra`` [N*Ho*Wo, C]: data-gradient rows of a parallel 1x1 convolution with the same stride (downsample path),
    added at the pixels it touches."""
    require_cuda(dcol, extra)
    assert extra is None or (extra.is_contiguous() and extra.shape == (dcol.shape[0], Cn))
    dx = empty(N * H * W, Cn, like=dcol)
    check(lib().tavsr_col2im2d(ptr(dcol), ptr(dx), N, H, W, Cn, KH, KW, stride, pad, ptr(extra), stream()), "tavsr_col2im2d")
    return dx


def stem_implicit_ok(x) -> bool:
    B, T, H, W = x.shape
    Ho, Wo = conv_out(H, 7, 2, 3), conv_out(W, 7, 2, 3)
    return (ops.STEM_IMPLICIT and H % 2 == 0 and W % 2 == 0 and W >= 8 and (B * T * Ho * Wo) % 32 == 0 and T < 1024 and H < 1000 and W < 1000
            and B * T * H * W < 2 ** 31 and x.data_ptr() % 16 == 0)


def stem_pad16_ok(x) -> bool:
    B, T, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    return (ops.STEM_IMPLICIT and ops.STEM_PAD16 and H % 2 == 0 and W % 4 == 0 and (B * T * Ho * Wo) % 32 == 0
            and B * (T + 5) * (H + 6) * (W + 8) < 2 ** 31)


def stem_pad(x):
    """x [B,T,H,W] -> zero-padded clips [B, T+5, H+6, W+8] (2/3 frames, 3/3 rows, 3/5 columns): every tap of the (5,7,7)
    stride (1,2,2) stem is inside the buffer, also the zero-weight tap columns."""
    return torch.nn.functional.pad(x, (3, 5, 3, 3, 2, 3)).contiguous()


def stem_weight_288(w):
    """Conv3d weight [Cout,1,5,7,7] -> [Cout, 288]: column ((kt*7 + kh)*8 + kw), zeros at kw = 7 and in the last 8 columns."""
    co = w.shape[0]
    return torch.nn.functional.pad(torch.nn.functional.pad(w.reshape(co, 35, 7), (0, 1)).reshape(co, 280), (0, 8)).contiguous()


def stem_weight_grad_from_288(g, shape):
    co = g.shape[0]
    return g[:, :280].reshape(co, 35, 8)[:, :, :7].reshape(shape).contiguous()


def stem_conv_fwd_pad16(xp, w288, B, T, H, W):
    """padded clips xp (stem_pad), w288 [Cout, 288] -> z [B*T*Ho*Wo, Cout]."""
    Ho, Wo = H // 2, W // 2
    M = B * T * Ho * Wo
    z = empty(M, w288.shape[0], like=xp)
    gemm(M, w288.shape[0], 288, xp, 4, w288, 288, z, w288.shape[0], conv=(6, H + 6, W + 8, T + 5))
    return z, Ho, Wo


def stem_conv_dw_pad16(dz, xp, T, H, W):
    """dW [Cout, 288] = dz^T patches(xp) in the 35 x 8 tap layout (the zero-weight columns receive values nobody reads)."""
    M, cout = dz.shape
    dw = empty(cout, 288, like=dz)
    gemm(cout, 288, M, dz, cout, xp, 4, dw, 288, a_kmajor=True, b_kmajor=True, conv=(7, H + 6, W + 8, T + 5))
    return dw


def stem_conv_fwd(x, w0p):
    """x [B,T,H,W] clips, w0p [64, 256] (245 taps of the (5,7,7) kernel + zero columns) -> z [B*T*Ho*Wo, 64]."""
    B, T, H, W = x.shape
    Ho, Wo = conv_out(H, 7, 2, 3), conv_out(W, 7, 2, 3)
    M = B * T * Ho * Wo
    z = empty(M, w0p.shape[0], like=x)
    gemm(M, w0p.shape[0], 256, x, 4, w0p, 256, z, w0p.shape[0], conv=(4, H, W, T))
    return z, Ho, Wo


def stem_conv_dw(dz, x):
    """dW0 [64, 256] = dz^T patches(x) (columns >= 245 are zero); dz [B*T*Ho*Wo, 64]."""
    B, T, H, W = x.shape
    M, cout = dz.shape
    dw = empty(cout, 256, like=dz)
    gemm(cout, 256, M, dz, cout, x, 4, dw, 256, a_kmajor=True, b_kmajor=True, conv=(5, H, W, T))
    return dw


def im2col_stem(x):
    """x [B,T,H,W] -> col [B*T*Ho*Wo, 256] (245 taps of the (5,7,7) kernel + zero padding)."""
    B, T, H, W = x.shape
    require_cuda(x)
    Ho, Wo = conv_out(H, 7, 2, 3), conv_out(W, 7, 2, 3)
    col = empty(B * T * Ho * Wo, 256, like=x)
    check(lib().tavsr_im2col_stem(ptr(x), ptr(col), B, T, H, W, stream()), "tavsr_im2col_stem")
    return col, Ho, Wo


def bn_stats(x, eps, momentum, running_mean=None, running_var=None, nbt=None):
    M, Cn = x.shape
    require_cuda(x, running_mean, running_var, nbt)
    mean, var, rstd = empty(Cn, like=x), empty(Cn, like=x), empty(Cn, like=x)
    ws = empty(lib().tavsr_bn_ws(M, Cn), like=x)
    check(lib().tavsr_bn_stats(ptr(x), M, Cn, eps, momentum, ptr(mean), ptr(var), ptr(rstd), ptr(running_mean), ptr(running_var), ptr(nbt),
                               ptr(ws), stream()), "tavsr_bn_stats")
    return mean, rstd


def rsqrt_eps(v, eps):
    out = torch.empty_like(v)
    check(lib().tavsr_rsqrt_eps(ptr(v), eps, ptr(out), v.numel(), stream()), "tavsr_rsqrt_eps")
    return out


def bn_apply_fwd(x, mean, rstd, gamma, beta, res=None, act=None):
    M, Cn = x.shape
    require_cuda(x, mean, rstd, gamma, beta, res)
    y = torch.empty_like(x)
    check(lib().tavsr_bn_apply_fwd(ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(res), ptr(y), M, Cn, ACT[act], stream()),
          "tavsr_bn_apply_fwd")
    return y


def bn_bwd(dy, x, mean, rstd, gamma, beta, res=None, act=None, need_dz=True):
    """returns dz (gradient w.r.t. the pre-activation, = gradient of ``res``), dx, dgamma, dbeta.  ``need_dz=False`` (only
    without ``res``): dz is not materialised (returned as None), which saves one [M, C] write."""
    M, Cn = x.shape
    require_cuda(dy, x, mean, rstd, gamma, beta, res)
    assert need_dz or res is None
    dz, dx = (torch.empty_like(x) if need_dz else None), torch.empty_like(x)
    dg, db = empty(Cn, like=x), empty(Cn, like=x)
    ws = empty(lib().tavsr_bn_ws(M, Cn), like=x)
    check(lib().tavsr_bn_bwd(ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(res), ptr(dz), ptr(dx), ptr(dg), ptr(db), M,
                             Cn, ACT[act], ptr(ws), stream()), "tavsr_bn_bwd")
    return dz, dx, dg, db


def bn_bwd_pooled(dpool, idx, x, mean, rstd, gamma, beta, N, H, W, act=None):
    """bn_bwd (no residual) whose incoming gradient is the pooled one of maxpool3x3s2_fwd(act(bn(x))): -> dx, dgamma, dbeta."""
    M, Cn = x.shape
    require_cuda(dpool, idx, x, mean, rstd, gamma, beta)
    assert M == N * H * W and dpool.is_contiguous() and idx.dtype == torch.uint8 and idx.is_contiguous()
    dx = torch.empty_like(x)
    dg, db = empty(Cn, like=x), empty(Cn, like=x)
    ws = empty(lib().tavsr_bn_ws(M, Cn), like=x)
    check(lib().tavsr_bn_bwd_pooled(ptr(dpool), ptr(idx), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(dx), ptr(dg), ptr(db), N,
                                    H, W, Cn, ACT[act], ptr(ws), stream()), "tavsr_bn_bwd_pooled")
    return dx, dg, db


def maxpool3x3s2_fwd(x, N, H, W, Cn):
    Ho, Wo = conv_out(H, 3, 2, 1), conv_out(W, 3, 2, 1)
    y = empty(N * Ho * Wo, Cn, like=x)
    idx = torch.empty((N * Ho * Wo, Cn), dtype=torch.uint8, device=x.device)
    check(lib().tavsr_maxpool3x3s2_fwd(ptr(x), ptr(y), ptr(idx), N, H, W, Cn, stream()), "tavsr_maxpool3x3s2_fwd")
    return y, idx, Ho, Wo


def bn_act_maxpool3x3s2_fwd(z, mean, rstd, gamma, beta, act, N, H, W, Cn):
    """maxpool(act(BatchNorm(z))) without writing the activation map: -> (pooled, idx, Ho, Wo)."""
    Ho, Wo = conv_out(H, 3, 2, 1), conv_out(W, 3, 2, 1)
    require_cuda(z, mean, rstd, gamma, beta)
    y = empty(N * Ho * Wo, Cn, like=z)
    idx = torch.empty((N * Ho * Wo, Cn), dtype=torch.uint8, device=z.device)
    check(lib().tavsr_bn_act_maxpool3x3s2_fwd(ptr(z), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ACT[act], ptr(y), ptr(idx), N, H, W, Cn,
                                              stream()), "tavsr_bn_act_maxpool3x3s2_fwd")
    return y, idx, Ho, Wo


def maxpool3x3s2_bwd(dy, idx, N, H, W, Cn):
    dx = empty(N * H * W, Cn, like=dy)
    check(lib().tavsr_maxpool3x3s2_bwd(ptr(dy), ptr(idx), ptr(dx), N, H, W, Cn, stream()), "tavsr_maxpool3x3s2_bwd")
    return dx


def avgpool_fwd(x, N, P, Cn):
    y = empty(N, Cn, like=x)
    check(lib().tavsr_avgpool_fwd(ptr(x), ptr(y), N, P, Cn, stream()), "tavsr_avgpool_fwd")
    return y


def avgpool_bwd(dy, N, P, Cn):
    dx = empty(N * P, Cn, like=dy)
    check(lib().tavsr_avgpool_bwd(ptr(dy), ptr(dx), N, P, Cn, stream()), "tavsr_avgpool_bwd")
    return dx


def conv_wflip(w2d, cout, cin):
    require_cuda(w2d)
    out = empty(cin, 9 * cout, like=w2d)
    check(lib().tavsr_conv_wflip(ptr(w2d), ptr(out), cout, cin, stream()), "tavsr_conv_wflip")
    return out


def conv_wsplit(w):
    """the B operand of a split-operand convolution (tavsr_conv_wsplit): w [N, K] fp32 -> one buffer of 5 N K / 2 floats: the dense
    copy of w, then its three bf16 planes [3, N, K] (high, middle and low part of every weight, k permuted inside 16-blocks as
    the kernel reads it)."""
    require_cuda(w)
    N, K = w.shape
    assert w.stride(1) == 1 and K % 16 == 0
    out = empty(5 * N * K // 2, like=w)
    check(lib().tavsr_conv_wsplit(ptr(w), w.stride(0), ptr(out), N, K, stream()), "tavsr_conv_wsplit")
    return out


def x6_takes(w, taps=9, pad0=False):
    """does the split-operand kernel take a forward / data-gradient launch with the GEMM weight ``w`` (csrc/gemm_conv.hip, conv_x6:
    the padded 3x3, or a 1x1 of at least 256 channels)?  False where ops.CONV_X6 is off."""
    return bool(ops.CONV_X6 and not pad0 and w.stride(1) == 1 and w.shape[1] % 32 == 0 and (taps == 9 or w.shape[1] >= 256))


def _x6(w, planes, taps=9, pad0=False):
    """(B operand, conv_posmajor bit) of a forward / data-gradient launch: the caller's conv_wsplit buffer, or one made here, with
    bit 4; (w, 0) where the launch is not one the split-operand kernel takes"""
    if not x6_takes(w, taps, pad0):
        return w, 0
    return (conv_wsplit(w) if planes is None else planes), 16


def x6_dw_takes(cin, cout, taps=9, pad0=False, mode=2, pixels=0):
    """does the split-operand kernel take the weight gradient of a convolution Cin -> Cout over ``pixels`` output pixels
    (csrc/gemm_conv.hip, conv_x6_dw: conv_mode 2 with the 9 padded taps, at any stride, or the 1x1; not the unpadded window, not the
    Conv3d stem's modes 5 / 7; whole K-steps of 32 pixels and column tiles inside one tap, as the implicit route needs)?  False where
    ops.CONV_X6_DW is off."""
    return bool(ops.CONV_X6_DW and mode == 2 and not pad0 and taps in (9, 1) and pixels % 32 == 0 and cin % 64 == 0)


def _tapskip_bits():
    return 1 | (0 if ops.CONV_TILEORDER else 2) | (0 if ops.CONV_DW_UNEVEN else 4)


def _tapskip(H, W, stride=1, taps=9, pad0=False, dw=False):
    on = ops.CONV_TAPSKIP and stride == 1 and taps == 9 and not pad0 and H * W <= (ops.CONV_TAPSKIP_MAXPOS_DW if dw else ops.CONV_TAPSKIP_MAXPOS)
    return _tapskip_bits() if on else 0


def _tapskip2(H, W, dw=False):
    """conv_posmajor of a stride-2 3x3 / pad 1 convolution over H x W input maps"""
    on = ops.CONV_TAPSKIP and (ops.CONV_TAPSKIP_STRIDE2_DW if dw else ops.CONV_TAPSKIP_STRIDE2)
    return (_tapskip_bits() | 8) if on and ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) <= ops.CONV_TAPSKIP_STRIDE2_MAXPOS else 0


def _tapskip_any(H, W, stride, taps, pad0, dw=False):
    return _tapskip2(H, W, dw) if stride == 2 and taps == 9 and not pad0 else _tapskip(H, W, stride, taps, pad0, dw)


def conv3x3_fwd(x, w2d, H, W, stride=1, taps=9, pad0=False, bias=None, act=None, planes=None):
    """implicit 3x3/p1 (taps 9) or 1x1/p0 (taps 1) convolution with stride: x [images*H*W, Cin] channels-last image rows,
    w2d [Cout, taps*Cin] -> [images*Ho*Wo, Cout].  ``pad0``: the 3x3 window without padding (Conv2dSubsampling).
    ``planes``: conv_wsplit(w2d), where the caller has it (ops.CONV_X6; made here otherwise)."""
    M, cin = x.shape
    cout = w2d.shape[0]
    if pad0:
        assert taps == 9
        Ho, Wo = (H - 3) // stride + 1, (W - 3) // stride + 1
    else:
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    Mo = M // (H * W) * Ho * Wo
    z = empty(Mo, cout, like=x)
    B, x6 = _x6(w2d, planes, taps, pad0)
    gemm(Mo, cout, taps * cin, x, cin, B, taps * cin, z, cout, conv=(1, H, W, cin, stride, 90 if pad0 else taps, _tapskip_any(H, W, stride, taps, pad0) | x6),
         bias=bias, act=act)
    return z


def conv3x3_dx(dz, wflip, H, W, res=None, planes=None):
    """data gradient: dz [pixels, Cout], wflip [Cin, 9*Cout] (conv_wflip) -> [pixels, Cin] (+ res: the skip path's
    gradient, added in the GEMM epilogue).  ``planes``: conv_wsplit(wflip), where the caller has it."""
    M, cout = dz.shape
    cin = wflip.shape[0]
    dx = empty(M, cin, like=dz)
    B, x6 = _x6(wflip, planes)
    gemm(M, cin, 9 * cout, dz, cout, B, 9 * cout, dx, cin, conv=(1, H, W, cout, 0, 0, _tapskip(H, W) | x6), R=res, ldr=0 if res is None else cin)
    return dx


def conv3x3_dw(dz, x, H, W, stride=1, taps=9, pad0=False, bias_grad=False, force=None):
    """weight gradient: dz [output pixels, Cout], x [images*H*W, Cin] -> [Cout, taps*Cin]; needs output pixels % 32 == 0.
    ``bias_grad``: also the column sums of dz (the bias gradient) from the same launch.  ``force`` = (-1, slices): ask the
    planner for that many K slices (tavsr_gemm_tune; tests)."""
    M, cout = dz.shape
    cin = x.shape[1]
    dw = empty(cout, taps * cin, like=dz)
    gb = empty(cout, like=dz) if bias_grad else None
    x6 = 32 if x6_dw_takes(cin, cout, taps, pad0, pixels=M) else 0
    gemm(cout, taps * cin, M, dz, cout, x, cin, dw, taps * cin, a_kmajor=True, b_kmajor=True,
         conv=(2, H, W, cin, stride, 90 if pad0 else taps, _tapskip_any(H, W, stride, taps, pad0, dw=True) | x6), a_rowsum=gb, force=force)
    return (dw, gb) if bias_grad else dw
