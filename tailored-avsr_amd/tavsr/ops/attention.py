"""Attention glue: head biases, softmax (+ dropout) and the fused attention core."""
from __future__ import annotations

import ctypes as C

import torch

from .._lib import AttnDesc, check, lib, ptr, require_cuda, stream
from .base import _addr, empty, f32
from .rng import _new_token

__all__ = ["add_head_bias", "pad4", "softmax_fwd", "softmax_bwd", "_attn_desc", "attn_fwd", "attn_bwd"]


# ---------------------------------------------------------------------------------------------- attention glue
def add_head_bias(q, u, v):
    M, D = q.shape
    qu, qv = empty(M, D, like=q), empty(M, D, like=q)
    require_cuda(q, u, v)
    check(lib().tavsr_add_head_bias(ptr(q), q.stride(0), ptr(u), ptr(v), ptr(qu), ptr(qv), M, D, stream()), "tavsr_add_head_bias")
    return qu, qv


def pad4(n: int) -> int:
    return (n + 3) // 4 * 4


def softmax_fwd(ac, bd, klens, scale, causal=False, T2=None, W=0, p_drop=0.0, token=None):
    """ac [H,B,T1,ld_s] (ld_s >= T2, padded rows), bd [H,B,T1,ld_w] or None -> attn like ac.
    ``p_drop`` > 0: also returns (pv, token) = dropout(attn, p_drop) computed by the same launch, with the mask and token
    ``dropout(attn, p_drop)`` would give (``token`` from a previous call reproduces its mask)."""
    H, B, T1, ld_s = ac.shape
    T2 = ld_s if T2 is None else T2
    attn = torch.empty_like(ac)
    ld_w = 0
    if bd is not None:
        ld_w = bd.shape[-1]
        W = W or ld_w
    require_cuda(ac, bd, klens)
    if p_drop and p_drop > 0.0:
        assert ac.is_contiguous() and ld_s % 4 == 0
        pv = torch.empty_like(ac)
        if token is None:
            token = _new_token(p_drop, ac.numel(), ac.device)
        check(lib().tavsr_softmax_dropout_fwd(ptr(ac), ptr(bd), ptr(klens), ptr(attn), ptr(pv), H, B, T1, T2, W, ld_s, ld_w, scale,
                                              int(causal), token[0], ptr(token[2]), token[1], stream()), "tavsr_softmax_dropout_fwd")
        return attn, pv, token
    check(lib().tavsr_softmax_fwd(ptr(ac), ptr(bd), ptr(klens), ptr(attn), H, B, T1, T2, W, ld_s, ld_w, scale, int(causal), stream()),
          "tavsr_softmax_fwd")
    return attn


def softmax_bwd(attn, dattn, scale, skew=False, T2=None, token=None):
    """``token`` (p, offset): dattn is the gradient of the DROPPED probabilities of softmax_fwd(p_drop=...): the mask is
    regenerated inside the launch."""
    H, B, T1, ld_s = attn.shape
    T2 = ld_s if T2 is None else T2
    ds = torch.empty_like(attn)
    W = 2 * T1 - 1 if skew else 0
    ld_w = pad4(W)
    sk = empty(H, B, T1, ld_w, like=attn) if skew else None
    if token is not None:
        check(lib().tavsr_softmax_dropout_bwd(ptr(attn), ptr(dattn), ptr(ds), ptr(sk), H, B, T1, T2, W, ld_s, ld_w, scale, token[0],
                                              ptr(token[2]), token[1], stream()), "tavsr_softmax_dropout_bwd")
        return ds, sk
    check(lib().tavsr_softmax_bwd(ptr(attn), ptr(dattn), ptr(ds), ptr(sk), H, B, T1, T2, W, ld_s, ld_w, scale, stream()),
          "tavsr_softmax_bwd")
    return ds, sk


def _attn_desc(q, q_off, k, k_off, v, v_off, B, T1, T2, H, dk, klens, causal, pos, bias_u, bias_v, token):
    require_cuda(q, k, v, klens, pos, bias_u, bias_v)
    d = AttnDesc()
    d.q, d.k, d.v = _addr(q, q_off), _addr(k, k_off), _addr(v, v_off)
    d.ldq, d.ldk, d.ldv = q.stride(0), k.stride(0), v.stride(0)
    if pos is not None:
        d.pos, d.ldp = _addr(pos), pos.stride(0)
    d.bias_u = _addr(bias_u)
    d.bias_v = _addr(bias_v)
    d.klens = _addr(klens)
    d.B, d.H, d.T1, d.T2, d.dk = B, H, T1, T2, dk
    d.scale, d.causal = 1.0 / (dk ** 0.5), int(bool(causal))
    if token is not None:
        d.p_drop, d.drop_offset, d.seed_dev = token[0], token[1], _addr(token[2])
    return d


def attn_fwd(q, q_off, k, k_off, v, v_off, B, T1, T2, H, dk, klens=None, causal=False, pos=None, bias_u=None, bias_v=None,
             p_drop=0.0):
    """q / k / v: 2-D row buffers (row b*T + t; head h at columns off + h*dk ..); pos [2*T1-1, H*dk] projected positions
    (rel-pos form) with the flat pos_bias_u / pos_bias_v.  -> (ctx [B*T1, H*dk], lse [B*H, T1], dropout token or None)."""
    tok = _new_token(p_drop, B * H * T1 * pad4(T2), q.device) if p_drop and p_drop > 0.0 else None
    d = _attn_desc(q, q_off, k, k_off, v, v_off, B, T1, T2, H, dk, klens, causal, pos, bias_u, bias_v, tok)
    ctx = empty(B * T1, H * dk, like=q)
    lse = empty(B * H, T1, like=q)
    check(lib().tavsr_attn_fwd(C.byref(d), ptr(ctx), ctx.stride(0), ptr(lse), stream()), "tavsr_attn_fwd")
    return ctx, lse, tok


def attn_bwd(dctx, ctx, lse, tok, q, q_off, k, k_off, v, v_off, B, T1, T2, H, dk, dq, dq_off, dk_buf, dk_off, dv_buf, dv_off,
             klens=None, causal=False, pos=None, bias_u=None, bias_v=None):
    """writes d/d(q + u) rows into dq, dK / dV into dk_buf / dv_buf (head-strided windows at the given offsets); rel-pos:
    returns (dqv [B*T1, H*dk], ds_skew [H, B, T1, pad4(2*T1-1)]) else (None, None)."""
    d = _attn_desc(q, q_off, k, k_off, v, v_off, B, T1, T2, H, dk, klens, causal, pos, bias_u, bias_v, tok)
    require_cuda(dctx, ctx, lse, dq, dk_buf, dv_buf)
    assert dctx.stride(0) == ctx.stride(0)
    dqv = sk = None
    ldw = 0
    if pos is not None:
        dqv = empty(B * T1, H * dk, like=q)
        ldw = pad4(2 * T1 - 1)
        sk = torch.zeros(H, B, T1, ldw, dtype=f32, device=q.device)      # the kernel writes the band of every row
        assert dqv.stride(0) == dq.stride(0)
    check(lib().tavsr_attn_bwd(C.byref(d), ptr(dctx), ptr(ctx), ctx.stride(0), ptr(lse), _addr(dq, dq_off), ptr(dqv), dq.stride(0),
                               _addr(dk_buf, dk_off), dk_buf.stride(0), _addr(dv_buf, dv_off), dv_buf.stride(0), ptr(sk), ldw, stream()),
          "tavsr_attn_bwd")
    return dqv, sk
