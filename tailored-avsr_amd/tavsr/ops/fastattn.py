"""Fastformer additive attention (csrc/fastattn.hip) and the absolute positional encodings' add."""
from __future__ import annotations

from .._lib import check, lib, ptr, require_cuda, stream
from .base import _addr, empty

__all__ = ["fastattn_ok", "fastattn_pool", "fastattn_scale_rows", "fastattn_bwd_pool", "fastattn_bwd_rows",
           "fastattn_fwd", "fastattn_bwd", "add_pe", "add_pe_dalpha"]


def fastattn_ok(D: int, H: int) -> bool:
    """the range of the kernels, without the library (constructors run on hosts that have not built it).  The same range is
    ``fa_shape_ok`` of csrc/fastattn.hip (tavsr_fastattn_ok) and, in words, ``ops.FASTATTN_LIMIT``: change the three together
    (tests/test_gpu_fastattn.py compares this one with the library's)."""
    return 1 <= H <= 8 and 4 <= D <= 512 and D % H == 0 and (D // H) % 4 == 0


def fastattn_pool(x, x_off, cs, w, bias, lens, B, T, D, H):
    """rows ``x[:, x_off: x_off + D]`` of a 2-D buffer (row b*T + t), ``cs`` [B, D] column scales or None, score weights ``w``
    [H, D] / ``bias`` [H] -> (weights [B, H, T]: the masked softmax over time, 0 at t >= lens[b]; pooled [B, D])"""
    require_cuda(x, cs, w, bias, lens)
    assert w.is_contiguous() and (cs is None or cs.is_contiguous())
    score, wout, pooled = empty(B, H, T, like=x), empty(B, H, T, like=x), empty(B, D, like=x)
    check(lib().tavsr_fastattn_pool(_addr(x, x_off), x.stride(0), ptr(cs), ptr(w), ptr(bias), ptr(lens), ptr(score), ptr(wout),
                                    ptr(pooled), B, T, D, H, stream()), "tavsr_fastattn_pool")
    return wout, pooled


def fastattn_scale_rows(q, q_off, pk, B, T, D):
    """wv [B*T, D] = pk[b] * q rows (every row)"""
    require_cuda(q, pk)
    wv = empty(B * T, D, like=q)
    check(lib().tavsr_fastattn_scale_rows(_addr(q, q_off), q.stride(0), ptr(pk), ptr(wv), B, T, D, stream()), "tavsr_fastattn_scale_rows")
    return wv


def fastattn_bwd_pool(dwv, q, q_off, lens, B, T, D):
    """dpk [B, D] = sum_t dwv * q"""
    require_cuda(dwv, q, lens)
    dpk = empty(B, D, like=q)
    check(lib().tavsr_fastattn_bwd_pool(ptr(dwv), dwv.stride(0), _addr(q, q_off), q.stride(0), ptr(lens), ptr(dpk), B, T, D, stream()),
          "tavsr_fastattn_bwd_pool")
    return dpk


def fastattn_bwd_rows(is_k, x, x_off, cs, w_pool, dpool, pool, w, lens, dx, dx_off, B, T, D, H, dres=None, dwv=None, pk=None):
    """the mirror of one ``fastattn_pool`` call (include/tavsr.h): writes the rows' gradient into ``dx[:, dx_off: dx_off + D]`` ->
    (dW [H, D], dbias [H], dcs [B, D] for the key rows / None for the query rows)"""
    require_cuda(x, cs, w_pool, dpool, pool, w, lens, dx, dres, dwv, pk)
    dwb = empty(H * D + H, like=x)
    dcs = empty(B, D, like=x) if is_k else None
    nws = lib().tavsr_fastattn_bwd_ws(B, T, D, H)
    ws = empty(max(nws, 4), like=x)
    check(lib().tavsr_fastattn_bwd_rows(int(bool(is_k)), _addr(x, x_off), x.stride(0), ptr(cs), ptr(w_pool), ptr(dpool), ptr(pool), ptr(w),
                                        ptr(lens), ptr(dres), 0 if dres is None else dres.stride(0), ptr(dwv),
                                        0 if dwv is None else dwv.stride(0), ptr(pk), _addr(dx, dx_off), dx.stride(0), ptr(dwb), ptr(dcs),
                                        ptr(ws), B, T, D, H, stream()), "tavsr_fastattn_bwd_rows")
    return dwb[: H * D].view(H, D), dwb[H * D:], dcs


def fastattn_fwd(qk, wq_att, bq_att, wk_att, bk_att, lens, B, T, D, H, p=0.0):
    """the additive-attention core on ``qk`` [B*T, 2D] = q | k: -> (wv [B*T, D] = pk * q, kept) with kept = (alpha, pq_pre, pq, t_pq,
    beta, pk_pre, pk, t_pk): the two pooling weights [B, H, T], the pooled vectors before and after their dropout (rate ``p``,
    the same tensor twice without) and the dropout tokens"""
    from .rng import dropout
    alpha, pq_pre = fastattn_pool(qk, 0, None, wq_att, bq_att, lens, B, T, D, H)
    pq, t_pq = dropout(pq_pre, p) if p and p > 0.0 else (pq_pre, None)
    beta, pk_pre = fastattn_pool(qk, D, pq, wk_att, bk_att, lens, B, T, D, H)
    pk, t_pk = dropout(pk_pre, p) if p and p > 0.0 else (pk_pre, None)
    return fastattn_scale_rows(qk, 0, pk, B, T, D), (alpha, pq_pre, pq, t_pq, beta, pk_pre, pk, t_pk)


def fastattn_bwd(dwv, dres, qk, kept, wq_att, wk_att, lens, B, T, D, H):
    """from ``dwv`` (gradient of wv) and ``dres`` (gradient arriving at q through the residual) -> (dqk [B*T, 2D],
    d query_att.weight, d query_att.bias, d key_att.weight, d key_att.bias)"""
    from .rng import dropout
    alpha, pq_pre, pq, t_pq, beta, pk_pre, pk, t_pk = kept
    dqk = empty(B * T, 2 * D, like=qk)
    dpk = fastattn_bwd_pool(dwv, qk, 0, lens, B, T, D)
    if t_pk is not None:
        dropout(dpk, t_pk[0], out=dpk, token=t_pk)
    gwk, gbk, dpq = fastattn_bwd_rows(True, qk, D, pq, beta, dpk, pk_pre, wk_att, lens, dqk, D, B, T, D, H)
    if t_pq is not None:
        dropout(dpq, t_pq[0], out=dpq, token=t_pq)
    gwq, gbq, _ = fastattn_bwd_rows(False, qk, 0, None, alpha, dpq, pq_pre, wq_att, lens, dqk, 0, B, T, D, H, dres=dres, dwv=dwv, pk=pk)
    return dqk, gwq, gbq, gwk, gbk


def add_pe(x, pe, alpha=None, xscale=1.0):
    """y = xscale * x + alpha * pe[t]; x [B, T, D] contiguous, pe [T, D], ``alpha`` a one-element device tensor or None (1)"""
    require_cuda(x, pe, alpha)
    B, T, D = x.shape
    assert x.is_contiguous() and pe.is_contiguous() and tuple(pe.shape) == (T, D)
    y = empty(B, T, D, like=x)
    check(lib().tavsr_add_pe(ptr(x), ptr(pe), ptr(alpha), xscale, ptr(y), B, T, D, stream()), "tavsr_add_pe")
    return y


def add_pe_dalpha(dy, pe):
    """sum(dy * pe) as a one-element tensor, the same bits every run"""
    require_cuda(dy, pe)
    B, T, D = dy.shape
    assert dy.is_contiguous() and pe.is_contiguous()
    out, ws = empty(1, like=dy), empty(lib().tavsr_add_pe_dalpha_ws(), like=dy)
    check(lib().tavsr_add_pe_dalpha(ptr(dy), ptr(pe), ptr(out), ptr(ws), B, T, D, stream()), "tavsr_add_pe_dalpha")
    return out
