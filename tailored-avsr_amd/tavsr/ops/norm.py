"""Column sums and LayerNorm, forward and backward; the grouped (dgamma, dbeta) reduction."""
from __future__ import annotations

from .. import ops
from .._lib import ACT, check, lib, ptr, require_cuda, stream
from .base import _addr, empty
from .blocks import DnSlabs
from .rng import dropout

__all__ = ["colsum", "add2_colsum", "layernorm_fwd", "layernorm_bwd", "layernorm_bwd_act", "LNGroup"]


def colsum(x, *, scale=1.0, out=None, accumulate=False):
    M, N = x.shape
    require_cuda(x)
    if out is None:
        out = empty(N, like=x)
    ws = empty(lib().tavsr_colsum_ws(M, N), like=x)
    check(lib().tavsr_colsum(ptr(x), x.stride(0), M, N, scale, ptr(out), int(accumulate), ptr(ws), stream()), "tavsr_colsum")
    return out


def add2_colsum(x, y, out, lazy_sums=False):
    """out = x + y (row-strided 2-D views); returns (column sums of x, column sums of y).  ``lazy_sums``: a third result, a function that
    reduces the launch's partial rows into the two sums - they are bias gradients; the caller runs it with its other weight gradients."""
    M, N = x.shape
    require_cuda(x, y, out)
    sx, sy = empty(N, like=x), empty(N, like=x)
    nws = lib().tavsr_colsum_ws(M, N)
    ws = empty(2 * nws, like=x)
    check(lib().tavsr_add2_colsum(ptr(x), x.stride(0), ptr(y), y.stride(0), ptr(out), out.stride(0), M, N, ptr(None if lazy_sums else sx),
                                  ptr(None if lazy_sums else sy), ptr(ws), stream()), "tavsr_add2_colsum")
    if not lazy_sums:
        return sx, sy

    def reduce():
        check(lib().tavsr_sum_partials2(ptr(ws), nws // N, 2 * N, ptr(sx), N, ptr(sy), N, 0, stream()), "tavsr_sum_partials2")
    return sx, sy, reduce


# ---------------------------------------------------------------------------------------------- norms
def layernorm_fwd(x, gamma, beta, eps, *, save=True):
    M, D = x.shape
    require_cuda(x, gamma, beta)
    y = empty(M, D, like=x)
    mean = empty(M, like=x) if save else None
    rstd = empty(M, like=x) if save else None
    check(lib().tavsr_layernorm_fwd(ptr(x), x.stride(0), ptr(gamma), ptr(beta), eps, ptr(y), D, ptr(mean), ptr(rstd), M, D, stream()),
          "tavsr_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, mean, rstd, gamma, *, dx_add=None, dx=None):
    """returns dx (= dx_add + LN'(dy)), dgamma, dbeta."""
    M, D = x.shape
    require_cuda(dy, x, mean, rstd, gamma, dx_add)
    if dx is None:
        dx = empty(M, D, like=x)
    dg, db = empty(D, like=x), empty(D, like=x)
    ws = empty(lib().tavsr_layernorm_bwd_ws(M, D), like=x)
    check(lib().tavsr_layernorm_bwd(ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(mean), ptr(rstd), ptr(gamma), ptr(dx_add),
                                    0 if dx_add is None else dx_add.stride(0), ptr(dx), dx.stride(0), ptr(dg), ptr(db), 0, ptr(ws), M, D,
                                    stream()), "tavsr_layernorm_bwd")
    return dx, dg, db


def layernorm_bwd_act(dy, x, mean, rstd, gamma, z, act, *, dx=None):
    """layernorm_bwd for x = act(z): dx is the gradient w.r.t. z; returns dx, dgamma, dbeta."""
    M, D = x.shape
    require_cuda(dy, x, mean, rstd, gamma, z)
    if dx is None:
        dx = empty(M, D, like=x)
    dg, db = empty(D, like=x), empty(D, like=x)
    ws = empty(lib().tavsr_layernorm_bwd_ws(M, D), like=x)
    check(lib().tavsr_layernorm_bwd_act(ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(mean), ptr(rstd), ptr(gamma), ptr(dx), dx.stride(0),
                                        ptr(dg), ptr(db), 0, ptr(ws), M, D, ptr(z), z.stride(0), ACT[act], stream()),
          "tavsr_layernorm_bwd_act")
    return dx, dg, db


class LNGroup:
    """LayerNorm backward passes of one backward node whose (dgamma, dbeta) partials share ONE reduction launch:
    ``bwd`` runs the main pass (dx is ready when it returns) and parks the per-block partials in a common slab,
    ``flush`` sums the slab once; the gradient tensors handed out by ``bwd`` are views that are valid after ``flush``.
    LayerNorms of another shape than the group's first one are reduced immediately (same results either way)."""

    def __init__(self, cap: int = 8):
        self.CAP = cap
        self.key, self.slab, self.out, self.k = None, None, None, 0

    def takes(self, M, D) -> bool:
        """the next ``bwd`` of this shape goes through the group's own launch (D = 256: also in the slab form)"""
        return D == 256 and (self.key is None or ((M, D) == self.key and self.k < self.CAP))

    def bwd(self, dy, x, mean, rstd, gamma, *, dx_add=None, dx=None, drop=None):
        """``drop`` (a dropout token): also returns dx * mask / keep as a fourth result (the masked gradient the next residual
        block's branch starts from) - from the same launch when the group takes the call, else from a dropout launch."""
        M, D = x.shape
        if isinstance(dy, DnSlabs):       # (callers ask ``takes`` first: the group's own launch is the only one that reads slabs)
            assert self.takes(M, D) and (drop is None or ops.LN_BWD_DROP)
        if drop is not None and not ops.LN_BWD_DROP:
            r = self.bwd(dy, x, mean, rstd, gamma, dx_add=dx_add, dx=dx)
            return r + (dropout(r[0], drop[0], token=drop)[0],)
        if self.key is None:
            self.key = (M, D)
            self.nb = lib().tavsr_layernorm_bwd_ws(M, D) // (2 * D)
            self.slab = empty(self.nb, self.CAP * 2 * D, like=x)
            self.out = empty(self.CAP * 2 * D, like=x)
        if (M, D) != self.key or self.k >= self.CAP:
            r = layernorm_bwd(dy, x, mean, rstd, gamma, dx_add=dx_add, dx=dx)
            return r if drop is None else r + (dropout(r[0], drop[0], token=drop)[0],)
        slabs = dy if isinstance(dy, DnSlabs) else None
        require_cuda(slabs.ws if slabs else dy, x, mean, rstd, gamma, dx_add)
        if dx is None:
            dx = empty(M, D, like=x)
        off = self.k * 2 * D
        if slabs is not None:
            dxd = empty(M, D, like=x) if drop is not None else None
            assert dx.is_contiguous()
            check(lib().tavsr_layernorm_bwd_partial_slab(ptr(slabs.ws), slabs.wpb, slabs.rb, ptr(x), x.stride(0), ptr(mean), ptr(rstd),
                                                         ptr(gamma), ptr(dx_add), 0 if dx_add is None else dx_add.stride(0), ptr(dx),
                                                         dx.stride(0), _addr(self.slab) + 4 * off, self.slab.stride(0), M, D, ptr(dxd),
                                                         drop[0] if drop is not None else 0.0, ptr(drop[2] if drop is not None else None),
                                                         drop[1] if drop is not None else 0, stream()), "tavsr_layernorm_bwd_partial_slab")
            self.k += 1
            r = (dx, self.out[off: off + D], self.out[off + D: off + 2 * D])
            return r if drop is None else r + (dxd,)
        if drop is not None:
            assert dx.is_contiguous()
            dxd = empty(M, D, like=x)
            check(lib().tavsr_layernorm_bwd_partial_drop(ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(mean), ptr(rstd), ptr(gamma),
                                                         ptr(dx_add), 0 if dx_add is None else dx_add.stride(0), ptr(dx), dx.stride(0),
                                                         _addr(self.slab) + 4 * off, self.slab.stride(0), M, D, ptr(dxd), drop[0],
                                                         ptr(drop[2]), drop[1], stream()), "tavsr_layernorm_bwd_partial_drop")
            self.k += 1
            return dx, self.out[off: off + D], self.out[off + D: off + 2 * D], dxd
        check(lib().tavsr_layernorm_bwd_partial(ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(mean), ptr(rstd), ptr(gamma), ptr(dx_add),
                                                0 if dx_add is None else dx_add.stride(0), ptr(dx), dx.stride(0),
                                                _addr(self.slab) + 4 * off, self.slab.stride(0), M, D, stream()),
              "tavsr_layernorm_bwd_partial")
        self.k += 1
        return dx, self.out[off: off + D], self.out[off + D: off + 2 * D]

    def flush(self):
        if self.k:
            n = self.k * 2 * self.key[1]
            check(lib().tavsr_sum_partials(ptr(self.slab), self.nb, self.slab.stride(0), ptr(self.out), n, 0, stream()),
                  "tavsr_sum_partials")
            self.k = 0
