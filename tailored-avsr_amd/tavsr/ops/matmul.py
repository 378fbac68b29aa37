"""tavsr_gemm and the Linear forms built on it; the grouped weight-gradient launches and their launch policy."""
from __future__ import annotations

import ctypes as C

import torch

from .. import ops
from .._lib import ACT, GemmDesc, check, lib, ptr, require_cuda, stream
from .base import _addr, _zero_page, empty, f32
from .blocks import axpby
from .data import multi_copy_
from .rng import _new_token, dropout, dropout_act_bwd, dropout_add

__all__ = ["GemmProfile", "gemm", "linear", "linear_dx", "rowdot_ok", "linear_drop", "linear_dx_drop", "linear_dx_cat", "linear_dw",
           "WgradGroup", "linear_group"]


class GemmProfile:
    """Optional per-launch timing of tavsr_gemm with HIP events on the launch stream (bench.py's roofline
    leg).  Off on the product path (``PROFILE is None``): zero overhead."""

    def __init__(self, by_shape: bool = False):
        self.records = []  # (key, flops, operand bytes, start_event, end_event)
        self.by_shape = by_shape

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for key, flops, nbytes, e0, e1 in self.records:
            a = agg.setdefault(key, [0, 0.0, 0.0, 0.0])
            a[0] += 1
            a[1] += flops
            a[2] += e0.elapsed_time(e1) * 1e-3
            a[3] += nbytes
        return {k: dict(calls=v[0], flops=v[1], seconds=v[2], bytes=v[3]) for k, v in agg.items()}


def _gemm_kernel_key(d) -> str:
    """Names the kernel family a launch runs (layout); the tile is the planner's choice (csrc/gemm.hip)."""
    return f"gemm_kernel<{'T' if d.a_kmajor else 'N'}{'N' if d.b_kmajor else 'T'}>"


# ---------------------------------------------------------------------------------------------- GEMM
def gemm(M, N, K, A, lda, B, ldb, Cc, ldc, *, a_off=0, b_off=0, c_off=0, a_kmajor=False, b_kmajor=False,
         nb1=1, nb2=1, sA=(0, 0), sB=(0, 0), sC=(0, 0), bias=None, act=None, alpha=1.0, Z=None,
         R=None, r_off=0, ldr=0, sR=(0, 0), DZ=None, dact=None, a_rowsum=None, conv=None, force=None, ws_cap=None,
         drop=None, rowstat=None, ln=None, rowdot=None):
    """Raw descriptor call; offsets are in elements into the given tensors.  ``force=(cfg, nsplit)`` bypasses
    the planner (tuning / tests); ``ws_cap`` caps the split-K workspace handed to the library (tests of its fallback).
    ``ln`` = (gamma, beta, eps, out [M, N]): also the LayerNorm of the result rows (tavsr_gemm_ln)."""
    require_cuda(A, B, Cc, bias, Z, R, DZ, a_rowsum)
    d = GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.a_kmajor, d.b_kmajor = int(a_kmajor), int(b_kmajor)
    d.A, d.lda = _addr(A, a_off), lda
    d.B, d.ldb = _addr(B, b_off), ldb
    d.C, d.ldc = _addr(Cc, c_off), ldc
    d.nb1, d.nb2 = nb1, nb2
    d.sA1, d.sA2 = sA
    d.sB1, d.sB2 = sB
    d.sC1, d.sC2 = sC
    d.bias = _addr(bias)
    d.act, d.alpha = ACT[act], alpha
    d.Z = None if Z is None else _addr(Z, c_off)
    if R is not None:
        d.R, d.ldr = _addr(R, r_off), ldr
        d.sR1, d.sR2 = sR
    if DZ is not None:
        d.DZ, d.dact = _addr(DZ, c_off), ACT[dact]
    if a_rowsum is not None:
        d.a_rowsum = _addr(a_rowsum)
    if drop is not None:        # dropout token (p, offset, seed tensor): the mask rides in the epilogue
        d.drop_p, d.drop_offset, d.drop_seed = drop[0], drop[1], _addr(drop[2])
    if rowstat is not None:     # [M, ceil(N / 64), 2]: per-row (sum, M2 about the tile's own mean) of every 64-column tile of the result
        d.rowstat = _addr(rowstat)
        if rowdot is not None:  # ... or the two weighted sums (<rowdot[0], row>, <rowdot[1], row>) per tile (tavsr_gemm_desc.rowdot_*)
            require_cuda(rowdot[0], rowdot[1])
            d.rowdot_a, d.rowdot_b = _addr(rowdot[0]), _addr(rowdot[1])
    if conv is not None:       # (mode, H, W, C[, stride, taps]): implicit convolution operand (include/tavsr.h)
        d.conv_mode, d.conv_H, d.conv_W, d.conv_C = conv[:4]
        if len(conv) > 4:
            d.conv_stride, d.conv_taps = conv[4], conv[5]
        if len(conv) > 6:
            d.conv_posmajor = int(conv[6])
        d.conv_zero = _addr(_zero_page(Cc.device))
    if force is not None and force[1] > 1:
        need = force[1] * max(1, nb1) * max(1, nb2) * M * N + force[1] * M
    else:
        need = lib().tavsr_gemm_ws(C.byref(d))
    if ws_cap is not None:
        need = min(need, int(ws_cap))
    if need > 0:
        ws = torch.empty(need, dtype=f32, device=Cc.device)
        d.ws, d.ws_floats = _addr(ws), need

    def call():
        if ln is not None:
            assert force is None
            require_cuda(ln[0], ln[1], ln[3])
            check(lib().tavsr_gemm_ln(C.byref(d), ptr(ln[0]), ptr(ln[1]), ln[2], ptr(ln[3]), ln[3].stride(0), stream()), "tavsr_gemm_ln")
        elif force is None:
            check(lib().tavsr_gemm(C.byref(d), stream()), "tavsr_gemm")
        else:
            check(lib().tavsr_gemm_tune(C.byref(d), int(force[0]), int(force[1]), stream()), "tavsr_gemm_tune")

    if ops.PROFILE is None:
        call()
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    key = _gemm_kernel_key(d)
    if ops.PROFILE.by_shape:
        key += f" M={M} N={N} K={K} nb={max(1, nb1) * max(1, nb2)}"
    nb = max(1, nb1) * max(1, nb2)
    a_el, b_el = M * K, K * N                 # each operand once; an implicit-conv operand is the image, not its 9 taps
    if conv is not None and conv[0] >= 4:      # Conv3d stem: the clip tensor is the gathered operand
        a_el, b_el = (A.numel(), b_el) if conv[0] in (4, 6) else (a_el, B.numel())
    elif conv is not None:
        a_el, b_el = (a_el // 9, b_el) if conv[0] == 1 else (a_el, b_el // 9)
    c_el = M * N * (1 + (R is not None) + (Z is not None) + (DZ is not None))
    fl = 2.0 * M * N * K * nb
    if conv is not None and conv[0] in (6, 7):    # padded-clip stem: 245 taps are algorithmic, the 288-wide layout is not
        fl = fl * 245.0 / 288.0
    elif conv is not None and conv[0] in (4, 5):  # 4-byte-gather stem: 245 taps padded to 256
        fl = fl * 245.0 / 256.0
    ops.PROFILE.records.append((key, fl, 4.0 * nb * (a_el + b_el + c_el), e0, e1))


def linear(x, w, b=None, *, act=None, alpha=1.0, res=None, save_z=False, out=None, out_off=0, ldc=None, force=None,
           rowstat=None, ln=None):
    """y = res + alpha*act(x @ w.T + b); x [M,K] (row stride x.stride(0)), w [N,K] torch layout.  ``rowstat`` (tensor
    [M, ceil(N / 64), 2]): receives the per-row (sum, M2 = sum of squared deviations from the tile's own mean) of every 64-column tile of y
    (tavsr_gemm_desc.rowstat).
    ``ln`` = (gamma, beta, eps): also returns LayerNorm(y) - (y, normed) - from the launch that finishes the rows (tavsr_gemm_ln)."""
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = empty(M, N, like=x)
        ldc = N
    z = empty(M, N, like=x) if save_z else None
    assert not save_z or (out_off == 0 and ldc == N)
    normed = empty(M, N, like=x) if ln is not None else None
    assert ln is None or (not save_z and rowstat is None and out_off == 0)
    gemm(M, N, K, x, x.stride(0), w, w.stride(0), out, ldc, c_off=out_off, bias=b, act=act, alpha=alpha, Z=z,
         R=res, ldr=0 if res is None else res.stride(0), force=force, rowstat=rowstat,
         ln=None if ln is None else (ln[0], ln[1], ln[2], normed))
    if ln is not None:
        return out, normed
    return (out, z) if save_z else out


def linear_dx(dy, w, *, alpha=1.0, DZ=None, dact=None, res=None, out=None, force=None):
    """dx = res + alpha * (dy @ w) * act'(DZ);  dy [M,N], w [N,K] -> [M,K]."""
    M, N = dy.shape
    K = w.shape[1]
    if out is None:
        out = empty(M, K, like=dy)
    gemm(M, K, N, dy, dy.stride(0), w, w.stride(0), out, out.stride(0), b_kmajor=True, alpha=alpha, DZ=DZ, dact=dact,
         R=res, ldr=0 if res is None else res.stride(0), force=force)
    return out


# Dropout fused into GEMM epilogues (tavsr_gemm_desc.drop_*): same mask as the stand-alone kernels draw for the contiguous
# [M, N] result, so a fused forward pairs with a stand-alone backward and vice versa.  TAVSR_GEMM_DROP=0: separate launches.


def _drop_fusable(x, N, K) -> bool:
    return N % 4 == 0 and K % 32 == 0 and K >= 32 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0


def rowdot_ok(x, w) -> bool:
    """can the Linear x @ w.T leave weighted row sums of its result (tavsr_gemm_desc.rowstat + rowdot_*: the fast kernel, no K split)?"""
    K, N = x.shape[1], w.shape[0]
    return (N % 64 == 0 and K % 32 == 0 and K <= 1024 and x.stride(0) % 4 == 0 and w.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0
            and w.data_ptr() % 16 == 0)


def linear_drop(x, w, b, p, *, act=None, alpha=1.0, res=None, save_z=False, rowdot=None):
    """out = res + alpha * dropout(act(x @ w.T + b), p) -> (out[, z], token); one launch when the GEMM's 16-byte epilogue
    can carry the mask (else GEMM + dropout / dropout_add launches with the same mask and token).  ``rowdot`` = (a [N], b [N]) with
    ``rowdot_ok(x, w)``: also returns rd [M, N / 64, 2] = per row and 64-column tile (<a, out row>, <b, out row>) as the LAST element."""
    M, K = x.shape
    N = w.shape[0]
    if rowdot is not None:
        assert not save_z and res is None and act is None and rowdot_ok(x, w)
        rd = empty(M, N // 64, 2, like=x)
        out = empty(M, N, like=x)
        tok = _new_token(p, M * N, x.device) if p and p > 0.0 else None
        gemm(M, N, K, x, x.stride(0), w, w.stride(0), out, N, bias=b, alpha=alpha, drop=tok, rowstat=rd, rowdot=rowdot)
        return out, tok, rd
    if not p or p <= 0.0:
        r = linear(x, w, b, act=act, alpha=alpha, res=res, save_z=save_z)
        return (r[0], r[1], None) if save_z else (r, None)
    if _drop_fusable(x, N, K) and w.stride(0) % 4 == 0 and (res is None or res.stride(0) % 4 == 0):
        tok = _new_token(p, M * N, x.device)
        out = empty(M, N, like=x)
        z = empty(M, N, like=x) if save_z else None
        gemm(M, N, K, x, x.stride(0), w, w.stride(0), out, N, bias=b, act=act, alpha=alpha, Z=z, R=res,
             ldr=0 if res is None else res.stride(0), drop=tok)
        return (out, z, tok) if save_z else (out, tok)
    r = linear(x, w, b, act=act, save_z=save_z)
    t, z = (r if save_z else (r, None))
    if res is None:
        out, tok = dropout(t, p, out=t)
        if alpha != 1.0:
            out = axpby(out, None, alpha, 0.0, out=out)
    else:
        out, tok = dropout_add(res, t, p, alpha=alpha)
    return (out, z, tok) if save_z else (out, tok)


def linear_dx_drop(dy, w, tok, *, alpha=1.0, DZ=None, dact=None):
    """dx = mask(tok) / keep * alpha * (dy @ w) * act'(DZ): the backward of y = dropout(act(z)) in the data-gradient GEMM's
    epilogue (tok None: no mask)."""
    M, N = dy.shape
    K = w.shape[1]
    if tok is None:
        return linear_dx(dy, w, alpha=alpha, DZ=DZ, dact=dact)
    if _drop_fusable(dy, K, N) and w.stride(0) % 4 == 0:
        out = empty(M, K, like=dy)
        gemm(M, K, N, dy, dy.stride(0), w, w.stride(0), out, K, b_kmajor=True, alpha=alpha, DZ=DZ, dact=dact, drop=tok)
        return out
    if DZ is not None and ACT[dact] > ACT["gelu"]:      # tanh / hardtanh / SELU: act'(DZ) in the GEMM's epilogue, then the mask
        dh = linear_dx(dy, w, alpha=alpha, DZ=DZ, dact=dact)
        return dropout(dh, tok[0], out=dh, token=tok)[0]
    dh = linear_dx(dy, w, alpha=alpha)
    if DZ is not None:
        return dropout_act_bwd(dh, DZ, dact, tok, out=dh)
    return dropout(dh, tok[0], out=dh, token=tok)[0]


def linear_dx_cat(dy_cat, ws, *, res=None, out=None):
    """dx = res + sum_j dy_j @ w_j for projections of ONE input whose output gradients sit side by side in ``dy_cat``
    [M, sum_j N_j] (query / key / value): the weights are stacked into one [sum_j N_j, K] operand (one multi-tensor copy)
    and the sum over j becomes the K loop of a single GEMM instead of a chain of accumulating launches."""
    K = ws[0].shape[1]
    rows = [w.shape[0] for w in ws]
    assert dy_cat.shape[1] == sum(rows) and all(w.shape[1] == K and w.is_contiguous() for w in ws)
    wcat = empty(sum(rows), K, like=dy_cat)
    offs = [sum(rows[:j]) for j in range(len(ws))]
    for i in range(0, len(ws), 24):
        multi_copy_([wcat[o: o + r] for o, r in zip(offs[i: i + 24], rows[i: i + 24])], list(ws[i: i + 24]))
    return linear_dx(dy_cat, wcat, res=res, out=out)


def _dw_gemm(dy, x, alpha, out, gb, force=None):
    """out [N, K] = alpha * dy.T @ x and, with ``gb`` [N], gb = alpha * dy.sum(0): ONE weight-gradient problem through the planner
    (its own K split) - ``linear_dw``, and what ``WgradGroup`` sheds or the grouped kernel does not take"""
    gemm(dy.shape[1], x.shape[1], dy.shape[0], dy, dy.stride(0), x, x.stride(0), out, out.stride(0), a_kmajor=True, b_kmajor=True,
         alpha=alpha, a_rowsum=gb, force=force)


def linear_dw(dy, x, *, alpha=1.0, out=None, bias_grad=False, force=None):
    """dW = alpha * dy.T @ x;  dy [M,N], x [M,K] -> [N,K] (torch weight layout).  With ``bias_grad`` also returns
    db = alpha * dy.sum(0), computed by the same launch from the A fragments (tavsr_gemm a_rowsum)."""
    M, N = dy.shape
    K = x.shape[1]
    if out is None:
        out = empty(N, K, like=dy)
    gb = empty(N, like=dy) if bias_grad else None
    _dw_gemm(dy, x, alpha, out, gb, force=force)
    return (out, gb) if bias_grad else out


class WgradGroup:
    """Deferred weight gradients of one backward node: ``add`` allocates the outputs and records the problem,
    ``flush`` computes all of them with ONE grouped launch (tavsr_gemm_grouped; chunks of 12).  The operands must stay
    unchanged between add and flush (the group keeps them alive).  Problems the fast kernel cannot take (unaligned,
    K % 32 != 0) fall back to individual tavsr_gemm calls - same results either way."""

    MAX = 12

    def __init__(self):
        self.items = []

    def add(self, dy, x, *, alpha=1.0, bias_grad=False):
        M, N = dy.shape
        K = x.shape[1]
        require_cuda(dy, x)
        out = empty(N, K, like=dy)
        gb = empty(N, like=dy) if bias_grad else None
        self.items.append((dy, x, float(alpha), out, gb))
        return (out, gb) if bias_grad else out

    @staticmethod
    def _desc(d, dy, x, alpha, out, gb):
        M, N = dy.shape
        K = x.shape[1]
        d.M, d.N, d.K = N, K, M
        d.a_kmajor, d.b_kmajor = 1, 1
        d.A, d.lda = _addr(dy), dy.stride(0)
        d.B, d.ldb = _addr(x), x.stride(0)
        d.C, d.ldc = _addr(out), out.stride(0)
        d.nb1 = d.nb2 = 1
        d.alpha = alpha
        d.a_rowsum = _addr(gb)

    @staticmethod
    def _tiles(it):
        dy, x = it[0], it[1]
        return -(-dy.shape[1] // 64) * -(-x.shape[1] // 64)

    @classmethod
    def _chunks(cls, items):
        """the grouped launches of ``items``: up to MAX problems each; more than MAX problems (many layers at once: the decoder): problems of
        one reduction length together (a launch lasts as long as its longest tile), at most 5 x 256 tiles per launch (what is resident at once)"""
        if len(items) <= cls.MAX:
            return [items] if items else []
        chunks, cur, cur_t = [], [], 0
        for it in sorted(items, key=lambda it: (-it[0].shape[0], -cls._tiles(it))):
            if cur and (len(cur) == cls.MAX or cur_t + cls._tiles(it) > 1280 or it[0].shape[0] != cur[0][0].shape[0]):
                chunks.append(cur)
                cur, cur_t = [], 0
            cur.append(it)
            cur_t += cls._tiles(it)
        chunks.append(cur)
        return chunks

    def flush(self):
        items, self.items = self.items, []
        # All tiles of a group are resident at once (5 block slots x 256 CUs) and equally long (same K), so the launch
        # lasts as long as the fullest CU: with 784 tiles 16 CUs hold 4 blocks and the other 240 idle a quarter of the
        # time.  Shedding the smallest problems down to a multiple of 256 tiles (they go through the planner's own
        # K split) evens that out; only worth it when one or two small problems do it.
        total = sum(self._tiles(it) for it in items)
        if len(items) <= self.MAX and total > 256 and total % 256:
            target, shed, rest = total // 256 * 256, [], []
            for it in sorted(items, key=self._tiles, reverse=True):      # fewest problems that add up to the surplus
                if self._tiles(it) <= total - target:
                    total -= self._tiles(it)
                    shed.append(it)
                else:
                    rest.append(it)
            if total == target and len(shed) <= 2:       # every shed problem costs a launch of its own
                for it in shed:
                    _dw_gemm(*it)
                keep = set(id(it) for it in rest)
                items = [it for it in items if id(it) in keep]
        for chunk in self._chunks(items):
            arr = (GemmDesc * len(chunk))()
            for d, it in zip(arr, chunk):
                self._desc(d, *it)
            if ops.PROFILE is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            rc = lib().tavsr_gemm_grouped(arr, len(chunk), stream()) if len(chunk) > 1 else -3
            if rc == -3:      # TAVSR_EUNSUPPORTED (or a single problem): one by one through the planner
                for it in chunk:
                    _dw_gemm(*it)
                continue
            check(rc, "tavsr_gemm_grouped")
            if ops.PROFILE is not None:
                e1.record()
                fl = sum(2.0 * dy.shape[0] * dy.shape[1] * x.shape[1] for dy, x, _, _, _ in chunk)
                nby = sum(4.0 * (dy.numel() + x.numel() + dy.shape[1] * x.shape[1]) for dy, x, _, _, _ in chunk)
                key = "gemm_kernel<TN>" + (f" grouped x{len(chunk)}" if ops.PROFILE.by_shape else "")
                ops.PROFILE.records.append((key, fl, nby, e0, e1))


def linear_group(x, wbs, out, ldc=None):
    """several y_j = x @ w_j.T + b_j of ONE input in one grouped launch (query/key/value projections): ``wbs`` is a
    list of (w_j, b_j, column offset of y_j in ``out``); out rows have stride ``ldc``.  Falls back to one GEMM per
    projection when the grouped kernel cannot take the problems (alignment / K % 32) - same results."""
    M, K = x.shape
    ldc = out.stride(0) if ldc is None else ldc
    require_cuda(x, out)
    arr = (GemmDesc * len(wbs))()
    for d, (w, b, off) in zip(arr, wbs):
        d.M, d.N, d.K = M, w.shape[0], K
        d.a_kmajor, d.b_kmajor = 0, 0
        d.A, d.lda = _addr(x), x.stride(0)
        d.B, d.ldb = _addr(w), w.stride(0)
        d.C, d.ldc = _addr(out, off), ldc
        d.nb1 = d.nb2 = 1
        d.bias = _addr(b)
        d.alpha = 1.0
    rc = lib().tavsr_gemm_grouped(arr, len(wbs), stream()) if (len(wbs) > 1 and ops.PROFILE is None) else -3
    if rc == -3:
        for w, b, off in wbs:
            gemm(M, w.shape[0], K, x, x.stride(0), w, w.stride(0), out, ldc, c_off=off, bias=b)
        return out
    check(rc, "tavsr_gemm_grouped")
    return out
