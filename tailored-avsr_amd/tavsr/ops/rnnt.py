"""Transducer training (csrc/rnnt.hip): LSTM, joint rows, lattice, RNN-T loss and the greedy step."""
from __future__ import annotations

import torch

from .. import ops
from .._lib import check, lib, ptr, require_cuda, stream
from .attention import pad4
from .base import empty
from .matmul import linear, linear_dw, linear_dx

__all__ = ["lstm_rows_per_wg", "lstm_wt", "lstm_fwd", "lstm_bwd", "lstm_step", "rnnt_mask_rows", "rnnt_chunk", "rnnt_joint_rows",
           "rnnt_lattice_lds_ok", "rnnt_lattice", "rnnt_joint_grad", "rnnt_loss", "rnnt_frame_z", "rnnt_greedy_pick"]


# ---------------------------------------------------------------------------------------------- transducer (csrc/rnnt.hip)
def lstm_rows_per_wg() -> int:
    """batch rows one workgroup of the LSTM kernels owns (the partition of DESIGN.md section 4h)"""
    return int(lib().tavsr_lstm_rows_per_wg())


def lstm_wt(w_hh):
    """weight_hh [4H, H] -> its transpose [H, 4H], the layout lstm_fwd / lstm_step stream"""
    require_cuda(w_hh)
    assert w_hh.dim() == 2 and w_hh.is_contiguous() and w_hh.shape[0] == 4 * w_hh.shape[1]
    H = w_hh.shape[1]
    wt = empty(H, 4 * H, like=w_hh)
    check(lib().tavsr_lstm_wt(ptr(w_hh), ptr(wt), H, stream()), "tavsr_lstm_wt")
    return wt


def lstm_fwd(x, w_ih, w_hh, b_ih, b_hh, h0=None, c0=None, lens=None, save=True):
    """one LSTM layer, batch first: x [B, L, I] -> (y [B, L, H], hN, cN [B, H], saved).  The input products are one GEMM, the
    recurrence one launch (tavsr_lstm_fwd).  ``lens`` int64 [B] (None: full length): padded steps keep the state and give y = 0."""
    B, Ln, I = x.shape
    H = w_hh.shape[1]
    require_cuda(x, w_ih, w_hh, b_ih, b_hh, h0, c0, lens)
    assert x.is_contiguous() and w_ih.shape == (4 * H, I) and (lens is None or (lens.dtype == torch.int64 and lens.is_contiguous()))
    x2 = x.view(B * Ln, I)
    xg = linear(x2, w_ih)
    wt = lstm_wt(w_hh)
    y = empty(B, Ln, H, like=x)
    hprev, c_all, gates = (empty(B, Ln, H, like=x), empty(B, Ln, H, like=x), empty(B, Ln, 4 * H, like=x)) if save else (None, None, None)
    hN, cN = empty(B, H, like=x), empty(B, H, like=x)
    check(lib().tavsr_lstm_fwd(ptr(xg), 4 * H, ptr(wt), ptr(b_ih), ptr(b_hh), ptr(h0), ptr(c0), ptr(lens), ptr(y), ptr(hprev), ptr(c_all),
                               ptr(gates), ptr(hN), ptr(cN), B, Ln, H, stream()), "tavsr_lstm_fwd")
    return y, hN, cN, (x2, hprev, c_all, gates)


def lstm_bwd(dy, saved, w_ih, w_hh, c0=None, lens=None, dhN=None, dcN=None, need_dx=True):
    """backward of ``lstm_fwd``: -> (dx [B, L, I] or None, dW_ih, dW_hh, db (of either bias), dh0, dc0)."""
    x2, hprev, c_all, gates = saved
    B, Ln, H = c_all.shape
    require_cuda(dy, dhN, dcN, c0, lens)
    assert dy is None or dy.is_contiguous()
    dgates = torch.empty_like(gates)
    dh0, dc0 = empty(B, H, like=gates), empty(B, H, like=gates)
    check(lib().tavsr_lstm_bwd(ptr(dy), ptr(dhN), ptr(dcN), ptr(w_hh), ptr(c0), ptr(lens), ptr(c_all), ptr(gates), ptr(dgates), ptr(dh0),
                               ptr(dc0), B, Ln, H, stream()), "tavsr_lstm_bwd")
    dg2 = dgates.view(B * Ln, 4 * H)
    dx = linear_dx(dg2, w_ih).view(B, Ln, -1) if need_dx else None
    dw_ih, db = linear_dw(dg2, x2, bias_grad=True)
    dw_hh = linear_dw(dg2, hprev.view(B * Ln, H))
    return dx, dw_ih, dw_hh, db, dh0, dc0


def lstm_step(xg, wt, b_ih, b_hh, h, c, commit=None, h_out=None, c_out=None):
    """one step for N rows (tavsr_lstm_step): xg [N, 4H] = x W_ih^T, wt = ``lstm_wt(weight_hh)``, states [N, H] in and out (in
    place when no output is given); ``commit`` uint8 [N]: rows with 0 keep their state.  No host read: capturable."""
    N, H = h.shape
    require_cuda(xg, wt, b_ih, b_hh, h, c, commit)
    assert xg.stride(1) == 1 and h.is_contiguous() and c.is_contiguous() and (commit is None or commit.dtype == torch.uint8)
    h_out = h if h_out is None else h_out
    c_out = c if c_out is None else c_out
    check(lib().tavsr_lstm_step(ptr(xg), xg.stride(0), ptr(wt), ptr(b_ih), ptr(b_hh), ptr(h), ptr(c), ptr(commit), ptr(h_out), ptr(c_out),
                                N, H, stream()), "tavsr_lstm_step")
    return h_out, c_out


def rnnt_mask_rows(x, lens, extra=0):
    """x [B, Tn, D] -> a copy whose rows r >= lens[b] + extra are 0 (tavsr_rnnt_mask_rows)"""
    B, Tn, D = x.shape
    require_cuda(x, lens)
    assert x.is_contiguous() and lens.dtype == torch.int64 and lens.is_contiguous()
    out = torch.empty_like(x)
    check(lib().tavsr_rnnt_mask_rows(ptr(x), ptr(lens), int(extra), ptr(out), B, Tn, D, stream()), "tavsr_rnnt_mask_rows")
    return out


def rnnt_chunk(V, rows) -> int:
    return max(1, min(int(rows), ops.RNNT_WS_FLOATS // pad4(V)))


def _rnnt_check(e, d, w_out, y, tlens, ulens):
    B, T, J = e.shape
    U1 = d.shape[1]
    V = w_out.shape[0]
    assert e.is_contiguous() and d.is_contiguous() and w_out.is_contiguous() and d.shape == (B, U1, J) and w_out.shape[1] == J
    assert y.dtype == torch.int32 and y.shape[0] == B and y.shape[1] >= U1 - 1 and (y.shape[1] <= 1 or y.stride(1) == 1)
    assert tlens.dtype == torch.int64 and ulens.dtype == torch.int64 and tlens.is_contiguous() and ulens.is_contiguous()
    return B, T, U1, J, V


def rnnt_joint_rows(e, d, w_out, b_out, y, tlens, ulens, blank=0, chunk=None):
    """e [B, T, J], d [B, U1, J] -> (lse, lp_blank, lp_label [B, T, U1]) in chunks of lattice rows (tavsr_rnnt_joint_rows)"""
    require_cuda(e, d, w_out, b_out, y, tlens, ulens)
    B, T, U1, J, V = _rnnt_check(e, d, w_out, y, tlens, ulens)
    chunk = rnnt_chunk(V, B * T * U1) if chunk is None else int(chunk)
    ws = empty(max(1, lib().tavsr_rnnt_ws(B, T, U1, J, V, chunk, 0)), like=e)
    lse, lpb, lpl = empty(B, T, U1, like=e), empty(B, T, U1, like=e), empty(B, T, U1, like=e)
    check(lib().tavsr_rnnt_joint_rows(ptr(e), ptr(d), ptr(w_out), ptr(b_out), ptr(y), max(y.stride(0), U1 - 1), ptr(tlens), ptr(ulens),
                                      int(blank), ptr(lse), ptr(lpb), ptr(lpl), ptr(ws), B, T, U1, J, V, chunk, stream()),
          "tavsr_rnnt_joint_rows")
    return lse, lpb, lpl


def rnnt_lattice_lds_ok(T, U1) -> bool:
    return bool(lib().tavsr_rnnt_lattice_lds_ok(int(T), int(U1)))


def rnnt_lattice(lp_blank, lp_label, tlens, ulens, route=None):
    """lp_blank, lp_label [B, T, U1] -> (nll [B], occ, p_blank, p_label [B, T, U1]) (tavsr_rnnt_lattice).  ``route``: None (LDS
    when alpha and beta fit, else the workspace), "lds" or "ws"."""
    B, T, U1 = lp_blank.shape
    require_cuda(lp_blank, lp_label, tlens, ulens)
    assert lp_blank.is_contiguous() and lp_label.is_contiguous() and lp_label.shape == lp_blank.shape
    assert tlens.dtype == torch.int64 and ulens.dtype == torch.int64 and tlens.is_contiguous() and ulens.is_contiguous()
    if route not in (None, "lds", "ws"):
        raise ValueError(f"rnnt_lattice: route must be None, 'lds' or 'ws': {route!r}")
    if route is None:
        route = "lds" if rnnt_lattice_lds_ok(T, U1) else "ws"
    ws = empty(max(1, lib().tavsr_rnnt_lattice_ws(B, T, U1)), like=lp_blank) if route == "ws" else None
    nll = empty(B, like=lp_blank)
    occ, pb, pl = torch.empty_like(lp_blank), torch.empty_like(lp_blank), torch.empty_like(lp_blank)
    check(lib().tavsr_rnnt_lattice(ptr(lp_blank), ptr(lp_label), ptr(tlens), ptr(ulens), ptr(nll), ptr(occ), ptr(pb), ptr(pl), ptr(ws),
                                   B, T, U1, stream()), "tavsr_rnnt_lattice")
    return nll, occ, pb, pl


def rnnt_joint_grad(e, d, w_out, b_out, y, tlens, ulens, lse, occ, p_blank, p_label, gscale, inv_b, blank=0, chunk=None):
    """-> (de [B, T, J], dd [B, U1, J], dW_out [V, J], db_out [V] or None) (tavsr_rnnt_joint_grad); ``gscale``: 1-element device
    tensor (the upstream gradient) or None."""
    require_cuda(e, d, w_out, b_out, y, tlens, ulens, lse, occ, p_blank, p_label, gscale)
    B, T, U1, J, V = _rnnt_check(e, d, w_out, y, tlens, ulens)
    chunk = rnnt_chunk(V, B * T * U1) if chunk is None else int(chunk)
    ws = empty(max(1, lib().tavsr_rnnt_ws(B, T, U1, J, V, chunk, 1)), like=e)
    de, dd, dw = torch.empty_like(e), torch.empty_like(d), torch.empty_like(w_out)
    db = None if b_out is None else empty(V, like=e)
    check(lib().tavsr_rnnt_joint_grad(ptr(e), ptr(d), ptr(w_out), ptr(b_out), ptr(y), max(y.stride(0), U1 - 1), ptr(tlens), ptr(ulens),
                                      int(blank), ptr(lse), ptr(occ), ptr(p_blank), ptr(p_label), ptr(gscale), float(inv_b), ptr(de),
                                      ptr(dd), ptr(dw), ptr(db), ptr(ws), B, T, U1, J, V, chunk, stream()), "tavsr_rnnt_joint_grad")
    return de, dd, dw, db


def rnnt_loss(e, d, w_out, b_out, y, tlens, ulens, blank=0, chunk=None, route=None):
    """joint rows + lattice: -> (nll [B], (lse, occ, p_blank, p_label)) - what ``rnnt_joint_grad`` needs"""
    lse, lpb, lpl = rnnt_joint_rows(e, d, w_out, b_out, y, tlens, ulens, blank, chunk)
    nll, occ, pb, pl = rnnt_lattice(lpb, lpl, tlens, ulens, route)
    return nll, (lse, occ, pb, pl)


def rnnt_frame_z(e, d, frame, out=None):
    """z [B, J] = tanh(e[b, frame] + d[b]) for the frame counter in device memory (tavsr_rnnt_frame_z)"""
    B, T, J = e.shape
    require_cuda(e, d, frame)
    assert e.is_contiguous() and d.is_contiguous() and d.shape == (B, J) and frame.dtype == torch.int32
    out = empty(B, J, like=e) if out is None else out
    check(lib().tavsr_rnnt_frame_z(ptr(e), ptr(d), ptr(frame), ptr(out), B, T, J, stream()), "tavsr_rnnt_frame_z")
    return out


def rnnt_greedy_pick(logits, tlens, blank, frame, tok, commit, hyp, hyp_len, score):
    """one frame of the greedy transducer search for a batch (tavsr_rnnt_greedy_pick); every output is updated in place"""
    B, V = logits.shape
    require_cuda(logits, tlens, frame, tok, commit, hyp, hyp_len, score)
    assert logits.stride(1) == 1 and tlens.dtype == torch.int64 and frame.dtype == torch.int32 and tok.dtype == torch.int64
    assert commit.dtype == torch.uint8 and hyp.dtype == torch.int64 and hyp.is_contiguous() and hyp_len.dtype == torch.int32
    check(lib().tavsr_rnnt_greedy_pick(ptr(logits), logits.stride(0), ptr(tlens), int(blank), ptr(frame), ptr(tok), ptr(commit), ptr(hyp),
                                       hyp.shape[1], ptr(hyp_len), ptr(score), B, V, stream()), "tavsr_rnnt_greedy_pick")
