"""CTC (loss, greedy, forced alignment), Mask-CTC, label smoothing, the LM's shifted rows and the embeddings."""
from __future__ import annotations

from collections import namedtuple

import torch

from .. import _lib as L
from .._lib import check, lib, ptr, require_cuda, stream
from .base import empty, f32
from .rng import _new_token

__all__ = ["ctc_loss", "ctc_greedy", "ctc_align_lds_ok", "ctc_align", "edit_distance_rows", "ErrorTables", "error_counts_ok", "error_counts",
           "maskctc_init", "maskctc_step", "mask_uniform", "count_recip", "lm_shift", "row_sums", "lsm_loss", "embed_pe", "embed_bwd"]


# ---------------------------------------------------------------------------------------------- CTC / losses
def ctc_loss(logits, hlens, targets, tlens, blank=0, zero_infinity=True):
    """logits [B,T,V] contiguous -> (nll [B], dnll/dlogits [B,T,V])."""
    B, T, V = logits.shape
    Lmax = targets.shape[1]
    require_cuda(logits, hlens, targets, tlens)
    loss, grad = empty(B, like=logits), torch.empty_like(logits)
    ws = empty(lib().tavsr_ctc_loss_ws(B, T, Lmax), like=logits)
    check(lib().tavsr_ctc_loss(ptr(logits), V, T * V, ptr(hlens), ptr(targets), targets.stride(0), ptr(tlens), blank, int(zero_infinity),
                               ptr(loss), ptr(grad), ptr(ws), B, T, V, Lmax, stream()), "tavsr_ctc_loss")
    return loss, grad


def ctc_greedy(logits, hlens=None, blank=0, collapse=True):
    B, T, V = logits.shape
    require_cuda(logits, hlens)
    ids = torch.empty((B, T), dtype=torch.int64, device=logits.device)
    hyp = torch.empty((B, T), dtype=torch.int64, device=logits.device) if collapse else None
    hl = torch.empty((B,), dtype=torch.int64, device=logits.device) if collapse else None
    check(lib().tavsr_ctc_greedy(ptr(logits), V, T * V, ptr(hlens), blank, ptr(ids), ptr(hyp), ptr(hl), B, T, V, stream()),
          "tavsr_ctc_greedy")
    return ids, hyp, hl


def ctc_align_lds_ok(T, Lmax) -> bool:
    """does the move table of (frames, longest target) fit a workgroup's LDS?  the library's answer (tavsr_ctc_align_lds_ok)"""
    return bool(lib().tavsr_ctc_align_lds_ok(int(T), int(Lmax)))


def ctc_align(logits, hlens, targets, tlens, blank=0, rows=None, route=None):
    """CTC forced alignment (tavsr_ctc_align: Viterbi over the CTC lattice with a back-trace, one launch, nothing read on the
    host).  logits [B, T, >= V] fp32 - a view whose row stride exceeds V (4-padded rows) is taken as it is; hlens int64 [B];
    targets int64 [N, Lmax] (any padding), tlens int64 [N]; rows int32 [N] (or None: N == B, problem n uses logits row n) names
    the logits row of every problem.  -> (align int64 [N, T], frame_lp fp32 [N, T], span int32 [N, Lmax, 2], score fp32 [N]);
    an infeasible problem has score -inf, align -1, frame_lp 0 and span -1.  ``route``: None (LDS when the move table fits,
    else the workspace), "lds" or "ws"."""
    B, T, V = logits.shape
    N, Lmax = targets.shape
    require_cuda(logits, hlens, targets, tlens, rows)
    assert logits.dtype == f32 and logits.stride(2) == 1 and logits.stride(1) >= V and (B <= 1 or logits.stride(0) >= T * logits.stride(1))
    assert hlens.dtype == torch.int64 and hlens.numel() == B and hlens.is_contiguous()
    assert tlens.dtype == torch.int64 and tlens.numel() == N and tlens.is_contiguous()
    assert targets.dtype == torch.int64 and (Lmax == 0 or targets.stride(1) == 1) and (N <= 1 or targets.stride(0) >= Lmax)
    if rows is None:
        assert N == B, "ctc_align: without rows every logits row is one problem"
    else:
        assert rows.dtype == torch.int32 and rows.numel() == N and rows.is_contiguous()
    if route not in (None, "lds", "ws"):
        raise ValueError(f"ctc_align: route must be None, 'lds' or 'ws': {route!r}")
    if route is None:
        route = "lds" if ctc_align_lds_ok(T, Lmax) else "ws"
    dev = logits.device
    align = torch.empty((N, T), dtype=torch.int64, device=dev)
    frame_lp = empty(N, T, like=logits)
    span = torch.empty((N, Lmax, 2), dtype=torch.int32, device=dev)
    score = empty(N, like=logits)
    ws = torch.empty((max(lib().tavsr_ctc_align_ws(N, T, Lmax), 4),), dtype=torch.uint8, device=dev) if route == "ws" else None
    check(lib().tavsr_ctc_align(ptr(logits), logits.stride(1), logits.stride(0), ptr(hlens), ptr(rows), ptr(targets),
                                max(targets.stride(0), Lmax), ptr(tlens), int(blank), ptr(align), ptr(frame_lp), ptr(span),
                                ptr(score), ptr(ws), N, T, V, Lmax, stream()), "tavsr_ctc_align")
    return align, frame_lp, span, score


# ---------------------------------------------------------------------------------------------- error rates
def edit_distance_rows(hyp, hyp_len, ref, ref_len):
    """Levenshtein distances of B pairs of padded symbol rows (tavsr_edit_distance_rows): hyp [B, n], ref [B, m] int32 (views of
    wider buffers are taken as they are), hyp_len / ref_len int32 [B] on the device -> dist int32 [B].  Nothing beyond a length
    is read.  (``ops.edit_distance`` is the packed-offsets form of the corpus evaluator.)"""
    require_cuda(hyp, hyp_len, ref, ref_len)
    B, n = hyp.shape
    m = ref.shape[1]
    assert ref.shape[0] == B and hyp.dtype == ref.dtype == torch.int32 and (n <= 1 or hyp.stride(1) == 1) and (m <= 1 or ref.stride(1) == 1)
    assert all(t.dtype == torch.int32 and t.shape == (B,) and t.is_contiguous() for t in (hyp_len, ref_len))
    dist = torch.empty((B,), dtype=torch.int32, device=hyp.device)
    check(lib().tavsr_edit_distance_rows(ptr(hyp), max(hyp.stride(0), n) if B > 1 else n, ptr(hyp_len), n, ptr(ref),
                                         max(ref.stride(0), m) if B > 1 else m, ptr(ref_len), m, ptr(dist), B, stream()),
          "tavsr_edit_distance_rows")
    return dist


ErrorTables = namedtuple("ErrorTables", "span cps cp_space drop V tok_max")      # device tensors of tavsr_error_counts' token tables


def error_counts_ok(modes, B, Th, L, tok_max) -> bool:
    """does tavsr_error_counts take this shape?  the library's answer (tavsr_error_counts_ok; include/tavsr.h states the bound)"""
    return bool(lib().tavsr_error_counts_ok(int(modes), int(B), int(Th), int(L), int(tok_max)))


def error_counts(ys_hat, ys_pad, tables, modes):
    """ys_hat [B, Th], ys_pad [B, L] int64 ids (-1 = padding), ``tables``: an ``ErrorTables``, ``modes``: bits 1 ctc_chars,
    2 att_chars, 4 att_words -> (errs, ref_n) int32 [n_modes, B], one row per set bit in rising order: the edit count and the
    reference length of every utterance (tavsr_error_counts, one launch).  No host read, no sync: capturable."""
    require_cuda(ys_hat, ys_pad, *tables[:4])
    if ys_hat.dtype != torch.int64 or (ys_hat.shape[1] > 1 and ys_hat.stride(1) != 1):
        ys_hat = ys_hat.to(torch.int64).contiguous()
    if ys_pad.dtype != torch.int64 or (ys_pad.shape[1] > 1 and ys_pad.stride(1) != 1):
        ys_pad = ys_pad.to(torch.int64).contiguous()
    (B, Th), L = ys_hat.shape, ys_pad.shape[1]
    assert ys_pad.shape[0] == B and tables.span.numel() == 3 * (tables.V + 1) and tables.drop.numel() == tables.V
    n_modes = bin(int(modes)).count("1")
    errs = torch.empty((n_modes, B), dtype=torch.int32, device=ys_hat.device)
    ref_n = torch.empty((n_modes, B), dtype=torch.int32, device=ys_hat.device)
    check(lib().tavsr_error_counts(ptr(ys_hat), max(ys_hat.stride(0), Th) if B > 1 else Th, Th, ptr(ys_pad),
                                   max(ys_pad.stride(0), L) if B > 1 else L, L, ptr(tables.span), ptr(tables.cps), ptr(tables.cp_space),
                                   ptr(tables.drop), tables.V, tables.tok_max, int(modes), ptr(errs), ptr(ref_n), B, stream()),
          "tavsr_error_counts")
    return errs, ref_n


def maskctc_init(logits, hlens, blank, mask_token, threshold, n_iterations):
    """CTC logits [B,T,V] -> (y_in, y_hat [B,max(T,1)] int64, tok_prob [B,max(T,1)], y_len [B] int64,
    plan [B,3] int32 = (mask_num, num_iter, per_iter)): the start of MaskCTCInference.forward (tavsr_maskctc_init)."""
    B, T, V = logits.shape
    require_cuda(logits, hlens)
    assert logits.is_contiguous() and logits.dtype == torch.float32
    Lc = max(T, 1)
    y_in = torch.empty((B, Lc), dtype=torch.int64, device=logits.device)
    y_hat = torch.empty((B, Lc), dtype=torch.int64, device=logits.device)
    tok_prob = empty(B, Lc, like=logits)
    y_len = torch.empty((B,), dtype=torch.int64, device=logits.device)
    plan = torch.empty((B, 3), dtype=torch.int32, device=logits.device)
    check(lib().tavsr_maskctc_init(ptr(logits), V, T * V, ptr(hlens), int(blank), int(mask_token), float(threshold), int(n_iterations),
                                   ptr(y_in), ptr(y_hat), ptr(tok_prob), Lc, ptr(y_len), ptr(plan), B, T, V, stream()),
          "tavsr_maskctc_init")
    return y_in, y_hat, tok_prob, y_len, plan


def maskctc_step(logits, y_in, y_len, plan, it, mask_token):
    """pass ``it`` of the Mask-CTC fill loop on decoder logits [B,L,V+1]; ``y_in`` [B,>=L] int64 is updated in place."""
    B, L, V1 = logits.shape
    require_cuda(logits, y_in, y_len, plan)
    assert logits.is_contiguous() and logits.dtype == torch.float32 and y_in.dtype == torch.int64 and y_in.stride(1) == 1
    assert y_len.dtype == torch.int64 and plan.dtype == torch.int32 and plan.is_contiguous() and y_in.shape[1] >= L
    check(lib().tavsr_maskctc_step(ptr(logits), V1, L * V1, ptr(y_in), y_in.stride(0), ptr(y_len), ptr(plan), int(it), int(mask_token), B,
                                   L, V1, stream()), "tavsr_maskctc_step")
    return y_in


def mask_uniform(text, mask_token, eos, ignore_id, token=None):
    """text [B, L] int64 -> (ys_in, ys_out [B, L] int64, n_target [B] int32, token): espnet ``mask_uniform`` drawn on the device
    (tavsr_mask_uniform; include/tavsr.h has the counter layout).  ``token`` follows the dropout contract: (offset, step-seed
    tensor), a fresh one reserves B * S counters of the current pass; a call with a previous token regenerates that draw bit
    for bit.  No host read, no sync: capturable, and a captured call draws new masks at every replay."""
    require_cuda(text)
    assert text.dim() == 2 and text.dtype == torch.int64 and (text.shape[1] <= 1 or text.stride(1) == 1)
    B, Lmax = text.shape
    if token is None:
        _, off, seed = _new_token(0.0, B * ((Lmax + 1 + 3) // 4 * 4), text.device)
        token = (off, seed)
    ys_in = torch.empty((B, Lmax), dtype=torch.int64, device=text.device)
    ys_out = torch.empty((B, Lmax), dtype=torch.int64, device=text.device)
    n_target = torch.empty((B,), dtype=torch.int32, device=text.device)
    check(lib().tavsr_mask_uniform(ptr(text), text.stride(0), B, Lmax, int(mask_token), int(eos), int(ignore_id), ptr(token[1]),
                                   token[0], ptr(ys_in), ptr(ys_out), Lmax, ptr(n_target), stream()), "tavsr_mask_uniform")
    return ys_in, ys_out, n_target, token


def count_recip(n):
    """n [B] int32 on the device -> 1 / max(1, sum(n)) as a one-element fp32 device tensor (tavsr_count_recip)."""
    require_cuda(n)
    assert n.dtype == torch.int32 and n.is_contiguous()
    inv = torch.empty((1,), dtype=f32, device=n.device)
    check(lib().tavsr_count_recip(ptr(n), n.numel(), ptr(inv), stream()), "tavsr_count_recip")
    return inv


def lm_shift(text, lengths, sos_eos, width=None):
    """text [B, W] int64, lengths [B] int64 -> (x, t [B, width] int64, x_lengths [B] int64, n [B] int32): the language model's
    shifted input / target rows built on the device (tavsr_lm_shift; include/tavsr.h has the row layout).  ``width`` defaults to
    W + 1.  Padded entries of ``text`` are never read as ids: x is 0 and t is -1 behind a sentence whatever ``text`` holds there.
    No host read, no sync: capturable."""
    require_cuda(text, lengths)
    assert text.dim() == 2 and text.dtype == torch.int64 and (text.shape[1] <= 1 or text.stride(1) == 1)
    assert lengths.dtype == torch.int64 and lengths.is_contiguous() and lengths.shape == (text.shape[0],)
    B, W = text.shape
    Wout = W + 1 if width is None else int(width)
    x = torch.empty((B, Wout), dtype=torch.int64, device=text.device)
    t = torch.empty((B, Wout), dtype=torch.int64, device=text.device)
    x_lengths = torch.empty((B,), dtype=torch.int64, device=text.device)
    n = torch.empty((B,), dtype=torch.int32, device=text.device)
    check(lib().tavsr_lm_shift(ptr(text), text.stride(0), ptr(lengths), B, W, int(sos_eos), ptr(x), ptr(t), Wout, Wout, ptr(x_lengths),
                               ptr(n), stream()), "tavsr_lm_shift")
    return x, t, x_lengths, n


def row_sums(x):
    """x [rows, cols] fp32 -> [rows] sums over the columns in a fixed order (tavsr_lm_row_sums)."""
    require_cuda(x)
    assert x.dim() == 2 and x.dtype == f32 and (x.shape[1] <= 1 or x.stride(1) == 1)
    out = empty(x.shape[0], like=x)
    check(lib().tavsr_lm_row_sums(ptr(x), x.stride(0), ptr(out), x.shape[0], x.shape[1], stream()), "tavsr_lm_row_sums")
    return out


def lsm_loss(logits2d, target, ignore, smoothing):
    rows, V = logits2d.shape
    require_cuda(logits2d, target)
    row_loss, grad = empty(rows, like=logits2d), torch.empty_like(logits2d)
    correct = torch.empty((rows,), dtype=torch.int32, device=logits2d.device)
    check(lib().tavsr_lsm_loss(ptr(logits2d), V, ptr(target), ignore, smoothing, ptr(row_loss), ptr(grad), ptr(correct), rows, V, stream()),
          "tavsr_lsm_loss")
    return row_loss, grad, correct


def embed_pe(ids, table, pe, scale, step_dev=None):
    """table[ids] * scale + pe; ``step_dev`` (int32 device scalar): ids is [N, 1] and every row takes pe[step] (tavsr_embed_pe_step)"""
    B, Lq = ids.shape
    D = table.shape[1]
    require_cuda(ids, table, pe)
    out = empty(B, Lq, D, like=table)
    if step_dev is not None:
        assert Lq == 1 and step_dev.dtype == torch.int32 and pe.is_contiguous() and pe.shape[1] == D
        check(lib().tavsr_embed_pe_step(ptr(ids), ptr(table), ptr(pe), scale, ptr(out), B, pe.shape[0], D, ptr(step_dev), stream()),
              "tavsr_embed_pe_step")
        return out
    check(lib().tavsr_embed_pe(ptr(ids), ptr(table), ptr(pe), scale, ptr(out), B * Lq, Lq, D, stream()), "tavsr_embed_pe")
    return out


def embed_bwd(ids, dout, scale, V):
    D = dout.shape[-1]
    dt = empty(V, D, like=dout)
    check(lib().tavsr_embed_bwd(ptr(ids), ptr(dout), scale, ptr(dt), ids.numel(), V, D, 0, stream()), "tavsr_embed_bwd")
    return dt
