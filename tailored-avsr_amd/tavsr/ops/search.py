"""Decode steps: the small-step Linear, tree attention, CTC prefix scores, beam updates, the one-launch and time-synchronous
searches and the transducer beam searches.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib as L
from .. import ops
from .._lib import ACT, check, lib, ptr, require_cuda, stream
from .base import _i32, empty, f32

__all__ = ["rowlin_ok", "RowParts", "rowlin", "tree_attn_step", "kv_append", "ctc_prefix_step", "ctc_prefix_step_topk", "log_softmax_rows",
           "ngram_score", "beam_combine", "beam_combine_topk_ok", "beam_combine_topk", "beam_select_topk_ok", "beam_select_topk",
           "beam_step_begin", "beam_reorder", "ctc_beam_search_ok", "ctc_beam_search", "timesync_ok", "timesync_ws", "timesync_init",
           "timesync_step", "timesync_search", "tree_attn_rows", "embed_pe_rows", "rnnt_search_ok", "rnnt_search_ws", "rnnt_search_init",
           "rnnt_search_z", "rnnt_row_topk", "rnnt_gather_state", "rnnt_alsd_step", "rnnt_tsd_step"]


def rowlin_ok(x, w, n_rows=None, ln=False, ksplit=1) -> bool:
    """does the one-launch small-step Linear (tavsr_rowlin / tavsr_rowlin_parts) take this call?  Up to 32 rows, K a power of two
    in 64 .. 2048; which (rows, K, LayerNorm prologue, K slices) combinations have a spill-free plan is the library's answer
    (tavsr_rowlin_ok: e.g. K = 2048 with more than 16 rows only in slices, K = 1024 with LayerNorm only up to 16 rows)."""
    if isinstance(x, RowParts):
        x = x.t[0]
    K = x.shape[1]
    N = x.shape[0] if n_rows is None else n_rows
    return bool(ops.ROWLIN and N <= 32 and x.stride(0) % 4 == 0 and w.stride(0) % 4 == 0
                and x.stride(1) == 1 and w.stride(1) == 1 and x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
                and lib().tavsr_rowlin_ok(int(N), int(K), int(bool(ln)), int(ksplit)))


class RowParts:
    """rows held as a SUM of tensors: ``t`` [P, N, D] contiguous - what a K-split ``rowlin`` leaves and the next launches of the
    chain add while they load (tavsr_rowlin_parts)"""
    __slots__ = ("t",)

    def __init__(self, t):
        assert t.dim() == 3 and t.is_contiguous()
        self.t = t

    @property
    def shape(self):
        return self.t.shape[1:]


def rowlin(x, w, b=None, *, ln=None, act=None, res=None, out=None, gather=None, ksplit=1, res_gather=None):
    """out = res + act(LN(x[gather]) @ w.T + b) in one launch (csrc/decode.hip:rowlin_kernel) - the Linear layers of a
    one-token scorer step.  ln = (gamma, beta, eps) or None; gather: int64 row indices into x (embedding lookup).
    ``x`` / ``res`` may be ``RowParts``; ``ksplit`` > 1 deals K to that many blocks per column tile and returns ``RowParts``."""
    if isinstance(x, RowParts) or isinstance(res, RowParts) or ksplit > 1:
        assert gather is None and res_gather is None
        xt, xp = (x.t[0], x.t.shape[0]) if isinstance(x, RowParts) else (x, 1)
        rt, rp = (res.t[0], res.t.shape[0]) if isinstance(res, RowParts) else (res, 1)
        N, K, Nout = xt.shape[0], xt.shape[1], w.shape[0]
        require_cuda(xt, w)
        assert w.shape[1] == K and out is None
        g, be, eps = ln if ln is not None else (None, None, 0.0)
        o = empty(ksplit, N, Nout, like=xt) if ksplit > 1 else empty(N, Nout, like=xt)
        check(lib().tavsr_rowlin_parts(ptr(xt), xt.stride(0), xp, x.t.stride(0) if xp > 1 else 0, ptr(g), ptr(be), eps, ptr(w), w.stride(0),
                                       ptr(b), ACT[act], ptr(rt), 0 if rt is None else rt.stride(0), rp, res.t.stride(0) if rp > 1 else 0,
                                       ptr(o), Nout, ksplit, N * Nout if ksplit > 1 else 0, N, K, Nout, stream()), "tavsr_rowlin_parts")
        return RowParts(o) if ksplit > 1 else o
    N = x.shape[0] if gather is None else gather.numel()
    K, Nout = x.shape[1], w.shape[0]
    require_cuda(x, w)
    assert w.shape[1] == K and (res_gather is None or (res is not None and res_gather.numel() == N and res_gather.dtype == torch.int64))
    if out is None:
        out = empty(N, Nout, like=x)
    assert out.data_ptr() != x.data_ptr()
    g, be, eps = ln if ln is not None else (None, None, 0.0)
    check(lib().tavsr_rowlin(ptr(x), x.stride(0), ptr(gather), ptr(g), ptr(be), eps, ptr(w), w.stride(0), ptr(b), ACT[act], ptr(res),
                             0 if res is None else res.stride(0), ptr(res_gather), ptr(out), out.stride(0), N, K, Nout, stream()),
          "tavsr_rowlin")
    return out


def tree_attn_step(q, kpool, vpool, anc, nkeys, H, dk, out=None, step_dev=None, k_new=None, v_new=None, group=1):
    """q [N, H*dk] (row stride q.stride(0)); kpool/vpool [nodes, H*dk]; anc int32 [N, >= nkeys] -> [N, H*dk].
    ``step_dev`` (int32 device scalar): use min(step + 1, nkeys) keys (graph replays).  ``k_new`` / ``v_new`` (row stride of
    q): this step's keys / values - the last key of every hypothesis - appended to the pools by the same launch."""
    N = q.shape[0]
    require_cuda(q, kpool, vpool, anc)
    assert anc.dtype == torch.int32 and kpool.stride(0) == vpool.stride(0)
    assert k_new is None or (k_new.stride(0) == q.stride(0) and v_new.stride(0) == q.stride(0))
    if out is None:
        out = empty(N, H * dk, like=q)
    check(lib().tavsr_tree_attn_step(ptr(q), q.stride(0), ptr(kpool), ptr(vpool), kpool.stride(0), ptr(anc), anc.stride(0), int(nkeys),
                                     ptr(out), out.stride(0), N, H, dk, 1.0 / (dk ** 0.5), ptr(step_dev), ptr(k_new), ptr(v_new),
                                     int(group), stream()), "tavsr_tree_attn_step")
    return out


def kv_append(k, v, kpool, vpool, N, max_steps, step_dev):
    """kpool/vpool[step * N + n] = k[n] / v[n] with the step index read from device memory."""
    require_cuda(k, v, kpool, vpool, step_dev)
    assert step_dev.dtype == torch.int32 and k.stride(0) == v.stride(0) and kpool.stride(0) == vpool.stride(0)
    assert kpool.shape[0] >= max_steps * N
    check(lib().tavsr_kv_append(ptr(k), ptr(v), k.stride(0), ptr(kpool), ptr(vpool), kpool.stride(0), N, k.shape[1], int(max_steps),
                                ptr(step_dev), stream()), "tavsr_kv_append")


def ctc_prefix_step(logp, lens, r_prev, s_prev, last_tok, cand, K, out_len, blank=0, step_dev=None):
    """-> (r_new [N,T,2,C], psi [N,C], psi_abs [N,C], eos [N], eos_abs [N]); see include/tavsr.h.
    ``step_dev`` (int32 device scalar) replaces ``out_len`` (graph replays).  ``cand`` None: every token is scored (C = V), with the
    sums of the one-launch search (``ctc_beam_search``), bit for bit."""
    U, T, V = logp.shape
    N, Cn = (s_prev.shape[0], V) if cand is None else cand.shape
    require_cuda(logp, lens, r_prev, s_prev, last_tok, cand)
    r_new = empty(N, T, 2, Cn, like=logp)
    psi, psi_abs = empty(N, Cn, like=logp), empty(N, Cn, like=logp)
    eos, eos_abs = empty(N, like=logp), empty(N, like=logp)
    check(lib().tavsr_ctc_prefix_step(ptr(logp), ptr(lens), ptr(r_prev), ptr(s_prev), ptr(last_tok), ptr(cand), ptr(r_new),
                                      ptr(psi), ptr(psi_abs), ptr(eos), ptr(eos_abs), N, K, T, V, Cn,
                                      0 if step_dev is not None else int(out_len), blank, ptr(step_dev), stream()),
          "tavsr_ctc_prefix_step")
    return r_new, psi, psi_abs, eos, eos_abs


def ctc_prefix_step_topk(logp, lens, r_prev, s_prev, last_tok, full, Cn, K, out_len, blank=0, step_dev=None):
    """pre-beam + prefix scores in one launch: -> (cand [N,C] int64, r_new, psi, psi_abs, eos, eos_abs); see include/tavsr.h."""
    U, T, V = logp.shape
    N = full.shape[0]
    require_cuda(logp, lens, r_prev, s_prev, last_tok, full)
    assert full.is_contiguous() and full.shape[1] == V
    cand = torch.empty(N, Cn, dtype=torch.int64, device=logp.device)
    r_new = empty(N, T, 2, Cn, like=logp)
    psi, psi_abs = empty(N, Cn, like=logp), empty(N, Cn, like=logp)
    eos, eos_abs = empty(N, like=logp), empty(N, like=logp)
    check(lib().tavsr_ctc_prefix_step_topk(ptr(logp), ptr(lens), ptr(r_prev), ptr(s_prev), ptr(last_tok), ptr(full), ptr(cand),
                                           ptr(r_new), ptr(psi), ptr(psi_abs), ptr(eos), ptr(eos_abs), N, K, T, V, Cn,
                                           0 if step_dev is not None else int(out_len), blank, ptr(step_dev), stream()),
          "tavsr_ctc_prefix_step_topk")
    return cand, r_new, psi, psi_abs, eos, eos_abs


def log_softmax_rows(x, V=None, out=None, alpha=1.0, add=0.0, accumulate=False):
    """out = (out if accumulate else 0) + alpha * log_softmax(x[:, :V]) + add"""
    M = x.shape[0]
    V = x.shape[1] if V is None else V
    require_cuda(x)
    if out is None:
        out = empty(M, V, like=x)
    assert not accumulate or out is not None
    check(lib().tavsr_log_softmax_rows(ptr(x), x.stride(0), ptr(out), out.stride(0), M, V, alpha, add, int(bool(accumulate)), stream()),
          "tavsr_log_softmax_rows")
    return out


def ngram_score(lm, yseq, step, out=None, alpha=1.0, add=0.0, accumulate=False, step_dev=None, cand=None):
    """out = (out if accumulate else 0) + alpha * (n-gram log10 scores of every token) + add for the hypotheses yseq[:, :step + 1]
    (tavsr_ngram_score; see include/tavsr.h for the semantics).  ``lm``: tavsr.lm.ngram.NgramLM on the device of ``yseq``;
    ``step_dev`` (int32 device scalar) replaces ``step`` (graph replays); ``cand`` int64 [N, C]: only these tokens of every row are
    written (``out`` must then be given)."""
    N, L = yseq.shape
    V = lm.word_map.numel()
    require_cuda(lm.word, lm.logp, lm.backoff, lm.child_begin, lm.word_map, yseq, out, step_dev, cand)
    assert yseq.dtype == torch.int64 and yseq.stride(1) == 1
    assert step_dev is None or step_dev.dtype == torch.int32
    assert cand is None or (cand.dtype == torch.int64 and cand.is_contiguous() and cand.shape[0] == N and out is not None)
    assert not accumulate or out is not None
    if out is None:
        out = torch.empty((N, V), dtype=f32, device=yseq.device)
    assert out.dtype == f32 and out.shape == (N, V) and out.stride(1) == 1
    check(lib().tavsr_ngram_score(ptr(lm.word), ptr(lm.logp), ptr(lm.backoff), ptr(lm.child_begin), lm.n_unigrams, lm.order,
                                  lm.bos_word, lm.unk_logp, ptr(lm.word_map), ptr(yseq), yseq.stride(0), L,
                                  0 if step_dev is not None else int(step), ptr(step_dev), ptr(cand),
                                  0 if cand is None else cand.shape[1], alpha, add, int(bool(accumulate)), ptr(out), out.stride(0),
                                  N, V, stream()), "tavsr_ngram_score")
    return out


def beam_combine(full, cand, psi, psi_abs, eos_s, eos_abs, s_prev, score, eos, w_ctc):
    """weighted = full + w_ctc * (partial CTC scorer row) + score; fixes psi_abs of <eos> candidates in place (tavsr.h).
    ``psi`` None: no CTC scorer - weighted = full + score, the other CTC operands are not read."""
    N, V = full.shape
    Cn = 0 if psi is None else cand.shape[1]
    require_cuda(full, cand, psi, psi_abs, eos_s, eos_abs, s_prev, score)
    weighted = empty(N, V, like=full)
    check(lib().tavsr_beam_combine(ptr(full), ptr(cand), ptr(psi), ptr(psi_abs), ptr(eos_s), ptr(eos_abs), ptr(s_prev), ptr(score),
                                   ptr(weighted), N, V, Cn, int(eos), w_ctc, stream()), "tavsr_beam_combine")
    return weighted


def beam_combine_topk_ok(K, V) -> bool:
    return K * V <= 8192


def beam_combine_topk(full, cand, psi, psi_abs, eos_s, eos_abs, s_prev, score, eos, w_ctc, K, keep_weighted=False):
    """``beam_combine`` and ``torch.topk(weighted.view(U, K * V), K)`` in one launch -> (top_s, top_i[, weighted]).
    ``psi`` None: no CTC scorer (weighted = full + score)."""
    N, V = full.shape
    Cn = 0 if psi is None else cand.shape[1]
    require_cuda(full, cand, psi, psi_abs, eos_s, eos_abs, s_prev, score)
    top_s = empty(N // K, K, like=full)
    top_i = torch.empty(N // K, K, dtype=torch.int64, device=full.device)
    weighted = empty(N, V, like=full) if keep_weighted else None
    check(lib().tavsr_beam_combine_topk(ptr(full), ptr(cand), ptr(psi), ptr(psi_abs), ptr(eos_s), ptr(eos_abs), ptr(s_prev), ptr(score),
                                        ptr(weighted), ptr(top_s), ptr(top_i), N, K, V, Cn, int(eos), w_ctc, stream()),
          "tavsr_beam_combine_topk")
    return (top_s, top_i, weighted) if keep_weighted else (top_s, top_i)


def beam_select_topk_ok(K, V) -> bool:
    return V <= 64 and K <= 16 and K <= V


def beam_select_topk(dec, z_lm, w_lm, add, psi_all, psi_abs_all, eos_s, eos_abs, s_prev, score, eos, w_ctc, K, Cn, keep=False):
    """the beam update behind the scorers in one launch (tavsr_beam_select_topk; V <= 64): -> (top_s, top_i) or, with ``keep``,
    (top_s, top_i, full, weighted, cand) - the intermediate values the separate launches would have produced.
    ``dec`` None: no decoder term (the row is w_lm * log_softmax(z_lm) + add, or ``add`` alone); ``psi_all`` None: no CTC scorer
    (no pre-beam, weighted = full + score; ``cand`` is then not produced)."""
    like = next(t for t in (dec, z_lm, psi_all) if t is not None)
    N, V = like.shape
    require_cuda(dec, z_lm, psi_all, psi_abs_all, eos_s, eos_abs, s_prev, score)
    assert all(t is None or t.is_contiguous() for t in (dec, z_lm, psi_all, psi_abs_all))
    top_s = empty(N // K, K, like=like)
    top_i = torch.empty(N // K, K, dtype=torch.int64, device=like.device)
    full = empty(N, V, like=like) if keep else None
    weighted = empty(N, V, like=like) if keep else None
    cand = torch.empty(N, Cn, dtype=torch.int64, device=like.device) if keep and psi_all is not None else None
    check(lib().tavsr_beam_select_topk(ptr(dec), ptr(z_lm), w_lm, add, ptr(psi_all), ptr(psi_abs_all), ptr(eos_s), ptr(eos_abs),
                                       ptr(s_prev), ptr(score), ptr(full), ptr(weighted), ptr(cand), ptr(top_s), ptr(top_i), N, K, V,
                                       int(Cn), int(eos), w_ctc, stream()), "tavsr_beam_select_topk")
    return (top_s, top_i, full, weighted, cand) if keep else (top_s, top_i)


def beam_step_begin(score, tok, anc, maxlen, K, eos, step_dev):
    """head of a captured search step (tavsr.h): ended hypotheses leave the beam, anc[:, step] names this step's rows."""
    N = score.numel()
    require_cuda(score, tok, anc, maxlen, step_dev)
    assert anc.dtype == torch.int32 and maxlen.dtype == torch.int32 and tok.dtype == torch.int64 and step_dev.dtype == torch.int32
    check(lib().tavsr_beam_step_begin(ptr(score), ptr(tok), ptr(anc), anc.stride(0), ptr(maxlen), N, K, int(eos), ptr(step_dev),
                                      stream()), "tavsr_beam_step_begin")


def beam_reorder(top_i, top_s, cand, r_new, psi_abs, yseq, anc, outs, K, V, step_dev, hist=None, maxlen=None, eos=0):
    """gathers the state of the extended slots into ``outs`` = (r, s, yseq, anc, tok, score) buffers (tavsr.h).  ``maxlen`` (int32
    [N / K]): the head of the next step rides along (tavsr_beam_reorder_begin).  ``r_new`` None: no CTC state to gather -
    ``cand`` / ``psi_abs`` and the first two of ``outs`` are not used (may be None)."""
    N = yseq.shape[0]
    Cn, T = (0, 0) if r_new is None else (cand.shape[1], r_new.shape[1])
    r_out, s_out, y_out, a_out, t_out, sc_out = outs
    if r_new is None:
        cand = psi_abs = r_out = s_out = None
    require_cuda(top_i, top_s, cand, r_new, psi_abs, yseq, anc, r_out, s_out, y_out, a_out, t_out, sc_out, step_dev, hist)
    assert hist is None or (hist.dtype == torch.int32 and hist.is_contiguous() and hist.shape[1:] == (3, N))
    assert top_i.is_contiguous() and top_s.is_contiguous() and top_i.numel() == N and yseq.dtype == torch.int64
    assert anc.dtype == torch.int32 and y_out.shape == yseq.shape and a_out.shape == anc.shape
    assert r_new is None or (cand.shape[0] == N and r_out.shape == (N, T, 2))
    if maxlen is not None:
        require_cuda(maxlen)
        assert maxlen.dtype == torch.int32 and maxlen.numel() == N // K
        check(lib().tavsr_beam_reorder_begin(ptr(top_i), ptr(top_s), ptr(cand), ptr(r_new), ptr(psi_abs), ptr(yseq), ptr(anc), ptr(r_out),
                                             ptr(s_out), ptr(y_out), ptr(a_out), ptr(t_out), ptr(sc_out), N, K, V, Cn, T, yseq.stride(0),
                                             anc.stride(0), ptr(step_dev), ptr(hist), 0 if hist is None else hist.shape[0],
                                             ptr(maxlen), int(eos), stream()), "tavsr_beam_reorder_begin")
        return
    check(lib().tavsr_beam_reorder(ptr(top_i), ptr(top_s), ptr(cand), ptr(r_new), ptr(psi_abs), ptr(yseq), ptr(anc), ptr(r_out),
                                   ptr(s_out), ptr(y_out), ptr(a_out), ptr(t_out), ptr(sc_out), N, K, V, Cn, T, yseq.stride(0),
                                   anc.stride(0), ptr(step_dev), ptr(hist), 0 if hist is None else hist.shape[0], stream()),
          "tavsr_beam_reorder")


def ctc_beam_search_ok(K, V, T) -> bool:
    """does the one-launch CTC prefix beam search take this (beam, vocabulary, frames)?  K <= V <= 64 and the beam's forward
    variables (16 K T bytes, two LDS buffers) plus a few KB within one workgroup's 160 KiB - the library's answer."""
    return bool(lib().tavsr_ctc_beam_search_ok(int(K), int(V), int(T)))


def ctc_beam_search(logp, lens, maxlen, hist, n_steps, K, sos, eos, w_ctc, add, end_detect, d_end, blank=0):
    """the whole CTC prefix beam search (scorers: CTC prefix scorer + length bonus, no pre-beam) of every utterance in one launch
    (tavsr_ctc_beam_search): logp [U, T, V], lens int64 [U], maxlen int32 [U] -> records in ``hist`` int32 [steps, 3, U * K] and
    the number of tokens searched per utterance in ``n_steps`` int32 [U]."""
    U, T, V = logp.shape
    require_cuda(logp, lens, maxlen, hist, n_steps)
    assert logp.is_contiguous() and logp.dtype == f32 and lens.dtype == torch.int64 and lens.numel() == U
    assert maxlen.dtype == torch.int32 and maxlen.numel() == U and n_steps.dtype == torch.int32 and n_steps.numel() == U
    assert hist.dtype == torch.int32 and hist.is_contiguous() and hist.shape[1:] == (3, U * K)
    check(lib().tavsr_ctc_beam_search(ptr(logp), ptr(lens), ptr(maxlen), ptr(hist), ptr(n_steps), U, int(K), T, V, hist.shape[0],
                                      int(sos), int(eos), int(blank), w_ctc, add, int(bool(end_detect)), d_end, stream()),
          "tavsr_ctc_beam_search")


# ---------------------------------------------------------------------------------------------- time-synchronous search
def timesync_ok(K, V, T, C) -> bool:
    """does the time-synchronous search take this (beam, vocabulary, frames, pre-beam)?  The library's answer (include/tavsr.h)."""
    return bool(lib().tavsr_timesync_ok(int(K), int(V), int(T), int(C)))


def timesync_ws(K, V, T, C):
    """(int32 words of an utterance's workspace, {name: word offset}) of ``tavsr_timesync_*``; raises where the shape is not taken"""
    words = int(lib().tavsr_timesync_ws(int(K), int(V), int(T), int(C)))
    if words <= 0:
        raise L.TavsrError(f"tavsr_timesync: beam {K}, {V} tokens, {T} frames, pre-beam {C} is not supported (tavsr_timesync_ok): "
                         "beam <= 64, the frame's tables within one workgroup's LDS, (3 + beam * frames) * tokens < 2^31")
    names = ("order", "node", "score", "misc", "parent", "token", "nodes", "cand_cap")
    return words, {n: int(lib().tavsr_timesync_ws_offset(int(K), int(V), int(T), int(C), i)) for i, n in enumerate(names)}


def _ts_scorer_ptrs(sc):
    """(tok int64 [N], pos, nkeys int32 [N], anc int32 [N, ld]) or None -> the operands' addresses and ld"""
    if sc is None:
        return (None, None, None, None), 0
    tok, pos, nkeys, anc = sc
    require_cuda(tok, pos, nkeys, anc)
    assert tok.dtype == torch.int64 and pos.dtype == nkeys.dtype == anc.dtype == torch.int32 and anc.is_contiguous()
    return (ptr(tok), ptr(pos), ptr(nkeys), ptr(anc)), anc.stride(0)


def timesync_init(ws, U, K, V, T, Cn, sos, blank=0, scorer=None, frame_dev=None):
    """the state before frame 0 (tavsr_timesync_init); ``scorer`` = (tok, pos, nkeys, anc): slot 0 of every utterance is new"""
    require_cuda(ws)
    assert ws.dtype == torch.int32 and ws.is_contiguous() and ws.shape[0] == U
    ptrs, ld = _ts_scorer_ptrs(scorer)
    check(lib().tavsr_timesync_init(ptr(ws), *ptrs, ld, ptr(frame_dev), U, int(K), V, T, int(Cn), int(sos), int(blank), stream()),
          "tavsr_timesync_init")


def timesync_step(lpz, lens, ws, frame_dev, K, Cn, sos, w_ctc, w_dec, w_lm, pen, dec=None, lm=None, scorer=None, anc_tmp=None, blank=0):
    """one frame of every utterance (tavsr_timesync_step).  ``dec`` / ``lm`` = (new rows, kept rows) [U K, V] or None."""
    U, T, V = lpz.shape
    require_cuda(lpz, lens, ws, frame_dev)
    assert lpz.is_contiguous() and lpz.dtype == f32 and lens.dtype == torch.int64 and frame_dev.dtype == torch.int32
    for pair in (dec, lm):
        assert pair is None or all(t.is_contiguous() and t.shape == (U * K, V) and t.dtype == f32 for t in pair)
    ptrs, ld = _ts_scorer_ptrs(scorer)
    dn, dr = (None, None) if dec is None else dec
    ln, lr = (None, None) if lm is None else lm
    check(lib().tavsr_timesync_step(ptr(lpz), ptr(lens), ptr(ws), ptr(dn), ptr(dr), ptr(ln), ptr(lr), *ptrs, ptr(anc_tmp), ld,
                                    ptr(frame_dev), U, int(K), V, T, int(Cn), int(sos), int(blank), w_ctc, w_dec, w_lm, pen, stream()),
          "tavsr_timesync_step")


def timesync_search(lpz, lens, ws, K, Cn, sos, w_ctc, pen, blank=0):
    """every frame of every utterance in one launch, no scorer rows (tavsr_timesync_search)"""
    U, T, V = lpz.shape
    require_cuda(lpz, lens, ws)
    assert lpz.is_contiguous() and lpz.dtype == f32 and lens.dtype == torch.int64
    check(lib().tavsr_timesync_search(ptr(lpz), ptr(lens), ptr(ws), U, int(K), V, T, int(Cn), int(sos), int(blank), w_ctc, pen, stream()),
          "tavsr_timesync_search")


def tree_attn_rows(q, kpool, vpool, anc, nkeys_row, max_keys, H, dk, k_new, v_new, out=None):
    """``tree_attn_step`` with a key count per row (int32 [N]): a row with 0 keys is skipped and its output row left alone; the row's
    own key / value goes to the pool row its last ancestor entry names (tavsr_tree_attn_rows)"""
    N = q.shape[0]
    require_cuda(q, kpool, vpool, anc, nkeys_row, k_new, v_new)
    assert anc.dtype == torch.int32 and nkeys_row.dtype == torch.int32 and kpool.stride(0) == vpool.stride(0)
    assert k_new.stride(0) == q.stride(0) and v_new.stride(0) == q.stride(0)
    if out is None:
        out = empty(N, H * dk, like=q)
    check(lib().tavsr_tree_attn_rows(ptr(q), q.stride(0), ptr(kpool), ptr(vpool), kpool.stride(0), ptr(anc), anc.stride(0),
                                     ptr(nkeys_row), int(max_keys), ptr(out), out.stride(0), N, H, dk, 1.0 / (dk ** 0.5), ptr(k_new),
                                     ptr(v_new), stream()), "tavsr_tree_attn_rows")
    return out


def embed_pe_rows(ids, table, pe, scale, pos):
    """table[ids] * scale + pe[pos]: ids int64 [N], pos int32 [N] (clamped to pe's rows) -> [N, D] (tavsr_embed_pe_rows)"""
    require_cuda(ids, table, pe, pos)
    N, D = ids.numel(), table.shape[1]
    assert pos.dtype == torch.int32 and pos.numel() == N and pe.is_contiguous() and pe.shape[1] == D and table.is_contiguous()
    out = empty(N, D, like=table)
    check(lib().tavsr_embed_pe_rows(ptr(ids), ptr(table), ptr(pe), scale, ptr(out), N, pe.shape[0], D, ptr(pos), stream()),
          "tavsr_embed_pe_rows")
    return out


# ---------------------------------------------------------------------------------------------- transducer beam searches (csrc/rnnt_search.hip)
def rnnt_search_ok(kind, K, V, T, u_max=50, max_sym_exp=2) -> bool:
    """does the transducer beam search ``kind`` ("alsd" / "tsd") take this shape?  The library's answer (include/tavsr.h)."""
    return bool(lib().tavsr_rnnt_search_ok(ops.RNNT_SEARCH_KINDS[kind], int(K), int(V), int(T), int(u_max), int(max_sym_exp)))


def rnnt_search_ws(kind, K, V, T, u_max=50, max_sym_exp=2):
    """(int32 words of an utterance's block, {name: word offset or bound}) of ``tavsr_rnnt_search_*``; ValueError where the shape
    is not taken, before anything is launched"""
    if not rnnt_search_ok(kind, K, V, T, u_max, max_sym_exp):
        raise ValueError(f"transducer {kind} search: beam {K}, {V} tokens, {T} frames, u_max {u_max}, max_sym_exp {max_sym_exp} is not "
                         f"supported (tavsr_rnnt_search_ok): {ops.RNNT_SEARCH_LIMIT}")
    args = (ops.RNNT_SEARCH_KINDS[kind], int(K), int(T), int(u_max), int(max_sym_exp))
    names = ("node", "score", "len", "parent", "token", "list_node", "list_score", "nodes", "list")
    return int(lib().tavsr_rnnt_search_ws(*args)), {n: int(lib().tavsr_rnnt_search_ws_offset(*args, i)) for i, n in enumerate(names)}


def rnnt_search_init(kind, ws, tlens, row_t, K, V, T, u_max=50, max_sym_exp=2):
    """the state before the first step of every utterance (tavsr_rnnt_search_init)"""
    _i32(ws, row_t)
    U = ws.shape[0]
    assert tlens.dtype == torch.int64 and tlens.is_cuda and tlens.shape == (U,) and row_t.numel() == U * K
    check(lib().tavsr_rnnt_search_init(ptr(ws), ptr(tlens), ptr(row_t), U, ops.RNNT_SEARCH_KINDS[kind], int(K), int(V), int(T), int(u_max),
                                       int(max_sym_exp), stream()), "tavsr_rnnt_search_init")


def rnnt_search_z(e, d, row_t, K, out=None):
    """z [N, J] = tanh(e[n // K, row_t[n]] + d[n]); rows with row_t < 0 are 0 (tavsr_rnnt_search_z)"""
    U, T, J = e.shape
    _i32(row_t)
    require_cuda(e, d)
    assert e.is_contiguous() and d.is_contiguous() and d.shape == (U * K, J) and row_t.numel() == U * K
    out = empty(U * K, J, like=e) if out is None else out
    check(lib().tavsr_rnnt_search_z(ptr(e), ptr(d), ptr(row_t), ptr(out), U * K, int(K), T, J, stream()), "tavsr_rnnt_search_z")
    return out


def rnnt_row_topk(logits, K, row_t=None, out=None):
    """logits [N, V] -> (lp_blank [N], topv [N, K], topi int32 [N, K]): the log-softmax's blank and its K best labels, the lower
    id first among equals; rows with row_t < 0 are left alone (tavsr_rnnt_row_topk)"""
    N, V = logits.shape
    require_cuda(logits, row_t)
    assert logits.stride(1) == 1 and logits.dtype == f32 and (row_t is None or (row_t.dtype == torch.int32 and row_t.numel() == N))
    lpb, topv, topi = (empty(N, like=logits), empty(N, K, like=logits), torch.empty((N, K), dtype=torch.int32, device=logits.device)) \
        if out is None else out
    check(lib().tavsr_rnnt_row_topk(ptr(logits), logits.stride(0), ptr(row_t), ptr(lpb), ptr(topv), ptr(topi), N, V, int(K), stream()),
          "tavsr_rnnt_row_topk")
    return lpb, topv, topi


def rnnt_gather_state(src, idx, dst):
    """dst (h, c) [L, Nd, H] row n = src (h, c) [L, Ns, H] row idx[n]; idx[n] < 0 leaves the row alone (tavsr_rnnt_gather_state)"""
    (sh, sc), (dh, dc) = src, dst
    _i32(idx)
    require_cuda(sh, sc, dh, dc)
    Ln, Ns, H = sh.shape
    Nd = dh.shape[1]
    assert all(t.is_contiguous() and t.dtype == f32 for t in (sh, sc, dh, dc)) and sc.shape == sh.shape and dc.shape == dh.shape
    assert dh.shape == (Ln, Nd, H) and idx.numel() == Nd
    check(lib().tavsr_rnnt_gather_state(ptr(sh), ptr(sc), ptr(idx), ptr(dh), ptr(dc), Ln, Ns, Nd, H, stream()), "tavsr_rnnt_gather_state")


def _rnnt_step_check(ws, tlens, lpb, topv, topi, row_t, parent, tok, commit):
    _i32(ws, topi, row_t, parent)
    require_cuda(tlens, lpb, topv, tok, commit)
    U, (N, K) = ws.shape[0], topv.shape
    assert N == U * K and tlens.dtype == torch.int64 and tok.dtype == torch.int64 and commit.dtype == torch.uint8
    assert lpb.is_contiguous() and topv.is_contiguous() and all(t.numel() == N for t in (lpb, row_t, parent, tok, commit))
    return U, K


def rnnt_alsd_step(ws, tlens, lpb, topv, topi, row_t, parent, tok, commit, V, T, u_max):
    """one value of i of ALSD for every utterance (tavsr_rnnt_alsd_step); ws, row_t, parent, tok, commit are updated in place"""
    U, K = _rnnt_step_check(ws, tlens, lpb, topv, topi, row_t, parent, tok, commit)
    check(lib().tavsr_rnnt_alsd_step(ptr(ws), ptr(tlens), ptr(lpb), ptr(topv), ptr(topi), ptr(row_t), ptr(parent), ptr(tok), ptr(commit),
                                     U, K, int(V), int(T), int(u_max), stream()), "tavsr_rnnt_alsd_step")


def rnnt_tsd_step(ws, tlens, lpb, topv, topi, row_t, parent, tok, commit, a_src, b_sel, v, V, T, max_sym_exp):
    """expansion ``v`` of the current frame of TSD for every utterance (tavsr_rnnt_tsd_step)"""
    U, K = _rnnt_step_check(ws, tlens, lpb, topv, topi, row_t, parent, tok, commit)
    _i32(a_src, b_sel)
    assert a_src.numel() == U * K * max_sym_exp and b_sel.numel() == U * K
    check(lib().tavsr_rnnt_tsd_step(ptr(ws), ptr(tlens), ptr(lpb), ptr(topv), ptr(topi), ptr(row_t), ptr(parent), ptr(tok), ptr(commit),
                                    ptr(a_src), ptr(b_sel), int(v), U, K, int(V), int(T), int(max_sym_exp), stream()), "tavsr_rnnt_tsd_step")
