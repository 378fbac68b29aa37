"""The transducer's two autograd nodes, hand-written forward and backward over csrc/rnnt.hip:

``TransducerDecoderFn`` - espnet2 asr/decoder/transducer_decoder.py TransducerDecoder.forward: embedding rows, dropout, a stack
of one-layer LSTMs with a dropout behind each, run over the full label length as espnet runs it.
``RNNTLossFn`` - espnet2 asr_transducer/joint_network.py JointNetwork.forward over every lattice node followed by
warp-transducer's RNNTLoss(blank, reduction="mean", fastemit_lambda=0) (src/models/espnet_model.py:125-129, 614-633): the joint
tensor [B, T, U+1, V] goes through in bounded chunks, forward and backward.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from . import ops
from ._lib import guarded
from .functional import _note_ctx
from .layer_blocks import _drop_, _drop_bwd_

LSTM_LAYER_PARAM_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


class TransducerDecoderFn(torch.autograd.Function):
    """P = [embed.weight, (weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0) x layers]; labels [B, U1] int64 ->
    dec_out [B, U1, H].  cfg: layers, pad (the embedding's padding row: no gradient), p_embed, p (dropout rates, training only).
    The initial states are zeros (espnet init_state)."""

    @staticmethod
    def forward(ctx, labels, cfg, *P):
        need = _note_ctx(ctx)
        B, U1 = labels.shape
        labels = labels.contiguous()
        x = P[0][labels.view(-1)].view(B, U1, -1)                   # embedding row gather (index plumbing)
        t_emb = _drop_(x, cfg.get("p_embed", 0.0))
        saved = []
        for li in range(cfg["layers"]):
            w_ih, w_hh, b_ih, b_hh = P[1 + 4 * li: 5 + 4 * li]
            y, _, _, sv = ops.lstm_fwd(x, w_ih, w_hh, b_ih, b_hh, save=need)
            tok = _drop_(y, cfg.get("p", 0.0))
            saved.append((sv, tok))
            x = y
        if need:
            ctx.saved, ctx.P, ctx.cfg, ctx.labels, ctx.t_emb = saved, P, cfg, labels, t_emb
        return x

    @staticmethod
    @guarded
    def backward(ctx, dy):
        P, cfg = ctx.P, ctx.cfg
        G: List[Optional[torch.Tensor]] = [None] * len(P)
        dy = dy.contiguous()
        if cfg.get("p", 0.0) > 0.0:
            dy = dy.clone()                                         # (the masks are applied in place)
        for li in reversed(range(cfg["layers"])):
            w_ih, w_hh = P[1 + 4 * li], P[2 + 4 * li]
            sv, tok = ctx.saved[li]
            _drop_bwd_(dy, tok)
            dy, G[1 + 4 * li], G[2 + 4 * li], db, _, _ = ops.lstm_bwd(dy, sv, w_ih, w_hh)
            G[3 + 4 * li], G[4 + 4 * li] = db, db.clone()         # (two parameters never share a gradient tensor)
        _drop_bwd_(dy, ctx.t_emb)
        V, E = P[0].shape
        ge = ops.embed_bwd(ctx.labels.view(-1), dy.view(-1, E), 1.0, V)
        pad = cfg.get("pad", None)
        if pad is not None and pad >= 0:
            ops.fill_(ge[pad], 0.0)
        G[0] = ge
        ctx.saved = None
        return (None, None, *G)


class RNNTLossFn(torch.autograd.Function):
    """(enc [B, T, De], dec [B, U1, Dd], t_len, u_len int64 [B], target int32 [B, U], cfg, lin_enc.weight, lin_enc.bias,
    lin_dec.weight, lin_out.weight, lin_out.bias) -> loss = sum_b nll[b] / B (0-dim).  cfg: blank, chunk (lattice rows per
    chunk; None: as many as fit ops.RNNT_WS_FLOATS), route (lattice route, tests).  Rows of ``enc`` at t >= t_len[b] and of ``dec``
    at u > u_len[b] are never multiplied: they may hold anything and get a zero gradient."""

    @staticmethod
    def forward(ctx, enc, dec, t_len, u_len, target, cfg, w_enc, b_enc, w_dec, w_out, b_out):
        need = _note_ctx(ctx)
        B, T, De = enc.shape
        U1, Dd = dec.shape[1], dec.shape[2]
        blank, chunk = cfg.get("blank", 0), cfg.get("chunk", None)
        encm = ops.rnnt_mask_rows(enc.contiguous(), t_len, 0).view(B * T, De)
        decm = ops.rnnt_mask_rows(dec.contiguous(), u_len, 1).view(B * U1, Dd)
        e = ops.linear(encm, w_enc, b_enc).view(B, T, -1)
        d = ops.linear(decm, w_dec).view(B, U1, -1)
        nll, (lse, occ, pb, pl) = ops.rnnt_loss(e, d, w_out, b_out, target, t_len, u_len, blank, chunk, cfg.get("route", None))
        if need:
            ctx.saved = (encm, decm, e, d, lse, occ, pb, pl, t_len, u_len, target, w_enc, w_dec, w_out, b_out)
            ctx.cfg, ctx.dims = cfg, (B, T, U1)
        return ops.colsum(nll.view(B, 1), scale=1.0 / B).view(())

    @staticmethod
    @guarded
    def backward(ctx, dl):
        encm, decm, e, d, lse, occ, pb, pl, t_len, u_len, target, w_enc, w_dec, w_out, b_out = ctx.saved
        B, T, U1 = ctx.dims
        de, dd, g_wout, g_bout = ops.rnnt_joint_grad(e, d, w_out, b_out, target, t_len, u_len, lse, occ, pb, pl,
                                                     dl.reshape(1).contiguous(), 1.0 / B, ctx.cfg.get("blank", 0), ctx.cfg.get("chunk", None))
        de2, dd2 = de.view(B * T, -1), dd.view(B * U1, -1)
        denc = ops.linear_dx(de2, w_enc).view(B, T, -1)
        g_wenc, g_benc = ops.linear_dw(de2, encm, bias_grad=True)
        ddec = ops.linear_dx(dd2, w_dec).view(B, U1, -1)
        g_wdec = ops.linear_dw(dd2, decm)
        ctx.saved = None
        return denc, ddec, None, None, None, None, g_wenc, g_benc, g_wdec, g_wout, g_bout
