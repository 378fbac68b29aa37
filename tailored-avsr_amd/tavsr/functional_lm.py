"""``TransformerLMFn`` - the Transformer language model's teacher-forced forward with a hand-written backward, as ONE autograd
node (espnet2 lm/transformer_lm.py TransformerLM.forward over espnet's ``Encoder(input_layer="linear", pos_enc: null)``; trained
through lm_main.py:22-43).  It is ``functional.TransformerDecoderFn`` without the source attention: the same kernels in the same
order (grouped q | k | v projections, the fused attention core where dk == 64, ``_FFN``, one ``LNGroup`` and one ``WgradGroup``
per backward pass), in front of it the LM's own input layer - embedding rows, Linear, LayerNorm, Dropout, ReLU."""
from __future__ import annotations

from typing import List, Optional

import torch

from . import ops
from ._lib import guarded
from .functional import _DEC_WGRAD, _note_ctx
from .layer_blocks import EPS_ESPNET, _AttnFused, _drop_, _drop_bwd, _drop_bwd_, _FFN, _SelfAttnCore

LM_LAYER_PARAM_NAMES = (
    "norm1.weight", "norm1.bias",
    "self_attn.linear_q.weight", "self_attn.linear_q.bias", "self_attn.linear_k.weight", "self_attn.linear_k.bias",
    "self_attn.linear_v.weight", "self_attn.linear_v.bias", "self_attn.linear_out.weight", "self_attn.linear_out.bias",
    "norm2.weight", "norm2.bias",
    "feed_forward.w_1.weight", "feed_forward.w_1.bias", "feed_forward.w_2.weight", "feed_forward.w_2.bias",
)
_NL = len(LM_LAYER_PARAM_NAMES)
_LI = {n: i for i, n in enumerate(LM_LAYER_PARAM_NAMES)}
_HEAD = 5      # embed.weight, encoder.embed.0.weight / .bias, encoder.embed.1.weight / .bias


class TransformerLMFn(torch.autograd.Function):
    """P = [embed.weight, encoder.embed.0.weight, .bias, encoder.embed.1.weight, .bias, (16 per layer) x layer,
    encoder.after_norm.weight, .bias, decoder.weight, decoder.bias];  ids [B, L] int64, lens [B] int64 (keys of row b beyond
    lens[b] are masked; with the padding at the tail and a causal mask that is espnet's ``ids != 0`` key mask for every row
    below lens[b]) -> logits [B, L, V].  cfg: heads, num_blocks, p (dropout rate, training only)."""

    @staticmethod
    def forward(ctx, ids, lens, cfg, *P):
        need = _note_ctx(ctx)
        B, L = ids.shape
        H, nb = cfg["heads"], cfg["num_blocks"]
        pd = cfg.get("p", 0.0)
        D = P[1].shape[0]
        dk = D // H
        M = B * L
        ids = ids.contiguous()
        e = P[0][ids.view(-1)]                                      # embedding row gather (index plumbing)
        # espnet input_layer="linear": Linear, LayerNorm, Dropout, ReLU (pos_enc: null is an identity)
        h0 = ops.linear(e, P[1], P[2])
        x, m0, r0 = ops.layernorm_fwd(h0, P[3], P[4], EPS_ESPNET)
        t_emb = _drop_(x, pd)
        ops.act_(x, "relu")
        x_in = x
        saved = []
        for li in range(nb):
            p = lambda n, li=li: P[_HEAD + li * _NL + _LI[n]]
            s = {}
            n1, m1, r1 = ops.layernorm_fwd(x, p("norm1.weight"), p("norm1.bias"), EPS_ESPNET)
            qkv = ops.empty(M, 3 * D, like=x)
            ops.linear_group(n1, [(p(f"self_attn.linear_{c}.weight"), p(f"self_attn.linear_{c}.bias"), j * D)
                                  for j, c in enumerate("qkv")], qkv)
            if ops.ATTN_FUSED and dk == 64:
                tk_a = "fused"
                cx, attn = _AttnFused.fwd(qkv, 0, qkv, D, qkv, 2 * D, B, L, L, H, dk, lens, True)
            else:      # (attention dropout is 0: espnet2's TransformerLM leaves the encoder's attention_dropout_rate at its default)
                cx, attn, tk_a = _SelfAttnCore.fwd(qkv, 3 * D, 0, qkv, 3 * D, D, qkv, 3 * D, 2 * D, B, L, L, H, dk, lens, True)
            x1, tk_r = ops.linear_drop(cx, p("self_attn.linear_out.weight"), p("self_attn.linear_out.bias"), pd, res=x)
            s["self"] = (x, m1, r1, n1, qkv, cx, attn, tk_a, tk_r)
            x, s["ff"] = _FFN.fwd(x1, p("norm2.weight"), p("norm2.bias"), p("feed_forward.w_1.weight"), p("feed_forward.w_1.bias"),
                                  p("feed_forward.w_2.weight"), p("feed_forward.w_2.bias"), "relu", 1.0, p=pd, save=need)
            saved.append(s)
        an_w, an_b, out_w, out_b = P[_HEAD + nb * _NL: _HEAD + nb * _NL + 4]
        xn, mf, rf = ops.layernorm_fwd(x, an_w, an_b, EPS_ESPNET)
        logits = ops.linear(xn, out_w, out_b)
        if need:
            ctx.saved, ctx.final, ctx.head = saved, (x, mf, rf, xn), (e, h0, m0, r0, x_in, t_emb)
            ctx.P, ctx.dims, ctx.ids, ctx.lens = P, (B, L, D, H, dk, nb), ids, lens
        return logits.view(B, L, -1)

    @staticmethod
    @guarded
    def backward(ctx, dlogits):
        P = ctx.P
        B, L, D, H, dk, nb = ctx.dims
        M = B * L
        G: List[Optional[torch.Tensor]] = [None] * len(P)
        an_i = _HEAD + nb * _NL
        an_w, an_b, out_w, out_b = P[an_i: an_i + 4]
        x, mf, rf, xn = ctx.final
        dl = dlogits.contiguous().view(M, -1)
        G[an_i + 2], G[an_i + 3] = ops.linear_dw(dl, xn, bias_grad=True)
        dxn = ops.linear_dx(dl, out_w)
        lng = ops.LNGroup(cap=2 * nb + 2)     # all LayerNorms of the model: one (dgamma, dbeta) reduction at the end
        dx, G[an_i], G[an_i + 1], *dyd = lng.bwd(dxn, x, mf, rf, an_w, drop=ctx.saved[nb - 1]["ff"][-1] if nb else None)
        grp = ops.WgradGroup()                # the weight gradients in grouped launches, flushed as the decoder's are
        beside = ops.wgrad_may_go_beside(P)
        for li in reversed(range(nb)):
            base = _HEAD + li * _NL
            p = lambda n, base=base: P[base + _LI[n]]

            def put(n, g, base=base):
                G[base + _LI[n]] = g

            s = ctx.saved[li]
            x0, m1, r1, n1, qkv, cx, attn, tk_a, tk_r = s["self"]
            dx1, gs, *dt1 = _FFN.bwd(dx, s["ff"], p("norm2.weight"), p("feed_forward.w_1.weight"), p("feed_forward.w_2.weight"),
                                     "relu", 1.0, grp=grp, lng=lng, dyd=dyd[0] if dyd else None, out_drop=tk_r)
            for n_, g in zip(("norm2.weight", "norm2.bias", "feed_forward.w_1.weight", "feed_forward.w_1.bias",
                              "feed_forward.w_2.weight", "feed_forward.w_2.bias"), gs):
                put(n_, g)
            dt1 = dt1[0] if dt1 else _drop_bwd(dx1, tk_r)
            gw_, gb_ = grp.add(dt1, cx, bias_grad=True)
            put("self_attn.linear_out.weight", gw_); put("self_attn.linear_out.bias", gb_)
            dcx = ops.linear_dx(dt1, p("self_attn.linear_out.weight"))
            dqkv = torch.empty_like(qkv)
            if tk_a == "fused":
                _AttnFused.bwd(dcx, cx, attn, qkv, 0, qkv, D, qkv, 2 * D, dqkv, 0, dqkv, D, dqkv, 2 * D, B, L, L, H, dk, ctx.lens, True)
            else:
                _SelfAttnCore.bwd(dcx, attn, qkv, 3 * D, 0, qkv, 3 * D, D, qkv, 3 * D, 2 * D, dqkv, 3 * D, 0, dqkv, 3 * D, D,
                                  dqkv, 3 * D, 2 * D, B, L, L, H, dk, tok=tk_a)
            for j, nm in enumerate(("q", "k", "v")):
                gw_, gb_ = grp.add(dqkv[:, j * D:(j + 1) * D], n1, bias_grad=True)
                put(f"self_attn.linear_{nm}.weight", gw_); put(f"self_attn.linear_{nm}.bias", gb_)
            dn1 = ops.linear_dx_cat(dqkv, [p(f"self_attn.linear_{c}.weight") for c in "qkv"])
            dx, g1, g2, *dyd = lng.bwd(dn1, x0, m1, r1, p("norm1.weight"), dx_add=dx1,
                                       drop=ctx.saved[li - 1]["ff"][-1] if li else None)
            put("norm1.weight", g1); put("norm1.bias", g2)
            if beside and li and (nb - li) % _DEC_WGRAD == 0:
                ops.wgrad_beside(grp.flush)
        # the input layer, backwards: ReLU, Dropout, LayerNorm, Linear, embedding rows
        e, h0, m0, r0, x_in, t_emb = ctx.head
        ops.act_bwd_(dx, x_in, "relu")        # (x_in = relu(.): positive exactly where its pre-activation was)
        _drop_bwd_(dx, t_emb)
        dh0, G[3], G[4] = lng.bwd(dx, h0, m0, r0, P[3])
        G[1], G[2] = grp.add(dh0, e, bias_grad=True)
        de = ops.linear_dx(dh0, P[1])
        grp.flush()
        lng.flush()
        G[0] = ops.embed_bwd(ctx.ids, de, 1.0, P[0].shape[0])
        ctx.saved = ctx.final = ctx.head = None
        return (None, None, None, *G)
