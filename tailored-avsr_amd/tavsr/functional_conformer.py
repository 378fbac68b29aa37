"""The Conformer encoder layer as one autograd node (espnet/nets/pytorch_backend/conformer/encoder_layer.py, EncoderLayer.forward
with ``normalize_before=True``, ``concat_after=False`` and no stochastic depth):

    if macaron:  x = x + ff_scale * drop(feed_forward_macaron(norm_ff_macaron(x)))
    x = x + drop(self_attn(norm_mha(x), pos_emb, mask))
    if conv:     x = x + drop(conv_module(norm_conv(x)))
    x = x + ff_scale * drop(feed_forward(norm_ff(x)));   if conv: x = norm_final(x)
    ff_scale = 0.5 with the macaron block, else 1.0

Sequenced from the blocks of ``tavsr.layer_blocks`` (feed-forward, relative-position attention branch, convolution module) with the
layer's weight gradients in one grouped launch and its LayerNorm gradients in one reduction, as ``BranchformerLayerFn``.  The
blocks follow one another, so nothing forks; the weight-gradient group may go beside the next layer's chain.  The layer has a
parameter list of its own (``CONFORMER_PARAM_NAMES``): the Branchformer lists and the C-side layer sequencer are not involved.
"""
from __future__ import annotations

import torch

from . import ops
from ._lib import guarded
from . import functional as F_      # (_POS_DW_BESIDE is read there at call time)
from .functional import _note_ctx
from .layer_blocks import CONV_PARAMS, EPS_ESPNET, FF_PARAMS, FFM_PARAMS, AttnBranch, ConvModuleBlock, _drop_bwd, _FFN

_ATTN = ("linear_q.weight", "linear_q.bias", "linear_k.weight", "linear_k.bias", "linear_v.weight", "linear_v.bias",
         "linear_out.weight", "linear_out.bias", "linear_pos.weight", "pos_bias_u", "pos_bias_v")
# parameter order of ConformerLayerFn (None entries for an absent macaron block / convolution module)
CONFORMER_PARAM_NAMES = (*FFM_PARAMS, "norm_mha.weight", "norm_mha.bias", *("self_attn." + n for n in _ATTN),
                         "norm_conv.weight", "norm_conv.bias", *CONV_PARAMS, *FF_PARAMS, "norm_final.weight", "norm_final.bias")
# AttnBranch reads and fills its parameters under the Branchformer layer's attribute name
_ALIAS = {"self_attn." + n: "attn." + n for n in _ATTN}


def _params(P):
    p = dict(zip(CONFORMER_PARAM_NAMES, P))
    p.update((a, p[n]) for n, a in _ALIAS.items())
    return p


def _eval_bn_refusal():
    """eval-mode BatchNorm backward (constant statistics) is not exposed by the C ABI and not on any reference path: refused, as
    in the lip front-end (functional_av._bn_eval_bwd)"""
    return NotImplementedError("backward through eval-mode BatchNorm (Conformer conv_module.norm) is not on the HIP path: "
                               "validation runs under torch.no_grad()")


class ConvModuleFn(torch.autograd.Function):
    """``ConvolutionModule.forward`` alone (espnet conformer/convolution.py): x [B, T, C] -> [B, T, C]; ``P`` in CONV_PARAMS order,
    ``cfg``: act, training, bn."""

    @staticmethod
    def forward(ctx, x, cfg, *P):
        _note_ctx(ctx)
        B, T, D = x.shape
        p = dict(zip(CONV_PARAMS, P))
        y, ctx.sv = ConvModuleBlock.fwd(x.reshape(B * T, D), None, None, p, cfg["bn"], B, T, cfg["act"], cfg["training"])
        ctx.cfg, ctx.P, ctx.shape = cfg, P, (B, T, D)
        return y.view(B, T, D)

    @staticmethod
    @guarded
    def backward(ctx, dy):
        if not ctx.cfg["training"]:
            raise _eval_bn_refusal()
        B, T, D = ctx.shape
        p, G, grp = dict(zip(CONV_PARAMS, ctx.P)), {}, ops.WgradGroup()
        dy = dy.contiguous().view(B * T, D)
        dx, _, _ = ConvModuleBlock.bwd(dy, ctx.sv, None, p, B, T, ctx.cfg["act"], grp, None, G, dyd=dy)
        grp.flush()
        ctx.sv = None
        return (dx.view(B, T, D), None, *[G[n] for n in CONV_PARAMS])


class ConformerLayerFn(torch.autograd.Function):
    """``cfg``: heads, ffn_act, conv_act (the convolution module's; ffn_act when absent), p / p_att (0 in eval), training, and ``bn`` =
    the convolution module's (running_mean, running_var, num_batches_tracked) or None without the module."""

    @staticmethod
    def forward(ctx, x, pos_emb, lens, cfg, *P):
        need = _note_ctx(ctx)
        p = _params(P)
        pd, act, training = cfg.get("p", 0.0), cfg["ffn_act"], cfg["training"]
        macaron, conv = p[FFM_PARAMS[2]] is not None, p[CONV_PARAMS[0]] is not None
        B, T, D = x.shape
        M = B * T
        ffs = 0.5 if macaron else 1.0
        sv = {}
        mha = (p["norm_mha.weight"], p["norm_mha.bias"])
        if macaron:      # the macaron block's finishing launch also normalises its output for the attention
            x1, sv["ffm"], (n1,), mean1, rstd1 = _FFN.fwd_ln(x.reshape(M, D), *[p[k] for k in FFM_PARAMS], act, ffs, [mha], p=pd, save=need)
        else:
            x1, sv["ffm"] = x.reshape(M, D), None
            n1, mean1, rstd1 = ops.layernorm_fwd(x1, *mha, EPS_ESPNET)
        cx, s = AttnBranch.fwd(n1, p, pos_emb, lens, B, T, cfg["heads"], cfg.get("p_att", 0.0))
        x2, t_att = ops.linear_drop(cx, p["attn.linear_out.weight"], p["attn.linear_out.bias"], pd, res=x1)
        sv["attn"] = s._replace(mean=mean1, rstd=rstd1, t_br=t_att)
        if conv:
            x3, sv["conv"] = ConvModuleBlock.fwd(x2, p["norm_conv.weight"], p["norm_conv.bias"], p, cfg["bn"], B, T,
                                                 cfg.get("conv_act") or act, training, pd)
            x4, sv["ff"], (y,), fmean, frstd = _FFN.fwd_ln(x3, *[p[k] for k in FF_PARAMS], act, ffs,
                                                           [(p["norm_final.weight"], p["norm_final.bias"])], p=pd, save=need)
            sv["final"] = (x4, fmean, frstd)
        else:
            sv["conv"] = sv["final"] = None
            y, sv["ff"] = _FFN.fwd(x2, *[p[k] for k in FF_PARAMS], act, ffs, p=pd, save=need)
        sv["x1"] = x1
        ctx.sv, ctx.cfg, ctx.P, ctx.lens, ctx.pos_emb = sv, cfg, P, lens, pos_emb
        ctx.shape = (B, T, D)
        return y.view(B, T, D)

    @staticmethod
    @guarded
    def backward(ctx, dy):
        sv, cfg, P = ctx.sv, ctx.cfg, ctx.P
        if sv["conv"] is not None and not cfg["training"]:
            raise _eval_bn_refusal()
        B, T, D = ctx.shape
        p = _params(P)
        act = cfg["ffn_act"]
        ffs = 0.5 if sv["ffm"] is not None else 1.0
        G = {}
        beside = ops.wgrad_may_go_beside(P)
        grp = ops.WgradGroup()     # every weight gradient of the layer in one grouped launch (flushed at the end)
        lng = ops.LNGroup()        # ... and the LayerNorms' (dgamma, dbeta) partials in one reduction
        sa, sc = sv["attn"], sv["conv"]
        dy = dy.contiguous().view(B * T, D)
        # each LayerNorm backward whose dx the next block's dropout mask is applied to also writes the masked copy
        dyd = []
        if sc is not None:
            x4, fmean, frstd = sv["final"]
            dy, G["norm_final.weight"], G["norm_final.bias"], *dyd = lng.bwd(dy, x4, fmean, frstd, p["norm_final.weight"],
                                                                            drop=sv["ff"].t_out)
        dx3, gs, *dxd = _FFN.bwd(dy, sv["ff"], p["norm_ff.weight"], p["feed_forward.w_1.weight"], p["feed_forward.w_2.weight"], act, ffs,
                                 grp=grp, lng=lng, dyd=dyd[0] if dyd else None, out_drop=sc.t_out if sc is not None else sa.t_br)
        G.update(zip(FF_PARAMS, gs))
        if sc is not None:
            dx2, G["norm_conv.weight"], G["norm_conv.bias"], *dxd = ConvModuleBlock.bwd(
                dx3, sc, p["norm_conv.weight"], p, B, T, cfg.get("conv_act") or act, grp, lng, G, dyd=dxd[0] if dxd else None,
                out_drop=sa.t_br)
        else:
            dx2 = dx3
        dxa = dxd[0] if dxd else _drop_bwd(dx2, sa.t_br)      # under the attention output's mask
        dn, late = AttnBranch.bwd(dxa, sa, p, ctx.pos_emb, ctx.lens, B, T, cfg["heads"], grp, G, lazy=beside and F_._POS_DW_BESIDE)
        t_ffm = sv["ffm"].t_out if sv["ffm"] is not None else None
        dx1, G["norm_mha.weight"], G["norm_mha.bias"], *dyd = lng.bwd(dn, sv["x1"], sa.mean, sa.rstd, p["norm_mha.weight"], dx_add=dx2,
                                                                      drop=t_ffm)
        if sv["ffm"] is not None:
            dx, gs = _FFN.bwd(dx1, sv["ffm"], p["norm_ff_macaron.weight"], p["feed_forward_macaron.w_1.weight"],
                              p["feed_forward_macaron.w_2.weight"], act, ffs, grp=grp, lng=lng, dyd=dyd[0] if dyd else None)
            G.update(zip(FFM_PARAMS, gs))
        else:
            dx = dx1
        if beside:       # no reader before the end of the pass: beside the next layer's chain (the positional chain first)
            ops.wgrad_beside(lambda: ([f() for f in late], grp.flush(), lng.flush()))
        else:
            for f in late:
                f()
            grp.flush()
            lng.flush()
        ctx.sv = None
        grads = [None if prm is None else G.get(_ALIAS.get(n, n)) for n, prm in zip(CONFORMER_PARAM_NAMES, P)]
        return (dx.view(B, T, D), None, None, None, *grads)
