"""``EBranchformerEncoderLayer`` - espnet2/asr/encoder/e_branchformer_encoder.py (Kim et al., "E-Branchformer", SLT 2022).

    if macaron:  x = x + ff_scale * drop(feed_forward_macaron(norm_ff_macaron(x)))
    x1 = drop(attn(norm_mha(x), ..., pos_emb, mask));  x2 = drop(cgmlp((norm_mlp(x), pos_emb), mask))
    c  = cat([x1, x2], -1)
    x  = x + drop(merge_proj(c + depthwise_conv_fusion(c^T)^T))
    if feed_forward:  x = x + ff_scale * drop(feed_forward(norm_ff(x)))
    x  = norm_final(x)

Same constructor, parameter names and forward signature as espnet's class; forward and backward are one autograd node
(``tavsr.functional.BranchformerLayerFn`` with the ``dwconv`` merge: the Branchformer layer's blocks around
``tavsr_dwconv_add_fwd / _bwd``).  Nothing masks ``c``: padded frames hold what the two branches computed there and the last
``(k-1)//2`` valid frames of a short utterance read them, as in espnet.
"""
from __future__ import annotations

from typing import Optional

import torch

from ... import functional as F_
from ...layers import LayerNorm


class EBranchformerEncoderLayer(torch.nn.Module):
    def __init__(self, size: int, attn: torch.nn.Module, cgmlp: torch.nn.Module, feed_forward: Optional[torch.nn.Module],
                 feed_forward_macaron: Optional[torch.nn.Module], dropout_rate: float, merge_conv_kernel: int = 3):
        super().__init__()
        if attn is None or cgmlp is None:
            raise ValueError("EBranchformerEncoderLayer needs both branches: attn and cgmlp")
        if merge_conv_kernel < 1 or merge_conv_kernel % 2 == 0:
            raise ValueError(f"merge_conv_kernel must be odd (cat + depthwise_conv_fusion(cat) needs equal lengths): {merge_conv_kernel}")
        if merge_conv_kernel > 31:
            raise ValueError(f"merge_conv_kernel: at most 31 on the HIP path (tavsr_dwconv_add_ok): {merge_conv_kernel}")
        self.size = size
        self.attn, self.cgmlp = attn, cgmlp
        self.feed_forward, self.feed_forward_macaron = feed_forward, feed_forward_macaron
        self.ff_scale = 1.0
        if feed_forward is not None:
            self.norm_ff = LayerNorm(size)
        if feed_forward_macaron is not None:
            self.ff_scale = 0.5
            self.norm_ff_macaron = LayerNorm(size)
        self.norm_mha = LayerNorm(size)
        self.norm_mlp = LayerNorm(size)
        self.norm_final = LayerNorm(size)
        self.dropout_rate = dropout_rate
        self.merge_conv_kernel = merge_conv_kernel
        self.depthwise_conv_fusion = torch.nn.Conv1d(size + size, size + size, kernel_size=merge_conv_kernel, stride=1,
                                                     padding=(merge_conv_kernel - 1) // 2, groups=size + size, bias=True)
        self.merge_proj = torch.nn.Linear(size + size, size)

    def _params(self):
        from ..._lib import cached_params
        return cached_params(self, F_.EBF_PARAM_NAMES)

    def forward(self, x_input, mask, cache=None, lens: Optional[torch.Tensor] = None):
        """x_input: (x[B,T,size], pos_emb[1,2T-1,size]); mask: (B,1,T) bool prefix mask; ``lens`` (int64 [B]) may be supplied by
        the encoder instead of being recomputed from the mask."""
        if cache is not None:
            raise NotImplementedError("cache is not None, which is not tested")
        if not isinstance(x_input, tuple):
            raise NotImplementedError("the HIP path implements the rel_pos form: x_input = (x, pos_emb)")
        x, pos_emb = x_input
        if lens is None and mask is not None:
            lens = mask.squeeze(1).sum(-1).to(torch.int64)
        ffn = self.feed_forward if self.feed_forward is not None else self.feed_forward_macaron
        act = ffn.activation if ffn is not None else None
        cfg = dict(heads=self.attn.h, ffn_act=act, merge="dwconv", has_attn=True, has_mlp=True, cgmlp_weight=0.5, coeff=1.0,
                   merge_identity=False, ff_scale=self.ff_scale,
                   p=self.dropout_rate if self.training else 0.0,
                   p_att=self.attn.dropout_rate if self.training else 0.0)
        y = F_.grad_apply(F_.BranchformerLayerFn, x, pos_emb, lens, cfg, *self._params())
        return (y, pos_emb), mask
