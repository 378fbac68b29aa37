"""``EncoderLayer`` - espnet/nets/pytorch_backend/conformer/encoder_layer.py (Gulati et al., "Conformer", Interspeech 2020).

    if macaron:  x = x + ff_scale * drop(feed_forward_macaron(norm_ff_macaron(x)))
    x = x + drop(self_attn(norm_mha(x), pos_emb, mask))
    if conv:     x = x + drop(conv_module(norm_conv(x)))
    x = x + ff_scale * drop(feed_forward(norm_ff(x)));   if conv: x = norm_final(x)

Same constructor, attribute names and forward signature as espnet's class; forward and backward are one autograd node
(``tavsr.functional_conformer.ConformerLayerFn``).  Pre-norm only, no ``concat_after``, no stochastic depth: each is refused by
name.  Nothing masks the convolution module: padded frames hold what the blocks computed there, the last ``(K-1)//2`` valid
frames of a short utterance read them and BatchNorm's batch statistics include them, as in espnet.
"""
from __future__ import annotations

from typing import Optional

import torch

from ... import functional as F_
from ... import functional_conformer as FC_
from ...layers import LayerNorm


class EncoderLayer(torch.nn.Module):
    def __init__(self, size: int, self_attn: torch.nn.Module, feed_forward: torch.nn.Module,
                 feed_forward_macaron: Optional[torch.nn.Module], conv_module: Optional[torch.nn.Module], dropout_rate: float,
                 normalize_before: bool = True, concat_after: bool = False, stochastic_depth_rate: float = 0.0):
        super().__init__()
        if not normalize_before:
            raise ValueError("normalize_before: only True is on the HIP path")
        if concat_after:
            raise ValueError("concat_after: only False is on the HIP path")
        if stochastic_depth_rate != 0.0:
            raise ValueError(f"stochastic_depth_rate: only 0.0 is on the HIP path: {stochastic_depth_rate}")
        if self_attn is None or feed_forward is None:
            raise ValueError("EncoderLayer needs self_attn and feed_forward")
        self.self_attn = self_attn
        self.feed_forward = feed_forward
        self.feed_forward_macaron = feed_forward_macaron
        self.conv_module = conv_module
        self.norm_ff = LayerNorm(size)
        self.norm_mha = LayerNorm(size)
        if feed_forward_macaron is not None:
            self.norm_ff_macaron = LayerNorm(size)
            self.ff_scale = 0.5
        else:
            self.ff_scale = 1.0
        if self.conv_module is not None:
            self.norm_conv = LayerNorm(size)
            self.norm_final = LayerNorm(size)
        self.dropout_rate = dropout_rate
        self.size = size
        self.normalize_before = normalize_before
        self.concat_after = concat_after
        self.stochastic_depth_rate = stochastic_depth_rate

    def _params(self):
        from ..._lib import cached_params
        return cached_params(self, FC_.CONFORMER_PARAM_NAMES)

    def forward(self, x_input, mask, cache=None, lens: Optional[torch.Tensor] = None):
        """x_input: (x[B,T,size], pos_emb[1,2T-1,size]); mask: (B,1,T) bool prefix mask; ``lens`` (int64 [B]) may be supplied by
        the encoder instead of being recomputed from the mask."""
        if cache is not None:
            raise NotImplementedError("cache is not None: streaming / caches are not on the HIP path")
        if not isinstance(x_input, tuple):
            raise NotImplementedError("the HIP path implements the rel_pos form: x_input = (x, pos_emb)")
        x, pos_emb = x_input
        if lens is None and mask is not None:
            lens = mask.squeeze(1).sum(-1).to(torch.int64)
        cm = self.conv_module
        cfg = dict(heads=self.self_attn.h, ffn_act=self.feed_forward.activation,
                   conv_act=cm.activation if cm is not None else None, training=self.training,
                   bn=cm.bn_buffers() if cm is not None else None,
                   p=self.dropout_rate if self.training else 0.0,
                   p_att=self.self_attn.dropout_rate if self.training else 0.0)
        y = F_.grad_apply(FC_.ConformerLayerFn, x, pos_emb, lens, cfg, *self._params())
        return (y, pos_emb), mask
