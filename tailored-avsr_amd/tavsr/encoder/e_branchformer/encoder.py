"""``EBranchformerEncoder`` - espnet2/asr/encoder/e_branchformer_encoder.py: constructor keywords, ``forward(xs_pad, ilens,
prev_states, ctc, max_layer)`` and state_dict keys follow espnet.

Supported subset: ``attention_layer_type="rel_selfattn"``, ``pos_enc_layer_type="rel_pos"``, ``rel_pos_type="latest"``,
``positionwise_layer_type="linear"``, ``input_layer`` in {"conv2d", "linear", None}, ``layer_drop_rate=0.0``, the cgMLP without
``use_linear_after_conv`` and with ``gate_activation="identity"``, ``zero_triu=False``.  Anything else raises a ``ValueError``
that names the option - so do an even ``merge_conv_kernel`` (espnet fails at the add), one above 31 (the kernel's limit) and
``macaron_ffn`` without ``use_ffn``.

The embedding, the layer loop, the intermediate-CTC taps and the self-conditioning are ``MyBranchformerEncoder``'s (same
``embed`` modules, same ``forward``); the layers are ``EBranchformerEncoderLayer`` and ``after_norm`` is always present.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from ...layers import (Conv2dSubsampling, ConvolutionalGatingMLP, LayerNorm, PositionwiseFeedForward, RelPositionalEncoding,
                       RelPositionMultiHeadedAttention)
from ..branchformer.encoder import MyBranchformerEncoder
from .encoder_layer import EBranchformerEncoderLayer


class EBranchformerEncoder(MyBranchformerEncoder):
    def __init__(self, input_size: int, output_size: int = 256, attention_heads: int = 4,
                 attention_layer_type: str = "rel_selfattn", pos_enc_layer_type: str = "rel_pos", rel_pos_type: str = "latest",
                 cgmlp_linear_units: int = 2048, cgmlp_conv_kernel: int = 31, use_linear_after_conv: bool = False,
                 gate_activation: str = "identity", num_blocks: int = 12, dropout_rate: float = 0.1,
                 positional_dropout_rate: float = 0.1, attention_dropout_rate: float = 0.0,
                 input_layer: Optional[str] = "conv2d", zero_triu: bool = False, padding_idx: int = -1,
                 layer_drop_rate: float = 0.0, max_pos_emb_len: int = 5000, use_ffn: bool = False, macaron_ffn: bool = False,
                 ffn_activation_type: str = "swish", linear_units: int = 2048, positionwise_layer_type: str = "linear",
                 merge_conv_kernel: int = 3, interctc_layer_idx: Optional[List[int]] = None,
                 interctc_use_conditioning: bool = False):
        torch.nn.Module.__init__(self)
        self._output_size = output_size
        if rel_pos_type != "latest":
            raise ValueError(f"rel_pos_type: only 'latest' is on the HIP path: {rel_pos_type}")
        if pos_enc_layer_type != "rel_pos":
            raise ValueError(f"pos_enc_layer_type: only 'rel_pos' is on the HIP path: {pos_enc_layer_type}")
        if attention_layer_type != "rel_selfattn":
            raise ValueError(f"attention_layer_type: only 'rel_selfattn' is on the HIP path: {attention_layer_type}")
        if positionwise_layer_type != "linear":
            raise ValueError(f"positionwise_layer_type: only 'linear' is on the HIP path: {positionwise_layer_type}")
        if layer_drop_rate != 0.0:
            raise ValueError(f"layer_drop_rate: only 0.0 is on the HIP path: {layer_drop_rate}")
        if use_linear_after_conv:
            raise ValueError("use_linear_after_conv: only False is on the HIP path")
        if gate_activation != "identity":
            raise ValueError(f"gate_activation: only 'identity' is on the HIP path: {gate_activation}")
        if zero_triu:
            raise ValueError("zero_triu: only False is on the HIP path")
        if not isinstance(merge_conv_kernel, int) or merge_conv_kernel < 1 or merge_conv_kernel % 2 == 0:
            raise ValueError(f"merge_conv_kernel must be odd: {merge_conv_kernel}")
        if merge_conv_kernel > 31:
            raise ValueError(f"merge_conv_kernel: at most 31 on the HIP path (tavsr_dwconv_add_ok): {merge_conv_kernel}")
        if macaron_ffn and not use_ffn:
            raise ValueError("macaron_ffn needs use_ffn (espnet would build no feed-forward block at all)")
        pos = lambda: RelPositionalEncoding(output_size, positional_dropout_rate, max_pos_emb_len)
        if input_layer == "conv2d":
            self.embed = Conv2dSubsampling(input_size, output_size, dropout_rate, pos())
        elif input_layer == "linear":
            self.embed = torch.nn.Sequential(torch.nn.Linear(input_size, output_size), torch.nn.LayerNorm(output_size),
                                             torch.nn.Dropout(dropout_rate), pos())
        elif input_layer is None:
            self.embed = None
        else:
            raise ValueError(f"input_layer: only 'conv2d', 'linear' and None are on the HIP path: {input_layer}")
        self.normalize_before = True          # (MyBranchformerEncoder.forward: after_norm is always applied)
        ffn = lambda: PositionwiseFeedForward(output_size, linear_units, dropout_rate, ffn_activation_type)
        self.encoders = torch.nn.ModuleList([
            EBranchformerEncoderLayer(
                output_size,
                RelPositionMultiHeadedAttention(attention_heads, output_size, attention_dropout_rate, zero_triu),
                ConvolutionalGatingMLP(output_size, cgmlp_linear_units, cgmlp_conv_kernel, dropout_rate, use_linear_after_conv,
                                       gate_activation),
                ffn() if use_ffn else None, ffn() if use_ffn and macaron_ffn else None, dropout_rate, merge_conv_kernel)
            for _ in range(num_blocks)])
        self.after_norm = LayerNorm(output_size)
        self.interctc_layer_idx = [] if interctc_layer_idx is None else list(interctc_layer_idx)
        if len(self.interctc_layer_idx) > 0:
            assert 0 < min(self.interctc_layer_idx) and max(self.interctc_layer_idx) < num_blocks
        self.interctc_use_conditioning = interctc_use_conditioning
        self.conditioning_layer = None
