"""``ConformerEncoder`` - espnet2/asr/encoder/conformer_encoder.py (espnet 202402): constructor keywords and defaults,
``forward(xs_pad, ilens, prev_states, ctc, max_layer)`` and state_dict keys follow espnet.

Supported subset: ``rel_pos_type="latest"``, ``pos_enc_layer_type="rel_pos"``, ``selfattention_layer_type="rel_selfattn"``,
``positionwise_layer_type="linear"``, ``normalize_before=True``, ``concat_after=False``, no stochastic depth, no layer drop,
``zero_triu=False``, ``input_layer`` in {"conv2d", "linear", None}, an odd ``cnn_module_kernel`` of at most 31.  Anything else
raises a ``ValueError`` that names the option.  espnet's default ``rel_pos_type="legacy"`` stays the default and is refused: a
legacy checkpoint run through the latest attention without saying so would be wrong, so the recipe has to say
``rel_pos_type: latest``.

The embedding, the layer loop, the intermediate-CTC taps and the self-conditioning are ``MyBranchformerEncoder``'s (same
``embed`` modules, same ``forward``); the layers are ``EncoderLayer`` and ``after_norm`` is always present.  ``activation_type``
is used by the feed-forward blocks and the convolution module alike, as in espnet.
"""
from __future__ import annotations

from typing import List, Optional, Union

import torch

from ...layers import Conv2dSubsampling, LayerNorm, PositionwiseFeedForward, RelPositionalEncoding, RelPositionMultiHeadedAttention
from ..branchformer.encoder import MyBranchformerEncoder
from .convolution import ConvolutionModule
from .encoder_layer import EncoderLayer


class ConformerEncoder(MyBranchformerEncoder):
    def __init__(self, input_size: int, output_size: int = 256, attention_heads: int = 4, linear_units: int = 2048,
                 num_blocks: int = 6, dropout_rate: float = 0.1, positional_dropout_rate: float = 0.1,
                 attention_dropout_rate: float = 0.0, input_layer: Optional[str] = "conv2d", normalize_before: bool = True,
                 concat_after: bool = False, positionwise_layer_type: str = "linear", positionwise_conv_kernel_size: int = 3,
                 macaron_style: bool = False, rel_pos_type: str = "legacy", pos_enc_layer_type: str = "rel_pos",
                 selfattention_layer_type: str = "rel_selfattn", activation_type: str = "swish", use_cnn_module: bool = True,
                 zero_triu: bool = False, cnn_module_kernel: int = 31, padding_idx: int = -1,
                 interctc_layer_idx: Optional[List[int]] = None, interctc_use_conditioning: bool = False,
                 stochastic_depth_rate: Union[float, List[float]] = 0.0, layer_drop_rate: float = 0.0, max_pos_emb_len: int = 5000):
        torch.nn.Module.__init__(self)
        self._output_size = output_size
        if rel_pos_type != "latest":
            raise ValueError(f"rel_pos_type: only 'latest' is on the HIP path, and it must be asked for (rel_pos_type: latest) - "
                             f"espnet's default 'legacy' is another attention: {rel_pos_type}")
        if pos_enc_layer_type != "rel_pos":
            raise ValueError(f"pos_enc_layer_type: only 'rel_pos' is on the HIP path: {pos_enc_layer_type}")
        if selfattention_layer_type != "rel_selfattn":
            raise ValueError(f"selfattention_layer_type: only 'rel_selfattn' is on the HIP path: {selfattention_layer_type}")
        if positionwise_layer_type != "linear":
            raise ValueError(f"positionwise_layer_type: only 'linear' is on the HIP path: {positionwise_layer_type}")
        if not normalize_before:
            raise ValueError("normalize_before: only True is on the HIP path")
        if concat_after:
            raise ValueError("concat_after: only False is on the HIP path")
        sdr = stochastic_depth_rate if isinstance(stochastic_depth_rate, (list, tuple)) else [stochastic_depth_rate]
        if any(float(r) != 0.0 for r in sdr):
            raise ValueError(f"stochastic_depth_rate: only 0.0 is on the HIP path: {stochastic_depth_rate}")
        if layer_drop_rate != 0.0:
            raise ValueError(f"layer_drop_rate: only 0.0 is on the HIP path: {layer_drop_rate}")
        if zero_triu:
            raise ValueError("zero_triu: only False is on the HIP path")
        if use_cnn_module:
            if not isinstance(cnn_module_kernel, int) or cnn_module_kernel < 1 or cnn_module_kernel % 2 == 0:
                raise ValueError(f"cnn_module_kernel must be odd: {cnn_module_kernel}")
            if cnn_module_kernel > 31:
                raise ValueError(f"cnn_module_kernel: at most 31 on the HIP path (tavsr_glu_dwconv_ok): {cnn_module_kernel}")
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
        self.normalize_before = True
        ffn = lambda: PositionwiseFeedForward(output_size, linear_units, dropout_rate, activation_type)
        self.encoders = torch.nn.ModuleList([
            EncoderLayer(
                output_size,
                RelPositionMultiHeadedAttention(attention_heads, output_size, attention_dropout_rate, zero_triu),
                ffn(), ffn() if macaron_style else None,
                ConvolutionModule(output_size, cnn_module_kernel, activation_type) if use_cnn_module else None,
                dropout_rate, normalize_before, concat_after, 0.0)
            for _ in range(num_blocks)])
        self.after_norm = LayerNorm(output_size)
        self.interctc_layer_idx = [] if interctc_layer_idx is None else list(interctc_layer_idx)
        if len(self.interctc_layer_idx) > 0:
            assert 0 < min(self.interctc_layer_idx) and max(self.interctc_layer_idx) < num_blocks
        self.interctc_use_conditioning = interctc_use_conditioning
        self.conditioning_layer = None
