"""``MLMDecoder`` - counterpart of espnet2.asr.decoder.mlm_decoder.MLMDecoder, the masked-language-model decoder of
Mask-CTC (registered as ``decoder: mlm``, src/tasks/asr.py:186, src/tasks/avsr.py:214).  It is the ``TransformerDecoder``
stack with the same ``state_dict`` keys and three differences: one more vocabulary row (``<mask>``) in the embedding and the
output layer, a self-attention that masks padded keys only (not causal), and no ``layer_drop_rate``.

Rows ``l >= ys_in_lens[b]`` of the returned logits are padding: espnet masks those query rows as well, the HIP kernels mask
keys only.  No valid row reads a padded one and the loss ignores them, so they are not part of the contract."""
from __future__ import annotations

import torch

from .. import functional as F_
from .transformer_decoder import TransformerDecoder


class MLMDecoder(TransformerDecoder):
    def __init__(self, vocab_size: int, encoder_output_size: int, attention_heads: int = 4, linear_units: int = 2048,
                 num_blocks: int = 6, dropout_rate: float = 0.1, positional_dropout_rate: float = 0.1,
                 self_attention_dropout_rate: float = 0.0, src_attention_dropout_rate: float = 0.0,
                 input_layer: str = "embed", use_output_layer: bool = True, pos_enc_class=None,
                 normalize_before: bool = True, concat_after: bool = False):
        if pos_enc_class is not None:
            raise ValueError("HIP path covers the default positional encoding (pos_enc_class is not a recipe key)")
        super().__init__(vocab_size + 1, encoder_output_size, attention_heads, linear_units, num_blocks, dropout_rate,
                         positional_dropout_rate, self_attention_dropout_rate, src_attention_dropout_rate, input_layer,
                         use_output_layer, normalize_before, concat_after)

    def _cfg(self):
        return dict(super()._cfg(), causal=False)

    @torch.no_grad()
    def prepare_memory(self, hs_pad, hlens=None):
        """The source-attention key / value projections of all layers, [B T, num_blocks * 2 D]: the decoder's only GEMMs over the
        encoder's rows.  They do not depend on ``ys_in_pad``: a decode loop computes them once and hands them to every pass.
        (``hlens`` is not read - padded frames are projected too and masked as keys later; it is there so that the call takes what
        ``forward`` takes.)"""
        B, T, D = hs_pad.shape
        return F_.TransformerDecoderFn.project_memory(hs_pad.reshape(B * T, D), self.num_blocks, D, self._params())

    def forward(self, hs_pad, hlens, ys_in_pad, ys_in_lens, memory_kv=None):
        """hs_pad (B,T,D), hlens (B), ys_in_pad (B,L) int64 with <mask> ids, ys_in_lens (B) -> (logits (B,L,V+1), olens);
        the lengths may be lists, as ``MaskCTCInference.forward`` of the reference passes them."""
        hlens, ys_in_lens = (torch.as_tensor(t, dtype=torch.int64, device=hs_pad.device) for t in (hlens, ys_in_lens))
        return super().forward(hs_pad, hlens, ys_in_pad, ys_in_lens, memory_kv=memory_kv)
