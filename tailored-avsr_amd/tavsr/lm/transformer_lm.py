"""``TransformerLM`` - parameter holder with espnet2.lm.transformer_lm.TransformerLM's constructor and state_dict keys
(configs/LM/lm-english.yaml: pos_enc null, embed 128, att 512, 8 heads, 2048 units, 16 layers), used as the ``lm``
scorer of the beam search (src/inference/avsr_inference.py:155-170) and trained through ``tavsr.tasks.lm.ESPnetLanguageModel``
(lm_main.py:22-57).  Its one-token scoring step runs inside ``tavsr.inference.beam_search`` on the HIP kernels; ``forward``
(whole sequences, no cache) is the same arithmetic in teacher-forced form: in eval mode without autograd the scoring pass the
search tests check against, in training mode ``tavsr.functional_lm.TransformerLMFn`` with its hand-written backward."""
from __future__ import annotations


import torch

from .. import ops
from ..layers import LayerNorm, MultiHeadedAttention, PositionwiseFeedForward

EPS = 1e-12


class _EncoderLayer(torch.nn.Module):
    def __init__(self, size, heads, units, dropout_rate):
        super().__init__()
        self.self_attn = MultiHeadedAttention(heads, size, 0.0)
        self.feed_forward = PositionwiseFeedForward(size, units, dropout_rate, "relu")
        self.norm1, self.norm2 = LayerNorm(size), LayerNorm(size)


class _Encoder(torch.nn.Module):
    def __init__(self, idim, attention_dim, attention_heads, linear_units, num_blocks, dropout_rate):
        super().__init__()
        # espnet Encoder(input_layer="linear"): Linear, LayerNorm, Dropout, ReLU, pos_enc (identity for pos_enc: null)
        self.embed = torch.nn.Sequential(torch.nn.Linear(idim, attention_dim), LayerNorm(attention_dim),
                                         torch.nn.Dropout(dropout_rate), torch.nn.ReLU(), torch.nn.Sequential())
        self.encoders = torch.nn.ModuleList([_EncoderLayer(attention_dim, attention_heads, linear_units, dropout_rate)
                                             for _ in range(num_blocks)])
        self.after_norm = LayerNorm(attention_dim)


class TransformerLM(torch.nn.Module):
    def __init__(self, vocab_size: int, pos_enc: str = None, embed_unit: int = 128, att_unit: int = 256, head: int = 2,
                 unit: int = 1024, layer: int = 4, dropout_rate: float = 0.5):
        super().__init__()
        if pos_enc is not None:
            raise ValueError("the shipped LM recipe uses pos_enc: null (configs/LM/lm-english.yaml)")
        self.embed = torch.nn.Embedding(vocab_size, embed_unit)
        self.encoder = _Encoder(embed_unit, att_unit, head, unit, layer, dropout_rate)
        self.decoder = torch.nn.Linear(att_unit, vocab_size)
        self.heads, self.att_unit, self.dropout_rate = head, att_unit, dropout_rate

    def _params(self):
        cached = self.__dict__.get("_tavsr_pcache")                        # Parameter identities never change: look up once
        if cached is not None:
            return cached
        from ..functional_lm import LM_LAYER_PARAM_NAMES
        emb = self.encoder.embed
        P = [self.embed.weight, emb[0].weight, emb[0].bias, emb[1].weight, emb[1].bias]
        for layer in self.encoder.encoders:
            named = dict(layer.named_parameters())
            P += [named[n] for n in LM_LAYER_PARAM_NAMES]
        P += [self.encoder.after_norm.weight, self.encoder.after_norm.bias, self.decoder.weight, self.decoder.bias]
        self.__dict__["_tavsr_pcache"] = P
        return P

    def forward(self, input: torch.Tensor, hidden=None, lengths=None):
        """input (B, L) int64 -> (logits (B, L, V), None).  ``lengths`` (B) int64: keys of row b from ``lengths[b]`` on are masked
        (espnet masks keys equal to 0; with the padding at the tail under the causal mask that is the same for every row below
        ``lengths[b]``, and a 0 inside a sentence is not supported); None: full-length rows with no 0 tokens.
        In training mode, or when autograd records and a parameter requires a gradient, the pass is ``TransformerLMFn`` (dropout,
        hand-written backward); otherwise the scoring pass below, unchanged."""
        P = self._params()
        if self.training or (torch.is_grad_enabled() and any(p.requires_grad for p in P)):
            from .. import functional as F_
            from ..functional_lm import TransformerLMFn
            B, Lq = input.shape
            lens = (torch.full((B,), Lq, dtype=torch.int64, device=input.device) if lengths is None
                    else lengths.to(torch.int64).contiguous())
            cfg = dict(heads=self.heads, num_blocks=len(self.encoder.encoders))
            if self.training:
                cfg["p"] = self.dropout_rate
            return F_.grad_apply(TransformerLMFn, input.to(torch.int64), lens, cfg, *P), None
        return self._score_forward(input, lengths)

    @torch.no_grad()
    def _score_forward(self, input: torch.Tensor, lengths=None):
        """the eval / no-grad pass (whole sequences, no cache): what the beam-search tests compare the one-token step against"""
        from ..functional import _SelfAttnCore
        B, Lq = input.shape
        D, H = self.att_unit, self.heads
        dk = D // H
        M = B * Lq
        lens = torch.full((B,), Lq, dtype=torch.int64, device=input.device) if lengths is None else lengths.to(torch.int64)
        e = self.embed.weight[input.reshape(-1)]                     # embedding row gather (index plumbing)
        emb = self.encoder.embed
        h = ops.linear(e.contiguous(), emb[0].weight, emb[0].bias)
        h = ops.layernorm_fwd(h, emb[1].weight, emb[1].bias, EPS)[0]
        ops.act_(h, "relu")
        for layer in self.encoder.encoders:
            a = layer.self_attn
            n1 = ops.layernorm_fwd(h, layer.norm1.weight, layer.norm1.bias, EPS)[0]
            qkv = ops.empty(M, 3 * D, like=h)
            for j, lin in enumerate((a.linear_q, a.linear_k, a.linear_v)):
                ops.linear(n1, lin.weight, lin.bias, out=qkv, out_off=j * D, ldc=3 * D)
            cx, _, _ = _SelfAttnCore.fwd(qkv, 3 * D, 0, qkv, 3 * D, D, qkv, 3 * D, 2 * D, B, Lq, Lq, H, dk, lens, True)
            h = ops.linear(cx, a.linear_out.weight, a.linear_out.bias, res=h)
            n2 = ops.layernorm_fwd(h, layer.norm2.weight, layer.norm2.bias, EPS)[0]
            f = layer.feed_forward
            t = ops.linear(n2, f.w_1.weight, f.w_1.bias, act="relu")
            h = ops.linear(t, f.w_2.weight, f.w_2.bias, res=h)
        y = ops.layernorm_fwd(h, self.encoder.after_norm.weight, self.encoder.after_norm.bias, EPS)[0]
        return ops.linear(y, self.decoder.weight, self.decoder.bias).view(B, Lq, -1), None
