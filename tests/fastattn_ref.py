"""The Branchformer attention options beyond rel_selfattn / rel_pos in plain torch on the CPU: the reference of
tests/test_fastattn_host.py and tests/test_gpu_fastattn.py.  The dtype follows the inputs: as ``.double()`` it is the float64
reference, in fp32 it sets the error scale.

New here: ``FastSelfAttentionRef`` (espnet2 asr/layers/fastformer.py, restated from the published class: Fastformer's additive
attention), its core written out by the kernels' formulas (``fast_core``: csrc/fastattn.hip takes q | k and returns pk * q), and
``BranchformerEncoderRef``, the encoder's constructor with the three attention forms and the three positional encodings.  The
plain ``MultiHeadedAttention``, ``PositionalEncoding`` / ``ScaledPositionalEncoding``, the cgMLP, the feed-forward block, the
embeddings, the layer and the encoder's layer loop (both take the tensor form: no ``pos_emb``) are oracle/'s, imported."""
import torch
import torch.nn as nn

from oracle import leaves as L
from oracle.model import BranchformerEncoderOracle, BranchformerLayerOracle


def masked_softmax(score, dead):
    """softmax over the last axis with the ``dead`` entries out: espnet fills them with the dtype's lowest finite value before
    the softmax and with 0 after it (``dead`` None: plain softmax)"""
    if dead is None:
        return torch.softmax(score, dim=-1)
    low = torch.finfo(score.dtype).min
    return torch.softmax(score.masked_fill(dead, low), dim=-1).masked_fill(dead, 0.0)


class FastSelfAttentionRef(nn.Module):
    def __init__(self, size, attention_heads, dropout_rate):
        super().__init__()
        if size % attention_heads != 0:
            raise ValueError(f"Hidden size ({size}) is not an integer multiple of attention heads ({attention_heads})")
        self.attention_head_size = size // attention_heads
        self.num_attention_heads = attention_heads
        self.query = nn.Linear(size, size)
        self.query_att = nn.Linear(size, attention_heads)
        self.key = nn.Linear(size, size)
        self.key_att = nn.Linear(size, attention_heads)
        self.transform = nn.Linear(size, size)
        self.dropout = nn.Dropout(dropout_rate)

    def espnet_initialization_fn(self):
        for m in self.modules():
            if isinstance(m, nn.Linear):
                m.weight.data.normal_(mean=0.0, std=0.02)
                if m.bias is not None:
                    m.bias.data.zero_()

    def transpose_for_scores(self, x):
        """(B, T, D) -> (B, H, T, dh)"""
        return x.reshape(*x.shape[:-1], self.num_attention_heads, self.attention_head_size).transpose(1, 2)

    def forward(self, xs_pad, *more):
        """``forward(xs_pad, mask)`` with mask (B, 1, T) or None.  (oracle's layer calls every attention that takes no positional
        rows as ``attn(n, n, n, mask)``: the mask is the last argument either way.)"""
        mask = more[-1]
        B, T, _ = xs_pad.shape
        H, dh = self.num_attention_heads, self.attention_head_size
        q, k = self.query(xs_pad), self.key(xs_pad)
        dead = None if mask is None else mask.eq(0)                                          # (B, 1, T)
        alpha = masked_softmax(self.query_att(q).transpose(1, 2) / dh ** 0.5, dead)          # (B, H, T)
        ql = self.transpose_for_scores(q)                                                    # (B, H, T, dh)
        pq = torch.matmul(alpha.unsqueeze(2), ql).transpose(1, 2).reshape(B, 1, H * dh)      # (B, 1, D)
        pq = self.dropout(pq)
        p = k * pq.repeat(1, T, 1)
        beta = masked_softmax((self.key_att(p) / dh ** 0.5).transpose(1, 2), dead)
        pk = self.dropout(torch.matmul(beta.unsqueeze(2), self.transpose_for_scores(p)))     # (B, H, 1, dh)
        wv = (pk * ql).transpose(1, 2)                                                       # value = query (shared parameters)
        wv = wv.reshape(wv.shape[:-2] + (H * dh,))
        return self.dropout(self.transform(wv)) + q


def fast_core(q, k, wq, bq, wk, bk, lens, H):
    """what csrc/fastattn.hip computes between the projections, by its formulas: q, k (B, T, D), score weights (H, D) / (H,),
    lens (B,) -> (wv = pk * q, alpha, beta (B, H, T), pq, pk (B, D))"""
    B, T, D = q.shape
    dh = D // H
    dead = (torch.arange(T)[None, :] >= lens[:, None])[:, None, :]
    head = torch.arange(D) // dh

    def pool(x, w, b):
        s = (torch.einsum("btd,hd->bht", x, w) + b[None, :, None]) / dh ** 0.5
        a = masked_softmax(s, dead)
        return a, torch.einsum("btd,bdt->bd", x, a[:, head, :])

    alpha, pq = pool(q, wq, bq)
    beta, pk = pool(k * pq[:, None, :], wk, bk)
    return pk[:, None, :] * q, alpha, beta, pq, pk


class BranchformerEncoderRef(BranchformerEncoderOracle):
    """src/encoder/branchformer/encoder.py:52-412 with ``attention_layer_type`` in {rel_selfattn, selfattn, fast_selfattn} and
    ``pos_enc_layer_type`` in {rel_pos, abs_pos, scaled_abs_pos}; ``forward`` is BranchformerEncoderOracle's."""

    def __init__(self, input_size=256, output_size=256, attention_heads=4, linear_units=2048, num_blocks=6, cgmlp_linear_units=2048,
                 cgmlp_conv_kernel=31, dropout_rate=0.1, positional_dropout_rate=0.1, attention_dropout_rate=0.1,
                 input_layer="conv3dresnet18", pos_enc_layer_type="rel_pos", attention_layer_type="rel_selfattn",
                 ffn_activation_type="relu", merge_method="learned_ave", interctc_use_conditioning=False, interctc_layer_idx=(),
                 max_pos_emb_len=5000, **same_as_default):
        nn.Module.__init__(self)
        for key in same_as_default:
            assert key in ("rel_pos_type", "positionwise_layer_type", "gate_activation", "use_linear_after_conv", "macaron",
                           "use_attn", "use_cgmlp", "normalize_before", "zero_triu", "cgmlp_weight", "attn_branch_drop_rate",
                           "stochastic_depth_rate", "ignore_id"), key
        self._output_size = output_size
        pos_cls = {"rel_pos": L.RelPositionalEncoding, "abs_pos": L.PositionalEncoding,
                   "scaled_abs_pos": L.ScaledPositionalEncoding}[pos_enc_layer_type]
        assert (pos_enc_layer_type == "rel_pos") == (attention_layer_type == "rel_selfattn")
        pos = lambda: pos_cls(output_size, positional_dropout_rate, max_pos_emb_len)
        if input_layer == "linear":
            self.embed = nn.Sequential(nn.Linear(input_size, output_size), nn.LayerNorm(output_size), nn.Dropout(dropout_rate), pos())
        elif input_layer in ("conv1d", "conv3dresnet18"):
            self.embed = nn.Sequential(nn.Linear(512, output_size), pos_cls(output_size, positional_dropout_rate))
        elif input_layer == "conv2d":
            self.embed = L.Conv2dSubsampling(input_size, output_size, dropout_rate, pos())
        else:
            assert input_layer is None
            self.embed = None
        self.normalize_before = True
        attn = {"rel_selfattn": lambda: L.RelPositionMultiHeadedAttention(attention_heads, output_size, attention_dropout_rate),
                "selfattn": lambda: L.MultiHeadedAttention(attention_heads, output_size, attention_dropout_rate),
                "fast_selfattn": lambda: FastSelfAttentionRef(output_size, attention_heads, attention_dropout_rate)}[attention_layer_type]
        ffn = lambda: L.PositionwiseFeedForward(output_size, linear_units, dropout_rate, L.get_activation(ffn_activation_type))
        self.encoders = L.repeat(num_blocks, lambda i: BranchformerLayerOracle(
            output_size, attn(), L.ConvolutionalGatingMLP(output_size, cgmlp_linear_units, cgmlp_conv_kernel, dropout_rate, False,
                                                          "identity"), ffn(), ffn(), dropout_rate, merge_method))
        self.after_norm = L.LayerNorm(output_size)
        self.interctc_layer_idx = list(interctc_layer_idx)
        self.interctc_use_conditioning = interctc_use_conditioning
        self.conditioning_layer = None
