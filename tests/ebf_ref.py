"""The E-Branchformer layer and encoder in plain torch on the CPU (espnet2/asr/encoder/e_branchformer_encoder.py, restated from
the published class): the reference of tests/test_ebf_host.py and tests/test_gpu_ebf.py.  The dtype follows the inputs: as
``.double()`` it is the float64 reference, in fp32 it sets the error scale.  The attention, the cgMLP, the feed-forward block,
the embeddings and the encoder's layer loop (intermediate CTC taps, self-conditioning) are oracle/'s, imported; new here are the
layer's merge - ``merge_proj(cat + depthwise_conv_fusion(cat))`` on ``torch.nn.Conv1d(groups=2D)`` - and the optional
feed-forward blocks.  Also the depthwise-add of csrc/dwconv_time.hip and its backward written out by their formulas."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import leaves as L
from oracle.model import BranchformerEncoderOracle


class EBranchformerLayerRef(nn.Module):
    def __init__(self, size, attn, cgmlp, feed_forward, feed_forward_macaron, dropout_rate, merge_conv_kernel=3):
        super().__init__()
        self.size = size
        self.attn, self.cgmlp = attn, cgmlp
        self.feed_forward, self.feed_forward_macaron = feed_forward, feed_forward_macaron
        self.ff_scale = 1.0
        if feed_forward is not None:
            self.norm_ff = L.LayerNorm(size)
        if feed_forward_macaron is not None:
            self.ff_scale = 0.5
            self.norm_ff_macaron = L.LayerNorm(size)
        self.norm_mha = L.LayerNorm(size)
        self.norm_mlp = L.LayerNorm(size)
        self.norm_final = L.LayerNorm(size)
        self.dropout = nn.Dropout(dropout_rate)
        self.depthwise_conv_fusion = nn.Conv1d(size + size, size + size, kernel_size=merge_conv_kernel, stride=1,
                                               padding=(merge_conv_kernel - 1) // 2, groups=size + size, bias=True)
        self.merge_proj = nn.Linear(size + size, size)

    def forward(self, x_input, mask, cache=None):
        if cache is not None:
            raise NotImplementedError("cache is not None, which is not tested")
        x, pos_emb = x_input
        if self.feed_forward_macaron is not None:
            x = x + self.ff_scale * self.dropout(self.feed_forward_macaron(self.norm_ff_macaron(x)))
        n = self.norm_mha(x)
        x1 = self.dropout(self.attn(n, n, n, pos_emb, mask))
        x2 = self.dropout(self.cgmlp((self.norm_mlp(x), pos_emb), mask)[0])
        c = torch.cat([x1, x2], dim=-1)
        c_tmp = self.depthwise_conv_fusion(c.transpose(1, 2)).transpose(1, 2)
        x = x + self.dropout(self.merge_proj(c + c_tmp))
        if self.feed_forward is not None:
            x = x + self.ff_scale * self.dropout(self.feed_forward(self.norm_ff(x)))
        return (self.norm_final(x), pos_emb), mask


class EBranchformerEncoderRef(BranchformerEncoderOracle):
    """embed -> encoders -> after_norm (always); ``forward`` is BranchformerEncoderOracle's"""

    def __init__(self, input_size, output_size=256, attention_heads=4, cgmlp_linear_units=2048, cgmlp_conv_kernel=31,
                 use_linear_after_conv=False, gate_activation="identity", num_blocks=12, dropout_rate=0.1,
                 positional_dropout_rate=0.1, attention_dropout_rate=0.0, input_layer="conv2d", zero_triu=False,
                 max_pos_emb_len=5000, use_ffn=False, macaron_ffn=False, ffn_activation_type="swish", linear_units=2048,
                 merge_conv_kernel=3, interctc_layer_idx=None, interctc_use_conditioning=False):
        nn.Module.__init__(self)
        self._output_size = output_size
        pos = lambda: L.RelPositionalEncoding(output_size, positional_dropout_rate, max_pos_emb_len)
        if input_layer == "conv2d":
            self.embed = L.Conv2dSubsampling(input_size, output_size, dropout_rate, pos())
        elif input_layer == "linear":
            self.embed = nn.Sequential(nn.Linear(input_size, output_size), nn.LayerNorm(output_size), nn.Dropout(dropout_rate), pos())
        else:
            assert input_layer is None
            self.embed = None
        self.normalize_before = True
        ffn = lambda: L.PositionwiseFeedForward(output_size, linear_units, dropout_rate, L.get_activation(ffn_activation_type))
        self.encoders = L.repeat(num_blocks, lambda i: EBranchformerLayerRef(
            output_size, L.RelPositionMultiHeadedAttention(attention_heads, output_size, attention_dropout_rate, zero_triu),
            L.ConvolutionalGatingMLP(output_size, cgmlp_linear_units, cgmlp_conv_kernel, dropout_rate, use_linear_after_conv,
                                     gate_activation),
            ffn() if use_ffn else None, ffn() if use_ffn and macaron_ffn else None, dropout_rate, merge_conv_kernel))
        self.after_norm = L.LayerNorm(output_size)
        self.interctc_layer_idx = [] if interctc_layer_idx is None else list(interctc_layer_idx)
        self.interctc_use_conditioning = interctc_use_conditioning
        self.conditioning_layer = None


def dwconv_add(x, w, bias):
    """u = x + depthwise_conv1d(x) over time: x [B, T, C], w [C, K] (K odd), bias [C] - on torch's grouped convolution"""
    C, K = w.shape
    return x + F.conv1d(x.transpose(1, 2), w.view(C, 1, K), bias, padding=(K - 1) // 2, groups=C).transpose(1, 2)


def dwconv_add_restated(x, w, bias):
    """the same by the kernel's formula: u[b,t,c] = x[b,t,c] + bias[c] + sum_j w[c,j] x[b,t+j-(K-1)/2,c], zero outside 0..T-1"""
    B, T, C = x.shape
    K = w.shape[1]
    p = (K - 1) // 2
    xp = F.pad(x, (0, 0, p, p))
    u = x + bias
    for j in range(K):
        u = u + w[:, j] * xp[:, j: j + T]
    return u


def dwconv_add_bwd_restated(du, x, w):
    """(dx, dw, dbias) by the kernel's formulas: dx = du + the correlation of du with the flipped taps,
    dw[c,j] = sum_{b,t} du[b,t,c] x[b,t+j-p,c], dbias[c] = sum_{b,t} du[b,t,c]"""
    B, T, C = x.shape
    K = w.shape[1]
    p = (K - 1) // 2
    dup, xp = F.pad(du, (0, 0, p, p)), F.pad(x, (0, 0, p, p))
    dx = du.clone()
    dw = torch.zeros_like(w)
    for j in range(K):
        dx = dx + w[:, j] * dup[:, 2 * p - j: 2 * p - j + T]       # du[t + p - j]
        dw[:, j] = (du * xp[:, j: j + T]).sum((0, 1))
    return dx, dw, du.sum((0, 1))
