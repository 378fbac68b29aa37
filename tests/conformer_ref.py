"""The Conformer convolution module, layer and encoder in plain torch on the CPU (espnet 202402: conformer/convolution.py,
conformer/encoder_layer.py, espnet2/asr/encoder/conformer_encoder.py, restated from the published classes): the reference of
tests/test_conformer_host.py and tests/test_gpu_conformer.py.  The dtype follows the inputs: as ``.double()`` it is the float64
reference, in fp32 it sets the error scale.  The attention, the feed-forward block, the embeddings and the encoder's layer loop
(intermediate CTC taps, self-conditioning) are oracle/'s, imported; new here are the convolution module on ``nn.Conv1d``,
``F.glu`` and ``nn.BatchNorm1d`` and the layer's sequence.  Also the GLU + depthwise convolution of csrc/dwconv_time.hip and
its backward written out by their formulas."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import leaves as L
from oracle.model import BranchformerEncoderOracle


class ConvolutionModuleRef(nn.Module):
    def __init__(self, channels, kernel_size, activation=None, bias=True):
        super().__init__()
        assert (kernel_size - 1) % 2 == 0
        self.pointwise_conv1 = nn.Conv1d(channels, 2 * channels, kernel_size=1, stride=1, padding=0, bias=bias)
        self.depthwise_conv = nn.Conv1d(channels, channels, kernel_size, stride=1, padding=(kernel_size - 1) // 2, groups=channels,
                                        bias=bias)
        self.norm = nn.BatchNorm1d(channels)
        self.pointwise_conv2 = nn.Conv1d(channels, channels, kernel_size=1, stride=1, padding=0, bias=bias)
        self.activation = activation if activation is not None else nn.ReLU()

    def forward(self, x):
        x = x.transpose(1, 2)
        x = self.pointwise_conv1(x)
        x = F.glu(x, dim=1)
        x = self.depthwise_conv(x)
        x = self.activation(self.norm(x))
        x = self.pointwise_conv2(x)
        return x.transpose(1, 2)


class ConformerLayerRef(nn.Module):
    """EncoderLayer.forward with normalize_before=True, concat_after=False, stochastic_depth_rate=0"""

    def __init__(self, size, self_attn, feed_forward, feed_forward_macaron, conv_module, dropout_rate):
        super().__init__()
        self.self_attn, self.feed_forward = self_attn, feed_forward
        self.feed_forward_macaron, self.conv_module = feed_forward_macaron, conv_module
        self.norm_ff = L.LayerNorm(size)
        self.norm_mha = L.LayerNorm(size)
        self.ff_scale = 1.0
        if feed_forward_macaron is not None:
            self.norm_ff_macaron = L.LayerNorm(size)
            self.ff_scale = 0.5
        if conv_module is not None:
            self.norm_conv = L.LayerNorm(size)
            self.norm_final = L.LayerNorm(size)
        self.dropout = nn.Dropout(dropout_rate)
        self.size = size

    def forward(self, x_input, mask, cache=None):
        assert cache is None
        x, pos_emb = x_input
        if self.feed_forward_macaron is not None:
            x = x + self.ff_scale * self.dropout(self.feed_forward_macaron(self.norm_ff_macaron(x)))
        n = self.norm_mha(x)
        x = x + self.dropout(self.self_attn(n, n, n, pos_emb, mask))
        if self.conv_module is not None:
            x = x + self.dropout(self.conv_module(self.norm_conv(x)))
        x = x + self.ff_scale * self.dropout(self.feed_forward(self.norm_ff(x)))
        if self.conv_module is not None:
            x = self.norm_final(x)
        return (x, pos_emb), mask


class ConformerEncoderRef(BranchformerEncoderOracle):
    """embed -> encoders -> after_norm (always); ``forward`` is BranchformerEncoderOracle's.  espnet2's keywords and defaults
    (the options the HIP path refuses are left out, except rel_pos_type, whose default the HIP path refuses)."""

    def __init__(self, input_size, output_size=256, attention_heads=4, linear_units=2048, num_blocks=6, dropout_rate=0.1,
                 positional_dropout_rate=0.1, attention_dropout_rate=0.0, input_layer="conv2d", macaron_style=False,
                 rel_pos_type="legacy", activation_type="swish", use_cnn_module=True, zero_triu=False, cnn_module_kernel=31,
                 interctc_layer_idx=None, interctc_use_conditioning=False, max_pos_emb_len=5000):
        nn.Module.__init__(self)
        assert rel_pos_type == "latest", "the restatement has the latest relative positions only"
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
        ffn = lambda: L.PositionwiseFeedForward(output_size, linear_units, dropout_rate, L.get_activation(activation_type))
        self.encoders = L.repeat(num_blocks, lambda i: ConformerLayerRef(
            output_size, L.RelPositionMultiHeadedAttention(attention_heads, output_size, attention_dropout_rate, zero_triu),
            ffn(), ffn() if macaron_style else None,
            ConvolutionModuleRef(output_size, cnn_module_kernel, L.get_activation(activation_type)) if use_cnn_module else None,
            dropout_rate))
        self.after_norm = L.LayerNorm(output_size)
        self.interctc_layer_idx = [] if interctc_layer_idx is None else list(interctc_layer_idx)
        self.interctc_use_conditioning = interctc_use_conditioning
        self.conditioning_layer = None


def glu_dwconv(h, w, bias):
    """z = depthwise_conv1d(glu(h)) over time: h [B, T, 2C], w [C, K] (K odd), bias [C] - on F.glu and torch's grouped convolution"""
    C, K = w.shape
    g = F.glu(h.transpose(1, 2), dim=1)
    return F.conv1d(g, w.view(C, 1, K), bias, padding=(K - 1) // 2, groups=C).transpose(1, 2)


def glu_dwconv_restated(h, w, bias):
    """the same by the kernel's formulas: g = h[..., :C] * sigmoid(h[..., C:]),
    z[b,t,c] = bias[c] + sum_j w[c,j] g[b,t+j-(K-1)/2,c], g = 0 outside 0..T-1"""
    B, T, _ = h.shape
    C, K = w.shape
    p = (K - 1) // 2
    gp = F.pad(h[..., :C] * torch.sigmoid(h[..., C:]), (0, 0, p, p))
    z = bias.expand(B, T, C)
    for j in range(K):
        z = z + w[:, j] * gp[:, j: j + T]
    return z


def glu_dwconv_bwd_restated(dz, h, w):
    """(dh, dw, dbias) by the kernel's formulas: dg[t] = sum_k w[k] dz[t + p - k], s = sigmoid(h[..., C:]),
    dh[..., :C] = dg * s, dh[..., C:] = dg * h[..., :C] * s * (1 - s), dw[c,k] = sum_{b,t} dz[t] g[t+k-p], dbias[c] = sum dz"""
    B, T, _ = h.shape
    C, K = w.shape
    p = (K - 1) // 2
    a, s = h[..., :C], torch.sigmoid(h[..., C:])
    dzp, gp = F.pad(dz, (0, 0, p, p)), F.pad(a * s, (0, 0, p, p))
    dg = torch.zeros_like(dz)
    dw = torch.zeros_like(w)
    for j in range(K):
        dg = dg + w[:, j] * dzp[:, 2 * p - j: 2 * p - j + T]       # dz[t + p - j]
        dw[:, j] = (dz * gp[:, j: j + T]).sum((0, 1))
    return torch.cat([dg * s, dg * a * s * (1 - s)], dim=-1), dw, dz.sum((0, 1))
