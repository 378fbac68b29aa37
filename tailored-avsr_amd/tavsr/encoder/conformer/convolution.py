"""``ConvolutionModule`` - espnet/nets/pytorch_backend/conformer/convolution.py (espnet 202402):

    pointwise_conv1 (C -> 2C) -> GLU -> depthwise Conv1d(K) -> BatchNorm1d -> activation -> pointwise_conv2 (C -> C)

Same constructor, parameters and buffers as espnet's class (``torch.nn.Conv1d`` / ``BatchNorm1d`` objects, so a checkpoint loads key
for key); the forward is one autograd node on the HIP kernels, which read the 1x1 convolutions' weights as 2-D views.  Nothing is
masked, as in espnet: the depthwise convolution reads padded rows and the batch statistics run over all B*T rows.
"""
from __future__ import annotations

import torch
from torch import nn

from ... import functional_conformer as FC_
from ...layers import get_activation_name


class ConvolutionModule(nn.Module):
    def __init__(self, channels: int, kernel_size: int, activation="swish", bias: bool = True):
        super().__init__()
        if not isinstance(kernel_size, int) or kernel_size < 1 or (kernel_size - 1) % 2 != 0:
            raise ValueError(f"cnn_module_kernel must be odd (espnet asserts (kernel_size - 1) % 2 == 0): {kernel_size}")
        if kernel_size > 31:
            raise ValueError(f"cnn_module_kernel: at most 31 on the HIP path (tavsr_glu_dwconv_ok): {kernel_size}")
        if not bias:
            raise ValueError("bias: only True is on the HIP path (ConvolutionModule)")
        if channels % 4 != 0:
            raise ValueError(f"channels: a multiple of 4 on the HIP path (channels-last BatchNorm kernels): {channels}")
        self.pointwise_conv1 = nn.Conv1d(channels, 2 * channels, kernel_size=1, stride=1, padding=0, bias=bias)
        self.depthwise_conv = nn.Conv1d(channels, channels, kernel_size, stride=1, padding=(kernel_size - 1) // 2, groups=channels,
                                        bias=bias)
        self.norm = nn.BatchNorm1d(channels)
        self.pointwise_conv2 = nn.Conv1d(channels, channels, kernel_size=1, stride=1, padding=0, bias=bias)
        self.activation = get_activation_name(activation)

    def bn_buffers(self):
        return self.norm.running_mean, self.norm.running_var, self.norm.num_batches_tracked

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, T, channels] -> [B, T, channels]"""
        from ..._lib import cached_params
        cfg = dict(act=self.activation, training=self.training, bn=self.bn_buffers())
        return FC_.F_.grad_apply(FC_.ConvModuleFn, x, cfg, *cached_params(self, _NAMES))


_NAMES = tuple(n[len("conv_module."):] for n in FC_.CONV_PARAMS)
