"""ConvBnReLU parameter container (reference vision_base/networks/blocks/blocks.py:33-54): keys
`sequence.0.{weight,bias}` (conv) and `sequence.1.*` (BatchNorm2d).  The arithmetic runs in the
HIP engine (fsnet_amd/engine/nets.py); standalone forward is a single fused conv+BN+ReLU unit.

DropPath (reference blocks.py:418-440): stochastic depth per sample.  The ConvNeXt runner draws the same numbers with the
same expression and hands the factor to fs_scale_residual_fwd (fsnet_amd/engine/convnext_net.py)."""
import torch
import torch.nn as nn


class ConvBnReLU(nn.Module):
    def __init__(self, input_features=1, output_features=1, kernel_size=(1, 1), stride=[1, 1], padding='SAME',
                 dilation=1, groups=1, relu=True, **kwargs):
        super().__init__()
        if isinstance(kernel_size, int):
            kernel_size = (kernel_size, kernel_size)
        if dilation != 1 or groups != 1:
            raise NotImplementedError("HIP ConvBnReLU supports dilation=1, groups=1")
        pad = int((kernel_size[0] - 1) / 2) if padding.lower() == 'same' else 0
        self.sequence = nn.Sequential(
            nn.Conv2d(input_features, output_features, kernel_size=kernel_size, stride=stride, padding=pad, **kwargs),
            nn.BatchNorm2d(output_features),
        )
        self.relu = True

    def forward(self, x):
        raise NotImplementedError(
            "ConvBnReLU is executed by its owning network's HIP runner (DepthDecoder); standalone use is not on "
            "the monodepth hot path")


class DropPath(nn.Module):
    """per-sample stochastic depth on a residual branch: a sample is kept with probability 1 - drop_prob and a kept one is
    scaled by 1 / (1 - drop_prob); the identity at rate 0 and in eval mode"""

    def __init__(self, drop_prob=0.):
        super().__init__()
        self.drop_prob = drop_prob
        self.keep_prob = 1 - drop_prob

    def keep_mask(self, n, dtype, device, ndim):
        """0 / 1 per sample, [n, 1, ..., 1]: floor(keep_prob + U[0, 1)) — one torch.rand draw of n numbers"""
        return (self.keep_prob + torch.rand((n,) + (1,) * (ndim - 1), dtype=dtype, device=device)).floor_()

    def forward(self, x):
        if self.drop_prob == 0. or not self.training:
            return x
        return x.div(self.keep_prob) * self.keep_mask(x.shape[0], x.dtype, x.device, x.ndim)
