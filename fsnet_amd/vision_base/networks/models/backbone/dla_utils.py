"""The upsampling half of Deep Layer Aggregation as RTM3D uses it: every projection and node is a modulated deformable
convolution followed by BatchNorm and ReLU.

Mirrors the reference's vision_base/networks/models/backbone/dla_utils.py (module names, attribute names, wiring and
initialisation, so its checkpoints load).  The deformable convolution runs on the HIP library
(fsnet_amd/vision_base/networks/ops/dcn); `conv_offset`, BatchNorm, ReLU and the depthwise transposed convolution are
plain torch modules.
"""
import math

import numpy as np
import torch.nn as nn
import torch.nn.functional as F

from fsnet_amd.vision_base.networks.ops.dcn.deform_conv import ModulatedDeformConvPack


class Identity(nn.Module):
    def forward(self, x):
        return x


def fill_fc_weights(layers):
    """zero the bias of every convolution under `layers` (dla_utils.py:21-25)"""
    for m in layers.modules():
        if isinstance(m, nn.Conv2d) and m.bias is not None:
            nn.init.constant_(m.bias, 0)


def fill_up_weights(up):
    """bilinear-interpolation kernel in every channel of a depthwise transposed convolution (dla_utils.py:28-37)"""
    w = up.weight.data
    k = w.size(2)
    f = math.ceil(k / 2)
    centre = (2 * f - 1 - f % 2) / (2.0 * f)
    for i in range(k):
        for j in range(w.size(3)):
            w[0, 0, i, j] = (1 - math.fabs(i / f - centre)) * (1 - math.fabs(j / f - centre))
    w[1:, 0] = w[0, 0]


class DeformConv(nn.Module):
    """modulated DCN 3x3 -> BatchNorm -> ReLU (dla_utils.py:40-54); `actf` is registered before `conv` as there"""

    def __init__(self, chi, cho):
        super().__init__()
        self.actf = nn.Sequential(nn.BatchNorm2d(cho), nn.ReLU(inplace=True))
        self.conv = ModulatedDeformConvPack(chi, cho, kernel_size=(3, 3), stride=1, padding=1, dilation=1,
                                            deformable_groups=1)

    def forward(self, x):
        return self.actf(self.conv(x))


class IDAUp(nn.Module):
    """iterative aggregation: level i is projected to `o` channels, upsampled by up_f[i] and merged with level i - 1
    through a node (dla_utils.py:57-83).  forward() updates `layers` in place."""

    def __init__(self, o, channels, up_f):
        super().__init__()
        for i in range(1, len(channels)):
            f = int(up_f[i])
            proj = DeformConv(channels[i], o)
            node = DeformConv(o, o)
            up = nn.ConvTranspose2d(o, o, f * 2, stride=f, padding=f // 2, output_padding=0, groups=o, bias=False)
            fill_up_weights(up)
            setattr(self, 'proj_%d' % i, proj)
            setattr(self, 'up_%d' % i, up)
            setattr(self, 'node_%d' % i, node)

    def forward(self, layers, startp, endp):
        for i in range(startp + 1, endp):
            k = i - startp
            layers[i] = getattr(self, 'up_%d' % k)(getattr(self, 'proj_%d' % k)(layers[i]))
            layers[i] = getattr(self, 'node_%d' % k)(layers[i] + layers[i - 1])


class DLAUp(nn.Module):
    """one IDAUp per level from the deepest upwards (dla_utils.py:87-110).  As in the reference, `in_channels` (by
    default the caller's `channels` list itself) is rewritten while the stages are built, and forward() rewrites `layers`."""

    def __init__(self, startp, channels, scales, in_channels=None):
        super().__init__()
        self.startp = startp
        if in_channels is None:
            in_channels = channels
        self.channels = channels
        channels = list(channels)
        scales = np.array(scales, dtype=int)
        for i in range(len(channels) - 1):
            j = -i - 2
            setattr(self, 'ida_%d' % i, IDAUp(channels[j], in_channels[j:], scales[j:] // scales[j]))
            scales[j + 1:] = scales[j]
            in_channels[j + 1:] = [channels[j] for _ in channels[j + 1:]]

    def forward(self, layers):
        out = [layers[-1]]
        for i in range(len(layers) - self.startp - 1):
            getattr(self, 'ida_%d' % i)(layers, len(layers) - i - 2, len(layers))
            out.insert(0, layers[-1])
        return out


class Interpolate(nn.Module):
    def __init__(self, scale, mode):
        super().__init__()
        self.scale, self.mode = scale, mode

    def forward(self, x):
        return F.interpolate(x, scale_factor=self.scale, mode=self.mode, align_corners=False)


class DLASegUpsample(nn.Module):
    """the upsampling part of DLASeg / RTM3D as a module of its own (dla_utils.py:124-153): a feature pyramid in, the
    map at 1 / down_ratio out"""

    def __init__(self, input_channels, down_ratio=4, final_kernel=1, last_level=5, out_channel=0):
        super().__init__()
        assert down_ratio in [2, 4, 8, 16]
        self.first_level = int(np.log2(down_ratio))
        self.last_level = last_level
        channels = input_channels
        tail = channels[self.first_level:]
        self.dla_up = DLAUp(self.first_level, tail, [2 ** i for i in range(len(tail))])
        if out_channel == 0:
            out_channel = channels[self.first_level]
        self.ida_up = IDAUp(out_channel, channels[self.first_level:self.last_level],
                            [2 ** i for i in range(self.last_level - self.first_level)])

    def forward(self, tensors):
        tensors = self.dla_up(tensors)
        y = [tensors[i].clone() for i in range(self.last_level - self.first_level)]
        self.ida_up(y, 0, len(y))
        return y[-1]
