"""Deep Layer Aggregation backbone with the reference's constructor, state_dict names and initialisation
(reference vision_base/networks/models/backbone/dla.py: blocks :39-152, Root :155-173, Tree :176-229, DLA :232-330,
factories :333-439), so its checkpoints load with strict=True.

A CUDA batch runs on the HIP engine (fsnet_amd/engine/dla_net.py): the nn.Conv2d / nn.BatchNorm2d children are then
parameter containers, and autograd sees one custom Function per call.  A CPU batch runs the plain-torch forward() of the
modules below over the same parameters, in whatever dtype they have: the wiring check and the timing baseline.

What the reference does and this file keeps (each pinned by tests/test_dla_cpu.py against tests/golden/dla.npz):
  * Tree.forward with levels > 1 runs `project` on the pooled input and hands the result to tree1, a Tree, which ignores
    it (dla.py:219-222): the BatchNorm buffers of that `project` move in training mode, its parameters get no gradient.
  * One `children` list is shared and appended to down the tree2 recursion: a root reads [x2, x1, *children].
  * All six levels run whatever out_indices asks for.
"""
import math
from os.path import join

import torch
import torch.nn as nn
import torch.nn.functional as F

WEB_ROOT = 'http://dl.yf.io/dla/models'
MODEL_HASH = {'dla34': 'ba72cf86', 'dla46_c': '2bfd52c3', 'dla46x_c': 'd761bae7', 'dla60x_c': 'b870c45c',
              'dla60': '24839fc4', 'dla60x': 'd15cacda', 'dla102': 'd94d9790', 'dla102x': 'ad62be81',
              'dla102x2': '262837b6', 'dla169': '0914e092'}


def get_model_url(name):
    return join(WEB_ROOT, 'imagenet', '%s-%s.pth' % (name, MODEL_HASH[name]))


def _conv_bn(block, j, x):
    return getattr(block, 'bn%d' % j)(getattr(block, 'conv%d' % j)(x))


class BasicBlock(nn.Module):
    def __init__(self, inplanes, planes, stride=1, dilation=1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=dilation, bias=False, dilation=dilation)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=1, padding=dilation, bias=False, dilation=dilation)
        self.bn2 = nn.BatchNorm2d(planes)
        self.stride = stride

    def forward(self, x, residual=None):
        residual = x if residual is None else residual
        out = F.relu(_conv_bn(self, 1, x))
        return F.relu(_conv_bn(self, 2, out) + residual)


class Bottleneck(nn.Module):
    expansion = 2

    def __init__(self, inplanes, planes, stride=1, dilation=1):
        super().__init__()
        mid = planes // Bottleneck.expansion
        self.conv1 = nn.Conv2d(inplanes, mid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid)
        self.conv2 = nn.Conv2d(mid, mid, 3, stride=stride, padding=dilation, bias=False, dilation=dilation)
        self.bn2 = nn.BatchNorm2d(mid)
        self.conv3 = nn.Conv2d(mid, planes, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.stride = stride

    def forward(self, x, residual=None):
        residual = x if residual is None else residual
        out = F.relu(_conv_bn(self, 1, x))
        out = F.relu(_conv_bn(self, 2, out))
        return F.relu(_conv_bn(self, 3, out) + residual)


class BottleneckX(nn.Module):
    """the grouped (ResNeXt) bottleneck: constructed and loaded like the reference's, executed by torch on the CPU only —
    the HIP engine has no grouped convolution"""
    expansion = 2
    cardinality = 32

    def __init__(self, inplanes, planes, stride=1, dilation=1):
        super().__init__()
        groups = BottleneckX.cardinality
        mid = planes * groups // 32
        self.conv1 = nn.Conv2d(inplanes, mid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid)
        self.conv2 = nn.Conv2d(mid, mid, 3, stride=stride, padding=dilation, bias=False, dilation=dilation, groups=groups)
        self.bn2 = nn.BatchNorm2d(mid)
        self.conv3 = nn.Conv2d(mid, planes, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.stride = stride

    def forward(self, x, residual=None):
        if x.is_cuda:
            raise NotImplementedError("BottleneckX: grouped 3x3 convolution (groups=%d) has no HIP kernel; the DLA-X "
                                      "variants construct and load, and run on the CPU only" % self.conv2.groups)
        return Bottleneck.forward(self, x, residual)


class Root(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, residual):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=1, bias=False, padding=(kernel_size - 1) // 2)
        self.bn = nn.BatchNorm2d(out_channels)
        self.relu = nn.ReLU(inplace=True)
        self.residual = residual

    def forward(self, *x):
        out = self.bn(self.conv(torch.cat(x, 1)))
        if self.residual:
            out = out + x[0]
        return F.relu(out)


class Tree(nn.Module):
    def __init__(self, levels, block, in_channels, out_channels, stride=1, level_root=False, root_dim=0,
                 root_kernel_size=1, dilation=1, root_residual=False):
        super().__init__()
        if root_dim == 0:
            root_dim = 2 * out_channels
        if level_root:
            root_dim += in_channels
        if levels == 1:
            self.tree1 = block(in_channels, out_channels, stride, dilation=dilation)
            self.tree2 = block(out_channels, out_channels, 1, dilation=dilation)
            self.root = Root(root_dim, out_channels, root_kernel_size, root_residual)
        else:
            self.tree1 = Tree(levels - 1, block, in_channels, out_channels, stride, root_dim=0,
                              root_kernel_size=root_kernel_size, dilation=dilation, root_residual=root_residual)
            self.tree2 = Tree(levels - 1, block, out_channels, out_channels, root_dim=root_dim + out_channels,
                              root_kernel_size=root_kernel_size, dilation=dilation, root_residual=root_residual)
        self.level_root = level_root
        self.root_dim = root_dim
        self.levels = levels
        # (registered after the trees and the root, as in the reference: modules() order drives the initialisation)
        self.downsample = nn.MaxPool2d(stride, stride=stride) if stride > 1 else None
        self.project = None
        if in_channels != out_channels:
            self.project = nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=1, bias=False),
                                         nn.BatchNorm2d(out_channels))

    def forward(self, x, residual=None, children=None):
        children = [] if children is None else children
        bottom = self.downsample(x) if self.downsample is not None else x
        # (with levels > 1 tree1 is a Tree and drops this argument: the projection still runs, see the module docstring)
        residual = self.project(bottom) if self.project is not None else bottom
        if self.level_root:
            children.append(bottom)
        x1 = self.tree1(x, residual)
        if self.levels == 1:
            return self.root(self.tree2(x1), x1, *children)
        children.append(x1)
        return self.tree2(x1, children=children)


class DLA(nn.Module):
    """features by stride: index -1 and 0 at 1/1, 1 at 1/2, 2 at 1/4, 3 at 1/8, 4 at 1/16, 5 at 1/32"""

    def __init__(self, levels, channels, num_classes=1000, block=BasicBlock, residual_root=False,
                 out_indices=(-1, 0, 1, 2, 3, 4, 5)):
        super().__init__()
        self.channels = channels
        self.out_indices = out_indices
        self.num_classes = num_classes
        self.base_layer = nn.Sequential(nn.Conv2d(3, channels[0], kernel_size=7, stride=1, padding=3, bias=False),
                                        nn.BatchNorm2d(channels[0]), nn.ReLU(inplace=True))
        self.level0 = self._make_conv_level(channels[0], channels[0], levels[0])
        self.level1 = self._make_conv_level(channels[0], channels[1], levels[1], stride=2)
        self.level2 = Tree(levels[2], block, channels[1], channels[2], 2, level_root=False, root_residual=residual_root)
        self.level3 = Tree(levels[3], block, channels[2], channels[3], 2, level_root=True, root_residual=residual_root)
        self.level4 = Tree(levels[4], block, channels[3], channels[4], 2, level_root=True, root_residual=residual_root)
        self.level5 = Tree(levels[5], block, channels[4], channels[5], 2, level_root=True, root_residual=residual_root)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()
        self._runner = None         # engine.dla_net.DLARunner, built at the first CUDA forward
        self._pending = 0
        self._plist = None

    @staticmethod
    def _make_conv_level(inplanes, planes, convs, stride=1, dilation=1):
        modules = []
        for i in range(convs):
            modules += [nn.Conv2d(inplanes, planes, kernel_size=3, stride=stride if i == 0 else 1, padding=dilation,
                                  bias=False, dilation=dilation),
                        nn.BatchNorm2d(planes), nn.ReLU(inplace=True)]
            inplanes = planes
        return nn.Sequential(*modules)

    def _select(self, base, levels):
        """the requested features in the reference's order: -1 (the base layer) first, then the levels ascending"""
        y = [base] if -1 in self.out_indices else []
        return y + [f for i, f in enumerate(levels) if i in self.out_indices]

    def forward_torch(self, x):
        """plain torch over the module's parameters (any device, any dtype)"""
        base = x = self.base_layer(x)
        levels = []
        for i in range(6):
            x = getattr(self, 'level%d' % i)(x)
            levels.append(x)
        return self._select(base, levels)

    def forward(self, x):
        H, W = int(x.shape[-2]), int(x.shape[-1])
        if H % 32 or W % 32:
            # (the reference fails inside level 2 with a shape mismatch: MaxPool2d floors, the stride-2 convolution does not)
            raise ValueError("DLA: input height and width must be multiples of 32, got H=%d W=%d" % (H, W))
        if not x.is_cuda:
            return self.forward_torch(x)
        from fsnet_amd.engine.dla_net import run_dla
        return self._select(*run_dla(self, x))

    def load_pretrained_model(self, data_name, name):
        import torch.utils.model_zoo as model_zoo
        model_url = get_model_url(name)
        print(model_url)
        self.load_state_dict(model_zoo.load_url(model_url), strict=False)


def _make(name, levels, channels, block, pretrained, **kwargs):
    model = DLA(levels, channels, block=block, **kwargs)
    if pretrained is not None:
        model.load_pretrained_model(pretrained, name)
    return model


def dla34(pretrained=True, **kwargs):
    return _make('dla34', [1, 1, 1, 2, 2, 1], [16, 32, 64, 128, 256, 512], BasicBlock, pretrained, **kwargs)


def dla46_c(pretrained=True, **kwargs):
    Bottleneck.expansion = 2
    return _make('dla46_c', [1, 1, 1, 2, 2, 1], [16, 32, 64, 64, 128, 256], Bottleneck, pretrained, **kwargs)


def dla46x_c(pretrained=True, **kwargs):
    BottleneckX.expansion = 2
    return _make('dla46x_c', [1, 1, 1, 2, 2, 1], [16, 32, 64, 64, 128, 256], BottleneckX, pretrained, **kwargs)


def dla60x_c(pretrained=True, **kwargs):
    BottleneckX.expansion = 2
    return _make('dla60x_c', [1, 1, 1, 2, 3, 1], [16, 32, 64, 64, 128, 256], BottleneckX, pretrained, **kwargs)


def dla60(pretrained=True, **kwargs):
    Bottleneck.expansion = 2
    return _make('dla60', [1, 1, 1, 2, 3, 1], [16, 32, 128, 256, 512, 1024], Bottleneck, pretrained, **kwargs)


def dla60x(pretrained=True, **kwargs):
    BottleneckX.expansion = 2
    return _make('dla60x', [1, 1, 1, 2, 3, 1], [16, 32, 128, 256, 512, 1024], BottleneckX, pretrained, **kwargs)


def dla102(pretrained=True, **kwargs):
    Bottleneck.expansion = 2
    return _make('dla102', [1, 1, 1, 3, 4, 1], [16, 32, 128, 256, 512, 1024], Bottleneck, pretrained,
                 residual_root=True, **kwargs)


def dla102x(pretrained=True, **kwargs):
    BottleneckX.expansion = 2
    return _make('dla102x', [1, 1, 1, 3, 4, 1], [16, 32, 128, 256, 512, 1024], BottleneckX, pretrained,
                 residual_root=True, **kwargs)


def dla102x2(pretrained=True, **kwargs):
    BottleneckX.cardinality = 64        # (stays 64 for every BottleneckX built afterwards, as in the reference)
    return _make('dla102x2', [1, 1, 1, 3, 4, 1], [16, 32, 128, 256, 512, 1024], BottleneckX, pretrained,
                 residual_root=True, **kwargs)


def dla169(pretrained=True, **kwargs):
    Bottleneck.expansion = 2
    return _make('dla169', [1, 1, 2, 3, 5, 1], [16, 32, 128, 256, 512, 1024], Bottleneck, pretrained,
                 residual_root=True, **kwargs)


def dlanet(depth, **kwargs):
    factories = {34: dla34, 60: dla60, 102: dla102, 169: dla169}
    if depth not in factories:
        raise ValueError('Unsupported model depth, must be one of 34, 60, 102, 169')
    return factories[depth](**kwargs)
