"""Deformable convolution v1 / v2 on the HIP library (dcn.hip).

Mirrors the public surface of the reference's vision_base/networks/ops/dcn/deform_conv.py:54-489: the two autograd
functions, their functional aliases and the four modules, with the same constructor signatures, parameter names,
shapes and initialisation, so that a configuration only changes its `name=` strings.  The CUDA extension behind them
(deform_conv_ext) is replaced by fs_dcn_fwd / fs_dcn_bwd_data / fs_dcn_bwd_weight: there is no column buffer, so
`im2col_step` is accepted and checked (it must divide the batch, :88-90) but sizes nothing.

The functions take logical-NCHW tensors on the device in any memory format.  Activations are computed in
RT.compute_dtype (NHWC, padded channels), offsets and masks stay fp32, weights are packed from the fp32 master per
call, every sum is fp32.  What the kernels do not take (groups > 1, kernels above 3x3, strides above 2) raises
NotImplementedError naming the option, on any device.
"""
import logging
import math

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair, _single

from fsnet_amd.engine.runtime import RT
from fsnet_amd.hip import ops


def _run_forward(ctx, input, offset, mask, weight, bias, stride, padding, dilation, groups, deformable_groups):
    if input.dim() != 4:
        raise ValueError("Expected 4D tensor as input, got %dD tensor instead." % input.dim())
    geo = ops.DcnGeometry(input.shape, weight.shape, stride, padding, dilation, groups, deformable_groups,
                          RT.compute_dtype)
    geo.check_offset(offset, mask)
    if not input.is_cuda:
        raise NotImplementedError("deformable convolution runs on the GPU only (input is on %s)" % input.device)
    x = ops.nchw_to_nhwc(input.detach().float(), None, geo.Ci_p, geo.dtype)
    off = offset.detach().float().contiguous()
    msk = None if mask is None else mask.detach().float().contiguous()
    b = None if bias is None else bias.detach().float().contiguous()
    out = ops.dcn_forward(geo, x, off, msk, ops.dcn_pack(geo, weight, 0), b)
    ctx.geo = geo
    ctx.in_dtypes = [None if t is None else t.dtype for t in (input, offset, mask, weight, bias)]
    ctx.save_for_backward(x, off, msk, weight)
    return out[..., :geo.Co].permute(0, 3, 1, 2).to(input.dtype)


def _run_backward(ctx, grad_output, need):
    """need: five flags (input, offset, mask, weight, bias) -> the five gradients, None where not asked for"""
    if not grad_output.is_cuda:
        raise NotImplementedError("deformable convolution runs on the GPU only")
    geo = ctx.geo
    x, off, msk, weight = ctx.saved_tensors
    dy = ops.nchw_to_nhwc(grad_output.float(), None, geo.Co_p, geo.dtype)
    grads = [None] * 5
    if need[0] or need[1] or need[2]:
        dx, d_off, d_mask = ops.dcn_backward_data(geo, x, off, msk, ops.dcn_pack(geo, weight, 1), dy)
        found = (dx[..., :geo.Ci].permute(0, 3, 1, 2), d_off, d_mask)
        for k in range(3):
            if need[k]:
                grads[k] = found[k].to(ctx.in_dtypes[k])
    if need[3] or need[4]:               # frozen weight and bias: fs_dcn_bwd_weight is not launched
        found = ops.dcn_backward_weight(geo, x, off, msk, dy, want_bias=need[4])
        for k in (3, 4):
            if need[k]:
                grads[k] = found[k - 3].to(ctx.in_dtypes[k])
    return grads


class DeformConvFunction(Function):
    """v1: deform_conv.py:54-150"""

    @staticmethod
    def forward(ctx, input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1,
                im2col_step=64):
        step = min(im2col_step, input.shape[0])
        assert input.shape[0] % step == 0, 'im2col step must divide batchsize'
        return _run_forward(ctx, input, offset, None, weight, None, stride, padding, dilation, groups,
                            deformable_groups)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        n = ctx.needs_input_grad
        g = _run_backward(ctx, grad_output, (n[0], n[1], False, n[2], False))
        return (g[0], g[1], g[3]) + (None,) * 6


class ModulatedDeformConvFunction(Function):
    """v2 (mask and bias): deform_conv.py:153-223"""

    @staticmethod
    def forward(ctx, input, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, groups=1,
                deformable_groups=1):
        return _run_forward(ctx, input, offset, mask, weight, bias, stride, padding, dilation, groups,
                            deformable_groups)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        n = ctx.needs_input_grad
        g = _run_backward(ctx, grad_output, (n[0], n[1], n[2], n[3], ctx.in_dtypes[4] is not None and n[4]))
        return tuple(g) + (None,) * 5


deform_conv = DeformConvFunction.apply
modulated_deform_conv = ModulatedDeformConvFunction.apply


def _uniform_fan_in(module):
    """weight ~ U(-1/sqrt(Ci*R*S), 1/sqrt(Ci*R*S)) (deform_conv.py:269-274, :407-414)"""
    bound = 1.0 / math.sqrt(module.in_channels * module.kernel_size[0] * module.kernel_size[1])
    module.weight.data.uniform_(-bound, bound)


def _offset_conv(module, planes_per_tap):
    """the plain convolution that predicts offsets (and masks): same geometry as the module, zero-initialised"""
    conv = nn.Conv2d(module.in_channels,
                     module.deformable_groups * planes_per_tap * module.kernel_size[0] * module.kernel_size[1],
                     kernel_size=module.kernel_size, stride=_pair(module.stride), padding=_pair(module.padding),
                     dilation=_pair(module.dilation), bias=True)
    return conv


def _zero(conv):
    conv.weight.data.zero_()
    conv.bias.data.zero_()


def _rename_legacy_offset_keys(state_dict, prefix, local_metadata):
    """checkpoints older than version 2 name the offset convolution `<module>_offset.*` (deform_conv.py:344-359, :469-485)"""
    version = local_metadata.get('version', None)
    if version is None or version < 2:
        for leaf in ('weight', 'bias'):
            new, old = prefix + 'conv_offset.' + leaf, prefix[:-1] + '_offset.' + leaf
            if new not in state_dict and old in state_dict:
                state_dict[new] = state_dict.pop(old)
    return version


class DeformConv(nn.Module):
    """deform_conv.py:230-292"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 deformable_groups=1, bias=False):
        super().__init__()
        assert not bias
        assert in_channels % groups == 0, 'in_channels %d is not divisible by groups %d' % (in_channels, groups)
        assert out_channels % groups == 0, 'out_channels %d is not divisible by groups %d' % (out_channels, groups)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride = _pair(kernel_size), _pair(stride)
        self.padding, self.dilation = _pair(padding), _pair(dilation)
        self.groups, self.deformable_groups = groups, deformable_groups
        self.transposed, self.output_padding = False, _single(0)      # as nn.Conv2d has them
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *self.kernel_size))
        self.reset_parameters()

    def reset_parameters(self):
        _uniform_fan_in(self)

    def forward(self, x, offset):
        # an input smaller than the kernel: pad input and offsets up to it at the bottom / right, crop the output
        # back (deform_conv.py:279-291)
        grow_h = max(self.kernel_size[0] - x.size(2), 0)
        grow_w = max(self.kernel_size[1] - x.size(3), 0)
        if grow_h or grow_w:
            x = F.pad(x, (0, grow_w, 0, grow_h)).contiguous()
            offset = F.pad(offset, (0, grow_w, 0, grow_h)).contiguous()
        out = deform_conv(x, offset, self.weight, self.stride, self.padding, self.dilation, self.groups,
                          self.deformable_groups)
        if grow_h or grow_w:
            out = out[:, :, :out.size(2) - grow_h, :out.size(3) - grow_w].contiguous()
        return out


class DeformConvPack(DeformConv):
    """DeformConv that predicts its own offsets with `conv_offset`; offset channels are (y0, x0, y1, x1, ...) over the
    taps in row-major order (deform_conv.py:295-369)"""

    _version = 2

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.conv_offset = _offset_conv(self, 2)
        self.init_offset()

    def init_offset(self):
        _zero(self.conv_offset)

    def forward(self, x):
        return deform_conv(x, self.conv_offset(x), self.weight, self.stride, self.padding, self.dilation, self.groups,
                           self.deformable_groups)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        version = _rename_legacy_offset_keys(state_dict, prefix, local_metadata)
        if version is not None and version > 1:
            logging.getLogger('root').info('DeformConvPack %s is upgraded to version 2.', prefix.rstrip('.'))
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)


class ModulatedDeformConv(nn.Module):
    """deform_conv.py:372-419 (stride / padding / dilation are kept as given, not as pairs)"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 deformable_groups=1, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size = _pair(kernel_size)
        self.stride, self.padding, self.dilation = stride, padding, dilation
        self.groups, self.deformable_groups = groups, deformable_groups
        self.with_bias = bias
        self.transposed, self.output_padding = False, _single(0)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *self.kernel_size))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.init_weights()

    def init_weights(self):
        _uniform_fan_in(self)
        if self.bias is not None:
            self.bias.data.zero_()

    def forward(self, x, offset, mask):
        return modulated_deform_conv(x, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation,
                                     self.groups, self.deformable_groups)


class ModulatedDeformConvPack(ModulatedDeformConv):
    """ModulatedDeformConv that predicts offsets and masks with `conv_offset` (deform_conv.py:422-490)"""

    _version = 2

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.conv_offset = _offset_conv(self, 3)
        self.init_weights()

    def init_weights(self):
        super().init_weights()
        if hasattr(self, 'conv_offset'):
            _zero(self.conv_offset)

    def forward(self, x):
        # chunk -> cat -> sigmoid of deform_conv.py:460-467
        o1, o2, mask = torch.chunk(self.conv_offset(x), 3, dim=1)
        return modulated_deform_conv(x, torch.cat((o1, o2), dim=1), torch.sigmoid(mask), self.weight, self.bias,
                                     self.stride, self.padding, self.dilation, self.groups, self.deformable_groups)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        _rename_legacy_offset_keys(state_dict, prefix, local_metadata)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)
