"""DCNv2 / DCN modules with the reference's interface (model/DCNv2/dcn_v2.py:14-70,
model/DCNv2/dcn_v2_func.py:13-38), backed by m3d_dcn_v2_forward, and the pooling half of the same two files (dcn_v2.py:73-171,
dcn_v2_func.py:76-146), backed by m3d_dcn_v2_psroi_pooling_forward / _backward."""
import math

import torch
from torch import nn
from torch.nn.modules.utils import _pair

from . import ops


class DCNv2Function:
    """Callable with the reference's legacy instance-style convention:
    ``DCNv2Function(stride, padding, dilation, deformable_groups)(input, offset, mask, weight, bias)``.
    With grad mode on and any of the five tensors requiring grad (the reference's rule, dcn_v2_func.py:25) the call goes through
    the differentiable ``ops.dcn_v2`` (backward of the reference: dcn_v2_func.py:40-62); otherwise it is the plain forward."""

    def __init__(self, stride, padding, dilation=1, deformable_groups=1):
        self.stride, self.padding, self.dilation, self.deformable_groups = stride, padding, dilation, deformable_groups

    def __call__(self, input, offset, mask, weight, bias):
        return self.forward(input, offset, mask, weight, bias)

    def forward(self, input, offset, mask, weight, bias):
        if not input.is_cuda:
            raise NotImplementedError
        if torch.is_grad_enabled() and any(t.requires_grad for t in (input, offset, mask, weight, bias)):
            return ops.dcn_v2(input, offset, mask, weight, bias, self.stride, self.padding, self.dilation, self.deformable_groups)
        with torch.no_grad():
            return ops.dcn_v2_forward(input, offset, mask, weight, bias, self.stride, self.padding, self.dilation,
                                      self.deformable_groups)


class DCNv2(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size = _pair(kernel_size)
        self.stride, self.padding, self.dilation = stride, padding, dilation
        self.deformable_groups = deformable_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, *self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        fan = self.in_channels * self.kernel_size[0] * self.kernel_size[1]
        bound = 1.0 / math.sqrt(fan)
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)
            self.bias.zero_()

    def forward(self, input, offset, mask):
        fn = DCNv2Function(self.stride, self.padding, self.dilation, self.deformable_groups)
        return fn(input, offset, mask, self.weight, self.bias)


class DCN(DCNv2):
    """DCNv2 whose offsets and mask come from its own zero-initialised conv (dcn_v2.py:44-70)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, deformable_groups)
        kk = self.kernel_size[0] * self.kernel_size[1]
        self.conv_offset_mask = nn.Conv2d(in_channels, deformable_groups * 3 * kk, kernel_size=self.kernel_size,
                                          stride=(stride, stride), padding=(padding, padding), bias=True)
        self.init_offset()

    def init_offset(self):
        with torch.no_grad():
            self.conv_offset_mask.weight.zero_()
            self.conv_offset_mask.bias.zero_()

    def forward(self, input):
        if input.is_cuda and torch.is_grad_enabled() and (input.requires_grad or any(p.requires_grad for p in self.parameters())):
            # differentiable form, the reference's composition (dcn_v2.py:64-70): the offset / mask convolution through torch
            out = self.conv_offset_mask(input)
            o1, o2, mask = torch.chunk(out, 3, dim=1)
            offset = torch.cat((o1, o2), dim=1)
            mask = torch.sigmoid(mask)
            return ops.dcn_v2(input.contiguous(), offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation,
                              self.deformable_groups)
        from .standalone import dcn_layer_forward
        return dcn_layer_forward(self, input)


class DCNv2PoolingFunction:
    """Callable with the reference's legacy instance-style convention (dcn_v2_func.py:76-146):
    ``DCNv2PoolingFunction(spatial_scale, pooled_size, output_dim, no_trans, ...)(data, rois, offset)``.  Differentiable in ``data``
    and ``offset`` through ``ops.psroi_pooling``; ``rois`` get no gradient.  ``offset`` is not looked at when ``no_trans`` (the
    modules pass ``data.new()`` there)."""

    def __init__(self, spatial_scale, pooled_size, output_dim, no_trans, group_size=1, part_size=None, sample_per_part=4, trans_std=.0):
        self.spatial_scale, self.pooled_size, self.output_dim, self.no_trans = spatial_scale, pooled_size, output_dim, no_trans
        self.group_size = group_size
        self.part_size = pooled_size if part_size is None else part_size
        self.sample_per_part, self.trans_std = sample_per_part, trans_std
        assert self.trans_std >= 0.0 and self.trans_std <= 1.0

    def __call__(self, data, rois, offset):
        return self.forward(data, rois, offset)

    def _conf(self):
        return (self.no_trans, self.spatial_scale, self.output_dim, self.group_size, self.pooled_size, self.part_size,
                self.sample_per_part, self.trans_std)

    def forward(self, data, rois, offset):
        if not data.is_cuda:
            raise NotImplementedError
        if torch.is_grad_enabled() and (data.requires_grad or (not self.no_trans and offset.requires_grad)):
            return ops.psroi_pooling(data, rois, offset, *self._conf())
        with torch.no_grad():
            return ops.psroi_pooling_forward(data, rois, offset, *self._conf())[0]

    def _infer_shape(self, data, rois):
        return (rois.shape[0], self.output_dim, self.pooled_size, self.pooled_size)


class DCNv2Pooling(nn.Module):
    def __init__(self, spatial_scale, pooled_size, output_dim, no_trans, group_size=1, part_size=None, sample_per_part=4, trans_std=.0):
        super().__init__()
        self.spatial_scale, self.pooled_size, self.output_dim, self.no_trans = spatial_scale, pooled_size, output_dim, no_trans
        self.group_size = group_size
        self.part_size = pooled_size if part_size is None else part_size
        self.sample_per_part, self.trans_std = sample_per_part, trans_std
        self.func = DCNv2PoolingFunction(self.spatial_scale, self.pooled_size, self.output_dim, self.no_trans, self.group_size,
                                         self.part_size, self.sample_per_part, self.trans_std)

    def forward(self, data, rois, offset):
        if self.no_trans:
            offset = data.new_empty(0)
        return self.func(data, rois, offset)


class DCNPooling(DCNv2Pooling):
    """DCNv2Pooling whose offsets and mask come from its own fully connected layers (dcn_v2.py:108-171): pool without offsets,
    offset_fc / mask_fc (last layers zero-initialised), pool with the offsets, times the mask."""

    def __init__(self, spatial_scale, pooled_size, output_dim, no_trans, group_size=1, part_size=None, sample_per_part=4, trans_std=.0,
                 deform_fc_dim=1024):
        super().__init__(spatial_scale, pooled_size, output_dim, no_trans, group_size, part_size, sample_per_part, trans_std)
        self.deform_fc_dim = deform_fc_dim
        if not no_trans:
            self.func_offset = DCNv2PoolingFunction(self.spatial_scale, self.pooled_size, self.output_dim, True, self.group_size,
                                                    self.part_size, self.sample_per_part, self.trans_std)
            feat = self.pooled_size * self.pooled_size * self.output_dim
            self.offset_fc = nn.Sequential(nn.Linear(feat, self.deform_fc_dim), nn.ReLU(inplace=True),
                                           nn.Linear(self.deform_fc_dim, self.deform_fc_dim), nn.ReLU(inplace=True),
                                           nn.Linear(self.deform_fc_dim, self.pooled_size * self.pooled_size * 2))
            self.mask_fc = nn.Sequential(nn.Linear(feat, self.deform_fc_dim), nn.ReLU(inplace=True),
                                         nn.Linear(self.deform_fc_dim, self.pooled_size * self.pooled_size * 1), nn.Sigmoid())
            with torch.no_grad():
                self.offset_fc[4].weight.zero_()
                self.offset_fc[4].bias.zero_()
                self.mask_fc[2].weight.zero_()
                self.mask_fc[2].bias.zero_()

    def forward(self, data, rois):
        if self.no_trans:
            return self.func(data, rois, data.new_empty(0))
        n = rois.shape[0]
        x = self.func_offset(data, rois, data.new_empty(0))
        offset = self.offset_fc(x.view(n, -1)).view(n, 2, self.pooled_size, self.pooled_size)
        mask = self.mask_fc(x.view(n, -1)).view(n, 1, self.pooled_size, self.pooled_size)
        return self.func(data, rois, offset) * mask
