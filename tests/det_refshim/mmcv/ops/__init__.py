"""mmcv.ops.ModulatedDeformConv2dPack (mmcv 1.6.2, deform_groups = groups = 1) restated in plain torch: parameters weight, bias and
conv_offset (zero-initialised); forward o1, o2, m = chunk(conv_offset(x), 3); offset = cat(o1, o2); mask = sigmoid(m); the sampling is
det_ref.dcn_v2."""
import math

import torch
import torch.nn as nn

import det_ref


class ModulatedDeformConv2dPack(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deform_groups=1, bias=True):
        super().__init__()
        assert groups == 1 and deform_groups == 1 and kernel_size in (3, (3, 3))
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.dilation = (3, 3), stride, padding, dilation
        self.weight = nn.Parameter(torch.Tensor(out_channels, in_channels, 3, 3))
        if bias:
            self.bias = nn.Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter('bias', None)
        stdv = 1.0 / math.sqrt(in_channels * 9)
        self.weight.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.zero_()
        self.conv_offset = nn.Conv2d(in_channels, 27, 3, stride=stride, padding=padding, dilation=dilation, bias=True)
        self.conv_offset.weight.data.zero_()
        self.conv_offset.bias.data.zero_()

    def forward(self, x):
        out = self.conv_offset(x)
        o1, o2, mask = torch.chunk(out, 3, dim=1)
        return det_ref.dcn_v2(x, torch.cat((o1, o2), dim=1), torch.sigmoid(mask), self.weight, self.bias, self.stride, self.padding,
                              self.dilation)
