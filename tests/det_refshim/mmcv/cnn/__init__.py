"""mmcv.cnn.ConvModule (mmcv 1.6.2) as the head and the FPN build it: conv (nn.Conv2d, or DCNv2 = ModulatedDeformConv2dPack) -> norm
(GroupNorm, registered as `gn`) -> ReLU (`activate`); bias='auto' keeps the conv bias only without a norm; kaiming init of a plain conv
(fan_out, relu), norm weight 1 / bias 0.  MODELS: the registry mm_builder's NECKS derive from."""
import torch.nn as nn

from mmcv.ops import ModulatedDeformConv2dPack
from mmcv.utils import Registry

MODELS = Registry('models')


class ConvModule(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias='auto', conv_cfg=None,
                 norm_cfg=None, act_cfg=dict(type='ReLU'), inplace=True, with_spectral_norm=False, padding_mode='zeros',
                 order=('conv', 'norm', 'act')):
        super().__init__()
        assert order == ('conv', 'norm', 'act') and not with_spectral_norm and padding_mode == 'zeros'
        self.with_norm = norm_cfg is not None
        self.with_activation = act_cfg is not None
        self.with_bias = (not self.with_norm) if bias == 'auto' else bias
        if conv_cfg is None:
            self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, dilation=dilation, groups=groups,
                                  bias=self.with_bias)
        else:
            assert conv_cfg['type'] == 'DCNv2'
            self.conv = ModulatedDeformConv2dPack(in_channels, out_channels, kernel_size, stride=stride, padding=padding,
                                                  dilation=dilation, groups=groups, bias=self.with_bias)
        if self.with_norm:
            assert norm_cfg['type'] == 'GN'
            self.norm_name = 'gn'
            self.add_module('gn', nn.GroupNorm(norm_cfg['num_groups'], out_channels))
        if self.with_activation:
            assert act_cfg['type'] == 'ReLU'
            self.activate = nn.ReLU(inplace=inplace)
        if isinstance(self.conv, nn.Conv2d):
            nn.init.kaiming_normal_(self.conv.weight, a=0, mode='fan_out', nonlinearity='relu')
            if self.conv.bias is not None:
                nn.init.constant_(self.conv.bias, 0)
        if self.with_norm:
            nn.init.constant_(self.gn.weight, 1)
            nn.init.constant_(self.gn.bias, 0)

    def forward(self, x):
        x = self.conv(x)
        if self.with_norm:
            x = self.gn(x)
        if self.with_activation:
            x = self.activate(x)
        return x
