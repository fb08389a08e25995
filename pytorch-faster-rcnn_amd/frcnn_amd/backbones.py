"""ResNet and VGG16 backbones.

ResNet (PyTorch-ROCm convs, MIOpen, with the fused HIP entries of ops where nothing needs a
gradient):

Behaviour follows the reference's own ResNet (`lib/backbones.py:133-255`):
bottleneck blocks with the stride on the 3x3 conv, a 1x1 conv + BN projection
on the first block of every stage, frozen-BN training mode and
`frozen_stages` parameter freezing.  Parameter names are kept identical
(`conv1`, `bn1`, `layerK.i.convJ`, `layerK.0.downsample.{0,1}`) so state
dicts move between the two frameworks unchanged.

No pretrained download exists here (no network); `init_weights` uses a
deterministic Kaiming init when `pretrained` is requested and cannot be
satisfied, and says so.

VGG16 (reference `lib/backbones.py:7-31`, a wrapper of torchvision's `vgg16.features[:30]`): the
layer list is restated here under torchvision's parameter names; its thirteen 3x3 convs run as
the fused Winograd HIP entries, the four max pools in their epilogues (`ops.vgg_conv`,
`ops.vgg_stem`), where nothing needs a gradient.
"""
import logging

import torch
from torch import nn

from . import ops
from .ops import (bn_act_maxpool, conv1x1_bn_act, conv1x1_pre_fused_ok, conv1x1_s2_bn_act, conv3x3_nchw_bn_act,
                  conv3x3_nchw_fused_ok)
from .utils import ChannelsLastConvs

# blocks per stage for each depth
_STAGE_BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
_STAGE_WIDTH = (64, 256, 512, 1024, 2048)


def _conv_bn(cin, cout, k, stride=1, pad=0):
    return nn.Conv2d(cin, cout, k, stride=stride, padding=pad, bias=False), nn.BatchNorm2d(cout)


class Bottleneck(nn.Module):
    """1x1 -> 3x3 (strided) -> 1x1, expansion 4 (reference `backbones.py:133-168`)."""

    def __init__(self, in_channels, out_channels, downsample=False):
        super().__init__()
        mid = out_channels // 4
        first_stage = in_channels * 4 == out_channels
        stride = 2 if (downsample and not first_stage) else 1
        self.conv1, self.bn1 = _conv_bn(in_channels, mid, 1)
        self.conv2, self.bn2 = _conv_bn(mid, mid, 3, stride=stride, pad=1)
        self.conv3, self.bn3 = _conv_bn(mid, out_channels, 1)
        self.relu = nn.ReLU(inplace=True)
        self.do_downsample = downsample
        if downsample:
            self.downsample = nn.Sequential(*_conv_bn(in_channels, out_channels, 1, stride=stride))

    def forward(self, x):
        # frozen BN (+ residual) + ReLU: inside the 1x1 convs' HIP GEMM where nothing needs a
        # gradient (ops.conv1x1_bn_act, ops.conv1x1_s2_bn_act for the stride-2 projections; every
        # training path falls through to conv + ops.bn_act).  The 3x3 conv's BN + ReLU is applied
        # on conv3's input side (pre_bn), or by one HIP epilogue pass (ops.bn_act) where it cannot.
        # A stride-1 3x3 conv runs as the fused NCHW Winograd entry where its class is dispatched
        # (ops.conv3x3_nchw_bn_act): raw where conv3 takes bn2 on its input side, with bn2 + ReLU
        # in its own epilogue where conv3 cannot (no separate pass either way).
        y = conv1x1_bn_act(self.conv1, self.bn1, x)
        fused2 = conv3x3_nchw_fused_ok(self.conv2, y, self.bn2)
        if not fused2:
            y = self.conv2(y)  # before the projection, as ever: the order of the autograd graph
        skip = x
        if self.do_downsample:
            proj = conv1x1_s2_bn_act if self.downsample[0].stride == (2, 2) else conv1x1_bn_act
            skip = proj(self.downsample[0], self.downsample[1], x, relu=False)
        if not fused2:
            return conv1x1_bn_act(self.conv3, self.bn3, y, skip=skip, pre_bn=self.bn2)
        # y stands in for conv2's output in conv3's predicate: same shape, layout and allocator
        if conv1x1_pre_fused_ok(self.conv3, self.bn3, y, self.bn2, skip):
            y = conv3x3_nchw_bn_act(self.conv2, y)
            return conv1x1_bn_act(self.conv3, self.bn3, y, skip=skip, pre_bn=self.bn2)
        y = conv3x3_nchw_bn_act(self.conv2, y, self.bn2, relu=True)
        return conv1x1_bn_act(self.conv3, self.bn3, y, skip=skip)


class ResNet(nn.Module):
    def __init__(self, depth=50, frozen_stages=1, out_layers=(1, 2, 3, 4), pretrained=True):
        super().__init__()
        if depth not in _STAGE_BLOCKS:
            raise AssertionError('unsupported ResNet depth {}'.format(depth))
        self.depth = depth
        self.pretrained = pretrained
        self.frozen_stages = frozen_stages
        self.out_layers = tuple(out_layers)
        self.conv_cfg = _STAGE_BLOCKS[depth]
        self.conv1, self.bn1 = _conv_bn(3, 64, 7, stride=2, pad=3)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        for s, nblk in enumerate(self.conv_cfg):
            cin, cout = _STAGE_WIDTH[s], _STAGE_WIDTH[s + 1]
            blocks = [Bottleneck(cin, cout, True)] + [Bottleneck(cout, cout) for _ in range(nblk - 1)]
            setattr(self, 'layer{}'.format(s + 1), nn.Sequential(*blocks))

    def forward(self, x):
        # frozen stem: BN + ReLU + max pool as one HIP pass (ops.bn_act_maxpool)
        x = bn_act_maxpool(self.conv1(x), self.bn1, self.maxpool)
        outs = []
        for s in range(1, 5):
            x = getattr(self, 'layer{}'.format(s))(x)
            if s in self.out_layers:
                outs.append(x)
        return outs

    def freeze_stages(self, stages):
        frozen = []
        if stages >= 0:
            self.bn1.eval()
            frozen += [self.conv1, self.bn1]
        for s in range(1, stages + 1):
            layer = getattr(self, 'layer{}'.format(s))
            layer.eval()
            frozen.append(layer)
        for m in frozen:
            for p in m.parameters():
                p.requires_grad = False

    def train(self, mode=True):
        super().train(mode)
        self.freeze_stages(self.frozen_stages)
        if mode:
            # BN statistics stay frozen during training (reference backbones.py:241-247)
            for m in self.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.eval()
        return self

    def init_weights(self):
        if self.pretrained:
            logging.warning('ResNet: pretrained weights unavailable offline; using random init')
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)


class ResLayerC5(nn.Module):
    """Stage-5 shared head for C4 detectors (reference `backbones.py:100-127`)."""

    def __init__(self, depth=50):
        super().__init__()
        nblk = _STAGE_BLOCKS[depth][3]
        self.res_layer = nn.Sequential(Bottleneck(1024, 2048, True),
                                       *[Bottleneck(2048, 2048) for _ in range(nblk - 1)])

    def train(self, mode=True):
        super().train(mode)
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()
        return self

    def forward(self, x):
        return self.res_layer(x)

    def init_weights(self):
        pass


# torchvision's vgg16 configuration 'D' up to conv5_3: output channels, 'M' a 2x2 / stride-2 max pool
_VGG16_LAYERS = (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512)


class VGG16(ChannelsLastConvs):
    """The reference's VGG16 (`lib/backbones.py:7-31`): `features` is torchvision's
    `vgg16.features[:30]` -- thirteen Conv2d 3x3 / padding 1 + ReLU, MaxPool2d(2, 2) at indices
    4, 9, 16, 23, ending on the ReLU at 29 (stride 16, 512 channels) -- with torchvision's state
    dict keys (`features.N.weight` / `.bias`), so its pretrained weights load unchanged.
    `freeze_first_layers` fixes the parameters of `features[:10]`.

    Deviations: forward returns `[x]`, the one-level list every detector
    consumes (the reference returns the bare tensor, which none of its detectors can take);
    `classifier_` / `get_classifier` is not mirrored (the fc6 / fc7 pair is
    `RCNNHead(fc_channels=[4096, 4096])` in the config)."""

    def __init__(self, freeze_first_layers=True, pretrained=True):
        super().__init__()
        self.pretrained = pretrained
        self.freeze_first_layers = freeze_first_layers
        layers, cin = [], 3
        for v in _VGG16_LAYERS:
            if v == 'M':
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        self.features = nn.Sequential(*layers)
        if freeze_first_layers:
            for layer in self.features[:10]:
                for p in layer.parameters():
                    p.requires_grad = False

    def forward(self, x):
        # conv + ReLU (+ the max pool behind it) per step: the fused entries where nothing needs
        # a gradient (inference; the frozen layers 0-9 in a training step), the modules' ops
        # otherwise and on the CPU.  No host synchronisation either way.
        if not x.is_cuda:
            return [self.features(x)]
        mods = list(self.features)
        x = ops.vgg_stem(mods[0], x)
        for i in range(2, len(mods)):
            if isinstance(mods[i], nn.Conv2d):
                pool = i + 2 < len(mods) and isinstance(mods[i + 2], nn.MaxPool2d)
                x = ops.vgg_conv(mods[i], x, pool=pool)
        return [x]

    def init_weights(self):
        if self.pretrained:
            logging.warning('VGG16: pretrained weights unavailable offline; using random init')
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                nn.init.zeros_(m.bias)
