"""DoubleHead (reference lib/heads/double_head.py): Double-Head R-CNN's box head.  The class
scores come from an FC branch over the flattened RoI tile; the box deltas come from a conv
branch (3x3 conv, BatchNorm, ReLU triples over the 7 x 7 tile) followed by FCs.

Each conv / BN / ReLU triple goes through ops.roi_conv3x3_bn_act: one fused HIP launch pair
(frh_roi_conv3x3_bn_act) for an eval-mode head when nothing needs a gradient, the PyTorch
modules otherwise (training: the BN is live and uses batch statistics).  The FCs stay on
PyTorch-ROCm (hipBLASLt).  Takes the RoI extractor's batch tensor directly when available.
"""
import torch
from torch import nn

from .. import ops
from ..utils import init_module_normal, to_pair
from .bbox_head import BBoxHead, HeadOutputs


def _fc_stack(in_features, widths):
    layers = []
    for width in widths:
        layers += [nn.Linear(in_features, width), nn.ReLU(inplace=True)]
        in_features = width
    return nn.Sequential(*layers), in_features


class DoubleHead(BBoxHead):
    def __init__(self, in_channels, roi_out_size=7, cls_fc_channels=(1024, 1024), reg_conv_channels=(256,),
                 reg_conv_strides=(1,), reg_conv_paddings=(1,), reg_fc_channels=(256 * 7 * 7, 1024, 1024),
                 num_classes=21, target_means=(0.0, 0.0, 0.0, 0.0), target_stds=(0.1, 0.1, 0.2, 0.2),
                 add_max_op=False, reg_class_agnostic=False, loss_cls=None, loss_bbox=None):
        super().__init__(num_classes, target_means, target_stds, reg_class_agnostic, loss_cls, loss_bbox)
        self.in_channels = in_channels
        self.roi_out_size = to_pair(roi_out_size)
        self.cls_fc_channels = list(cls_fc_channels)
        self.reg_conv_channels = list(reg_conv_channels)
        self.reg_conv_strides = list(reg_conv_strides)
        self.reg_conv_paddings = list(reg_conv_paddings)
        self.reg_fc_channels = list(reg_fc_channels)
        self.add_max_op = add_max_op
        if len(self.reg_fc_channels) == 0:
            raise AssertionError('reg_fc_channels must name at least the conv branch output width')
        if not (self.roi_out_size[0] == self.roi_out_size[1] == 7):
            raise AssertionError('DoubleHead works on 7 x 7 RoI tiles')
        if not (len(self.reg_conv_channels) == len(self.reg_conv_strides) == len(self.reg_conv_paddings)):
            raise AssertionError('reg_conv_channels / _strides / _paddings: one entry per conv')
        self.init_layers()

    def init_layers(self):
        # class scores: FCs over the flattened tile
        flat = self.in_channels * self.roi_out_size[0] * self.roi_out_size[1]
        self.fc_layer, width = _fc_stack(flat, self.cls_fc_channels)
        self.fc_classifier = nn.Linear(width, self.cls_channels)
        # box deltas: conv / BN / ReLU triples, then FCs from reg_fc_channels[0] inputs
        triples, ch = [], self.in_channels
        for out_ch, stride, pad in zip(self.reg_conv_channels, self.reg_conv_strides, self.reg_conv_paddings):
            triples += [nn.Conv2d(ch, out_ch, 3, stride=stride, padding=pad, bias=False), nn.BatchNorm2d(out_ch),
                        nn.ReLU(inplace=True)]
            ch = out_ch
        self.conv_layer = nn.ModuleList(triples)
        self.reg_fc_layer, width = _fc_stack(self.reg_fc_channels[0], self.reg_fc_channels[1:])
        self.conv_regressor = nn.Linear(width, 4 if self.reg_class_agnostic else self.num_classes * 4)

    def init_weights(self):
        for m in list(self.fc_layer) + list(self.reg_fc_layer):
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                nn.init.constant_(m.bias, 0)
        init_module_normal(self.fc_classifier, mean=0.0, std=0.01)
        for m in self.conv_layer:
            if isinstance(m, nn.Conv2d):
                init_module_normal(m, mean=0.0, std=0.01)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        init_module_normal(self.conv_regressor, mean=0.0, std=0.001)

    def forward(self, rois):
        sizes = [r.shape[0] for r in rois]
        flat = getattr(rois, 'flat', None)
        x = flat if flat is not None else torch.cat(list(rois), 0)
        n = x.shape[0]
        cls_out = self.fc_classifier(self.fc_layer(x.reshape(n, -1)))

        y = x
        for i in range(0, len(self.conv_layer), 3):
            y = ops.roi_conv3x3_bn_act(self.conv_layer[i], self.conv_layer[i + 1], y, relu=True)
        if self.add_max_op:
            y = y.max(dim=-1, keepdim=True)[0] + y.max(dim=-2, keepdim=True)[0]
        reg_out = self.conv_regressor(self.reg_fc_layer(y.reshape(n, -1)))

        cls_outs, reg_outs = HeadOutputs(), HeadOutputs()
        off = 0
        for s in sizes:
            cls_outs.append(cls_out[off:off + s])
            reg_outs.append(reg_out[off:off + s])
            off += s
        cls_outs.flat = (cls_out, reg_out)
        return cls_outs, reg_outs
