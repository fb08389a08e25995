"""DeformConv: the deformable (DCNv1) convolution module the reference imports from
mmdet.ops.dcn (lib/heads/guided_head.py:3,95), for the one form the reference uses: kernel 3,
stride 1, padding 1, dilation 1, no bias, `deformable_groups` offset groups.

Inference runs the fused HIP kernel (ops.deform_conv3x3: frh_deform_conv3x3_act).  Wherever a
gradient is needed the module by default takes ops.deform_conv3x3_torch, the gather + matmul
restatement autograd differentiates; with the class attribute `hip_grad = True` it keeps the HIP
forward and runs frh_deform_conv3x3_bwd (csrc/deform_conv3x3_bwd.hip) as its backward wherever
ops.deform_conv3x3 allows it (HIP f32 tensors, accepted shapes, no deterministic backward asked
for)."""
import math

import torch
from torch import nn

from . import ops


class DeformConv(nn.Module):
    hip_grad = False  # True: training runs on the HIP forward and backward entries

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, groups=1,
                 deformable_groups=1, bias=False):
        super().__init__()
        if (kernel_size, stride, padding, dilation, groups) not in ((3, 1, 1, 1, 1), ((3, 3), (1, 1), (1, 1), (1, 1), 1)):
            raise ValueError('DeformConv: only kernel 3, stride 1, padding 1, dilation 1, groups 1 is implemented')
        if bias:
            raise ValueError('DeformConv has no bias (mmdet.ops.dcn.DeformConv)')
        if in_channels % deformable_groups:
            raise ValueError('in_channels must be divisible by deformable_groups')
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.deformable_groups = deformable_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 3, 3))
        self.reset_parameters()

    def reset_parameters(self):
        # mmdet v1's DeformConv.reset_parameters: uniform(-stdv, stdv), stdv = 1 / sqrt(cin * 9)
        stdv = 1.0 / math.sqrt(self.in_channels * 9)
        with torch.no_grad():
            self.weight.uniform_(-stdv, stdv)

    def forward(self, x, offset, relu=False):
        return ops.deform_conv3x3(x, offset, self.weight, self.deformable_groups, relu, hip_grad=self.hip_grad)

    def extra_repr(self):
        return '{}, {}, kernel_size=3, padding=1, deformable_groups={}, bias=False'.format(
            self.in_channels, self.out_channels, self.deformable_groups)
