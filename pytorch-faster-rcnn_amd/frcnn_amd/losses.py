"""Detection losses (reference lib/losses.py), sum reductions.

On HIP tensors FocalLoss, CrossEntropyLoss and SmoothL1Loss run the fused loss
kernels (csrc/losses.hip): one streaming pass forward and one
backward instead of a dozen elementwise torch passes.  The torch expressions
below are the reference restatement; they serve CPU tensors and are the
numerics reference of the GPU tests.  Semantics follow the reference, including
its quirk that FocalLoss ignores the configured alpha/gamma/loss_weight
(losses.py:106-109).
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import ops, utils


def zero_loss(device):
    return torch.zeros((), device=device, requires_grad=True)


def smooth_l1_loss_v2(x, y, beta):
    """losses.py:77-83: sum of 0.5 d^2 / beta (d < beta) or d - 0.5 beta."""
    if beta <= 0 or x.shape != y.shape:
        raise AssertionError('bad smooth-l1 arguments')
    d = torch.abs(x - y)
    small = (d < beta).float()
    return (small * (d ** 2) / (2 * beta) + (1 - small) * (d - 0.5 * beta)).sum()


def sigmoid_focal_loss(pred, target, alpha=0.25, gamma=2.0, fix_alpha=False):
    """losses.py:33-61: pred [n, C] logits, target [n] in 0..C (0 = background)."""
    n, c = pred.shape
    onehot = utils.one_hot_embedding(target, c + 1)[:, 1:].to(pred.dtype)
    p = pred.sigmoid()
    pt = p * onehot + (1 - p) * (1 - onehot)
    w = alpha if fix_alpha else alpha * onehot + (1 - alpha) * (1 - onehot)
    w = w * (1 - pt).pow(gamma)
    return (F.binary_cross_entropy_with_logits(pred, onehot, reduction='none') * w).sum()


def giou_loss(a, b):
    """losses.py:13-30: 1 - GIoU on [4, n] boxes (no +1 widths)."""
    tl = torch.max(a[:2], b[:2])
    br = torch.min(a[2:], b[2:])
    area_i = torch.prod(br - tl, dim=0) * (tl < br).all(0).float()
    area_a = torch.prod(a[2:] - a[:2], dim=0)
    area_b = torch.prod(b[2:] - b[:2], dim=0)
    area_u = area_a + area_b - area_i
    iou = area_i / area_u
    lo = torch.min(a[:2], b[:2])
    hi = torch.max(a[2:], b[2:])
    area_c = torch.prod(hi - lo, dim=0)
    return 1 - (iou - (area_c - area_u) / area_c)


class FocalLoss(nn.Module):
    def __init__(self, alpha=0.25, gamma=2.0, use_sigmoid=True, loss_weight=1.0):
        if not use_sigmoid:
            raise AssertionError('FocalLoss for non sigmoid is not implemented')
        super().__init__()
        self.use_sigmoid = True
        self.alpha, self.gamma, self.loss_weight = 0.25, 2.0, 1.0  # reference ignores the cfg values

    def forward(self, pred, target):
        if pred.is_cuda:
            return self.loss_weight * ops.cls_loss(pred, target, ops.CLS_FOCAL, self.alpha, self.gamma)
        return self.loss_weight * sigmoid_focal_loss(pred, target, self.alpha, self.gamma)


class SmoothL1Loss(nn.Module):
    def __init__(self, beta=1.0, loss_weight=1.0):
        super().__init__()
        self.beta, self.loss_weight = beta, loss_weight

    def forward(self, x, y):
        if x.is_cuda and x.dim() == 2:
            return self.loss_weight * ops.smooth_l1_loss(x, y, self.beta)
        return self.loss_weight * smooth_l1_loss_v2(x, y, self.beta)

    def masked(self, x, y, label, rows_dim=0):
        """Sum over the rows with label > 0 only (the reference's positive-row selection,
        anchor_head.py:126-128, without its boolean-index host sync)."""
        if x.is_cuda:
            return self.loss_weight * ops.smooth_l1_loss(x, y, self.beta, label, rows_dim)
        m = (label > 0).view(-1, 1) if rows_dim == 0 else (label > 0).view(1, -1)
        z = x.new_zeros(())
        return self.loss_weight * smooth_l1_loss_v2(torch.where(m, x, z), torch.where(m, y, z), self.beta)

    def class_selected(self, reg_out, num_classes, target, label):
        """bbox_head.py:70-76: the labelled class's deltas of reg_out [n, 4*C] at the positive rows."""
        if reg_out.is_cuda:
            return self.loss_weight * ops.smooth_l1_class_select(reg_out, num_classes, target, label, self.beta)
        n = len(label)
        sel = reg_out.view(-1, 4, num_classes)[torch.arange(n), :, label]
        return self.masked(sel, target, label, 0)


def balanced_l1_loss(pred, target, beta=1.0, alpha=0.5, gamma=1.5):
    """losses.py:158-168 (elementwise; borrowed from mmdet by the reference)."""
    if pred.size() != target.size():
        raise AssertionError('balanced_l1_loss: shape mismatch')
    diff = torch.abs(pred - target)
    b = np.e ** (gamma / alpha) - 1
    return torch.where(diff < beta,
                       alpha / b * (b * diff + 1) * torch.log(b * diff / beta + 1) - alpha * diff,
                       gamma * diff + gamma / b - alpha * beta)


def balanced_l1_slope(d, beta=1.0, alpha=0.5, gamma=1.5):
    """d/dd of the balanced-L1 element at d = |pred - target| (what the HIP backward
    multiplies by sign(pred - target)): alpha log(b d / beta + 1) + alpha (b d + 1) / (b d + beta)
    - alpha below beta, gamma from beta on."""
    b = np.e ** (gamma / alpha) - 1
    return torch.where(d < beta, alpha * torch.log(b * d / beta + 1) + alpha * (b * d + 1) / (b * d + beta) - alpha,
                       torch.full_like(d, gamma))


class BalancedL1Loss(nn.Module):
    """losses.py:170-180; the HIP forms mirror SmoothL1Loss's (plain, masked, class-selected)."""

    def __init__(self, alpha=0.5, gamma=1.5, beta=1.0, loss_weight=1.0):
        super().__init__()
        self.alpha, self.gamma, self.beta, self.loss_weight = alpha, gamma, beta, loss_weight

    def _cpu(self, x, y):
        return balanced_l1_loss(x, y, beta=self.beta, alpha=self.alpha, gamma=self.gamma).sum()

    def forward(self, pred, label):
        if pred.is_cuda and pred.dim() == 2:
            return self.loss_weight * ops.balanced_l1_loss(pred, label, self.beta, self.alpha, self.gamma)
        return self._cpu(pred, label) * self.loss_weight

    def masked(self, x, y, label, rows_dim=0):
        if x.is_cuda:
            return self.loss_weight * ops.balanced_l1_loss(x, y, self.beta, self.alpha, self.gamma, label, rows_dim)
        m = (label > 0).view(-1, 1) if rows_dim == 0 else (label > 0).view(1, -1)
        z = x.new_zeros(())
        return self.loss_weight * self._cpu(torch.where(m, x, z), torch.where(m, y, z))

    def class_selected(self, reg_out, num_classes, target, label):
        if reg_out.is_cuda:
            return self.loss_weight * ops.balanced_l1_class_select(reg_out, num_classes, target, label, self.beta,
                                                                   self.alpha, self.gamma)
        n = len(label)
        sel = reg_out.view(-1, 4, num_classes)[torch.arange(n), :, label]
        return self.masked(sel, target, label, 0)


class CrossEntropyLoss(nn.Module):
    def __init__(self, use_sigmoid=False, loss_weight=1.0):
        super().__init__()
        self.use_sigmoid, self.loss_weight = use_sigmoid, loss_weight

    def forward(self, pred, label):
        c = pred.shape[1]
        if pred.is_cuda:
            if self.use_sigmoid:
                kind = ops.CLS_SIGMOID_BCE
                label = label.reshape(-1)  # C == 1: label.view(-1, 1).float() is the target itself
            else:
                kind = ops.CLS_SOFTMAX_CE
            return ops.cls_loss(pred, label, kind) * self.loss_weight
        if self.use_sigmoid:
            if c == 1:
                tgt = label.view(-1, 1).float()
            else:
                tgt = utils.one_hot_embedding(label, c + 1)[:, 1:].to(pred.dtype)
            return F.binary_cross_entropy_with_logits(pred, tgt, reduction='none').sum() * self.loss_weight
        return F.cross_entropy(pred, label, reduction='none').sum() * self.loss_weight


class BoundedIoULoss(nn.Module):
    """losses.py:182-193: smooth-L1 (beta) of 1 - min(x / y, y / x) on x + 1e-6, y + 1e-6 against
    zero, summed; the Guided Anchoring shape loss on (dw, dh).  loss_weight is accepted and, as in
    the reference, not applied.  Torch ops (a few hundred sampled positives)."""

    def __init__(self, beta=0.2, loss_weight=1.0):
        super().__init__()
        self.beta, self.loss_weight = beta, loss_weight

    def forward(self, x, y):
        if x.shape != y.shape:
            raise AssertionError('BoundedIoULoss: x and y shapes differ')
        x = x + 1e-6
        y = y + 1e-6
        loss = 1 - torch.min(x / y, y / x)
        return smooth_l1_loss_v2(loss, loss.new_zeros(loss.size()), self.beta)


def fused_kinds(loss_cls, loss_bbox):
    """True when head_losses can run this pair of loss modules as one launch."""
    return isinstance(loss_bbox, SmoothL1Loss) and isinstance(loss_cls, (FocalLoss, CrossEntropyLoss))


def head_losses(loss_cls, loss_bbox, cls_x, cls_label, l1_args, avg_factor, div_count=None):
    """(loss_cls(cls_x, cls_label) / avg_factor, loss_bbox.<masked | class_selected>(...) /
    avg_factor) as ONE HIP launch (ops.det_losses) when both modules are the HIP-backed
    kinds, the tensors are on the GPU and avg_factor is a host number (the sampled count);
    l1_args() builds the regression loss's arguments.  None when it does not apply (the
    caller then runs the modules one by one).  div_count (device int32 [1]) replaces
    avg_factor for sync-free targets: padding rows (label -1) are ignored."""
    if div_count is not None:
        if not (cls_x.is_cuda and fused_kinds(loss_cls, loss_bbox)):
            raise AssertionError('sync-free targets need the fused HIP head losses')
        avg_factor = div_count
    elif not (cls_x.is_cuda and isinstance(loss_bbox, SmoothL1Loss)) or isinstance(avg_factor, torch.Tensor):
        return None
    if isinstance(loss_cls, FocalLoss):
        kind, alpha, gamma = ops.CLS_FOCAL, loss_cls.alpha, loss_cls.gamma
    elif isinstance(loss_cls, CrossEntropyLoss):
        kind, alpha, gamma = (ops.CLS_SIGMOID_BCE if loss_cls.use_sigmoid else ops.CLS_SOFTMAX_CE), 0.25, 2.0
    else:
        return None
    return ops.det_losses(cls_x, cls_label.reshape(-1), kind, alpha, gamma, loss_cls.loss_weight, l1_args(),
                          loss_bbox.beta, loss_bbox.loss_weight, avg_factor)


class GIoULoss(nn.Module):
    def __init__(self, loss_weight=1.0):
        super().__init__()
        self.loss_weight = loss_weight

    def forward(self, a, b, weight=None, avg_factor=1.0):
        loss = giou_loss(a, b)
        if weight is not None:
            loss = loss * weight
        return loss.sum() * self.loss_weight / avg_factor


class IoULoss(nn.Module):
    def __init__(self, loss_weight=1.0):
        super().__init__()
        self.loss_weight = loss_weight

    def forward(self, a, b, weight=None, avg_factor=None):
        loss = -utils.elem_iou(a, b).log()
        if weight is not None:
            loss = loss * weight
        if avg_factor is not None:
            loss = loss / avg_factor
        return loss.sum() * self.loss_weight


def generalized_focal_loss(pred, tar, beta=2.0):
    """losses.py:221-224 (elementwise, logits pred)."""
    focal_weight = (tar - pred.sigmoid()).abs().pow(beta)
    return focal_weight * F.binary_cross_entropy_with_logits(pred, tar, reduction='none')


class QualityFocalLoss(nn.Module):
    """losses.py:226-249: pred [n, C] logits, quality [n], label [n] in 0..C."""

    def __init__(self, beta=2.0, use_sigmoid=True, loss_weight=1.0):
        if not use_sigmoid:
            raise AssertionError('QualityFocalLoss only support sigmoid activation')
        super().__init__()
        self.use_sigmoid, self.beta, self.loss_weight = use_sigmoid, beta, loss_weight

    def forward(self, pred, quality, label, weight=None, avg_factor=1.0):
        n, n_cls = pred.shape
        tar = pred.new_zeros((n, n_cls + 1))
        tar[torch.arange(n, device=pred.device), label] = quality
        loss = generalized_focal_loss(pred, tar[:, 1:], beta=self.beta)
        if weight is not None:
            loss = loss * weight
        return loss.sum() * self.loss_weight / avg_factor


def log_softmax_with_logits(logits):
    """losses.py:251-254: row-wise stable log-softmax."""
    c, _ = logits.detach().max(1)
    s = logits - c.unsqueeze(1)
    return s - s.exp().sum(1).log().unsqueeze(1)


class DistributionFocalLoss(nn.Module):
    """losses.py:256-285: pred [n, cls_channels] logits, y [n], left_idx [n]."""

    def __init__(self, cls_channels, stride, norm_prob, loss_weight=1.0):
        super().__init__()
        self.cls_channels, self.stride, self.norm_prob, self.loss_weight = cls_channels, stride, norm_prob, loss_weight

    def forward(self, pred, y, left_idx, weight=None, avg_factor=1.0):
        n = pred.shape[0]
        ar = torch.arange(n, device=pred.device)
        log_sigma = log_softmax_with_logits(pred)
        right_idx = left_idx + 1
        y_left, y_right = left_idx * self.stride, right_idx * self.stride
        loss = (y_right - y) * log_sigma[ar, left_idx] + (y - y_left) * log_sigma[ar, right_idx]
        if self.norm_prob:
            loss = loss / self.stride
        return -loss.sum() * self.loss_weight / avg_factor


def gfl_head_losses_torch(cls_outs, reg_outs, labels, ltrb, bins, stride, reg_mean=0.0, reg_std=1.0,
                          norm_prob=False, beta=2.0, cls_weight=1.0, dfl_weight=1.0, bbox_weight=1.0,
                          dfl_avg_factor=4.0):
    """The GFL head's three losses (reference FCOSHead.calc_loss with QualityFocalLoss,
    DistributionFocalLoss and GIoULoss, fcos_head.py:419-515) restated in torch ops, expression
    for expression: the numerics reference of ops.gfl_losses (csrc/gfl.hip) and what FCOSHead
    runs off the fused path.  CPU (f32 / f64) or HIP tensors; no ops call.

    cls_outs [C, M] and reg_outs [4*bins, M] logits (regression channel = bin*4 + side), labels
    [M] int64 (-1 ignored, 0 negative, > 0 the class), ltrb [M, 4] pixels; positions ordered
    images outer, levels inner.  Returns (cls_loss, dfl_loss, bbox_loss, num_pos [int64 0-d]).

    Two points where the reference raises and this (like the kernel) does not: with no positive
    the sums are divided by max(num_pos, 1); and a target in the top bin (left == bins-1, the
    reference indexes bin `bins`) keeps the left-hand DFL term only."""
    chosen, pos = labels >= 0, labels > 0
    num_pos = pos.sum()
    div = num_pos.clamp(min=1).to(cls_outs.dtype)
    w, _ = cls_outs.detach()[:, pos].sigmoid().max(0)
    y4 = (ltrb[pos, :].t() - reg_mean) / reg_std                       # [4, m]
    y = y4.contiguous().view(-1)                                       # [4m], side-major
    # length2class (fcos_head.py:10-29): f32 whatever the input's dtype
    left = (y.float().clamp(0, (bins - 1) * stride) / stride).long()
    right = left + 1
    x = reg_outs[:, pos].reshape(bins, -1).t()                         # [4*bins, m] -> [bins, 4m] -> [4m, bins]
    ar = torch.arange(x.shape[0], device=x.device)
    log_sigma = log_softmax_with_logits(x)
    y_left, y_right = left * stride, right * stride
    right_term = (y - y_left) * log_sigma[ar, right.clamp(max=bins - 1)]
    loss = (y_right - y) * log_sigma[ar, left] + torch.where(right < bins, right_term, torch.zeros_like(right_term))
    if norm_prob:
        loss = loss / stride
    dfl_loss = -loss.sum() * dfl_weight / dfl_avg_factor
    # class2length (fcos_head.py:32-42) and simple_ltrb2bbox around (0, 0)
    rand_var = x.new_tensor([i * stride for i in range(bins)])
    out4 = (x.softmax(-1) * rand_var).sum(-1).view(4, -1)
    a = torch.stack([0.0 - out4[0], 0.0 - out4[1], 0.0 + out4[2], 0.0 + out4[3]])
    b = torch.stack([0.0 - y4[0], 0.0 - y4[1], 0.0 + y4[2], 0.0 + y4[3]])
    a_d = a.detach()
    tl, br = torch.max(a_d[:2], b[:2]), torch.min(a_d[2:], b[2:])      # utils.elem_iou (lib/utils.py:174-182)
    area_i = torch.prod(br - tl, dim=0) * (tl < br).all(0).float()
    quality = area_i / (torch.prod(a_d[2:] - a_d[:2], dim=0) + torch.prod(b[2:] - b[:2], dim=0) - area_i)
    bbox_loss = (giou_loss(a, b) * w).sum() * bbox_weight / div
    q_all = quality.new_zeros(labels.numel())
    q_all[pos] = quality
    pred = cls_outs[:, chosen].t()
    n, n_cls = pred.shape
    tar = pred.new_zeros((n, n_cls + 1))
    tar[torch.arange(n, device=pred.device), labels[chosen]] = q_all[chosen]
    cls_loss = generalized_focal_loss(pred, tar[:, 1:], beta=beta).sum() * cls_weight / div
    return cls_loss, dfl_loss, bbox_loss, num_pos


def fcos_head_losses_torch(cls_outs, reg_outs, ctr_outs, labels, ltrb, ctr_tars, reg_mean=0.0, reg_std=1.0,
                           alpha=0.25, gamma=2.0, cls_weight=1.0, bbox_weight=1.0, ctr_weight=1.0):
    """The FCOS head's three losses without GFL (the last arm of the reference's FCOSHead.calc_loss,
    fcos_head.py:419-515, with FocalLoss, GIoULoss and the one-channel sigmoid CrossEntropyLoss)
    restated in torch ops, expression for expression: the numerics reference of ops.fcos_losses
    (csrc/fcos.hip) and what FCOSHead runs for CPU tensors.  CPU (f32 / f64) or HIP tensors; no
    ops call.

    cls_outs [C, M] logits, reg_outs [4, M] ltrb predictions (the head's exp output), ctr_outs
    [M] or [1, M] logits, labels [M] int64 (-1 ignored, 0 negative, > 0 the class), ltrb [M, 4]
    pixels, ctr_tars [M]; positions ordered images outer, levels inner.  Returns (cls_loss,
    bbox_loss, ctr_loss, num_pos [int64 0-d]).  With no positive the sums are divided by
    max(num_pos, 1); the reference divides by zero there."""
    chosen, pos = labels >= 0, labels > 0
    num_pos = pos.sum()
    div = num_pos.clamp(min=1).to(cls_outs.dtype)
    pos_ctr_outs = ctr_outs.reshape(-1, 1)[pos, :]
    pos_ctr_tars = ctr_tars[pos]
    # CrossEntropyLoss with one channel (losses.py:144-147) takes label.view(-1, 1).float(): with
    # f64 inputs the element is still formed in f32, in the reference and here
    ctr_sum = F.binary_cross_entropy_with_logits(pos_ctr_outs, pos_ctr_tars.view(-1, 1).float(),
                                                 reduction='none').sum()
    ctr_loss = ctr_sum * ctr_weight / div.to(ctr_sum.dtype)
    y4 = (ltrb[pos, :].t() - reg_mean) / reg_std                       # [4, m]
    p4 = reg_outs[:, pos]
    a = torch.stack([0.0 - p4[0], 0.0 - p4[1], 0.0 + p4[2], 0.0 + p4[3]])
    b = torch.stack([0.0 - y4[0], 0.0 - y4[1], 0.0 + y4[2], 0.0 + y4[3]])
    bbox_loss = (giou_loss(a, b) * pos_ctr_tars).sum() * bbox_weight / div
    cls_loss = cls_weight * sigmoid_focal_loss(cls_outs[:, chosen].t(), labels[chosen], alpha, gamma) / div
    return cls_loss, bbox_loss, ctr_loss, num_pos
