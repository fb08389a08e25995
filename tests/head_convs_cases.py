"""What test_gpu_head_convs.py and test_head_convs_cpu.py share: the four one-stage heads at a
given width, their levels, and the heads' forward as the module expressions it has always been
(the reference the fused forward is compared with, and the fallbacks must equal bit for bit)."""
import torch

MODES = ('retina', 'fcos', 'atss', 'gfl')
LEVELS = ((12, 20), (6, 10), (3, 5), (2, 3), (1, 2))
STRIDES = (8, 16, 32, 64, 128)
_FOCAL = dict(type='FocalLoss', use_sigmoid=True, loss_weight=1.0)
_GIOU = dict(type='GIoULoss', loss_weight=2.0)
_CTR = dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)


def make_head(mode, feat=64, stacked=2, seed=3, **kw):
    """RetinaHead, or FCOSHead plain / with ATSS / with ATSS + GFL (16 bins): 21 classes, feat input
    and tower channels, PyTorch's default init under a fixed seed."""
    torch.manual_seed(seed)
    if mode == 'retina':
        from frcnn_amd.heads.retina_head import RetinaHead
        return RetinaHead(21, feat, stacked, feat, anchor_strides=STRIDES, loss_cls=_FOCAL,
                          loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0))
    from frcnn_amd.heads.fcos_head import FCOSHead
    args = dict(num_classes=21, in_channels=feat, stacked_convs=stacked, feat_channels=feat, strides=list(STRIDES),
                reg_std=300, reg_mean=0, reg_coef=[1.0, 0.75, 1.25, 0.5, 1.5], loss_bbox=_GIOU)
    if mode == 'gfl':
        args.update(atss_cfg=dict(topk=9, scale=8), loss_cls=dict(type='QualityFocalLoss', use_sigmoid=True, loss_weight=1.0),
                    loss_dfl=dict(type='DistributionFocalLoss', cls_channels=16, stride=0.08, norm_prob=False,
                                  loss_weight=0.25))
    else:
        args.update(loss_cls=_FOCAL, loss_centerness=_CTR)
        if mode == 'atss':
            args.update(atss_cfg=dict(topk=9, scale=8))
    args.update(kw)
    return FCOSHead(**args)


def make_levels(dev, cin=64, n=2, levels=LEVELS, seed=9):
    """Channels-last seeded-normal levels [n, cin, h, w]."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, cin, h, w, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
            for h, w in levels]


def module_forward(head, xs):
    """The head's forward as the module expressions (RetinaHead.forward and FCOSHead.forward before
    the fused convolutions existed)."""
    if hasattr(head, 'retina_cls'):
        cls = [head.retina_cls(head.cls_convs(x)) for x in xs]
        reg = [head.retina_reg(head.reg_convs(x)) for x in xs]
        return cls, reg
    cls_t = [head.cls_convs(x) for x in xs]
    reg_t = [head.reg_convs(x) for x in xs]
    cls_outs = [head.fcos_cls(x) for x in cls_t]
    ctr_outs = [head.fcos_center(x) for x in reg_t]
    if head.use_dfl:
        reg_outs = []
        for i, x in enumerate(reg_t):
            coef = torch.cat([head.reg_coef[i].view(-1, 1)] * 4, dim=1)
            reg_outs.append(head.fcos_reg(x) * coef.view(-1, 1, 1))
    else:
        reg_outs = [torch.exp(head.fcos_reg(x) * head.reg_coef[i]) for i, x in enumerate(reg_t)]
    return cls_outs, reg_outs, ctr_outs


def flat(outs):
    return [t for group in outs for t in group]
