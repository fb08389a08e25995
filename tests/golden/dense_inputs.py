"""Deterministic inputs of the dense-head candidate tests (ops.dense_candidates, the one-stage
heads' inference): small seeded head outputs and metas, shared by tests/golden/gen_dense_golden.py
(which runs the reference's predict_single_image on them) and the tests.  Nothing here reads the
reference."""
import numpy as np

STRIDES = [8, 16, 32, 64, 128]
GRIDS = [(12, 16), (6, 8), (3, 4), (2, 2), (1, 1)]  # a 96 x 128 padded image
# two images with their own visible size and scale factor (min_size = scale_factor * min_bbox_size)
METAS = [{'img_shape': (90, 120, 3), 'pad_shape': (96, 128, 3), 'scale_factor': 1.0},
         {'img_shape': (96, 128, 3), 'pad_shape': (96, 128, 3), 'scale_factor': 1.5}]
GAP = 1e-5  # relative distance of the k-th and (k+1)-th largest key of every segment

_FOCAL = dict(type='FocalLoss', use_sigmoid=True, loss_weight=1.0)
_QFL = dict(type='QualityFocalLoss', use_sigmoid=True, loss_weight=1.0)
_GIOU = dict(type='GIoULoss', loss_weight=2.0)
_CTR = dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)
_DFL = dict(type='DistributionFocalLoss', cls_channels=16, stride=0.08, norm_prob=False, loss_weight=0.25)

# tag -> the head, the seed of its outputs and the test_cfg.  The level of 192 cells (1728 anchors)
# is cut by pre_nms in every case; fcos_ctr also filters by min_bbox_size.
PREDICT_CASES = {
    'fcos_ctr': dict(kind='fcos', seed=11, C=20, reg_std=64.0, reg_mean=0.0,
                     head=dict(loss_cls=_FOCAL, loss_bbox=_GIOU, loss_centerness=_CTR),
                     test_cfg=dict(pre_nms=40, min_bbox_size=10, min_score=0.05, nms_iou=0.5, nms_type='strict',
                                   max_per_img=100)),
    'fcos_noctr': dict(kind='fcos', seed=12, C=20, reg_std=64.0, reg_mean=0.0,
                       head=dict(loss_cls=_QFL, loss_bbox=_GIOU, atss_cfg=dict(topk=9, scale=8)),
                       test_cfg=dict(pre_nms=40, min_bbox_size=0, min_score=0.05, nms_iou=0.5, nms_type='official',
                                     max_per_img=100)),
    'gfl': dict(kind='gfl', seed=13, C=20, reg_std=100.0, reg_mean=0.0,
                head=dict(loss_cls=_QFL, loss_bbox=_GIOU, loss_dfl=_DFL, atss_cfg=dict(topk=9, scale=8)),
                test_cfg=dict(pre_nms=40, min_bbox_size=0, min_score=0.05, nms_iou=0.6, nms_type='official',
                              max_per_img=100)),
    'retina': dict(kind='retina', seed=14, C=20, A=9,
                   head=dict(loss_cls=_FOCAL, loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0)),
                   test_cfg=dict(pre_nms=300, min_bbox_size=12, min_score=0.05, nms_iou=0.5, nms_type='official',
                                 max_per_img=100)),
}


def fcos_head_kwargs(case, wrap=lambda d: d):
    """Constructor arguments of FCOSHead (the project's or the reference's; `wrap` turns the loss
    dicts into the attribute dicts the reference expects)."""
    kw = dict(num_classes=case['C'] + 1, in_channels=8, stacked_convs=1, feat_channels=8, strides=list(STRIDES),
              reg_std=case['reg_std'], reg_mean=case['reg_mean'])
    kw.update({k: wrap(v) for k, v in case['head'].items()})
    return kw


def retina_head_args(case, wrap=lambda d: d):
    """(positional, keyword) constructor arguments of RetinaHead."""
    return (case['C'] + 1, 8, 1, 8), {k: wrap(v) for k, v in case['head'].items()}


def fcos_outputs(seed, grids, C, batch, kind='fcos', reg_std=64.0, bins=16, ctr=True, strides=None):
    """Per-level (cls [B, C, H, W], reg [B, 4 | 4*bins, H, W], ctr [B, 1, H, W]) f32 arrays: class
    logits around -2, LTRB distances of 0.1 .. 3 cells (some boxes below a min size of a few
    pixels), DFL logits of scale 2."""
    rng = np.random.default_rng(seed)
    strides = strides or STRIDES
    cls, reg, ctrs = [], [], []
    for (h, w), s in zip(grids, strides):
        cls.append((rng.standard_normal((batch, C, h, w)) * 2.0 - 2.0).astype(np.float32))
        if kind == 'gfl':
            reg.append((rng.standard_normal((batch, 4 * bins, h, w)) * 2.0).astype(np.float32))
        else:
            reg.append((rng.uniform(0.1, 3.0, (batch, 4, h, w)) * s / reg_std).astype(np.float32))
        ctrs.append(rng.standard_normal((batch, 1, h, w)).astype(np.float32) if ctr else None)
    return cls, reg, ctrs


def retina_outputs(seed, grids, A, C, batch, cls_scale=2.0, reg_scale=0.4):
    rng = np.random.default_rng(seed)
    cls = [(rng.standard_normal((batch, C * A, h, w)) * cls_scale - 1.0).astype(np.float32) for h, w in grids]
    reg = [(rng.standard_normal((batch, 4 * A, h, w)) * reg_scale).astype(np.float32) for h, w in grids]
    return cls, reg


def predict_inputs(tag):
    """The head outputs of a PREDICT_CASES entry for the two METAS images: (cls, reg, ctr) lists of
    per-level arrays (ctr entries None without centerness; ctr itself None for retina)."""
    c = PREDICT_CASES[tag]
    if c['kind'] == 'retina':
        cls, reg = retina_outputs(c['seed'], GRIDS, c['A'], c['C'], len(METAS))
        return cls, reg, None
    return fcos_outputs(c['seed'], GRIDS, c['C'], len(METAS), kind=c['kind'], reg_std=c['reg_std'],
                        ctr='loss_centerness' in c['head'])


def fcos_levels(head, cls_outs, reg_outs, ctr_outs, meta, test_cfg):
    """FCOSHead.image_candidates' per-level tables on CPU tensors of ONE image, with its own torch
    expressions: per level a dict of score [C, n], ctr [n] or None, box [4, n], cand (bool [n]: the
    columns the min-size filter keeps), key [n] and sel (the columns the level contributes, in
    image_candidates' order).  The tests check sel against image_candidates itself."""
    import torch
    from frcnn_amd import utils
    from frcnn_amd.heads.fcos_head import class2length, ltrb2bbox
    min_size = meta['scale_factor'] * test_cfg['min_bbox_size']
    out = []
    for i in range(len(cls_outs)):
        if head.use_dfl:
            r = reg_outs[i]
            gs = r.shape[-2:]
            r = r.reshape(head.loss_dfl.cls_channels, -1).t().softmax(-1)
            ltrb = class2length(r, head.loss_dfl.stride) * head.reg_std + head.reg_mean
            bbox = ltrb2bbox(ltrb.view(4, *gs), head.strides[i])
        else:
            bbox = ltrb2bbox(reg_outs[i] * head.reg_std + head.reg_mean, head.strides[i])
        score = cls_outs[i].sigmoid().reshape(head.cls_channels, -1)
        ctr = ctr_outs[i].sigmoid().reshape(-1) if head.use_centerness else None
        bbox = utils.clamp_bbox(bbox.reshape(4, -1), meta['img_shape'][:2])
        cand = ((bbox[2] - bbox[0] + 1) > min_size) & ((bbox[3] - bbox[1] + 1) > min_size)
        key = (score * ctr.view(1, -1)).max(0)[0] if ctr is not None else score.max(0)[0]
        cols = torch.nonzero(cand).view(-1)
        if 0 < test_cfg['pre_nms'] < cols.numel():
            cols = cols[key[cols].topk(test_cfg['pre_nms'])[1]]
        out.append(dict(score=score, ctr=ctr, box=bbox, cand=cand, key=key, sel=cols))
    return out


def retina_levels(head, cls_outs, reg_outs, level_anchors, meta, test_cfg, param2bbox):
    """AnchorHead.image_candidates' per-level tables on CPU tensors of ONE image (sigmoid head);
    param2bbox(anchors [4, n], reg [4, n], means, stds, img_size) is the decode.  cand is all
    true; valid marks the rows the min-size mask keeps."""
    import torch
    min_size = meta['scale_factor'] * test_cfg['min_bbox_size']
    out = []
    for co, ro, an in zip(cls_outs, reg_outs, level_anchors):
        score = co.reshape(head.cls_channels, -1).sigmoid()
        box = param2bbox(an.reshape(4, -1), ro.reshape(4, -1), head.target_means, head.target_stds,
                         meta['img_shape'][:2])
        key = score.max(0)[0]
        cols = torch.arange(score.shape[1])
        if 0 < test_cfg['pre_nms'] < score.shape[1]:
            cols = key.topk(test_cfg['pre_nms'])[1]
        valid = torch.ones(score.shape[1], dtype=torch.bool)
        if min_size > 0:
            valid = ((box[2] - box[0] + 1) >= min_size) & ((box[3] - box[1] + 1) >= min_size)
        out.append(dict(score=score, ctr=None, box=box, cand=torch.ones_like(valid), valid=valid, key=key, sel=cols))
    return out


def cpu_anchors(head, grids=None, strides=None):
    """Per-level [4, A, H, W] anchors of an AnchorHead on the CPU (the oracle's numpy grid: the
    package's own is a HIP op)."""
    import oracle
    import torch
    return [torch.from_numpy(oracle.anchor_grid(s, head.anchor_scales, head.anchor_ratios, s, g))
            for s, g in zip(strides or STRIDES, grids or GRIDS)]


def cpu_param2bbox(an, ro, means, stds, img_size=None):
    """utils.param2bbox on CPU tensors through the oracle's numpy restatement."""
    import oracle
    import torch
    return torch.from_numpy(oracle.param2bbox(an.contiguous().numpy(), ro.contiguous().numpy(), means, stds,
                                              img_size))


def check_gaps(levels, pre_nms):
    """The smallest cut gap over the levels' candidate keys (inf when no level is cut)."""
    return min([cut_gaps(lv['key'][lv['cand']].numpy(), pre_nms) for lv in levels] + [np.inf])


def cut_gaps(keys, k):
    """keys: the candidates' keys of one segment (1-d); the relative distance of the k-th and the
    (k+1)-th largest, inf when the cut takes every candidate."""
    keys = np.sort(np.asarray(keys, np.float64))[::-1]
    if k <= 0 or k >= keys.size:
        return np.inf
    a, b = keys[k - 1], keys[k]
    return (a - b) / max(abs(a), 1e-300)
