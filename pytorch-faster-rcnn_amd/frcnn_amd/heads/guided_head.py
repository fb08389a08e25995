"""GuidedAnchor and GARPNHead: the Guided Anchoring RPN (reference lib/heads/guided_head.py).

The reference file has drifted from its own helpers and cannot run as written; this mirror
implements its text with four repairs ("GA-RPN deviations"):
  1. the anchor creators are anchor.AnchorCreator, called with the level's stride
     (region.AnchorCreator no longer exists; the head passes the input size);
  2. region.inside_grid_mask is called as (num_anchors, img_size, grid_size, stride, device);
  3. region.map_gt2level measures the width as gt[2] - gt[0] (the reference reads gt[1]);
  4. the post-NMS cut tests and slices by cfg.post_nms (the reference slices by cfg.pos_nms).

What runs where.  The adaption layer (offset_layer + DeformConv + ReLU) of all levels is one
fused HIP launch pair where nothing needs a gradient (ops.deform_conv3x3_levels, guided mode:
the 18 dg-channel offset map is never written).  Training by default takes the torch restatement;
with the class attribute GuidedAnchor.hip_grad = True it is that one forward call
(frh_deform_conv3x3_act_levels) and one frh_deform_conv3x3_bwd call per level in the backward.
The location and shape targets of the whole batch are one launch
(ops.ga_targets) instead of the reference's per-gt painting loops; the location loss runs over
the un-compacted logits with -1 labels, which the focal-loss kernel skips.  GuidedAnchor.loss
still meets the host twice a batch: targets() reads the smallest gt coordinate back (its
precondition), and the shape loss indexes the sampled positives (torch.nonzero) and divides by
their count, as the reference does.  The RPN targets and
the proposals follow the reference image by image and level by level with the existing ops
(MaxIoU assignment, sampler, bbox2param / param2bbox, nms); their mask indexing synchronises
with the host as the reference's does.
"""
import numpy as np
import torch
from torch import nn

from .. import ops, utils, region, losses
from ..anchor import AnchorCreator, anchor_target
from ..dcn import DeformConv
from ..utils import ChannelsLastConvs, init_module_normal, multi_apply, unpack_multi_result


class GuidedAnchor(ChannelsLastConvs):
    hip_grad = False  # True: the adaption layer trains on the HIP forward and backward entries

    def __init__(self, in_channels=256, out_channels=256, anchor_scales=None, anchor_ratios=None, anchor_strides=None,
                 anchoring_means=(0.0, 0.0, 0.0, 0.0), anchoring_stds=(0.07, 0.07, 0.14, 0.14), deformable_groups=4,
                 sigma=8, loc_filter_thr=0.01, loss_loc=None, loss_shape=None):
        super().__init__()
        from ..builder import build_module
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.anchor_scales = list(anchor_scales)
        self.anchor_ratios = list(anchor_ratios)
        self.anchor_strides = list(anchor_strides)
        self.anchoring_means = list(anchoring_means)
        self.anchoring_stds = list(anchoring_stds)
        self.deformable_groups = deformable_groups
        self.sigma = sigma
        self.loc_filter_thr = loc_filter_thr
        self.loss_loc = build_module(loss_loc)
        self.loss_shape = build_module(loss_shape)
        self.square_anchor_creators = [AnchorCreator(base=b, scales=[self.anchor_scales[0]], aspect_ratios=[1.0])
                                       for b in self.anchor_strides]
        self._square_cache = {}
        self.init_layers()

    def init_layers(self):
        self.loc_layer = nn.Conv2d(self.in_channels, 1, 1)
        self.shape_layer = nn.Conv2d(self.in_channels, 2, 1)
        self.offset_layer = nn.Conv2d(2, 3 * 3 * 2 * self.deformable_groups, 1, bias=False)
        self.adapt_layer = DeformConv(self.in_channels, self.out_channels, 3, padding=1,
                                      deformable_groups=self.deformable_groups)
        self.relu = nn.ReLU(inplace=True)

    def init_weights(self):
        init_module_normal(self.offset_layer, std=0.1)
        init_module_normal(self.adapt_layer, std=0.01)
        init_module_normal(self.shape_layer, std=0.01)
        init_module_normal(self.loc_layer, std=0.01)
        prior_prob = 0.01
        self.loc_layer.bias.data.fill_(float(-np.log((1 - prior_prob) / prior_prob)))

    # ------------------------------------------------------------ anchors
    def create_square_anchors(self, grid_sizes):
        """Per level [4, 1, H, W]: one square anchor of side scale * stride per cell."""
        key = tuple((int(h), int(w)) for h, w in grid_sizes)
        a = self._square_cache.get(key)
        if a is None:
            a = self._square_cache[key] = [c(s, g) for c, s, g in
                                           zip(self.square_anchor_creators, self.anchor_strides, key)]
        return a

    def create_rpn_anchors_single_image(self, loc_outs, shape_outs, square_anchors, img_meta):
        """guided_head.py:114-132: the guided anchors [4, H W] of every level (the square anchor
        reshaped by the predicted dw / dh) and the cells kept: sigmoid(loc) > loc_filter_thr inside
        the image's part of the grid."""
        img_size = img_meta['img_shape'][:2]
        anchors, in_masks = [], []
        for lo, so, sq, stride in zip(loc_outs, shape_outs, square_anchors, self.anchor_strides):
            grid = lo.shape[-2:]
            in_grid = region.inside_grid_mask(1, img_size, grid, stride, lo.device).view(tuple(grid)).bool()
            in_masks.append(((lo.sigmoid() > self.loc_filter_thr) & in_grid).reshape(tuple(grid)))
            param = torch.cat([torch.zeros_like(so), so], dim=0).reshape(4, -1).float()
            anchors.append(utils.param2bbox(sq.reshape(4, -1), param, self.anchoring_means, self.anchoring_stds))
        return anchors, in_masks

    def create_rpn_anchors(self, loc_outs, shape_outs, img_metas):
        """guided_head.py:136-155; the anchors carry no gradient (as in mmdet's guided anchors)."""
        with torch.no_grad():
            square = self.create_square_anchors([lo.shape[-2:] for lo in loc_outs])
            res = [self.create_rpn_anchors_single_image([lo[i] for lo in loc_outs], [so[i] for so in shape_outs],
                                                        square, meta) for i, meta in enumerate(img_metas)]
        return unpack_multi_result(res)

    # ------------------------------------------------------------ forward
    def forward(self, feats):
        if len(feats) != len(self.anchor_strides):
            raise AssertionError('one feature level per anchor stride')
        loc_outs = [self.loc_layer(f) for f in feats]
        shape_outs = [self.shape_layer(f) for f in feats]
        # relu(adapt_layer(feat, offset_layer(shape.detach()))) of every level: one fused launch pair
        # where nothing needs a gradient; otherwise the torch restatement, or with hip_grad the same
        # forward with the HIP backward
        adapt_feats = ops.deform_conv3x3_levels(feats, [so.detach() for so in shape_outs], self.adapt_layer.weight,
                                                self.deformable_groups, relu=True,
                                                offset_weight=self.offset_layer.weight, hip_grad=self.hip_grad)
        return loc_outs, shape_outs, adapt_feats

    # ------------------------------------------------------------ targets and loss
    def targets(self, grid_sizes, gt_bboxes, img_metas, cfg):
        """GuidedAnchor.loc_target (guided_head.py:328-397) and the painted maps of
        shape_target_single_image_v2 (:195-231) for the batch in one launch: loc [B, N] (1 / 0 /
        -1), shape_mask [B, N], shape_box [B, N, 4] over the level-concatenated cells."""
        lows = [g.min() for g in gt_bboxes if g.numel()]
        if lows and float(torch.stack(lows).min()) < 0:
            # the reference's negative slice indices wrap around the maps: not reproduced
            raise ValueError('GuidedAnchor targets need gt coordinates >= 0')
        levels = [region.map_gt2level(self.anchor_scales[0], self.anchor_strides, g) for g in gt_bboxes]
        return ops.ga_targets(grid_sizes, [float(s) for s in self.anchor_strides], list(gt_bboxes), levels,
                              [m['img_shape'][:2] for m in img_metas], cfg.center_ratio, cfg.ignore_ratio,
                              cfg.get('shape_center_ratio', 0.5))

    def loss(self, loc_outs, shape_outs, adapt_feats, gt_bboxes, gt_labels, img_metas, cfg):
        """guided_head.py:409-456."""
        from ..builder import build_module
        dev = loc_outs[0].device
        B = loc_outs[0].shape[0]
        grid_sizes = [tuple(lo.shape[-2:]) for lo in loc_outs]
        loc, mask, box = self.targets(grid_sizes, gt_bboxes, img_metas, cfg)
        N = loc.shape[1]

        # location: every cell's logit, image-major and level-concatenated as the targets; the
        # focal-loss kernel skips the -1 labels the reference indexes away
        logits = torch.cat([lo.reshape(B, -1) for lo in loc_outs], dim=1).reshape(-1, 1)
        loc_loss = self.loss_loc(logits, loc.view(-1)) / (loc == 1).sum()

        # shape: the sampler keeps a subset of the painted cells of each image (in image order, as
        # the reference's per-image calls draw); only the kept positives enter the loss
        sampler = cfg.get('ga_sampler', None)
        if sampler is None:
            raise AssertionError('GuidedAnchor.loss needs cfg.ga_sampler (the reference leaves labels undefined without)')
        if isinstance(sampler, dict):
            sampler = build_module(sampler)
        num = torch.full((B,), N, dtype=torch.int32, device=dev)
        labels = ops.sample_labels(mask, num, N, sampler.max_num, sampler.pos_num)
        pos = torch.nonzero(labels.view(-1) == 1).view(-1)
        avg_factor = int(pos.numel())
        shape_loss = losses.zero_loss(dev)
        if avg_factor > 0:
            square = torch.cat([a.reshape(4, -1) for a in self.create_square_anchors(grid_sizes)], dim=1)
            shape_out = torch.cat([so.reshape(B, 2, -1) for so in shape_outs], dim=2)  # [B, 2, N]
            tar_shape = shape_out.permute(1, 0, 2).reshape(2, -1)[:, pos]
            tar_params = utils.bbox2param(square[:, pos % N].contiguous(), box.view(-1, 4)[pos].t().contiguous(),
                                          self.anchoring_means, self.anchoring_stds)
            shape_loss = (self.loss_shape(tar_shape[0], tar_params[2]) + self.loss_shape(tar_shape[1], tar_params[3])) \
                / avg_factor
        return {'loc_loss': loc_loss, 'shape_loss': shape_loss}


class GARPNHead(ChannelsLastConvs):
    def __init__(self, in_channels=256, feat_channels=256, octave_base_scale=8, scales_per_octave=3,
                 octave_ratios=(0.5, 1.0, 2.0), anchor_strides=(4, 8, 16, 32, 64),
                 anchoring_means=(0.0, 0.0, 0.0, 0.0), anchoring_stds=(0.07, 0.07, 0.14, 0.14),
                 target_means=(0.0, 0.0, 0.0, 0.0), target_stds=(0.07, 0.07, 0.11, 0.11), deformable_groups=4,
                 loc_filter_thr=0.01,
                 loss_loc=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                 loss_shape=dict(type='BoundedIoULoss', beta=0.2, loss_weight=1.0),
                 loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                 loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0)):
        super().__init__()
        from ..builder import build_module
        self.in_channels = in_channels
        self.feat_channels = feat_channels
        self.octave_base_scale = octave_base_scale
        self.scales_per_octave = scales_per_octave
        self.octave_ratios = list(octave_ratios)
        self.anchor_strides = list(anchor_strides)
        self.anchoring_means = list(anchoring_means)
        self.anchoring_stds = list(anchoring_stds)
        self.target_means = list(target_means)
        self.target_stds = list(target_stds)
        self.loc_filter_thr = loc_filter_thr
        self.loss_cls = build_module(loss_cls)
        self.loss_bbox = build_module(loss_bbox)
        self.anchor_scales = [octave_base_scale * 2 ** (i / scales_per_octave) for i in range(scales_per_octave)]
        self.guided_anchor = GuidedAnchor(in_channels, in_channels, anchor_scales=self.anchor_scales,
                                          anchor_ratios=self.octave_ratios, anchor_strides=self.anchor_strides,
                                          anchoring_means=anchoring_means, anchoring_stds=anchoring_stds,
                                          deformable_groups=deformable_groups, loc_filter_thr=loc_filter_thr,
                                          loss_loc=loss_loc, loss_shape=loss_shape)
        self.num_anchors = 1
        self.num_classes = 2
        self.cls_channels = 1
        self.use_sigmoid = loss_cls.get('use_sigmoid', False)
        self.init_layers()

    def init_layers(self):
        self.conv = nn.Conv2d(self.in_channels, self.feat_channels, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.classifier = nn.Conv2d(self.feat_channels, self.num_anchors * self.cls_channels, 1)
        self.regressor = nn.Conv2d(self.feat_channels, self.num_anchors * 4, 1)

    def init_weights(self):
        self.guided_anchor.init_weights()
        for m in (self.conv, self.classifier, self.regressor):
            init_module_normal(m, mean=0.0, std=0.01)

    def forward_conv(self, adapt_feats):
        # as RPNHead.forward: the fused Winograd conv and the one-launch 1x1 heads where nothing
        # needs a gradient, the modules otherwise
        hidden = ops.conv3x3_bias_act_levels(self.conv, adapt_feats, relu=True)
        return ops.rpn_head1x1_levels(self.classifier, self.regressor, hidden)

    def forward(self, feats):
        loc_outs, shape_outs, adapt_feats = self.guided_anchor(feats)
        cls_outs, reg_outs = self.forward_conv(adapt_feats)
        return cls_outs, reg_outs, loc_outs, shape_outs, adapt_feats

    # ------------------------------------------------------------ RPN targets and loss
    def rpn_target_single_image(self, cls_outs, reg_outs, anchors, in_masks, gt_bbox, gt_label, img_meta, cfg):
        """guided_head.py:557-572: the image's kept guided anchors through the MaxIoU assigner, the
        sampler and the target encoder."""
        cls_out = torch.cat([c.reshape(1, -1) for c in cls_outs], dim=1)
        reg_out = torch.cat([r.reshape(4, -1) for r in reg_outs], dim=1)
        anchor = torch.cat([a.reshape(4, -1) for a in anchors], dim=1)
        in_mask = torch.cat([m.reshape(-1) for m in in_masks])
        in_anchors = anchor[:, in_mask.bool()]
        return anchor_target(cls_out, reg_out, 1, in_anchors, in_mask, gt_bbox, None, assigner=cfg.assigner,
                             sampler=cfg.get('sampler', None), target_means=self.target_means,
                             target_stds=self.target_stds)

    def rpn_target(self, cls_outs, reg_outs, anchors, in_masks, gt_bboxes, gt_labels, img_metas, cfg):
        return unpack_multi_result(multi_apply(self.rpn_target_single_image, utils.split_by_image(cls_outs),
                                               utils.split_by_image(reg_outs), anchors, in_masks, list(gt_bboxes),
                                               list(gt_labels), list(img_metas), cfg))

    def loss(self, cls_outs, reg_outs, loc_outs, shape_outs, adapt_feats, gt_bboxes, gt_labels, img_metas, cfg):
        """guided_head.py:594-619: {'cls_loss', 'reg_loss', 'loc_loss', 'shape_loss'}."""
        ga_loss = self.guided_anchor.loss(loc_outs, shape_outs, adapt_feats, gt_bboxes, gt_labels, img_metas, cfg)
        anchors, in_masks = self.guided_anchor.create_rpn_anchors(loc_outs, shape_outs, img_metas)
        tar_cls_outs, tar_reg_outs, tar_labels, _, _, tar_params = self.rpn_target(
            cls_outs, reg_outs, anchors, in_masks, gt_bboxes, gt_labels, img_metas, cfg)
        tar_label = torch.cat(tar_labels)
        tar_cls_out = torch.cat(tar_cls_outs, dim=1)
        tar_reg_out = torch.cat(tar_reg_outs, dim=1)
        tar_param = torch.cat(tar_params, dim=1)
        avg_factor = tar_label.shape[0]
        cls_loss = self.loss_cls(tar_cls_out.t(), tar_label) / avg_factor
        if isinstance(self.loss_bbox, losses.SmoothL1Loss):
            # the positive columns as a masked sum: no boolean-index synchronisation
            reg_loss = self.loss_bbox.masked(tar_reg_out, tar_param, tar_label, rows_dim=1) / avg_factor
        else:
            pos = tar_label == 1
            reg_loss = self.loss_bbox(tar_reg_out[:, pos], tar_param[:, pos]) / avg_factor
        rpn_loss = {'cls_loss': cls_loss, 'reg_loss': reg_loss}
        rpn_loss.update(ga_loss)
        return rpn_loss

    # ------------------------------------------------------------ proposals
    def predict_bboxes_single_image(self, cls_outs, reg_outs, anchors, in_masks, img_meta, cfg):
        """guided_head.py:621-669 (the post-NMS cut by cfg.post_nms: repair 4)."""
        img_size = img_meta['img_shape'][:2]
        min_size = img_meta['scale_factor'] * cfg.min_bbox_size
        scores, boxes = [], []
        for co, ro, an, im in zip(cls_outs, reg_outs, anchors, in_masks):
            im = im.reshape(-1)
            cls_score = co.reshape(1, -1)[:, im].sigmoid()[0]
            reg_out = ro.reshape(4, -1)[:, im]
            anchor = an.reshape(4, -1)[:, im]
            if 0 < cfg.pre_nms < len(cls_score):
                _, topk = cls_score.topk(cfg.pre_nms)
                cls_score, reg_out, anchor = cls_score[topk], reg_out[:, topk], anchor[:, topk]
            pred = utils.param2bbox(anchor.contiguous(), reg_out.float().contiguous(), self.target_means,
                                    self.target_stds, img_size)
            if min_size > 0:
                ok = (pred[2] - pred[0] + 1 >= min_size) & (pred[3] - pred[1] + 1 >= min_size)
                cls_score, pred = cls_score[ok], pred[:, ok]
            keep = ops.nms(pred.t().contiguous(), cls_score.contiguous(), cfg.nms_iou)
            cls_score, pred = cls_score[keep], pred[:, keep]
            if 0 < cfg.post_nms < len(cls_score):
                cls_score, pred = cls_score[:cfg.post_nms], pred[:, :cfg.post_nms]
            scores.append(cls_score)
            boxes.append(pred)
        score, box = torch.cat(scores), torch.cat(boxes, dim=1)
        if 0 < cfg.max_num < len(score):
            _, topk = score.topk(cfg.max_num)
            score, box = score[topk], box[:, topk]
        return box, score, None

    def predict_bboxes_from_output(self, cls_outs, reg_outs, loc_outs, shape_outs, adapt_feats, img_metas, cfg):
        with torch.no_grad():
            anchors, in_masks = self.guided_anchor.create_rpn_anchors(loc_outs, shape_outs, img_metas)
            return unpack_multi_result(multi_apply(self.predict_bboxes_single_image, utils.split_by_image(cls_outs),
                                                   utils.split_by_image(reg_outs), anchors, in_masks, list(img_metas),
                                                   cfg))

    def predict_bboxes(self, feats, img_metas, cfg):
        return self.predict_bboxes_from_output(*(tuple(self.forward(feats)) + (img_metas, cfg)))
