# Faster R-CNN R50-FPN with the Guided Anchoring RPN (GARPNHead), in the reference's config-file
# format (plain Python dicts read by frcnn_amd.config.Config.fromfile).
#
# This is the project's OWN config: the reference registers GARPNHead and BoundedIoULoss and has
# a CascadeRCNN branch for the head, but ships no config that uses it.  Everything but the RPN is
# configs/faster_rcnn_r50_fpn.py (BASELINE config 2); the RPN head's arguments are the
# reference's GARPNHead defaults, and the Guided Anchoring values are mmdet's ga_rpn ones:
# center_ratio 0.2, ignore_ratio 0.5, loc_filter_thr 0.01, a ga_sampler of 256 cells with at
# most 128 positives; shape_center_ratio 0.5 is the reference's own default
# (lib/heads/guided_head.py:202).  The data pipeline section is out of this build's scope.

_strides = [4, 8, 16, 32, 64]


def _loss(kind, **kw):
    return dict(type=kind, **kw)


model = dict(
    type='CascadeRCNN',
    num_stages=1,
    backbone=dict(type='ResNet', depth=50, frozen_stages=1, out_layers=(1, 2, 3, 4), pretrained=False),
    neck=dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=5),
    rpn_head=dict(type='GARPNHead', in_channels=256, feat_channels=256, octave_base_scale=8, scales_per_octave=3,
                  octave_ratios=[0.5, 1.0, 2.0], anchor_strides=_strides,
                  anchoring_means=[0.0] * 4, anchoring_stds=[0.07, 0.07, 0.14, 0.14],
                  target_means=[0.0] * 4, target_stds=[0.07, 0.07, 0.11, 0.11],
                  deformable_groups=4, loc_filter_thr=0.01,
                  loss_loc=_loss('FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                  loss_shape=_loss('BoundedIoULoss', beta=0.2, loss_weight=1.0),
                  loss_cls=_loss('CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                  loss_bbox=_loss('SmoothL1Loss', beta=1.0, loss_weight=1.0)),
    roi_extractor=dict(type='BasicRoIExtractor', output_size=(7, 7),
                       roi_layers=[dict(type='RoIAlign', spatial_scale=1.0 / s, sampling_ratio=2)
                                   for s in _strides[:4]]),
    rcnn_head=[dict(type='RCNNHead', in_channels=256, roi_out_size=(7, 7), fc_channels=[1024, 1024],
                    with_avg_pool=False, num_classes=21, target_means=[0.0] * 4,
                    target_stds=[0.1, 0.1, 0.2, 0.2], reg_class_agnostic=False,
                    loss_cls=_loss('CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                    loss_bbox=_loss('SmoothL1Loss', beta=1.0, loss_weight=1.0))],
)

train_cfg = dict(
    rpn=dict(assigner=dict(type='MaxIoUAssigner', pos_iou=0.7, neg_iou=0.3, min_pos_iou=0.3),
             sampler=dict(type='RandomSampler', max_num=256, pos_num=128),
             ga_sampler=dict(type='RandomSampler', max_num=256, pos_num=128),
             allowed_border=-1, center_ratio=0.2, ignore_ratio=0.5, shape_center_ratio=0.5),
    # both spellings of the post-NMS cut: the reference tests post_nms and slices by pos_nms
    rpn_proposal=dict(pre_nms=2000, post_nms=2000, pos_nms=2000, max_num=2000, nms_iou=0.7, min_bbox_size=0),
    rcnn=[dict(assigner=dict(type='MaxIoUAssigner', pos_iou=0.5, neg_iou=0.5, min_pos_iou=0.5),
               sampler=dict(type='RandomSampler', max_num=512, pos_num=128))],
    stage_loss_weight=[1.0],
)

test_cfg = dict(
    rpn=dict(pre_nms=1000, post_nms=1000, pos_nms=1000, max_num=1000, nms_iou=0.7, min_bbox_size=0.0),
    rcnn=dict(min_score=0.05, nms_iou=0.5, max_per_img=100),
)

data = dict(train=dict(imgs_per_gpu=2), test=dict(imgs_per_gpu=2))

optimizer = dict(type='SGD', lr=0.0025, momentum=0.9, weight_decay=0.0001)
optimizer_config = dict(grad_clip=dict(max_norm=35, norm_type=2))
