# Double-Head R-CNN on Faster R-CNN R50-FPN, in the reference's config-file format
# (plain Python dicts read by frcnn_amd.config.Config.fromfile).  Hyper-parameters
# follow the reference's configs/dh_rcnn_r50_fpn.py: the RCNN stage's head is a
# DoubleHead (class scores from two FCs over the flattened 7 x 7 tile, class-specific
# box deltas from a 3x3 conv + BN + ReLU over the tile followed by two FCs), both of
# its losses weighted 2.0.  The data pipeline section is out of this build's scope.

_strides = [4, 8, 16, 32, 64]


def _loss(kind, **kw):
    return dict(type=kind, **kw)


model = dict(
    type='CascadeRCNN',
    num_stages=1,
    backbone=dict(type='ResNet', depth=50, frozen_stages=1, out_layers=(1, 2, 3, 4), pretrained=False),
    neck=dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=5),
    rpn_head=dict(type='RPNHead', in_channels=256, feat_channels=256, anchor_scales=[8],
                  anchor_ratios=[0.5, 1.0, 2.0], anchor_strides=_strides,
                  target_means=[0.0] * 4, target_stds=[1.0] * 4,
                  loss_cls=_loss('CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                  loss_bbox=_loss('SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0)),
    roi_extractor=dict(type='BasicRoIExtractor', output_size=(7, 7),
                       roi_layers=[dict(type='RoIAlign', spatial_scale=1.0 / s, sampling_ratio=2)
                                   for s in _strides[:4]]),
    rcnn_head=[dict(type='DoubleHead', in_channels=256, roi_out_size=7, cls_fc_channels=[1024, 1024],
                    reg_conv_channels=[256], reg_conv_strides=[1], reg_conv_paddings=[1],
                    reg_fc_channels=[256 * 7 * 7, 1024, 1024], num_classes=21, target_means=[0.0] * 4,
                    target_stds=[0.1, 0.1, 0.2, 0.2], reg_class_agnostic=False,
                    loss_cls=_loss('CrossEntropyLoss', use_sigmoid=False, loss_weight=2.0),
                    loss_bbox=_loss('SmoothL1Loss', beta=1.0, loss_weight=2.0))],
)

train_cfg = dict(
    rpn=dict(assigner=dict(type='MaxIoUAssigner', pos_iou=0.7, neg_iou=0.3, min_pos_iou=0.3),
             sampler=dict(type='RandomSampler', max_num=256, pos_num=128),
             allowed_border=0),
    rpn_proposal=dict(pre_nms=2000, post_nms=2000, max_num=2000, nms_iou=0.7, min_bbox_size=0),
    rcnn=[dict(assigner=dict(type='MaxIoUAssigner', pos_iou=0.5, neg_iou=0.5, min_pos_iou=0.5),
               sampler=dict(type='RandomSampler', max_num=512, pos_num=128))],
    stage_loss_weight=[1.0],
)

test_cfg = dict(
    rpn=dict(pre_nms=1000, post_nms=1000, max_num=1000, nms_iou=0.7, min_bbox_size=0.0),
    rcnn=dict(min_score=0.05, nms_iou=0.5, max_per_img=100, nms_type='official'),
)

data = dict(train=dict(imgs_per_gpu=2), test=dict(imgs_per_gpu=2))

# optimiser of the reference config (lib/trainer: OptimizerHook clips, then SGD steps)
optimizer = dict(type='SGD', lr=0.0025, momentum=0.9, weight_decay=0.0001)
optimizer_config = dict(grad_clip=dict(max_norm=35, norm_type=2))
