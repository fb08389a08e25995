"""Deterministic inputs of the Guided Anchoring tests (location / shape targets, deformable
convolution), shared by tests/golden/gen_ga_golden.py (which runs the reference on them) and the
tests, and the numpy restatement of the per-cell target rule.  Nothing here reads the reference."""
import numpy as np

# ----------------------------------------------------------------- targets
STRIDES = [4, 8, 16, 32, 64]
PAD_SHAPE = (96, 160)
GRIDS = [(24, 40), (12, 20), (6, 10), (3, 5), (2, 3)]  # 1301 cells
NUM_CELLS = sum(h * w for h, w in GRIDS)
IMG_SHAPES = [(90, 150, 3), (96, 160, 3), (61, 97, 3)]
# one anchor scale of 1: region.map_gt2level puts a gt of side sqrt(w h) on level
# floor(log2(side / 4)), so a 96 x 160 image reaches every level
ANCHOR_SCALE = 1
RATIOS = dict(center_ratio=0.2, ignore_ratio=0.5, shape_center_ratio=0.5)

# Image 0, eight gts (x1, y1, x2, y2) and their levels:
#   0 a 4 x 4 gt: its centre region (21.1 .. 21.9) / 4 rounds to the single cell (5, 5)
#   1, 2 overlap on level 0: shape regions x 3..4, y 10..11 and x 3..4, y 11..12 (46 / 4 = 11.5
#     rounds to 12); on row 11 the later index (2) owns the box
#   3 level 1: the shape / ignore region's left edge is 20 / 8 = 2.5 -> 2 and its top 36 / 8 = 4.5
#     -> 4 (half to even; half up would give 3 and 5)
#   4 at the image corner (0, 0)
#   5 at the far corner of the image, level 2
#   6 level 3, 7 level 4: level 0 has no lvl - 1 and level 4 no lvl + 1 neighbour
BOXES_0 = np.array([[20, 20, 23, 23], [10, 40, 16, 46], [12, 42, 18, 47], [17, 33, 30, 46], [0, 0, 9, 9],
                    [130, 70, 149, 89], [60, 20, 100, 60], [10, 5, 140, 85]], np.float32).T.copy()
LEVELS_0 = np.array([0, 0, 0, 1, 1, 2, 3, 4], np.int64)
BOXES_2 = np.array([[5, 5, 40, 30], [50, 10, 90, 55], [2, 40, 8, 47], [30, 20, 45, 36]], np.float32).T.copy()
LEVELS_2 = np.array([2, 3, 0, 1], np.int64)
EMPTY = np.zeros((4, 0), np.float32)

# the case the reference runs: three images of different img_shape, the middle one without gts
REF_BOXES = [BOXES_0, EMPTY, BOXES_2]
REF_LEVELS = [LEVELS_0, np.zeros(0, np.int64), LEVELS_2]


def many_case(n=200, seed=5):
    """One image of n random gts on random levels (checked against cell_rule only: the
    reference's loop is too slow to fixture at this size); the kernel stages 256 gts at a time."""
    rs = np.random.RandomState(seed)
    x1 = rs.randint(0, 140, n).astype(np.float32)
    y1 = rs.randint(0, 80, n).astype(np.float32)
    w = rs.randint(2, 60, n).astype(np.float32)
    h = rs.randint(2, 50, n).astype(np.float32)
    boxes = np.stack([x1, y1, np.minimum(x1 + w, 159), np.minimum(y1 + h, 95)]).astype(np.float32)
    return boxes, rs.randint(0, 5, n).astype(np.int64)


def img_metas():
    return [{'img_shape': s, 'pad_shape': PAD_SHAPE + (3,), 'scale_factor': 1.0} for s in IMG_SHAPES]


def _region(box, ratio, stride):
    """The rounded region of one gt at `ratio` on a level of `stride`, in f32 in the reference's
    operation order (guided_head.py:212-217 with paint_value's scale and round)."""
    f = np.float32
    x1, y1, x2, y2 = [f(v) for v in box]
    w, h = (x2 - x1 + f(1)) * f(ratio), (y2 - y1 + f(1)) * f(ratio)
    cx, cy = (x2 + x1) / f(2), (y2 + y1) / f(2)
    sc = f(1.0 / stride)
    r = np.array([cx - w / f(2), cy - h / f(2), cx + w / f(2), cy + h / f(2)], np.float32) * sc
    return np.rint(r).astype(np.int64)


def cell_rule(boxes, levels, img_shape, center_ratio, ignore_ratio, shape_center_ratio, grids=GRIDS, strides=STRIDES):
    """The per-cell rule of include/frcnn_amd.h (frh_ga_targets) for one image: loc [N] i64,
    shape_mask [N] i64, shape_box [N, 4] f32 over the level-concatenated cells."""
    locs, masks, sboxes = [], [], []
    for l, ((gh, gw), s) in enumerate(zip(grids, strides)):
        ys, xs = np.mgrid[0:gh, 0:gw]
        in_h, in_w = min(gh, int(img_shape[0] * (1.0 / s)) + 1), min(gw, int(img_shape[1] * (1.0 / s)) + 1)
        pos = np.zeros((gh, gw), bool)
        ign = np.zeros((gh, gw), bool)
        mask = np.zeros((gh, gw), np.int64)
        sbox = np.zeros((gh, gw, 4), np.float32)

        def covers(g, ratio):
            r = _region(boxes[:, g], ratio, s)
            return (r[0] <= xs) & (xs <= r[2]) & (r[1] <= ys) & (ys <= r[3])

        for g in range(boxes.shape[1]):
            if abs(int(levels[g]) - l) > 1:
                continue
            ign |= covers(g, ignore_ratio)
            if int(levels[g]) != l:
                continue
            pos |= covers(g, center_ratio)
            c = covers(g, shape_center_ratio)
            mask[c] = 1
            sbox[c] = boxes[:, g]
        loc = np.where(pos, 1, np.where(ign, -1, np.where((ys < in_h) & (xs < in_w), 0, -1))).astype(np.int64)
        locs.append(loc.reshape(-1))
        masks.append(mask.reshape(-1))
        sboxes.append(sbox.reshape(-1, 4))
    return np.concatenate(locs), np.concatenate(masks), np.concatenate(sboxes)


def map_gt2level(scale, strides, boxes):
    """region.map_gt2level with the index slip repaired (gt[2] - gt[0]), in numpy f32."""
    b = boxes.astype(np.float32)
    side = np.sqrt((b[2] - b[0]) * (b[3] - b[1])) / np.float32(scale * strides[0])
    with np.errstate(divide='ignore'):
        return np.clip(np.floor(np.log2(side)), 0, len(strides) - 1).astype(np.int64)


# ----------------------------------------------------------------- head losses
# an 8-channel GARPNHead (deformable_groups 2, anchor scale 1) on images 0 and 2 of the target
# case; both samplers are small enough to drop cells (the reference's np.random stream)
LOSS_CFG = dict(RATIOS, allowed_border=-1,
                assigner=dict(type='MaxIoUAssigner', pos_iou=0.7, neg_iou=0.3, min_pos_iou=0.3),
                sampler=dict(type='RandomSampler', max_num=64, pos_num=32),
                ga_sampler=dict(type='RandomSampler', max_num=24, pos_num=8))
LOSS_NP_SEED = 777


def head_kwargs():
    return dict(in_channels=8, feat_channels=8, octave_base_scale=ANCHOR_SCALE, scales_per_octave=1,
                anchor_strides=list(STRIDES), deformable_groups=2)


def head_state(shapes):
    import inputs
    return inputs.seeded_state(shapes)


def loss_case():
    rs = np.random.RandomState(99)
    feats = [rs.randn(2, 8, h, w).astype(np.float32) for h, w in GRIDS]
    metas = img_metas()
    return dict(feats=feats, boxes=[BOXES_0, BOXES_2], metas=[metas[0], metas[2]], np_seed=LOSS_NP_SEED)


# ----------------------------------------------------------------- whole detector
WHOLE_CONFIG = 'ga_faster_rcnn_r50_fpn.py'
WHOLE_SHAPE = (384, 640)
WHOLE_TEST_OVERRIDES = {'rcnn': {'min_score': 0.0}}  # as cfg2's fixture (inputs.WHOLE_DETECTORS)
# prefixed to the RPN head's keys before seeding: another value is another draw of the head's
# weights, to be chosen if gen_ga_golden.py finds a cut within 1e-4 of flipping
WHOLE_SEED_SALT = 'ga20:'
# inputs.seeded_state leaves every location probability above loc_filter_thr, so all 20 460 cells
# become candidates; their scores (classifier ~ N(0, 0.01^2)) lie within a few percent of each
# other, and neither a 1e-4 gap at a top-k boundary nor a stable order among 1000 kept proposals
# survives the last-bit differences of another machine's CPU convolutions.  The whole-detector
# case lowers the location layer's bias by WHOLE_LOC_SHIFT so that the filter does what it is
# for: with this draw 117 cells pass, on the two finest levels (the other three pass none), and
# no two candidate scores of a level are closer than 1e-5 relative (ten times the 1e-6 the tests
# allow a score).  None of the 117 guided anchors reaches an IoU of 0.7 with a gt, so this case's
# RPN regression loss is 0; tests/test_gpu_ga.py holds that loss on its own head.
WHOLE_LOC_SHIFT = 5.75


def whole_state(shapes):
    import inputs
    rpn = {k: v for k, v in shapes.items() if k.startswith('rpn_head.')}
    out = inputs.seeded_state({k: v for k, v in shapes.items() if k not in rpn})
    salted = inputs.seeded_state({WHOLE_SEED_SALT + k: v for k, v in rpn.items()})
    out.update({k[len(WHOLE_SEED_SALT):]: v for k, v in salted.items()})
    key = 'rpn_head.guided_anchor.loc_layer.bias'
    out[key] = out[key] - np.float32(WHOLE_LOC_SHIFT)
    return out


# ----------------------------------------------------------------- BoundedIoULoss
def bounded_iou_inputs(n=37, seed=11):
    rs = np.random.RandomState(seed)
    x, y = rs.randn(n) * 0.5, rs.randn(n) * 0.5  # shape deltas dw / dh, either sign
    y[:5] = x[:5] * (1 + 0.05 * rs.randn(5))     # a few inside the quadratic zone of beta = 0.2
    return x.astype(np.float32), y.astype(np.float32)


# ----------------------------------------------------------------- deformable convolution
def deform_case(n, cin, cout, dg, h, w, kind, seed):
    """x [n, cin, h, w], offset [n, 18 dg, h, w], weight [cout, cin, 3, 3] f32.  kind: 'eighths'
    (random multiples of 1/8 in [-3, 3]: every coordinate and bilinear weight is exact in f32),
    'zero', 'integer' (random integers in [-3, 3]), 'far' (+-1e4 and +-3e9, mixed)."""
    rs = np.random.RandomState(seed)
    x = rs.randn(n, cin, h, w).astype(np.float32)
    wt = (rs.randn(cout, cin, 3, 3) * 0.05).astype(np.float32)
    shp = (n, 18 * dg, h, w)
    if kind == 'eighths':
        off = rs.randint(-24, 25, shp).astype(np.float32) / np.float32(8)
    elif kind == 'zero':
        off = np.zeros(shp, np.float32)
    elif kind == 'integer':
        off = rs.randint(-3, 4, shp).astype(np.float32)
    elif kind == 'far':
        off = rs.choice(np.array([1e4, -1e4, 3e9, -3e9], np.float32), shp)
    else:
        raise ValueError(kind)
    return x, off, wt
