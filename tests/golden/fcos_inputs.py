"""Deterministic inputs of the plain-FCOS tests (scale-range target assignment, fused focal / GIoU /
centerness head loss): shared by tests/golden/gen_fcos_golden.py (which runs the reference on
them) and the tests.  Nothing here reads the reference."""
import numpy as np

# ----------------------------------------------------------------- targets
STRIDES = [8, 16, 32, 64, 128]
PAD_SHAPE = (320, 512)
GRIDS = [(40, 64), (20, 32), (10, 16), (5, 8), (3, 4)]  # 3412 cells
NUM_CELLS = sum(h * w for h, w in GRIDS)
REAL_THR = [0, 64, 128, 256, 512, 1e6]      # FCOSHead.level_scale_thr
SMALL_THR = [0, 32, 64, 128, 256, 1e6]      # a 512-px image reaches the last level only with these
# image 0: (300, 500): 300/8 = 37.5 -> 38 and 500/8 = 62.5 -> 62 (half to even, both ways), 500/32 =
# 15.625 -> 16; image 1: (320, 512): the paint reaches one past the grid and is clipped
IMG_SHAPES = [(300, 500, 3), (320, 512, 3)]

# Six gts of distinct areas (x1, y1, x2, y2):
#   0 covers the image: the coarse levels; it loses every cell another gt matches on the same level
#   1, 2 nested: around (100, 84) both match on level 0 and the smaller (2) must win
#   3 x1 = 204 is a level-0 cell centre (4 + 8*25): ltrb_l == 0 there is not positive
#   4 128 x 128 around the level-0 cell centre (364, 164): max(ltrb) is exactly 64 there, which
#     level 0 (< 64) refuses
#   5 128 wide, 120 high around the level-1 cell centre (136, 232): max(ltrb) exactly 64, which
#     level 1 (>= 64) takes
# The coordinates are chosen so that every centerness of the fixture is the correctly rounded
# f32 square root: some vectorised CPU square roots are a last bit off at a few values, and the
# fixture must not depend on which one made it (gen_fcos_golden.py asserts this).
BOXES_A = np.array([[10, 10, 490, 288], [40, 28, 160, 140], [84, 60, 124, 110], [204, 180, 250, 230],
                    [300, 100, 428, 228], [72, 172, 200, 292]], np.float32).T.copy()
LABELS_A = np.array([7, 3, 12, 5, 20, 1], np.int64)
LABELS_B = np.array([7, 3, 12, 0, 20, 1], np.int64)   # gt 3 carries label 0
# two equal areas (61 x 61) overlapping in x 120..160, y 100..140, and a larger one under both
BOXES_TIE = np.array([[100, 80, 160, 140], [120, 100, 180, 160], [60, 40, 220, 200]], np.float32).T.copy()
LABELS_TIE = np.array([4, 9, 2], np.int64)

# tag -> (per-image boxes [4, G], per-image labels, level_scale_thr); two images under one padded size
TARGET_CASES = {
    'a': ([BOXES_A, np.zeros((4, 0), np.float32)], [LABELS_A, np.zeros(0, np.int64)], REAL_THR),
    'b': ([BOXES_A, np.zeros((4, 0), np.float32)], [LABELS_B, np.zeros(0, np.int64)], SMALL_THR),
    # checked against a numpy restatement in the tests, not against the reference: its order of
    # equal areas rests on a sort the API does not promise to be stable
    'tie': ([BOXES_TIE, BOXES_TIE[:, ::-1].copy()], [LABELS_TIE, LABELS_TIE[::-1].copy()], REAL_THR),
}
REFERENCE_TARGET_CASES = ('a', 'b')


def img_metas():
    return [{'img_shape': s, 'pad_shape': PAD_SHAPE + (3,), 'scale_factor': 1.0} for s in IMG_SHAPES]


def level_outputs(batch=None):
    """Shapes only: what single_image_targets reads of the head outputs ([C, H, W] per level, or
    [B, C, H, W] with a batch)."""
    lead = () if batch is None else (batch,)
    return [np.zeros(lead + (1, h, w), np.float32) for h, w in GRIDS]


# ----------------------------------------------------------------- losses
# the loss weights and scalars of configs/fcos_r50_fpn.py (FocalLoss keeps alpha 0.25, gamma 2)
WEIGHTS = dict(cls_weight=1.0, bbox_weight=2.0, ctr_weight=1.0, alpha=0.25, gamma=2.0)
REG_STD, REG_MEAN = 1200.0, 0.0

# tag -> dict(seed, batch, grids, C, labels drawn from, reg_std, reference: whether the reference's
# calc_loss runs on it).  M = 1, 255, 257 (either side of one 256-thread workgroup) and 2 * 3412; C
# in {1, 3, 20}.  The reference squeezes a one-position mask to 0-d and divides by a zero positive
# count: those cases are checked against the restatement only.
LOSS_CASES = {
    'one': dict(seed=1, batch=1, grids=[(1, 1)], C=20, draw=(5,), reg_std=REG_STD, reference=False),
    'm255': dict(seed=2, batch=1, grids=[(15, 17)], C=20, draw=(-1, 0, 0, 0, 1, 3, 20), reg_std=REG_STD,
                 reference=True),
    'm257': dict(seed=3, batch=1, grids=[(16, 16), (1, 1)], C=1, draw=(-1, 0, 0, 1), reg_std=REG_STD,
                 reference=True, positives=(-1,)),
    'full': dict(seed=4, batch=2, grids=GRIDS, C=3, draw=(-1,) + (0,) * 40 + (1, 2, 3), reg_std=REG_STD,
                 reference=True),
    'no_pos': dict(seed=5, batch=1, grids=[(16, 16), (1, 1)], C=20, draw=(-1, 0, 0, 0), reg_std=REG_STD,
                   reference=False),
    'ignored': dict(seed=6, batch=1, grids=[(15, 17)], C=3, draw=(-1,), reg_std=REG_STD, reference=False),
    # reg_std a power of two, so prediction == target holds in f32 and in f64 alike: every fourth
    # positive has its l and r sides tied, every eighth all four (the two boxes are then equal)
    'tie': dict(seed=7, batch=1, grids=[(16, 16), (1, 1)], C=3, draw=(-1, 0, 1, 2, 3), reg_std=1024.0,
                reference=True, tie=True),
}
REFERENCE_LOSS_CASES = tuple(sorted(t for t, c in LOSS_CASES.items() if c['reference']))


def _centerness(ltrb):
    v = ltrb + np.float32(1e-6)
    l, t, r, b = v[:, 0], v[:, 1], v[:, 2], v[:, 3]
    return np.sqrt((np.minimum(l, r) / np.maximum(l, r)) * (np.minimum(t, b) / np.maximum(t, b))).astype(np.float32)


def loss_case(tag):
    """dict(cls [C, M] f32 logits, reg [4, M] f32 positive ltrb predictions, ctr [M] f32 logits,
    labels [M] i64, ltrb [M, 4] f32, ctr_t [M] f32; positions ordered images outer, levels inner,
    row-major in a level) plus the case's scalars.  The targets are consistent with an assigner's:
    positives carry a positive ltrb and its centerness, the others ltrb -1 and centerness 0 (label
    0) or -1 (label -1).  The two boxes of a positive both contain the origin, so they are never
    disjoint."""
    c = dict(LOSS_CASES[tag])
    rng = np.random.default_rng(7500 + c['seed'])
    m = c['batch'] * sum(h * w for h, w in c['grids'])
    labels = rng.choice(np.array(c['draw'], np.int64), size=m)
    for p in c.get('positives', ()):
        labels[p] = 1 + (p % c['C'])
    pos = labels > 0
    ltrb = rng.uniform(0.5, 500.0, (m, 4)).astype(np.float32)
    y = ((ltrb - np.float32(REG_MEAN)) / np.float32(c['reg_std'])).astype(np.float32)
    reg = (y * np.exp(0.5 * rng.standard_normal((m, 4))).astype(np.float32)).astype(np.float32)
    if c.get('tie'):
        idx = np.nonzero(pos)[0]
        reg[idx[::4, None], [0, 2]] = y[idx[::4, None], [0, 2]]
        reg[idx[::8]] = y[idx[::8]]
    ctr_t = np.where(pos, _centerness(ltrb), np.where(labels == 0, 0.0, -1.0)).astype(np.float32)
    ltrb[~pos] = -1.0
    cls = rng.standard_normal((c['C'], m)).astype(np.float32)
    ctr = rng.standard_normal(m).astype(np.float32)
    c.update(cls=cls, reg=reg.T.copy(), ctr=ctr, labels=labels, ltrb=ltrb, ctr_t=ctr_t, M=m, reg_mean=REG_MEAN)
    return c


def loss_kwargs(c):
    """The keyword arguments of ops.fcos_losses / losses.fcos_head_losses_torch for a case."""
    return dict(reg_mean=c['reg_mean'], reg_std=c['reg_std'], **WEIGHTS)


def level_slices(c):
    """(image, level, grid, column slice into the flat tensors) in the flat order."""
    out, off = [], 0
    for b in range(c['batch']):
        for lv, (h, w) in enumerate(c['grids']):
            out.append((b, lv, (h, w), slice(off, off + h * w)))
            off += h * w
    return out


# ----------------------------------------------------------------- whole detector
WHOLE_FCOS = ('fcos', 'fcos_r50_fpn.py', {}, (384, 640))
