"""Deterministic inputs of the GFL tests (fused QFL / DFL / GIoU head loss, DFL box decode):
shared by tests/golden/gen_gfl_golden.py (which runs the reference on them) and the tests.
Nothing here reads the reference."""
import numpy as np

# the loss weights and scalars of configs/fcos_r50_fpn_atss_gfl.py
WEIGHTS = dict(cls_weight=1.0, dfl_weight=0.25, bbox_weight=2.0, beta=2.0, dfl_avg_factor=4.0)
REG_STD, REG_MEAN = 1200.0, 0.0
GRIDS3 = [(5, 7), (3, 4), (2, 2)]
# one positive with two sides exactly on bin boundaries (96 / 1200 = 0.08, 192 / 1200 = 0.16), one in
# the last legal bin and one near zero
PLANTED = (96.0, 192.0, 1439.0, 1e-3)

# tag -> dict(seed, batch, grids, C, bins, stride, labels drawn from, logit scale, ltrb upper bound, norm_prob)
LOSS_CASES = {
    'mixed': dict(seed=1, batch=2, grids=GRIDS3, C=20, bins=16, stride=0.08, draw=(-1, 0, 0, 0, 1, 3, 20), scale=1.0,
                  hi=1400.0, norm_prob=False),
    'sharp': dict(seed=1, batch=2, grids=GRIDS3, C=20, bins=16, stride=0.08, draw=(-1, 0, 0, 0, 1, 3, 20), scale=12.0,
                  hi=1400.0, norm_prob=False),
    'one': dict(seed=2, batch=2, grids=GRIDS3, C=20, bins=16, stride=0.08, draw=(0,), scale=1.0, hi=1400.0,
                norm_prob=False, positives=(-1,)),
    'first_last': dict(seed=3, batch=1, grids=[(17, 19)], C=20, bins=16, stride=0.08, draw=(-1, 0, 0), scale=1.0,
                       hi=1400.0, norm_prob=False, positives=(0, -1)),
    'bins8': dict(seed=4, batch=2, grids=GRIDS3, C=3, bins=8, stride=0.16, draw=(-1, 0, 0, 0, 1, 2, 3), scale=1.0,
                  hi=1300.0, norm_prob=False),
    'norm_prob': dict(seed=1, batch=2, grids=GRIDS3, C=20, bins=16, stride=0.08, draw=(-1, 0, 0, 0, 1, 3, 20),
                      scale=1.0, hi=1400.0, norm_prob=True),
}


def loss_case(tag):
    """dict(cls [C, M] f32, reg [4*bins, M] f32 (channel = bin*4 + side), labels [M] i64, ltrb [M, 4]
    f32; positions ordered images outer, levels inner, row-major in a level) plus the case's
    scalars.  `sharp` and `norm_prob` share `mixed`'s draws."""
    c = dict(LOSS_CASES[tag])
    rng = np.random.default_rng(7100 + c['seed'])
    m = c['batch'] * sum(h * w for h, w in c['grids'])
    labels = rng.choice(np.array(c['draw'], np.int64), size=m)
    for p in c.get('positives', ()):
        labels[p] = 1 + (p % c['C'])
    cls = rng.standard_normal((c['C'], m)).astype(np.float32) * np.float32(c['scale'])
    reg = rng.standard_normal((4 * c['bins'], m)).astype(np.float32) * np.float32(c['scale'])
    ltrb = rng.uniform(0.5, c['hi'], (m, 4)).astype(np.float32)
    pos = np.nonzero(labels > 0)[0]
    if c['hi'] == 1400.0:
        ltrb[pos[len(pos) // 2]] = PLANTED
    c.update(cls=cls, reg=reg, labels=labels, ltrb=ltrb, M=m, reg_std=REG_STD, reg_mean=REG_MEAN)
    return c


def loss_kwargs(c):
    """The keyword arguments of ops.gfl_losses / losses.gfl_head_losses_torch for a case."""
    return dict(bins=c['bins'], stride=c['stride'], reg_mean=c['reg_mean'], reg_std=c['reg_std'],
                norm_prob=c['norm_prob'], **WEIGHTS)


def level_slices(c):
    """(image, level, grid, column slice into the flat tensors) in the flat order."""
    out, off = [], 0
    for b in range(c['batch']):
        for lv, (h, w) in enumerate(c['grids']):
            out.append((b, lv, (h, w), slice(off, off + h * w)))
            off += h * w
    return out


# ----------------------------------------------------------------- decode
DECODE_BINS, DECODE_STRIDE = 16, 0.08
DECODE_IMG = (600, 1000)
DECODE_LEVELS = [(8, (13, 17)), (16, (7, 9)), (32, (4, 5))]  # (cell stride, grid)


def decode_case():
    """Per level (cell stride, reg [2, 64, H, W] f32): N(0, 3) logits; every other position gets
    +8 on one of its two lowest bins per side, so short distances (boxes inside the image, not
    clamped) occur next to the long ones that clamp."""
    rng = np.random.default_rng(7200)
    out = []
    for cell, (h, w) in DECODE_LEVELS:
        r = (3.0 * rng.standard_normal((2, 4 * DECODE_BINS, h, w))).astype(np.float32)
        low = rng.integers(0, 2, (2, 4, h, w))
        peaked = rng.random((2, 1, h, w)) < 0.5
        for side in range(4):
            for b in range(2):
                ch = b * 4 + side
                r[:, ch] += np.float32(8.0) * (peaked[:, 0] & (low[:, side] == b))
        out.append((cell, r))
    return out


# ----------------------------------------------------------------- whole detector
WHOLE_GFL = ('gfl', 'fcos_r50_fpn_atss_gfl.py', {}, (384, 640))
