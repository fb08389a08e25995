"""Deterministic inputs of the Libra R-CNN tests (BFP neck, IoU-balanced sampler, balanced
L1): shared by tests/golden/gen_libra_golden.py (which runs the reference on them) and the
tests.  Nothing here reads the reference."""
import numpy as np

import inputs

# ----------------------------------------------------------------- BFP
BFP_RAGGED = [(13, 11), (7, 6), (4, 3), (2, 2), (1, 1)]   # every window ragged and overlapping
BFP_DIVISIBLE = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]


def bfp_levels(seed, sizes, channels, batch=2, quantise=0):
    """[B, C, H, W] f32 levels; quantise > 0 rounds the values to that many distinct levels,
    so most pooling windows hold tied maxima."""
    rng = np.random.default_rng(seed)
    out = []
    for h, w in sizes:
        a = rng.standard_normal((batch, channels, h, w)).astype(np.float32)
        if quantise:
            a = np.clip(np.round(a), -(quantise // 2), quantise // 2).astype(np.float32)
        out.append(a)
    return out


# ----------------------------------------------------------------- IoU-balanced sampler
def bin_edges(num_bins, max_iou):
    """The reference's own expressions (lib/region.py:150-152), Python floats."""
    bin_size = max_iou / num_bins
    starts = [i * bin_size for i in range(num_bins)]
    ends = [s + bin_size for s in starts]
    return starts, ends


def _edge_ious(num_bins, max_iou):
    """IoUs exactly at, one ulp below and one ulp above every f32 bin edge."""
    starts, ends = bin_edges(num_bins, max_iou)
    vals = []
    for e in sorted(set(starts + ends)):
        f = np.float32(e)
        vals += [f, np.nextafter(f, np.float32(-1)), np.nextafter(f, np.float32(2))]
    return np.array([v for v in vals if v >= 0], np.float32)


def _image(rng, n, npos, nign, num_bins, max_iou, neg_range, ngt=5):
    """(labels [n] i64, ious [n] f32): npos positives (labels 1..ngt), nign ignored, the rest
    negatives whose IoUs are the edge values followed by uniform draws from neg_range."""
    labels = np.zeros(n, np.int64)
    perm = rng.permutation(n)
    labels[perm[:npos]] = rng.integers(1, ngt + 1, npos)
    labels[perm[npos:npos + nign]] = -1
    ious = rng.uniform(0.5, 1.0, n).astype(np.float32)
    neg = np.nonzero(labels == 0)[0]
    v = rng.uniform(neg_range[0], neg_range[1], len(neg)).astype(np.float32)
    edge = _edge_ious(num_bins, max_iou)
    k = min(len(edge), len(v))
    v[:k] = edge[:k]
    ious[neg] = v[rng.permutation(len(v))]
    return labels, ious


# tag -> (np seed, max_num, pos_num, num_bins, max_iou, [per image (n, npos, nign, neg IoU range)])
SAMPLER_CASES = {
    'more_pos': (11, 128, 32, 3, 0.5, [(300, 60, 20, (0.0, 0.6))]),
    'few_pos': (12, 128, 32, 3, 0.5, [(300, 10, 20, (0.0, 0.6))]),
    'starved_top': (13, 128, 32, 3, 0.5, [(300, 40, 10, (0.0, 0.3))]),      # top bin: edge values only
    'all_starved': (14, 128, 32, 3, 0.5, [(300, 20, 240, (0.0, 0.6))]),     # 40 negatives in all
    'no_neg': (15, 128, 32, 3, 0.5, [(300, 50, 250, (0.0, 0.6))]),
    'one_bin': (16, 128, 32, 1, 0.5, [(300, 40, 20, (0.0, 0.6))]),
    'two_images': (17, 128, 32, 3, 0.5, [(300, 60, 20, (0.0, 0.6)), (260, 8, 30, (0.0, 0.55))]),
    # device mode only (no fixture): more than one register slot per thread is live
    'big': (18, 512, 128, 3, 0.5, [(2500, 200, 100, (0.0, 0.6))]),
}
SAMPLER_FIXTURE_CASES = [t for t in SAMPLER_CASES if t != 'big']


def sampler_case(tag):
    """dict(labels=[..], ious=[..] per image, np_seed, max_num, pos_num, num_bins, max_iou)."""
    seed, max_num, pos_num, nb, max_iou, imgs = SAMPLER_CASES[tag]
    rng = np.random.default_rng(4000 + seed)
    labels, ious = [], []
    for n, npos, nign, rg in imgs:
        lab, iou = _image(rng, n, npos, nign, nb, max_iou, rg)
        labels.append(lab)
        ious.append(iou)
    return dict(labels=labels, ious=ious, np_seed=seed, max_num=max_num, pos_num=pos_num, num_bins=nb,
                max_iou=max_iou)


# ----------------------------------------------------------------- sampler feeding bbox_target
TARGET_NP_SEED = 3100
TARGET_SAMPLER = dict(max_num=128, pos_num=32, num_bins=3, max_iou=0.5)
TARGET_ASSIGNER = (0.5, 0.5, 0.5)
TARGET_STDS = (0.1, 0.1, 0.2, 0.2)


def target_case():
    """Two images: (proposals [4, n_i] f32, gt boxes [4, G_i], gt labels [G_i])."""
    gts = inputs.voc_gts()
    out = []
    for i, n in enumerate((600, 450)):
        gb, gl = gts[4 + i]
        rng = np.random.default_rng(3200 + i)
        # half the proposals are jittered ground truth (a spread of IoUs), half random boxes
        k = n // 2
        src = gb[:, rng.integers(0, gb.shape[1], k)]
        w, h = src[2] - src[0], src[3] - src[1]
        jit = rng.uniform(-0.45, 0.45, (4, k)).astype(np.float32) * np.stack([w, h, w, h])
        near = (src + jit).astype(np.float32)
        near[2] = np.maximum(near[2], near[0] + 2)
        near[3] = np.maximum(near[3], near[1] + 2)
        props = np.concatenate([near, inputs.random_boxes(3300 + i, n - k, min_wh=8, max_wh=300)], 1)
        out.append((np.ascontiguousarray(props.astype(np.float32)), gb, gl))
    return out


# ----------------------------------------------------------------- balanced L1
def balanced_l1_inputs(seed, n, m):
    """(x, y) [n, m] f32 with differences on both sides of beta = 1."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, m)).astype(np.float32)
    y = (x + rng.standard_normal((n, m)) * 1.2).astype(np.float32)
    return x, y


# ----------------------------------------------------------------- whole detector
WHOLE_LIBRA = ('libra', 'libra_faster_rcnn_r50_fpn.py', {'rcnn': {'min_score': 0.0}}, inputs.FTRAIN_SHAPE)
