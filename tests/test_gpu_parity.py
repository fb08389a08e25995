"""GPU parity: the HIP kernels (through the C-ABI) against the reference's
golden vectors and the CPU oracle, on the same seeded inputs.

Bars: bit-exact for anchors, masks, IoU tables, assignment labels/IoUs,
sampling (numpy-parity mode), chosen indices and NMS keep lists; float
tolerances are stated per test (encode/decode log/exp, RoIAlign 1e-5)."""
import os

import numpy as np
import pytest
import torch

import inputs
import oracle
import support
from support import canon_ties, sha

pytestmark = pytest.mark.gpu


def T(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


ANCHOR_CASES = {
    'fpn': (inputs.FPN_STRIDES, inputs.FPN_GRIDS, [8], [0.5, 1.0, 2.0]),
    'retina': (inputs.RETINA_STRIDES, inputs.RETINA_GRIDS, [4 * 2 ** (i / 3) for i in range(3)], [0.5, 1.0, 2.0]),
    'atss': (inputs.RETINA_STRIDES, inputs.RETINA_GRIDS, [8], [1.0]),
    'c4': ([16], inputs.C4_GRIDS, [4, 8, 16, 32], [0.5, 1.0, 2.0]),
}


def fpn_setup(dev):
    from frcnn_amd.heads.rpn_head import RPNHead
    head = RPNHead(256, 256, loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                   loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0)).to(dev)
    anchors = head._flat_anchors(inputs.FPN_GRIDS, dev)
    return head, anchors


# ----------------------------------------------------------------- a1/a2
@pytest.mark.parametrize('name', sorted(ANCHOR_CASES))
def test_anchor_grid_bit_exact(dev, golden, name):
    from frcnn_amd.anchor import AnchorCreator
    g = golden('anchors.npz')
    strides, grids, scales, ratios = ANCHOR_CASES[name]
    for l, (s, grid) in enumerate(zip(strides, grids)):
        a = AnchorCreator(base=s, scales=scales, aspect_ratios=ratios, device=dev)(s, grid)
        assert tuple(a.shape) == (4, len(scales) * len(ratios)) + tuple(grid)
        assert sha(a.cpu().numpy()) == str(g['{}_{}_sha'.format(name, l)]), (name, l)


def test_inside_mask_bit_exact(dev, golden):
    g = golden('assign.npz')
    head, anchors = fpn_setup(dev)
    m = head._valid_masks(anchors, inputs.FPN_GRIDS, [inputs.img_meta()], 0)[0]
    assert int(m.sum()) == int(g['mask_count'])
    assert sha(m.cpu().numpy()) == str(g['mask_sha'])


# ----------------------------------------------------------------- a3
def test_iou_bit_exact(dev, golden):
    from frcnn_amd import utils
    g = golden('assign.npz')
    a, b = T(inputs.random_boxes(11, 3000), dev), T(inputs.random_boxes(12, 40), dev)
    np.testing.assert_array_equal(utils.calc_iou(a, b).cpu().numpy(), g['rand_iou'])
    np.testing.assert_array_equal(utils.elem_iou(a[:, :40], b).cpu().numpy(), g['rand_elem_iou'])
    head, anchors = fpn_setup(dev)
    m = head._valid_masks(anchors, inputs.FPN_GRIDS, [inputs.img_meta()], 0)[0].bool()
    ina = anchors[:, m]
    gts = inputs.voc_gts()
    for i in range(2):
        t = utils.calc_iou(ina, T(gts[i][0], dev)).cpu().numpy()
        assert sha(t) == str(g['iou_{}_sha'.format(i)])


# ----------------------------------------------------------------- a4
@pytest.mark.parametrize('tag,thr', [('rpn', (0.7, 0.3, 0.3)), ('rcnn', (0.5, 0.5, 0.5)), ('retina', (0.5, 0.4, 0.0))])
def test_assign_batched_bit_exact(dev, golden, tag, thr):
    """All 8 images in ONE fused launch over the full anchor set with validity masks."""
    from frcnn_amd import ops
    g = golden('assign.npz')
    head, anchors = fpn_setup(dev)
    masks = head._valid_masks(anchors, inputs.FPN_GRIDS, [inputs.img_meta()] * 8, 0)
    gts = inputs.voc_gts()[:8]
    gb, gc, gm = ops.pack_boxes([T(x[0], dev) for x in gts], dev)
    N = anchors.shape[1]
    num = torch.full((8,), N, dtype=torch.int32, device=dev)
    labels, miou = ops.maxiou_assign(anchors, 0, num, N, gb, gc, gm, *thr, valid=masks,
                                     valid_seg_stride=masks.stride(0))
    m0 = masks[0].bool()
    for i in range(8):
        lab = labels[i][m0].cpu().numpy()
        np.testing.assert_array_equal(lab.astype(np.int8), g['{}_{}_labels'.format(tag, i)])
        assert sha(miou[i][m0].cpu().numpy()) == str(g['{}_{}_miou_sha'.format(tag, i)])
        assert bool((labels[i][~m0] == -1).all())


def test_assigner_api_random_boxes(dev, golden):
    from frcnn_amd.region import MaxIoUAssigner
    g = golden('assign.npz')
    lab, miou = MaxIoUAssigner(0.5, 0.4, 0.0)(T(inputs.random_boxes(11, 3000), dev),
                                             T(inputs.random_boxes(12, 40), dev))
    np.testing.assert_array_equal(lab.cpu().numpy(), g['rand_labels'])
    np.testing.assert_array_equal(miou.cpu().numpy(), g['rand_miou'])


def test_assign_ties_and_nan_free_edges(dev):
    """Identical boxes (all tie at a gt's max), boxes touching gts, far-away boxes."""
    from frcnn_amd.region import MaxIoUAssigner
    gts = np.array([[10, 10, 50, 50], [100, 100, 140, 180], [10, 10, 50, 50]], np.float32).T
    boxes = np.concatenate([np.tile(gts[:, :1], (1, 5)), np.array([[51, 51, 90, 90], [500, 500, 600, 600],
                                                                  [100, 100, 140, 180]], np.float32).T,
                            inputs.random_boxes(7, 500)], 1)
    for thr in ((0.7, 0.3, 0.3), (0.5, 0.4, 0.0), (0.5, 0.5, 0.5)):
        lab, miou = MaxIoUAssigner(*thr)(T(boxes, dev), T(gts, dev))
        rl, ri = oracle.maxiou_assign(boxes, gts, *thr)
        np.testing.assert_array_equal(lab.cpu().numpy(), rl)
        np.testing.assert_array_equal(miou.cpu().numpy(), ri)


def test_assign_one_launch_handoff_cases(dev):
    """The single-launch assignment's hand-off: boxes tied at a gt's maximum in many
    workgroups (the last workgroup labels them), a gt no box overlaps with min_pos_iou 0
    (every box a candidate: the whole segment goes through the hand-off), a segment with no
    gts and an empty segment in the same launch, and the same workspace reused (its
    counters must come back zero)."""
    from frcnn_amd import ops
    gts = np.array([[10, 10, 50, 50], [100, 100, 140, 180], [9000, 9000, 9050, 9050]], np.float32).T
    n = 20000
    boxes = inputs.random_boxes(8, n)
    for pos in (3, 300, 301, 700, 5000, 12345, 19999):  # one gt's exact copy in many workgroups
        boxes[:, pos] = gts[:, pos % 2]
    segs = [(boxes, gts), (boxes[:, :9000], gts[:, :2]), (boxes[:, :5000], gts[:, :0]), (boxes[:, :0], gts)]
    S = len(segs)
    bb = torch.zeros(S, 4, n, device=dev)
    for s, (b, _) in enumerate(segs):
        bb[s, :, :b.shape[1]] = T(b, dev)
    num = torch.tensor([b.shape[1] for b, _ in segs], dtype=torch.int32, device=dev)
    gb, gc, gm = ops.pack_boxes([T(g, dev) for _, g in segs], dev)
    for thr in ((0.7, 0.3, 0.3), (0.5, 0.4, 0.0), (0.5, 0.5, 0.5), (0.7, 0.3, 0.3)):
        labels, miou = ops.maxiou_assign(bb, bb.stride(0), num, n, gb, gc, gm, *thr)
        for s, (b, g) in enumerate(segs):
            k = b.shape[1]
            if k == 0:
                continue
            if g.shape[1] == 0:
                assert bool((labels[s, :k] == -1).all()) and bool((miou[s, :k] == 0).all())
                continue
            rl, ri = oracle.maxiou_assign(b, g, *thr)
            np.testing.assert_array_equal(labels[s, :k].cpu().numpy(), rl)
            np.testing.assert_array_equal(miou[s, :k].cpu().numpy(), ri)


# ----------------------------------------------------------------- a5/a6 anchor targets (numpy-parity sampler)
def test_anchor_target_single_image_vs_reference(dev, golden):
    from frcnn_amd import anchor as A
    from frcnn_amd.region import MaxIoUAssigner, RandomSampler
    from frcnn_amd import set_sampler_mode
    set_sampler_mode('numpy')
    g = golden('targets.npz')
    head, anchors = fpn_setup(dev)
    m = head._valid_masks(anchors, inputs.FPN_GRIDS, [inputs.img_meta()], 0)[0].bool()
    ina = anchors[:, m]
    gts = inputs.voc_gts()
    for i in range(4):
        cls, reg = inputs.head_outputs(100 + i, inputs.FPN_GRIDS, 3, 1)
        cls_out = T(np.concatenate([c[0].reshape(1, -1) for c in cls], 1), dev)
        reg_out = T(np.concatenate([r[0].reshape(4, -1) for r in reg], 1), dev)
        np.random.seed(1000 + i)
        out = A.anchor_target(cls_out, reg_out, 1, ina, m, T(gts[i][0], dev),
                              torch.ones(gts[i][0].shape[1], dtype=torch.long, device=dev),
                              MaxIoUAssigner(0.7, 0.3, 0.3), RandomSampler(256, 128), [0.0] * 4, [1.0] * 4)
        names = ('tar_cls_out', 'tar_reg_out', 'tar_labels', 'tar_anchors', 'tar_bbox')
        for k, v in zip(names, out[:5]):
            np.testing.assert_array_equal(v.cpu().numpy(), g['rpn_{}_{}'.format(i, k)], err_msg=k)
        np.testing.assert_allclose(out[5].cpu().numpy(), g['rpn_{}_tar_param'.format(i)], rtol=1e-5, atol=1e-5)
        assert np.random.randint(0, 2 ** 31 - 1) == int(g['rpn_{}_rng_after'.format(i)])


def test_rpn_targets_batched_equal_per_image_oracle(dev):
    """B=4 batched targets == per-image oracle results concatenated (one numpy stream)."""
    from frcnn_amd.config import wrap
    from frcnn_amd import set_sampler_mode
    set_sampler_mode('numpy')
    head, anchors = fpn_setup(dev)
    gts = inputs.voc_gts()[10:14]
    cls, reg = inputs.head_outputs(900, inputs.FPN_GRIDS, 3, 1, batch=4)
    cfg = wrap(dict(assigner=dict(type='MaxIoUAssigner', pos_iou=0.7, neg_iou=0.3, min_pos_iou=0.3),
                    sampler=dict(type='RandomSampler', max_num=256, pos_num=128), allowed_border=0))
    np.random.seed(77)
    tc, tr, tl, tp = head.targets_batched([T(c, dev) for c in cls], [T(r, dev) for r in reg],
                                          [T(x[0], dev) for x in gts],
                                          [torch.ones(x[0].shape[1], dtype=torch.long, device=dev) for x in gts],
                                          [inputs.img_meta()] * 4, cfg)
    anc = anchors.cpu().numpy()
    mask = head._valid_masks(anchors, inputs.FPN_GRIDS, [inputs.img_meta()], 0)[0].bool().cpu().numpy()
    np.random.seed(77)
    ref = {k: [] for k in range(6)}
    for b in range(4):
        co = np.concatenate([c[b].reshape(1, -1) for c in cls], 1)
        ro = np.concatenate([r[b].reshape(4, -1) for r in reg], 1)
        out = oracle.anchor_target(co, ro, 1, anc[:, mask], mask, gts[b][0], np.ones(gts[b][0].shape[1], np.int64),
                                   (0.7, 0.3, 0.3), (256, 128), [0.0] * 4, [1.0] * 4)
        for k in range(6):
            ref[k].append(out[k])
    np.testing.assert_array_equal(tc.detach().cpu().numpy(), np.concatenate(ref[0], 1))
    np.testing.assert_array_equal(tr.detach().cpu().numpy(), np.concatenate(ref[1], 1))
    np.testing.assert_array_equal(tl.cpu().numpy(), np.concatenate(ref[2]))
    np.testing.assert_allclose(tp.cpu().numpy(), np.concatenate(ref[5], 1), rtol=1e-5, atol=1e-5)


def test_rpn_loss_vs_reference(dev, golden):
    from frcnn_amd.config import wrap
    from frcnn_amd import set_sampler_mode
    set_sampler_mode('numpy')
    g = golden('rpn_loss.npz')
    head, _ = fpn_setup(dev)
    gts = inputs.voc_gts()
    cfg = wrap(dict(assigner=dict(type='MaxIoUAssigner', pos_iou=0.7, neg_iou=0.3, min_pos_iou=0.3),
                    sampler=dict(type='RandomSampler', max_num=256, pos_num=128), allowed_border=0))
    for i in range(2):
        cls, reg = inputs.head_outputs(700 + i, inputs.FPN_GRIDS, 3, 1, batch=2)
        np.random.seed(3000 + i)
        c, r = head.loss([T(x, dev) for x in cls], [T(x, dev) for x in reg],
                         [T(gts[2 * i + j][0], dev) for j in range(2)],
                         [torch.ones(gts[2 * i + j][0].shape[1], dtype=torch.long, device=dev) for j in range(2)],
                         [inputs.img_meta()] * 2, cfg)
        np.testing.assert_allclose([float(c), float(r)], g['loss_{}'.format(i)], rtol=2e-5)


@pytest.mark.parametrize('max_num,pos_num', [(256, 128), (512, 128), (6000, 3000)])
def test_device_sampler_properties(dev, max_num, pos_num):
    """Device sampler (one top-k workgroup per (image, pos/neg); max_num > 4096 takes the
    global-index path): exact pos/neg counts, kept rows keep their labels, rows past num
    untouched, empty and candidate-poor segments."""
    from frcnn_amd import ops
    rng = np.random.default_rng(3)
    S, n = 5, 130001
    lab = rng.choice([-1, 0, 0, 0, 1, 2], size=(S, n), p=[0.3, 0.2, 0.2, 0.2, 0.05, 0.05]).astype(np.int64)
    lab[2, :] = np.where(lab[2] > 0, 0, lab[2])  # a segment with no positives
    lab[4, :3000] = np.where(lab[4, :3000] == 0, -1, lab[4, :3000])  # fewer negatives than slots
    lt = T(lab, dev)
    num = torch.tensor([n, n - 5, 1000, 0, 3000], dtype=torch.int32, device=dev)
    out = ops.sample_labels(lt, num, n, max_num, pos_num, mode='device').cpu().numpy()
    for s in range(S):
        ns = int(num[s])
        src, o = lab[s, :ns], out[s, :ns]
        npos, nneg = int((src > 0).sum()), int((src == 0).sum())
        kp = min(npos, pos_num)
        assert int((o > 0).sum()) == kp
        assert int((o == 0).sum()) == min(nneg, max_num - kp)
        kept = o >= 0
        np.testing.assert_array_equal(o[kept], src[kept])  # kept rows keep their labels
    # fresh draws differ, and a fixed (seed, call) reproduces
    out2 = ops.sample_labels(lt, num, n, max_num, pos_num, mode='device').cpu().numpy()
    assert not np.array_equal(out, out2)


def _hash_u32(seed, a, b):
    """block_ops.h hash_u32 (splitmix64 finaliser of seed ^ (a << 32 | b)), vectorised over b."""
    m = np.uint64(0xFFFFFFFFFFFFFFFF)
    z = np.uint64(seed) ^ ((np.uint64(a) << np.uint64(32)) | b.astype(np.uint64))
    with np.errstate(over='ignore'):
        z = z + np.uint64(0x9e3779b97f4a7c15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    z = (z ^ (z >> np.uint64(31))) & m
    return (z >> np.uint64(32)).astype(np.uint32)


@pytest.mark.parametrize('n,max_num,pos_num', [(200003, 256, 128), (2050, 512, 128), (16384, 512, 128),
                                               (3000, 4000, 1000)])
def test_device_sampler_selects_top_hash_keys(dev, n, max_num, pos_num):
    """The device sampler's selection is exactly its definition: per image, the kp = min(npos,
    pos_num) positives and kn = min(nneg, max_num - kp) negatives with the largest keys
    (~hash(seed, 2s (+1), box) | 1), ties by box index -- recomputed here in numpy.  Images
    up to 16384 boxes take the one-workgroup radix select, larger ones the two-launch
    segmented top-k."""
    from frcnn_amd import ops
    rng = np.random.default_rng(21)
    S = 3
    lab = rng.choice([-1, 0, 1], size=(S, n), p=[0.4, 0.5, 0.1] if n < 20000 else [0.4, 0.59, 0.01]).astype(np.int64)
    lab[1, :] = np.where(lab[1] > 0, -1, lab[1])  # no positives
    num = torch.tensor([n, n - 11, n // 3], dtype=torch.int32, device=dev)
    ops.set_sampler_mode('device', seed=5)
    out = ops.sample_labels(T(lab, dev), num, n, max_num, pos_num, mode='device').cpu().numpy()
    seed = (ops._SAMPLER['seed'] * 0x9E3779B97F4A7C15 + ops._SAMPLER['calls']) & 0xFFFFFFFFFFFFFFFF
    ops.set_sampler_mode('numpy')
    for s in range(S):
        ns = int(num[s])
        idx = np.arange(ns, dtype=np.uint32)
        src = lab[s, :ns]
        want = np.full(ns, -1, np.int64)
        pos, neg = np.nonzero(src > 0)[0], np.nonzero(src == 0)[0]
        kp = min(len(pos), pos_num)
        kn = min(len(neg), max_num - kp)
        for cand, v, k in ((pos, 2 * s, kp), (neg, 2 * s + 1, kn)):
            key = (~_hash_u32(seed, v, idx[cand])) | np.uint32(1)
            order = np.lexsort((cand, -key.astype(np.int64)))  # key desc, index asc
            want[cand[order[:k]]] = src[cand[order[:k]]]
        np.testing.assert_array_equal(out[s, :ns], want)


@pytest.mark.parametrize('max_num,pos_num,n', [(256, 128, 20000), (512, 128, 20000), (512, 128, 3000)])
def test_device_sampler_lists_feed_targets(dev, max_num, pos_num, n):
    """The device sampler's selection lists (frh_sample_random sel / sel_counts) fed straight
    into the target gathers (rank-by-counting into ascending box order, no compaction pass)
    give exactly the targets of the sampled-labels path (labels >= 0 compacted in order), for
    the same draw; also for an image with fewer candidates than slots and an empty one."""
    from frcnn_amd import ops
    rng = np.random.default_rng(8)
    S = 4
    lab = rng.choice([-1, 0, 1, 2, 3], size=(S, n), p=[0.3, 0.6, 0.04, 0.03, 0.03]).astype(np.int64)
    lab[3, :] = np.where(lab[3] >= 0, -1, lab[3])
    lab[3, :40] = 0  # 40 candidates for max_num slots
    lt = T(lab, dev)
    num = torch.tensor([n, n - 7, 0, n], dtype=torch.int32, device=dev)
    anchors = T(inputs.random_boxes(12, n), dev)
    gts, gcnt, gmax = ops.pack_boxes([T(inputs.random_boxes(13 + s, 3), dev) for s in range(S)], dev)
    glab = ops.pack_labels([torch.tensor([4, 9, 17], device=dev)] * S, gmax, dev)
    res = []
    for lists in (False, True):
        ops.set_sampler_mode('device', seed=77)
        sl = ops.sample_labels(lt, num, n, max_num, pos_num, mode='device', lists=lists)
        res.append(ops.anchor_target_batched(sl, num, n, anchors, gts, glab, None, None, max_num))
    a, b = res
    assert a['counts'] == b['counts'] and a['counts'][2] == 0 and a['counts'][3] == 40
    for k in ('chosen_idx', 'seg_of', 'tar_labels', 'tar_anchors', 'tar_bbox', 'tar_param'):
        assert torch.equal(a[k], b[k]), k
    ops.set_sampler_mode('numpy')


@pytest.mark.parametrize('case,pre', [('all_equal', 2000), ('four_values', 2000), ('sparse_high', 2000),
                                      ('near_half', 2000), ('near_half', 6000), ('four_values', 6000)])
def test_rpn_selection_tie_heavy_vs_oracle(dev, case, pre):
    """The per-segment top-k (seg_topk.h) on score sets that stress its radix passes: every
    score equal (bucket and prefix overflow -> restricted radix fallback, lowest indices
    win), four distinct values (tie groups of ~29k), a few high scores over a flat floor,
    and scores within 1e-3 of 0.5 (random-init RPN; quantised so that one ulp of sigmoid
    cannot reorder them).  The oracle orders by (score desc,
    index asc), as the kernel does, so boxes compare in order with no tie canonicalisation.
    pre_nms 6000 (> 4096) takes the unfused path (separate sort + decode launch)."""
    from frcnn_amd.config import wrap
    head, _ = fpn_setup(dev)
    rng = np.random.default_rng(7)
    post, mx, thr = 1000, 1000, 0.7
    cls_l, reg_l = [], []
    for i in range(2):
        cls, reg = inputs.head_outputs(900 + i, inputs.FPN_GRIDS, 3, 1, reg_scale=0.5)
        for c in cls:
            if case == 'all_equal':
                c[...] = 0.0
            elif case == 'four_values':
                c[...] = rng.choice(np.array([-1.0, 0.0, 0.5, 2.0], np.float32), size=c.shape)
            elif case == 'sparse_high':
                c[...] = -5.0
                flat = c.reshape(-1)
                flat[rng.choice(flat.size, min(flat.size, 150), replace=False)] = rng.uniform(1, 3, min(flat.size, 150))
            else:
                # 8001 logit values 1e-6 apart: scores >= 4 ulp apart, ~15-way ties at P2
                c[...] = (rng.integers(-4000, 4001, c.shape) * 1e-6).astype(np.float32)
        cls_l.append(cls)
        reg_l.append(reg)
    cls_b = [T(np.concatenate([cls_l[0][l], cls_l[1][l]], 0), dev) for l in range(5)]
    reg_b = [T(np.concatenate([reg_l[0][l], reg_l[1][l]], 0), dev) for l in range(5)]
    tcfg = wrap(dict(pre_nms=pre, post_nms=post, max_num=mx, nms_iou=thr, min_bbox_size=0.0))
    props, scores, _ = head.predict_bboxes_from_output(cls_b, reg_b, [inputs.img_meta()] * 2, tcfg)
    anchors = [oracle.anchor_grid(s, [8], [0.5, 1.0, 2.0], s, gr) for s, gr in zip(inputs.FPN_STRIDES, inputs.FPN_GRIDS)]
    for i in range(2):
        # identical scores on both sides (the device's sigmoid), so the order is comparable
        sc = [torch.sigmoid(cls_b[l][i]).reshape(-1).cpu().numpy() for l in range(5)]
        b, s = oracle.rpn_predict_single_image([c[0] for c in cls_l[i]], [r[0] for r in reg_l[i]], anchors,
                                               inputs.IMG_SHAPE, 0.0, pre, post, mx, thr, scores=sc)
        pb, ps = props[i].cpu().numpy(), scores[i].cpu().numpy()
        assert pb.shape == b.shape, (case, i, pb.shape, b.shape)
        np.testing.assert_allclose(ps, s, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(pb, b, rtol=1e-5, atol=1e-3)


# ----------------------------------------------------------------- a12
def test_bbox_target_vs_reference(dev, golden):
    from frcnn_amd import bbox as B
    from frcnn_amd.region import MaxIoUAssigner, RandomSampler
    from frcnn_amd import set_sampler_mode
    set_sampler_mode('numpy')
    g = golden('targets.npz')
    gts = inputs.voc_gts()
    for i in range(4):
        props = T(inputs.random_boxes(200 + i, 2000, min_wh=8, max_wh=300), dev)
        np.random.seed(2000 + i)
        out = B.bbox_target(props, T(gts[i][0], dev), T(gts[i][1], dev), MaxIoUAssigner(0.5, 0.5, 0.5),
                            RandomSampler(512, 128), (0.0,) * 4, (0.1, 0.1, 0.2, 0.2))
        for k, v in zip(('tar_props', 'tar_bbox', 'tar_label'), out[:3]):
            np.testing.assert_array_equal(v.cpu().numpy(), g['rcnn_{}_{}'.format(i, k)], err_msg=k)
        np.testing.assert_allclose(out[3].cpu().numpy(), g['rcnn_{}_tar_param'.format(i)], rtol=1e-5, atol=1e-5)
        np.testing.assert_array_equal(out[4].cpu().numpy(), g['rcnn_{}_tar_is_gt'.format(i)])


# ----------------------------------------------------------------- a7/a8
def test_encode_decode(dev, golden):
    from frcnn_amd import utils
    g = golden('targets.npz')
    base, box = T(inputs.random_boxes(300, 1000), dev), T(inputs.random_boxes(301, 1000), dev)
    delta = T(np.random.default_rng(302).standard_normal((4 * 21, 1000)).astype(np.float32) * 0.5, dev)
    sd = [0.1, 0.1, 0.2, 0.2]
    np.testing.assert_allclose(utils.bbox2param(base, box).cpu().numpy(), g['enc'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(utils.bbox2param(base, box, [0.0] * 4, sd).cpu().numpy(), g['enc_norm'], rtol=1e-5,
                               atol=1e-5)
    np.testing.assert_allclose(utils.param2bbox(base, delta[:4], [0.0] * 4, sd, inputs.IMG_SHAPE).cpu().numpy(),
                               g['dec'], rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(utils.batched_param2bbox(base, delta, [0.0] * 4, sd, inputs.IMG_SHAPE).cpu().numpy(),
                               g['dec_batched'], rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(utils.param2bbox(base, delta[:4]).cpu().numpy(), g['dec_noclamp'], rtol=1e-5,
                               atol=1e-3)


# ----------------------------------------------------------------- a9/a10
@pytest.mark.parametrize('tag,cfg', [('train', (2000, 2000, 2000, 0.7, 0.0)), ('test', (1000, 1000, 1000, 0.7, 0.0)),
                                     ('minsz', (1000, 300, 1000, 0.5, 16.0))])
def test_rpn_proposals_vs_reference(dev, golden, tag, cfg):
    from frcnn_amd.config import wrap
    g = golden('rpn.npz')
    pre, post, mx, thr, minb = cfg
    head, _ = fpn_setup(dev)
    tcfg = wrap(dict(pre_nms=pre, post_nms=post, max_num=mx, nms_iou=thr, min_bbox_size=minb))
    cls_l, reg_l = [], []
    for i in range(2):
        cls, reg = inputs.head_outputs(500 + i, inputs.FPN_GRIDS, 3, 1, reg_scale=0.5)
        cls_l.append(cls)
        reg_l.append(reg)
    cls_b = [T(np.concatenate([cls_l[0][l], cls_l[1][l]], 0), dev) for l in range(5)]
    reg_b = [T(np.concatenate([reg_l[0][l], reg_l[1][l]], 0), dev) for l in range(5)]
    props, scores, _ = head.predict_bboxes_from_output(cls_b, reg_b, [inputs.img_meta()] * 2, tcfg)
    for i in range(2):
        rb, rs = g['{}_{}_boxes'.format(tag, i)], g['{}_{}_scores'.format(tag, i)]
        b, s = props[i].cpu().numpy(), scores[i].cpu().numpy()
        assert b.shape == rb.shape, (b.shape, rb.shape)
        np.testing.assert_allclose(s, rs, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(canon_ties(b, s), canon_ties(rb, rs), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize('tag,cfg', [('c4train', (12000, 2000, 2000, 0.7, 16.0)), ('c4test', (6000, 300, 300, 0.7, 0.0))])
def test_rpn_proposals_c4_vs_reference(dev, golden, tag, cfg):
    """cfg1's single-level RPN (configs/faster_rcnn_r50.py:14-20,60-66): 12 anchors per cell on the
    38x64 stride-16 grid (29 184), pre_nms 12 000 -> one 12 000-box NMS -> 2 000 with min size
    16 x 1.6, against the reference's own RPNHead.predict_single_image (gen_golden.gen_rpn)."""
    from frcnn_amd.config import wrap
    from frcnn_amd.heads.rpn_head import RPNHead
    g = golden('rpn.npz')
    pre, post, mx, thr, minb = cfg
    head = RPNHead(1024, 256, anchor_scales=[4, 8, 16, 32], anchor_strides=[16],
                   loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True),
                   loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0)).to(dev)
    tcfg = wrap(dict(pre_nms=pre, post_nms=post, max_num=mx, nms_iou=thr, min_bbox_size=minb))
    outs = [inputs.head_outputs(550 + i, inputs.C4_GRIDS, 12, 1, reg_scale=0.5) for i in range(2)]
    cls_b = [T(np.concatenate([outs[0][0][0], outs[1][0][0]], 0), dev)]
    reg_b = [T(np.concatenate([outs[0][1][0], outs[1][1][0]], 0), dev)]
    props, scores, _ = head.predict_bboxes_from_output(cls_b, reg_b, [inputs.img_meta()] * 2, tcfg)
    for i in range(2):
        rb, rs = g['{}_{}_boxes'.format(tag, i)], g['{}_{}_scores'.format(tag, i)]
        b, s = props[i].cpu().numpy(), scores[i].cpu().numpy()
        assert b.shape == rb.shape, (b.shape, rb.shape)
        np.testing.assert_allclose(s, rs, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(canon_ties(b, s), canon_ties(rb, rs), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize('n,thr', [(2000, 0.7), (1000, 0.5), (5000, 0.3), (12000, 0.7), (1, 0.5), (63, 0.5),
                                   (64, 0.5), (65, 0.5)])
def test_nms_keep_bit_exact(dev, n, thr):
    from frcnn_amd import ops
    rng = np.random.default_rng(n)
    boxes = inputs.random_boxes(n, n, min_wh=5, max_wh=200).T.copy()
    boxes[::17] = boxes[::17][:, [0, 1, 2, 3]]  # duplicates
    if n > 10:
        boxes[5] = boxes[3]
    scores = rng.random(n).astype(np.float32)
    scores[::7] = scores[0]  # ties resolved by input order (stable)
    keep = ops.nms(T(boxes, dev), T(scores, dev), thr).cpu().numpy()
    np.testing.assert_array_equal(keep, oracle.nms(boxes, scores, thr))


@pytest.mark.parametrize('pattern', ['all_kept', 'chain', 'late_suppressors', 'block_edges'])
def test_nms_scan_adversarial(dev, pattern):
    """Deterministic inputs aimed at the scan's resolver / loader hand-offs (nms.hip
    'Progress' / sync protocol), n = 5000 (79 column blocks, spans wrap the 8-slot ring):
      all_kept          disjoint boxes: every block keeps 64 rows, so the loaders fold the
                        largest possible partial sums and the resolver never idles;
      chain             box i overlaps i+1 only (IoU 0.6 > 0.5): keeps alternate, every
                        decision depends on the previous one, across every block edge;
      late_suppressors  rows of block b suppressed only by kept rows of block b-1 / b-2
                        (the tiles the resolver ORs itself, not the loaders' fold);
      block_edges       rows 63 / 64 of each block pair overlap (cross-block chains).
    Keep lists must equal the oracle's exactly, on each of 3 launches."""
    from frcnn_amd import ops
    n = 5000
    i = np.arange(n, dtype=np.float64)
    if pattern == 'all_kept':
        x = (i % 100) * 30.0
        y = (i // 100) * 30.0
        boxes = np.stack([x, y, x + 20, y + 20], 1)
    elif pattern == 'chain':
        x = i * 2.5  # width 10, shift 2.5: IoU(i, i+1) = 0.6 > 0.5, IoU(i, i+2) = 1/3
        boxes = np.stack([x, np.zeros(n), x + 10.0, np.full(n, 10.0)], 1)
    elif pattern == 'late_suppressors':
        blk, r = i // 64, i % 64
        x = r * 40.0 + (blk % 2) * 5.0  # row r of block b sits near row r of block b-1 (shift 5 / width 30)
        y = (blk // 2) * 40.0
        boxes = np.stack([x, y, x + 30.0, y + 30.0], 1)
    else:
        blk, r = i // 64, i % 64
        x = blk * 50.0 + np.where(r == 63, 30.0, np.where(r == 0, 33.0, r * 0.0 - 1000.0 - r * 40.0))
        boxes = np.stack([x, np.zeros(n), x + 20.0, np.full(n, 20.0)], 1)
    boxes = boxes.astype(np.float32)
    scores = (1.0 - i / n).astype(np.float32)  # already in index order
    want = oracle.nms(boxes, scores, 0.5)
    assert 0 < len(want) <= n
    for _ in range(3):
        keep = ops.nms(T(boxes, dev), T(scores, dev), 0.5).cpu().numpy()
        np.testing.assert_array_equal(keep, want)


@pytest.mark.parametrize('thr', [0.7, 0.5])
def test_nms_degenerate_boxes(dev, thr):
    """RPN-like degenerate boxes, the case the mask kernel's float filter decides without
    the exact test: zero-width / zero-height boxes clamped to the image edge (union 0 with
    each other), negative-area boxes (union < 0), 1e-30-sized boxes (union in (0, 2^-100],
    the exact path), duplicates of each, negative coordinates (the float min / max path)
    mixed with ordinary boxes.  Keep lists must equal the oracle's."""
    from frcnn_amd import ops
    rng = np.random.default_rng(7)
    n = 3000
    b = inputs.random_boxes(11, n, min_wh=1, max_wh=300).T.copy()
    k = rng.integers(0, 6, n)
    edge_y = rng.choice([0.0, 599.0], n).astype(np.float32)
    b[k == 1, 1] = edge_y[k == 1]
    b[k == 1, 3] = edge_y[k == 1]          # zero height on the top / bottom edge
    b[k == 2, 0] = 999.0
    b[k == 2, 2] = 999.0                   # zero width on the right edge
    b[k == 3, 2] = b[k == 3, 0] - 5.0      # negative width
    t = np.float32(1e-30)
    b[k == 4, 2] = b[k == 4, 0] + t
    b[k == 4, 3] = b[k == 4, 1] + t        # tiny boxes
    b[k == 5] -= np.float32(400.0)         # negative coordinates
    b[1::9] = b[0::9][:len(b[1::9])]       # duplicates
    scores = rng.random(n).astype(np.float32)
    keep = ops.nms(T(b, dev), T(scores, dev), thr).cpu().numpy()
    np.testing.assert_array_equal(keep, oracle.nms(b, scores, thr))


@pytest.mark.parametrize('thr', [0.7, 0.5, 0.3])
def test_nms_threshold_boundary(dev, thr):
    """Pairs of boxes whose IoU straddles the threshold by a few float ulps: the kernel's
    division-free test (inter > mid * union in double) must decide exactly like the
    reference's float division followed by the double comparison."""
    from frcnn_amd import ops
    rng = np.random.default_rng(int(thr * 100))
    n = 1024
    w = np.float32(100.0)
    # IoU of [0, 0, w, w] and its x-shift by d: (w - d) / (w + d); the crossing at d* = w (1 - thr) / (1 + thr)
    dstar = float(w) * (1 - thr) / (1 + thr)
    d = (dstar + rng.integers(-40, 41, n // 2) * dstar * 2e-7).astype(np.float32)
    base = (np.arange(n // 2) * 1000.0).astype(np.float32)  # pairs far apart: no cross-pair overlap
    a = np.stack([base, np.zeros_like(base), base + w, np.full_like(base, w)], 1)
    b = np.stack([base + d, np.zeros_like(base), base + d + w, np.full_like(base, w)], 1)
    boxes = np.ascontiguousarray(np.stack([a, b], 1).reshape(n, 4))
    scores = np.tile(np.array([0.9, 0.8], np.float32), n // 2)
    keep = ops.nms(T(boxes, dev), T(scores, dev), thr).cpu().numpy()
    ref = oracle.nms(boxes, scores, thr)
    np.testing.assert_array_equal(keep, ref)
    assert 0 < len(ref) - n // 2 < n // 2  # both outcomes occur


def test_nms_empty_and_batched(dev):
    from frcnn_amd import ops, utils
    e = ops.nms(torch.zeros(0, 4, device=dev), torch.zeros(0, device=dev), 0.5)
    assert e.numel() == 0
    boxes = inputs.random_boxes(3, 3000, min_wh=5, max_wh=100).T.copy()
    scores = np.random.default_rng(4).random(3000).astype(np.float32)
    labels = np.random.default_rng(5).integers(1, 21, 3000)
    kb, ks, kl = utils.batched_nms(T(boxes, dev), T(scores, dev), T(labels, dev), 0.5)
    off = boxes + (labels.astype(np.float32) * np.float32(boxes.max()))[:, None]
    k = oracle.nms(off, scores, 0.5)
    np.testing.assert_array_equal(kl.cpu().numpy(), labels[k])
    np.testing.assert_array_equal(ks.cpu().numpy(), scores[k])


@pytest.mark.parametrize('n', [100000, 184320])
def test_nms_large_segment_structured(dev, n):
    """Segments past 65 536 boxes (up to the 184 320 limit): kept sets beyond 1024 words and the
    loaders' global-memory fold of tiles older than the staged span.  Structured input with a
    known answer (an O(n^2) oracle run is too slow at this size): disjoint 10 x 10 cells, each
    with a twin shifted by one pixel (IoU 90/110 = 0.818 > 0.7), rows in a random score order;
    the keep list is every box whose twin comes later.  One past the limit is refused."""
    from frcnn_amd import ops
    pairs = n // 2
    gx = 512
    cell = np.arange(pairs)
    x = (cell % gx).astype(np.float32) * 20.0
    y = (cell // gx).astype(np.float32) * 20.0
    base = np.stack([x, y, x + 10.0, y + 10.0], 1)
    twin = base + np.array([1.0, 0.0, 1.0, 0.0], np.float32)
    boxes = np.concatenate([base, twin]).astype(np.float32)
    order = np.random.default_rng(n).permutation(n)
    rows = boxes[order][None]
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)  # row position of box i
    partner = np.concatenate([np.arange(pairs) + pairs, np.arange(pairs)])
    want = np.sort(pos[np.arange(n)[pos < pos[partner]]])
    keep, kc = ops.nms_sorted(T(rows, dev), T(np.array([n], np.int32), dev), n, 0.7)
    k = int(kc.cpu()[0])
    assert k == pairs
    np.testing.assert_array_equal(keep[0, :k].cpu().numpy(), want)
    if n == 184320:
        with pytest.raises(RuntimeError, match='exceeds'):
            ops.nms_sorted(T(np.zeros((1, n + 64, 4), np.float32), dev), T(np.array([n + 64], np.int32), dev),
                           n + 64, 0.7)


@pytest.mark.parametrize('S,max_keep', [(12, -1), (12, 1), (12, 37), (12, 500), (150, 20)])
def test_nms_sorted_segments_max_keep(dev, S, max_keep):
    """frh_nms_sorted over S pre-sorted segments of ragged counts (0, 1, 63, 64, 65, ...,
    2500) in one call, with the RPN's max_keep stop (the scan's early exit and its loaders'
    stop protocol).  Each segment's keep list equals the oracle's greedy NMS cut at
    max_keep."""
    from frcnn_amd import ops
    rng = np.random.default_rng(S * 1000 + max_keep)
    base = [0, 1, 63, 64, 65, 300, 1000, 2000, 2500, 129, 7, 1999]
    counts = np.array([base[i % len(base)] for i in range(S)], np.int32)
    n_max = int(counts.max())
    rows = np.zeros((S, n_max, 4), np.float32)
    for i in range(S):
        if counts[i]:
            rows[i, :counts[i]] = inputs.random_boxes(i + 1, int(counts[i]), min_wh=5, max_wh=150).T
    keep, kc = ops.nms_sorted(T(rows, dev), T(counts, dev), n_max, 0.6, max_keep)
    keep, kc = keep.cpu().numpy(), kc.cpu().numpy()
    for i in range(S):
        n = int(counts[i])
        want = oracle.nms(rows[i, :n], np.linspace(1.0, 0.0, max(n, 1), dtype=np.float32)[:n], 0.6, max_keep) \
            if n else np.zeros(0, np.int64)
        assert kc[i] == len(want), (i, n, kc[i], len(want))
        np.testing.assert_array_equal(keep[i, :kc[i]], want)


@pytest.mark.parametrize('n', [16385, 20000])
def test_nms_above_16384_boxes(dev, n):
    """torchvision.ops.nms takes any n; the reference's offset-trick batched_nms
    (lib/utils.py:211-221) runs one NMS over up to 1000 proposals x 20 classes = 20 000
    boxes at RCNN test.  Keep list bit-exact vs the oracle, through ops.nms and through
    utils.batched_nms on 20 class labels."""
    from frcnn_amd import ops, utils
    rng = np.random.default_rng(n)
    boxes = inputs.random_boxes(n, n, min_wh=5, max_wh=120).T.copy()
    scores = rng.random(n).astype(np.float32)
    scores[::11] = scores[1]
    keep = ops.nms(T(boxes, dev), T(scores, dev), 0.5).cpu().numpy()
    np.testing.assert_array_equal(keep, oracle.nms(boxes, scores, 0.5))
    labels = rng.integers(1, 21, n)
    kb, ks, kl = utils.batched_nms(T(boxes, dev), T(scores, dev), T(labels, dev), 0.5)
    off = boxes + (labels.astype(np.float32) * np.float32(boxes.max()))[:, None]
    k = oracle.nms(off, scores, 0.5)
    np.testing.assert_array_equal(kl.cpu().numpy(), labels[k])
    np.testing.assert_array_equal(ks.cpu().numpy(), scores[k])


# ----------------------------------------------------------------- a13/a14
def test_roi_level_map(dev, golden):
    from frcnn_amd import ops
    g = golden('levels.npz')
    r = g['rois']
    r5 = np.concatenate([np.zeros((1, r.shape[1]), np.float32), r], 0).T.copy()
    np.testing.assert_array_equal(ops.roi_level_map(T(r5, dev), 56, 4).cpu().numpy(), g['levels'])


def test_roi_rows_flat_and_batched(dev, golden):
    """frh_roi_rows: the (image, box) rows and levels of three images' boxes from a flat
    [4, sum n] buffer and from a padded [B, 4, cap] buffer (including an empty image) equal
    the reference's per-image index column + concatenation, and the level fixture."""
    from frcnn_amd import ops
    g = golden('levels.npz')
    r = g['rois']
    n = r.shape[1]
    counts = [n // 3, 0, n - n // 3]
    bidx = np.repeat(np.arange(3, dtype=np.float32), counts)
    want = np.concatenate([bidx[None], r], 0).T
    rois, lv = ops.roi_rows(T(r, dev), counts, 56, 4)
    np.testing.assert_array_equal(rois.cpu().numpy(), want)
    np.testing.assert_array_equal(lv.cpu().numpy(), g['levels'])
    cap = max(counts) + 5
    buf = torch.full((3, 4, cap), 7.0, device=dev)
    off = 0
    for b, c in enumerate(counts):
        buf[b, :, :c] = T(r[:, off:off + c], dev)
        off += c
    rois2, lv2 = ops.roi_rows(buf, counts, 56, 4, seg_stride=buf.stride(0), flat=False)
    np.testing.assert_array_equal(rois2.cpu().numpy(), want)
    np.testing.assert_array_equal(lv2.cpu().numpy(), g['levels'])
    rois1, lv1 = ops.roi_rows(T(r, dev), [n], 56, 1)
    assert lv1 is None and np.array_equal(rois1.cpu().numpy()[:, 1:], r.T)


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
def test_roi_align_forward_default_vs_oracle_p2(dev, layout):
    """The product forward on P2-sized maps, 600 RoIs incl. border / degenerate / outside ones,
    against the oracle: bit-identical.  C = 96: NCHW runs the channel-pair kernel, channels-last the
    band kernel (96 % 64 != 0) on all three of its paths (107 windows of <= 192 cells: quad stages,
    383 of <= 480: interleaved stages, 109 larger: row bands; 1 without a valid sample)."""
    from frcnn_amd import ops
    grids = [(152, 256), (76, 128), (38, 64), (19, 32)]
    feats = inputs.feature_maps(42, grids, 96, 2)
    rois = support.rois(43, 600, 2)
    levels = oracle.roi_level_map(rois, 56.0, 4)
    scales = [1 / 4, 1 / 8, 1 / 16, 1 / 32]
    ref = oracle.roi_align(feats, rois, levels, scales, (7, 7), 2)
    ft = [T(f, dev) for f in feats]
    if layout == 'nhwc':
        ft = [f.contiguous(memory_format=torch.channels_last) for f in ft]
    out = ops.roi_align_multilevel(ft, T(rois, dev), T(levels, dev), scales, (7, 7), 2).cpu().numpy()
    np.testing.assert_array_equal(out, ref)  # same operation order as the oracle: bit-identical
    odd = [T(f[:, :95], dev).contiguous() for f in feats]  # odd C: the per-RoI LDS kernel
    out2 = ops.roi_align_multilevel(odd, T(rois, dev), T(levels, dev), scales, (7, 7), 2).cpu().numpy()
    np.testing.assert_array_equal(out2, out[:, :95])


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('roi_set', ['cfg2_rois.npz', 'cfg2_rois_voc.npz', 'cfg2_rois_train.npz'])
def test_roi_align_forward_bench_config_bit_exact(dev, layout, roi_set):
    """The forward at the bench's own configuration, C = 256, P2-P5 of a 2-image 608x1024
    batch (152x256 ... 19x32), NCHW (channel-pair kernel) and channels-last (the FPN's NHWC
    levels: channel-group kernel), on three RoI sets: the 1024 RoIs of a random-init cfg2
    step (cfg2_rois.npz, 873 / 102 / 42 / 7 on P2..P5: tiny), VOC-sized RoIs in the RCNN
    sampler's mix around the bench images' gts (cfg2_rois_voc.npz, gen_voc_rois.py: 235 /
    369 / 219 / 201, tap grids up to 27 x 29 cells) and the RoIs of a `bench.py --mode
    train` step (cfg2_rois_train.npz, when dumped): every output bit-identical to the oracle
    (lib/region.py:271-296, torchvision legacy RoIAlign semantics)."""
    from frcnn_amd import ops
    if not os.path.exists(inputs.golden_path(roi_set)):
        pytest.skip('{} not generated'.format(roi_set))
    z = np.load(inputs.golden_path(roi_set))
    rois, levels = z['r5'], z['lv']
    shapes = [tuple(int(v) for v in s) for s in z['shapes']]
    scales = [float(v) for v in z['scales']]
    feats = inputs.feature_maps(44, [s[2:] for s in shapes], shapes[0][1], shapes[0][0])
    ref = oracle.roi_align(feats, rois, levels, scales, (7, 7), 2)
    ft = [T(f, dev) for f in feats]
    if layout == 'nhwc':
        ft = [f.contiguous(memory_format=torch.channels_last) for f in ft]
    out = ops.roi_align_multilevel(ft, T(rois, dev), T(levels, dev), scales, (7, 7), 2).cpu().numpy()
    np.testing.assert_array_equal(out, ref)


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('sampling', [2, 0])
def test_roi_align_multilevel_vs_oracle(dev, layout, sampling):
    from frcnn_amd import ops
    grids = [(76, 128), (38, 64), (19, 32), (10, 16)]
    feats = inputs.feature_maps(40, grids, 64, 2)
    rois = support.rois(41, 300, 2)
    levels = oracle.roi_level_map(rois, 56.0, 4)
    scales = [1 / 8, 1 / 16, 1 / 32, 1 / 64]
    ref = oracle.roi_align(feats, rois, levels, scales, (7, 7), sampling)
    ft = [T(f, dev) for f in feats]
    if layout == 'nhwc':
        ft = [f.contiguous(memory_format=torch.channels_last) for f in ft]
    out = ops.roi_align_multilevel(ft, T(rois, dev), T(levels, dev), scales, (7, 7), sampling).cpu().numpy()
    np.testing.assert_array_equal(out, ref)  # every forward kernel keeps the oracle's operation order


@pytest.mark.parametrize('pooled,C', [((7, 7), 64), ((7, 7), 192), ((4, 5), 128), ((8, 8), 64), ((1, 1), 64)])
def test_roi_align_channel_group_kernel_vs_oracle(dev, pooled, C):
    """The channel-group forward (roi_align_fwd_cg_kernel: channels-last levels with C % 64 == 0,
    one 4-wave workgroup per (RoI, 64 channels), 120-cell slab, bands of bin rows, list-row bands
    for bin rows spanning more rows than the slab holds) against the oracle, bit-identical: random
    RoIs over four levels (windows from 1 cell to 28 x 28, single- and multi-band), pathological
    RoIs on a 10 x 30 level, pooled sizes 1x1 .. 7x7.  8x8 bins reach none of the staged kernels:
    16 * 8 tap-list columns exceed the 120-cell slab (cg_ok) and quad_max_cells(8, 8) = 1056 cells
    the 832 of the quad and pair slabs (quad_ok, pair_ok), so that case runs the per-RoI LDS-window
    kernel (roi_align_fwd_lds_kernel) on channels-last features."""
    from frcnn_amd import ops
    grids = [(76, 128), (38, 64), (19, 32), (10, 30)]
    feats = inputs.feature_maps(60, grids, C, 2)
    rois = np.concatenate([support.rois(61, 300, 2), support.pathological_rois(2)], 0)
    levels = oracle.roi_level_map(rois, 56.0, 4)
    levels[-11:] = 3  # the pathological RoIs on the 10 x 30 level
    scales = [1 / 8, 1 / 16, 1 / 32, 1 / 4]
    ref = oracle.roi_align(feats, rois, levels, scales, pooled, 2)
    ft = [T(f, dev).contiguous(memory_format=torch.channels_last) for f in feats]
    out = ops.roi_align_multilevel(ft, T(rois, dev), T(levels, dev), scales, pooled, 2).cpu().numpy()
    np.testing.assert_array_equal(out, ref)


@pytest.mark.parametrize('C', [16, 40])
def test_roi_align_standalone_quad_kernel_vs_oracle(dev, C):
    """The standalone channel-quad forward (roi_align_fwd_quad_kernel): channels-last levels whose
    shape neither the channel-group kernel (C % 64 != 0) nor the band kernel takes -- 4 x 12 bins:
    quad_max_cells(4, 12) = 16 * 49 = 784 <= 832 (quad_ok), but a band of 5 rows of the 49-column
    window needs 245 > 240 cells (band_fits).  Against the oracle, bit-identical: random, border and
    degenerate RoIs on a 19 x 32 level, pathological ones on a 10 x 30 level, and three wide RoIs, so
    that windows of every stage depth occur (<= 192 cells: 4 quads per stage, <= 384: 2, above: 1);
    C = 40 adds a second and a partial third 16-channel chunk."""
    from frcnn_amd import ops
    grids = [(19, 32), (10, 30)]
    feats = inputs.feature_maps(70, grids, C, 2)
    wide = np.array([[1, 0, 0, 119, 39], [0, 2, 1, 110, 38], [1, 30, 20, 1000, 500]], np.float32)
    rois = np.concatenate([support.rois(71, 40, 2), wide[2:], support.pathological_rois(2), wide[:2]], 0)
    levels = np.zeros(len(rois), np.int64)
    levels[-13:] = 1  # the pathological and the first two wide RoIs on the 10 x 30 level
    scales = [1 / 32, 1 / 4]
    ref = oracle.roi_align(feats, rois, levels, scales, (4, 12), 2)
    ft = [T(f, dev).contiguous(memory_format=torch.channels_last) for f in feats]
    out = ops.roi_align_multilevel(ft, T(rois, dev), T(levels, dev), scales, (4, 12), 2).cpu().numpy()
    np.testing.assert_array_equal(out, ref)


def test_roi_align_module_and_strided_view(dev):
    from frcnn_amd.ops import RoIAlign
    f = inputs.feature_maps(50, [(40, 60)], 32, 2)[0]
    ft = T(f, dev)[:, :, ::2, ::2]  # non-contiguous (FPN P6 style)
    rois = support.rois(51, 200, 2)
    out = RoIAlign((7, 7), 0.25, 2)(ft, T(rois, dev)).cpu().numpy()
    ref = oracle.roi_align([np.ascontiguousarray(f[:, :, ::2, ::2])], rois, None, [0.25], (7, 7), 2)
    np.testing.assert_array_equal(out, ref)


@pytest.mark.parametrize('case', ['small', 'small_nhwc', 'p2', 'p2_nhwc', 'adaptive', 'bins9x7'])
def test_roi_align_backward_vs_oracle(dev, case):
    """Backward against the oracle: the separable row-run kernel (sampling 2, up to 8x8
    bins, NCHW gradients), its lane = channel form for channels_last gradients
    (roi_align_bwd_nhwc_kernel: 16 channels, and 80 = one full and one partial 64-channel
    group), the LDS-window kernel (9x7 bins) and per-tap atomics (adaptive sampling).  Float
    atomics reorder the sums, so the tolerance is f32-accumulation level."""
    from frcnn_amd import ops
    if case in ('small', 'small_nhwc', 'adaptive'):
        grids, scales, C, K, L = [(38, 64), (19, 32)], [1 / 16, 1 / 32], 16, 120, 2
    else:
        grids, scales, C, K, L = [(152, 256), (76, 128)], [1 / 4, 1 / 8], 80, 300, 2
    sr = 0 if case == 'adaptive' else 2
    ph, pw = (9, 7) if case == 'bins9x7' else (7, 7)
    feats = inputs.feature_maps(60, grids, C, 2)
    rois = support.rois(61, K, 2)
    levels = oracle.roi_level_map(rois, 56.0, L)
    g = np.random.default_rng(62).standard_normal((K, C, ph, pw)).astype(np.float32)
    ft = [T(f, dev) for f in feats]
    if case.endswith('_nhwc'):
        ft = [f.contiguous(memory_format=torch.channels_last) for f in ft]
    ft = [f.requires_grad_(True) for f in ft]
    out = ops.roi_align_multilevel(ft, T(rois, dev), T(levels, dev), scales, (ph, pw), sr)
    out.backward(T(g, dev))
    if case.endswith('_nhwc'):
        assert all(f.grad.stride(1) == 1 for f in ft)  # the gradient keeps the features' format
    ref = oracle.roi_align_bwd([f.shape for f in feats], rois, levels, scales, g, sr)
    for a, r in zip(ft, ref):
        np.testing.assert_allclose(a.grad.cpu().numpy(), r, rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize('case,gscale', [('p2', 1.0), ('p2_nhwc', 1.0), ('voc_nhwc', 1.0), ('p2', 1e-8),
                                         ('voc_nhwc', 1e-8), ('p2_nhwc', 3e4)])
def test_roi_align_backward_deterministic(dev, case, gscale):
    """The deterministic backward (frh_roi_align_bwd_fixed: fixed-point integer atomics,
    SURVEY §5): within f32-accumulation tolerance of the oracle, bit-identical across runs AND
    under any permutation of the RoIs (the sum over RoIs is order-independent), where the
    float-atomic form is not (reference: autograd of lib/region.py:276).  The fixed-point unit
    follows the gradient's own magnitude (ABI 3): training-sized gradients (grad_out ~1e-8) keep
    the same RELATIVE tolerance as unit-scale ones (a fixed 2^-40 unit would floor them at
    ~1e-12 absolute), and large ones (3e4) do not overflow."""
    from frcnn_amd import ops
    if case == 'voc_nhwc':
        z = np.load(inputs.golden_path('cfg2_rois_voc.npz'))
        rois, levels = z['r5'][::4].copy(), z['lv'][::4].copy()
        grids, scales, C = [tuple(int(v) for v in s[2:]) for s in z['shapes']], [float(v) for v in z['scales']], 64
    else:
        grids, scales, C = [(152, 256), (76, 128)], [1 / 4, 1 / 8], 80
        rois = support.rois(61, 300, 2)
        levels = oracle.roi_level_map(rois, 56.0, 2)
    K = rois.shape[0]
    feats = inputs.feature_maps(60, grids, C, 2)
    g = (np.random.default_rng(62).standard_normal((K, C, 7, 7)) * gscale).astype(np.float32)
    ref = oracle.roi_align_bwd([f.shape for f in feats], rois, levels, scales, g, 2)

    def run(order):
        ft = [T(f, dev) for f in feats]
        if case.endswith('nhwc'):
            ft = [f.contiguous(memory_format=torch.channels_last) for f in ft]
        ft = [f.requires_grad_(True) for f in ft]
        out = ops.roi_align_multilevel(ft, T(rois[order], dev), T(levels[order], dev), scales, (7, 7), 2)
        out.backward(T(g[order], dev))
        return [f.grad.clone() for f in ft]
    ops.set_deterministic_backward(True)
    try:
        a = run(np.arange(K))
        b = run(np.arange(K))
        c = run(np.random.default_rng(63).permutation(K))
    finally:
        ops.set_deterministic_backward(False)
    for x, y, z_, r in zip(a, b, c, ref):
        assert torch.equal(x, y) and torch.equal(x, z_)
        np.testing.assert_allclose(x.cpu().numpy(), r, rtol=1e-4, atol=2e-5 * gscale)


def test_roi_align_backward_deterministic_nonfinite_and_unsupported(dev):
    """A NaN in grad_out makes every element of the deterministic gradient NaN (no undefined
    float -> int64 conversion); a shape the fixed-point form does not cover raises under
    set_deterministic_backward instead of silently running the float atomics."""
    from frcnn_amd import ops
    grids, scales, C = [(38, 64)], [1 / 16], 16
    feats = inputs.feature_maps(64, grids, C, 2)
    rois = support.rois(65, 40, 2)
    g = np.random.default_rng(66).standard_normal((40, C, 7, 7)).astype(np.float32)
    g[3, 2, 1, 1] = np.nan
    ops.set_deterministic_backward(True)
    try:
        ft = [T(f, dev).requires_grad_(True) for f in feats]
        ops.roi_align_multilevel(ft, T(rois, dev), None, scales, (7, 7), 2).backward(T(g, dev))
        assert torch.isnan(ft[0].grad).all()
        ft = [T(f, dev).requires_grad_(True) for f in feats]
        out = ops.roi_align_multilevel(ft, T(rois, dev), None, scales, (7, 7), 0)  # adaptive sampling
        with pytest.raises(RuntimeError, match='no deterministic form'):
            out.backward(T(np.nan_to_num(g), dev))
    finally:
        ops.set_deterministic_backward(False)


def test_roi_pool_vs_oracle(dev):
    from frcnn_amd.ops import RoIPool
    f = inputs.feature_maps(70, [(38, 64)], 32, 2)[0]
    rois = support.rois(71, 150, 2)
    out = RoIPool((7, 7), 1 / 16, sampling_ratio=2)(T(f, dev), T(rois, dev)).cpu().numpy()
    ref, _ = oracle.roi_pool(f, rois, (7, 7), 1 / 16)
    np.testing.assert_array_equal(out, ref)


def test_basic_roi_extractor_matches_reference_flow(dev):
    """Level mapping + per-level RoIAlign + scatter back (region.py:280-296) in one launch."""
    from frcnn_amd.region import BasicRoIExtractor
    ex = BasicRoIExtractor([dict(type='RoIAlign', spatial_scale=1 / s, sampling_ratio=2) for s in (4, 8, 16, 32)],
                           output_size=(7, 7))
    grids = [(152, 256), (76, 128), (38, 64), (19, 32)]
    feats = inputs.feature_maps(80, grids, 32, 2)
    props = [inputs.random_boxes(81, 300, min_wh=4, max_wh=599), inputs.random_boxes(82, 200, min_wh=4, max_wh=599)]
    outs = ex([T(f, dev) for f in feats], [T(p, dev) for p in props])
    for b, p in enumerate(props):
        r5 = np.concatenate([np.full((1, p.shape[1]), b, np.float32), p], 0).T.copy()
        lv = oracle.roi_level_map(r5, 56.0, 4)
        ref = oracle.roi_align(feats, r5, lv, [1 / 4, 1 / 8, 1 / 16, 1 / 32], (7, 7), 2)
        np.testing.assert_array_equal(outs[b].cpu().numpy(), ref)


# ----------------------------------------------------------------- end to end (cfg2 shapes)
def test_faster_rcnn_fpn_forward_train_runs(dev):
    import bench
    from frcnn_amd import set_sampler_mode
    set_sampler_mode('numpy')
    model, batch = bench.make_model_and_batch(dev, batch=2, seed=0)
    losses = model.forward_train(*batch)
    assert set(losses) == {'rpn_cls_loss', 'rpn_reg_loss', 'rcnn_0_cls_loss', 'rcnn_0_reg_loss'}
    for k, v in losses.items():
        assert torch.isfinite(v).all(), k
    sum(losses.values()).backward()


# ----------------------------------------------------------------- a16 ATSS / LTRB
def _atss_anchor_flat(dev):
    from frcnn_amd import ops
    from frcnn_amd.anchor import AnchorCreator
    parts = []
    for s, g in zip(inputs.RETINA_STRIDES, inputs.RETINA_GRIDS):
        c = AnchorCreator(base=s, scales=[8], aspect_ratios=[1.0])
        parts.append(ops.anchor_grid([g], [float(s)], c.ws, c.hs, 1, False, dev))
    return torch.cat(parts, 1).contiguous()


def test_atss_assign_batched_vs_oracle(dev):
    """All ATSS cases as ONE batch (ragged gt counts 1..40): labels, ltrb and centerness
    bit-exact against the oracle (both use correctly rounded f32 sqrt/div)."""
    from frcnn_amd import ops
    cases = inputs.atss_cases()
    anchors = _atss_anchor_flat(dev)
    o_anchors = [oracle.anchor_grid(s, [8], [1.0], s, g).reshape(4, -1)
                 for s, g in zip(inputs.RETINA_STRIDES, inputs.RETINA_GRIDS)]
    assert np.array_equal(anchors.cpu().numpy(), np.concatenate(o_anchors, 1))
    cls, reg, ctr = ops.atss_assign(anchors, inputs.RETINA_GRIDS, [float(s) for s in inputs.RETINA_STRIDES],
                                    [T(b, dev) for b, _ in cases], [T(l, dev) for _, l in cases],
                                    [inputs.IMG_SHAPE] * len(cases), 9)
    cls, reg, ctr = cls.cpu().numpy(), reg.cpu().numpy(), ctr.cpu().numpy()
    for i, (b, l) in enumerate(cases):
        c, r, t = oracle.atss_targets(o_anchors, inputs.RETINA_GRIDS, inputs.RETINA_STRIDES, b, l, inputs.IMG_SHAPE)
        assert np.array_equal(cls[i], c), (i, np.nonzero(cls[i] != c)[0][:10])
        assert np.array_equal(reg[i], r), i
        assert np.array_equal(ctr[i], t), i


def test_atss_head_single_image_and_edges(dev):
    """FCOSHead.single_image_targets_atss (reference signature, per-level [H, W, k] outputs),
    an image with no gts, and a smaller img_shape (paint region)."""
    from frcnn_amd import ops
    from frcnn_amd.heads.fcos_head import FCOSHead
    head = FCOSHead(num_classes=21, in_channels=8, stacked_convs=1, feat_channels=8,
                    strides=inputs.RETINA_STRIDES, reg_std=1200, atss_cfg=dict(topk=9, scale=8),
                    loss_cls=dict(type='FocalLoss', use_sigmoid=True, loss_weight=1.0),
                    loss_bbox=dict(type='GIoULoss', loss_weight=2.0),
                    loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)).to(dev)
    b, l = inputs.atss_cases()[0]
    outs = [torch.zeros(20, h, w, device=dev) for h, w in inputs.RETINA_GRIDS]
    cls_t, reg_t, ctr_t = head.single_image_targets_atss(outs, outs, outs, [None] * 5, T(b, dev), T(l, dev),
                                                        {'img_shape': (600, 1000, 3)}, None)
    o_anchors = [oracle.anchor_grid(s, [8], [1.0], s, g).reshape(4, -1)
                 for s, g in zip(inputs.RETINA_STRIDES, inputs.RETINA_GRIDS)]
    c, r, t = oracle.atss_targets(o_anchors, inputs.RETINA_GRIDS, inputs.RETINA_STRIDES, b, l, inputs.IMG_SHAPE)
    assert [tuple(x.shape) for x in cls_t] == [(h, w, 1) for h, w in inputs.RETINA_GRIDS]
    assert np.array_equal(torch.cat([x.reshape(-1) for x in cls_t]).cpu().numpy(), c)
    assert np.array_equal(torch.cat([x.reshape(-1, 4) for x in reg_t]).cpu().numpy(), r)
    assert np.array_equal(torch.cat([x.reshape(-1) for x in ctr_t]).cpu().numpy(), t)
    # no gts + a small image: only painting
    anchors = _atss_anchor_flat(dev)
    empty = torch.zeros(4, 0, device=dev)
    cls, reg, ctr = ops.atss_assign(anchors, inputs.RETINA_GRIDS, [float(s) for s in inputs.RETINA_STRIDES],
                                    [empty, T(b, dev)], [torch.zeros(0, dtype=torch.int64, device=dev), T(l, dev)],
                                    [(300, 500), (300, 500)], 9)
    c0, _, _ = oracle.atss_targets(o_anchors, inputs.RETINA_GRIDS, inputs.RETINA_STRIDES, np.zeros((4, 0), np.float32),
                                   np.zeros(0, np.int64), (300, 500))
    c1, r1, t1 = oracle.atss_targets(o_anchors, inputs.RETINA_GRIDS, inputs.RETINA_STRIDES, b, l, (300, 500))
    assert np.array_equal(cls[0].cpu().numpy(), c0) and (c0 > 0).sum() == 0 and (c0 == -1).sum() > 0
    assert np.array_equal(cls[1].cpu().numpy(), c1)
    assert np.array_equal(reg[1].cpu().numpy(), r1) and np.array_equal(ctr[1].cpu().numpy(), t1)


def test_fcos_atss_forward_train_loss(dev):
    """cfg5 head forward+loss through the HIP targets equals the same losses computed from the
    oracle's targets (reference calc_loss, fcos_head.py:418-534)."""
    from frcnn_amd.heads.fcos_head import FCOSHead
    torch.manual_seed(0)
    head = FCOSHead(num_classes=21, in_channels=16, stacked_convs=1, feat_channels=16,
                    strides=inputs.RETINA_STRIDES, reg_std=1200, atss_cfg=dict(topk=9, scale=8),
                    loss_cls=dict(type='FocalLoss', use_sigmoid=True, loss_weight=1.0),
                    loss_bbox=dict(type='GIoULoss', loss_weight=2.0),
                    loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)).to(dev)
    head.init_weights()
    feats = [torch.randn(2, 16, h, w, device=dev) for h, w in inputs.RETINA_GRIDS]
    cases = inputs.atss_cases()[:2]
    metas = [inputs.img_meta(), inputs.img_meta()]
    losses = head.forward_train(feats, [T(b, dev) for b, _ in cases], [T(l, dev) for _, l in cases], metas, None)
    assert set(losses) == {'cls_loss', 'ctr_loss', 'bbox_loss'}
    o_anchors = [oracle.anchor_grid(s, [8], [1.0], s, g).reshape(4, -1)
                 for s, g in zip(inputs.RETINA_STRIDES, inputs.RETINA_GRIDS)]
    tars = [oracle.atss_targets(o_anchors, inputs.RETINA_GRIDS, inputs.RETINA_STRIDES, b, l, inputs.IMG_SHAPE)
            for b, l in cases]
    with torch.no_grad():
        co, ro, to = head.forward(feats)
    flat = lambda xs: torch.cat([x.reshape(2, x.shape[1], -1) for x in xs], -1).permute(1, 0, 2).reshape(
        xs[0].shape[1], -1)
    ref = head.calc_loss_flat(flat(co), flat(ro), flat(to), T(np.concatenate([t[0] for t in tars]), dev),
                              T(np.concatenate([t[1] for t in tars]), dev), T(np.concatenate([t[2] for t in tars]), dev))
    for k in losses:
        assert torch.isfinite(losses[k]).all()
        torch.testing.assert_close(losses[k].detach(), ref[k], rtol=1e-6, atol=0)
    sum(losses.values()).backward()
    assert head.fcos_cls.weight.grad is not None


# ----------------------------------------------------------------- a11 multiclass NMS
@pytest.mark.parametrize('i', range(len(inputs.MCNMS_CASES)))
def test_multiclass_nms_vs_reference(dev, golden, i):
    """utils.multiclass_nms on the HIP NMS (official / strict, class-specific boxes, score
    factor) against the reference's outputs: bit-exact."""
    from frcnn_amd import utils
    g = golden('mcnms.npz')
    bbox, score, sf, channels = inputs.mcnms_inputs(i)
    mode = inputs.MCNMS_CASES[i][0]
    kb, ks, kl = utils.multiclass_nms(T(bbox, dev), T(score, dev), channels, 0.5, 0.05, 100,
                                      T(sf, dev) if sf is not None else None, mode=mode)
    np.testing.assert_array_equal(kb.cpu().numpy(), g['boxes_{}'.format(i)])
    np.testing.assert_array_equal(ks.cpu().numpy(), g['scores_{}'.format(i)])
    np.testing.assert_array_equal(kl.cpu().numpy(), g['labels_{}'.format(i)])


def _mcnms_batch(seed, mode, per_class, factor, neg, B=3, C=9):
    rng = np.random.default_rng(seed)
    rows = [300, 0, 257][:B]
    n = 320
    ctr = rng.uniform(60, 900, (10, 2))
    boxes, scores, sfs, valid = [], [], [], []
    for b in range(B):
        k = rng.integers(0, 10, n)
        wh = rng.uniform(20, 160, (n, 2))
        c = ctr[k] + rng.normal(0, 12, (n, 2))
        base = np.stack([c[:, 0] - wh[:, 0] / 2, c[:, 1] - wh[:, 1] / 2, c[:, 0] + wh[:, 0] / 2,
                         c[:, 1] + wh[:, 1] / 2], 1)
        if neg:
            base[:40] -= 120.0  # coordinates < 0: the by-image fallback
        else:
            base = np.clip(base, 0.0, 999.0)
        if per_class:
            bx = np.clip(base[:, :, None] + rng.normal(0, 3, (n, 4, C)), 0.0 if not neg else -1e9, 999.0)
            bx = bx.reshape(n, 4 * C)
        else:
            bx = base
        logits = rng.normal(0, 2, (n, C))
        sc = 1 / (1 + np.exp(-logits)) if mode == 'strict' else np.exp(logits) / np.exp(logits).sum(1, keepdims=True)
        sc = np.round(sc * 64) / 64  # exact ties
        boxes.append(bx.astype(np.float32))
        scores.append(sc.astype(np.float32))
        sfs.append(None if factor is None else rng.choice([0.5, 0.75, 1.0], (n,) if factor == 'row' else (n, C))
                   .astype(np.float32))
        valid.append(rng.uniform(size=n) > 0.1)
    chans = list(range(1, C)) if mode == 'official' else [c for c in range(C) if c != 4]
    return rows, n, boxes, scores, sfs, valid, chans


@pytest.mark.parametrize('mode,per_class,factor,neg', [('official', False, None, False),
                                                       ('official', True, 'row', False),
                                                       ('official', False, 'class', False),
                                                       ('strict', False, 'row', False),
                                                       ('strict', True, None, False),
                                                       ('official', False, None, True),
                                                       ('strict', True, 'row', True)])
def test_mcnms_batched_vs_per_image_oracle(dev, mode, per_class, factor, neg):
    """a11 as one class-wise batched kernel (csrc/mcnms.hip): 3 images (one empty) of padded
    rows with removed rows masked (row_valid), score ties (scores on a 1/64 grid), per-row /
    per-class score factors, class-specific boxes, a channel subset and max_num = 50, against
    the oracle's per-image restatement of utils.multiclass_nms (lib/utils.py:211-269) on
    the rows the reference would see: bit-exact boxes, scores, labels and order.  neg: some
    coordinates < 0, where the reference's shifted classes can overlap -> one segment per
    image."""
    from frcnn_amd import ops
    rows, n, boxes, scores, sfs, valid, chans = _mcnms_batch(70 + 3 * int(neg), mode, per_class, factor, neg)
    B = len(rows)
    rv = np.stack(valid)
    for b in range(B):
        rv[b, rows[b]:] = False
    sf = None if factor is None else T(np.stack(sfs), dev)
    res = ops.multiclass_nms_batched(T(np.stack(boxes), dev), T(np.stack(scores), dev), chans, 0.5, 0.05, 50, sf,
                                     mode=mode, num_rows=torch.tensor(rows, dtype=torch.int32, device=dev),
                                     row_valid=T(rv, dev))
    total = 0
    for b in range(B):
        keep = rv[b, :rows[b]]
        kb, ks, kl = oracle.multiclass_nms(boxes[b][:rows[b]][keep], scores[b][:rows[b]][keep], chans, 0.5, 0.05, 50,
                                           None if factor is None else sfs[b][:rows[b]][keep], mode=mode)
        gb, gs, gl = (x.cpu().numpy() for x in res[b])
        np.testing.assert_array_equal(gb, kb)
        np.testing.assert_array_equal(gs, ks)
        np.testing.assert_array_equal(gl, kl)
        total += len(ks)
    assert total > 20


def _mcnms_check(dev, boxes, scores, chans, thr, min_score, max_num, mode='official'):
    from frcnn_amd import ops
    res = ops.multiclass_nms_batched(T(np.stack(boxes), dev), T(np.stack(scores), dev), chans, thr, min_score,
                                     max_num, None, mode=mode)
    total = 0
    for b in range(len(boxes)):
        kb, ks, kl = oracle.multiclass_nms(boxes[b], scores[b], chans, thr, min_score, max_num, None, mode=mode)
        gb, gs, gl = (x.cpu().numpy() for x in res[b])
        np.testing.assert_array_equal(gb, kb)
        np.testing.assert_array_equal(gs, ks)
        np.testing.assert_array_equal(gl, kl)
        total += len(ks)
    return total


def test_mcnms_one_dense_class_many_segments(dev):
    """8 images x 80 classes (640 segments) where one class per image keeps ~5000
    candidates above min_score and the others a handful: each segment's NMS mask is sized
    by its own count (a square per segment sized by the largest would need ~2 GB here);
    bit-exact vs the per-image oracle (lib/utils.py:224-269)."""
    rng = np.random.default_rng(91)
    B, C, n = 8, 80, 5000
    boxes, scores = [], []
    for b in range(B):
        ctr = rng.uniform(50, 950, (n, 2))
        wh = rng.uniform(10, 120, (n, 2))
        bx = np.clip(np.concatenate([ctr - wh / 2, ctr + wh / 2], 1), 0, 999).astype(np.float32)
        sc = np.full((n, C), 0.01, np.float32)
        sc[:, 1 + b % (C - 1)] = rng.uniform(0.06, 1.0, n).astype(np.float32)  # the dense class
        few = rng.integers(0, n, 40)
        sc[few, rng.integers(1, C, 40)] = 0.5
        boxes.append(bx)
        scores.append(sc)
    assert _mcnms_check(dev, boxes, scores, list(range(1, C)), 0.5, 0.05, 100) > 100 * B // 2


def test_mcnms_by_image_above_sort_chunk(dev):
    """Negative coordinates send every class of an image into ONE segment (the reference's
    single offset pass); 1000 rows x 20 classes = 20 000 candidates exceed the 16 384 records
    one workgroup sorts in LDS, so the chunked sort + rank merge runs.  Bit-exact vs the oracle."""
    rng = np.random.default_rng(92)
    n, C = 1000, 21
    ctr = rng.uniform(-50, 950, (n, 2))
    wh = rng.uniform(10, 200, (n, 2))
    bx = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)
    sc = rng.uniform(0.06, 1.0, (n, C)).astype(np.float32)
    sc = (np.round(sc * 256) / 256).astype(np.float32)  # exact ties across the chunks
    assert bx.min() < 0
    assert _mcnms_check(dev, [bx], [sc], list(range(1, C)), 0.5, 0.05, None) > 1000


def test_retina_predict_batched_equals_per_image(dev):
    """RetinaHead.predict_bboxes_from_output on 2 images (one batched multiclass NMS) equals
    predict_single_image per image, with the min-size filter active (masked rows)."""
    from frcnn_amd.config import ConfigDict
    head = _retina_head(dev)
    cfg = ConfigDict(dict(pre_nms=1000, min_bbox_size=8, min_score=0.05, nms_iou=0.5, nms_type='official',
                          max_per_img=100))
    cls, reg = inputs.head_outputs(951, inputs.RETINA_GRIDS, 9, 20, batch=2, cls_scale=2.0, reg_scale=0.6)
    cls, reg = [T(c, dev) for c in cls], [T(r, dev) for r in reg]
    metas = [inputs.img_meta(), dict(inputs.img_meta(), scale_factor=1.2)]
    bb, ss, ll = head.predict_bboxes_from_output(cls, reg, metas, cfg)
    anchors = head.create_anchors(inputs.RETINA_GRIDS)
    for i in range(2):
        kb, ks, kl = head.predict_single_image([c[i] for c in cls], [r[i] for r in reg], anchors, metas[i], cfg)
        assert ks.numel() > 10
        assert torch.equal(bb[i], kb) and torch.equal(ss[i], ks) and torch.equal(ll[i], kl)


def test_bbox_head_predict_batched_equals_per_image(dev):
    """BBoxHead.predict_bboxes_batched (ragged proposals per image, one batched multiclass NMS)
    equals predict_bboxes_single_image per image."""
    from frcnn_amd.config import ConfigDict
    from frcnn_amd.heads.bbox_head import BBoxHead
    torch.manual_seed(0)
    head = BBoxHead(21, target_means=[0.0] * 4, target_stds=[0.1, 0.1, 0.2, 0.2])
    cfg = ConfigDict(dict(min_score=0.05, nms_iou=0.5, max_per_img=100))
    props = [T(inputs.random_boxes(40 + i, k, min_wh=8, max_wh=300), dev) for i, k in enumerate((600, 437))]
    cls = [torch.randn(p.shape[1], 21, device=dev) * 3 for p in props]
    reg = [torch.randn(p.shape[1], 84, device=dev) * 0.3 for p in props]
    sizes = [(600, 1000), (580, 990)]
    bb, ss, ll = head.predict_bboxes_batched(props, cls, reg, sizes, cfg)
    for i in range(2):
        kb, ks, kl = head.predict_bboxes_single_image(props[i], cls[i], reg[i], sizes[i], cfg)
        assert ks.numel() > 10
        assert torch.equal(bb[i], kb) and torch.equal(ss[i], ks) and torch.equal(ll[i], kl)


# ----------------------------------------------------------------- a15 Retina dense path, a17 refine
def _retina_head(dev):
    from frcnn_amd.heads.retina_head import RetinaHead
    return RetinaHead(21, 256, 1, 8, loss_cls=dict(type='FocalLoss', use_sigmoid=True),
                      loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0)).to(dev)


def test_retina_loss_vs_reference(dev, golden):
    """cfg3 dense path: A=9 anchors, MaxIoU (0.5, 0.4, 0.0), no sampler, focal + smooth-L1,
    two images batched; f32 sums over ~116k x 20 terms -> rtol 1e-5."""
    from frcnn_amd.config import ConfigDict
    g = golden('retina.npz')
    gts = inputs.voc_gts()
    head = _retina_head(dev)
    cfg = ConfigDict(dict(assigner=dict(type='MaxIoUAssigner', pos_iou=0.5, neg_iou=0.4, min_pos_iou=0.0),
                          allowed_border=-1))
    for i in range(2):
        cls, reg = inputs.head_outputs(900 + i, inputs.RETINA_GRIDS, 9, 20, batch=2, cls_scale=1.0, reg_scale=0.2)
        c, r = head.loss([T(x, dev) for x in cls], [T(x, dev) for x in reg],
                         [T(gts[2 * i + j][0], dev) for j in range(2)], [T(gts[2 * i + j][1], dev) for j in range(2)],
                         [inputs.img_meta(), inputs.img_meta()], cfg)
        np.testing.assert_allclose([float(c), float(r)], g['loss_{}'.format(i)], rtol=1e-5)


def test_retina_loss_batch8_equal_per_image_oracle(dev):
    """cfg3 at its benchmark batch: RetinaHead.loss on 8 images in ONE batched target pass.
    The batched targets (chosen outputs, labels exact; params 1e-5) equal the per-image oracle
    results concatenated in image order, and the focal / smooth-L1 losses equal the oracle's
    float64 sums over them (f32 device sums over ~1M terms -> rtol 2e-5)."""
    from frcnn_amd.config import ConfigDict
    gts = inputs.voc_gts()[4:12]
    head = _retina_head(dev)
    cfg = ConfigDict(dict(assigner=dict(type='MaxIoUAssigner', pos_iou=0.5, neg_iou=0.4, min_pos_iou=0.0),
                          allowed_border=-1))
    cls, reg = inputs.head_outputs(960, inputs.RETINA_GRIDS, 9, 20, batch=8, cls_scale=1.0, reg_scale=0.2)
    args = ([T(x, dev) for x in cls], [T(x, dev) for x in reg], [T(x[0], dev) for x in gts],
            [T(x[1], dev) for x in gts], [inputs.img_meta()] * 8, cfg)
    tc, tr, tl, tp = head.targets_batched(*args)
    c, r = head.loss(*args)
    strides, grids = inputs.RETINA_STRIDES, inputs.RETINA_GRIDS
    anc = [oracle.anchor_grid(s, [4 * 2 ** (i / 3) for i in range(3)], [0.5, 1.0, 2.0], s, g)
           for s, g in zip(strides, grids)]
    rc, rr, (oc, orr, ol, op) = oracle.anchor_head_loss(cls, reg, anc, strides, [x[0] for x in gts],
                                                        [x[1] for x in gts], inputs.IMG_SHAPE, (0.5, 0.4, 0.0), -1,
                                                        1.0 / 9.0, 20)
    assert tl.numel() == ol.size and int((ol > 0).sum()) > 8
    np.testing.assert_array_equal(tl.cpu().numpy(), ol)
    np.testing.assert_array_equal(tc.detach().cpu().numpy(), oc)
    np.testing.assert_array_equal(tr.detach().cpu().numpy(), orr)
    np.testing.assert_allclose(tp.cpu().numpy(), op, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose([float(c), float(r)], [rc, rr], rtol=2e-5)


def test_retina_predict_vs_reference(dev, golden):
    """cfg3 test path (anchor_head.py:207-262, strict multiclass NMS).  sigmoid / exp are
    device math (<= 1 ulp from torch CPU), so boxes/scores to 1e-4 and labels exact."""
    from frcnn_amd.config import ConfigDict
    g = golden('retina.npz')
    head = _retina_head(dev)
    anchors = head.create_anchors(inputs.RETINA_GRIDS)
    cfg = ConfigDict(dict(pre_nms=1000, min_bbox_size=0, min_score=0.05, nms_iou=0.5, nms_type='strict',
                          max_per_img=100))
    cls, reg = inputs.head_outputs(950, inputs.RETINA_GRIDS, 9, 20, batch=1, cls_scale=2.0, reg_scale=0.2)
    kb, ks, kl = head.predict_single_image([T(c[0], dev) for c in cls], [T(r[0], dev) for r in reg], anchors,
                                           inputs.img_meta(), cfg)
    # detections whose scores differ by < 1 ulp may swap rank: compare as sets keyed by
    # (label, rounded box), then values
    def canon(b, s, l):
        o = np.lexsort((np.round(b[1], 1), np.round(b[0], 1), l))
        return b[:, o], s[o], l[o]
    b, s, l = canon(kb.cpu().numpy(), ks.cpu().numpy(), kl.cpu().numpy())
    rb, rs, rl = canon(g['pred_boxes'], g['pred_scores'], g['pred_labels'])
    np.testing.assert_array_equal(l, rl)
    np.testing.assert_allclose(s, rs, rtol=1e-5)
    np.testing.assert_allclose(b, rb, rtol=0, atol=1e-3)
    np.testing.assert_allclose(np.sort(ks.cpu().numpy())[::-1], ks.cpu().numpy())  # score order kept


@pytest.mark.parametrize('agnostic', [False, True])
def test_cascade_refine_vs_reference(dev, golden, agnostic):
    """a17 BBoxHead.refine_bboxes_single_image: class column select, gt rows dropped,
    decode with cascade stds, clamp (HIP param2bbox; exp within 1 ulp -> atol 1e-3 px)."""
    from frcnn_amd.heads.bbox_head import BBoxHead
    g = golden('retina.npz')
    bh = BBoxHead(21, target_means=(0.0,) * 4, target_stds=(0.05, 0.05, 0.1, 0.1), reg_class_agnostic=agnostic,
                  loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False),
                  loss_bbox=dict(type='SmoothL1Loss', beta=1.0))
    props, label, reg_out, is_gt = inputs.refine_inputs(agnostic)
    out = bh.refine_bboxes_single_image(T(props, dev), T(label, dev), T(reg_out, dev), T(is_gt, dev),
                                        inputs.img_meta())
    ref = g['refine_{}'.format(int(agnostic))]
    assert tuple(out.shape) == ref.shape
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=0, atol=1e-3)


# ----------------------------------------------------------------- all BASELINE configs end to end
@pytest.mark.parametrize('config,batch', [('faster_rcnn_r50', 2), ('faster_rcnn_r50_fpn', 2),
                                          ('retinanet_r50_fpn', 2), ('retinanet_r50_fpn', 8),
                                          ('cascade_rcnn_r50_fpn', 2), ('fcos_r50_fpn_atss', 2)])
def test_baseline_config_train_and_test(dev, config, batch):
    """Every BASELINE.json config builds from its config file through the registry and runs
    forward_train (+ backward) and forward_test on the HIP path (600x1000 images; 2 per
    batch, and cfg3 also at its benchmark batch of 8)."""
    import os
    import bench
    from frcnn_amd import set_sampler_mode
    set_sampler_mode('device', seed=3)
    path = os.path.join(bench.REPO, 'pytorch-faster-rcnn_amd', 'configs', config + '.py')
    model, _ = bench.make_model(dev, seed=0, config=path)
    imgs, boxes, labels, metas = bench.make_batch(dev, batch, seed=1)
    losses = model.forward_train(imgs, boxes, labels, metas)
    assert len(losses) >= 2
    for k, v in losses.items():
        assert torch.isfinite(v).all(), (config, k)
    sum(losses.values()).backward()
    model.eval()
    with torch.no_grad():
        preds = model.forward_test(imgs, metas)
    assert len(preds) == 3 and len(preds[0]) == batch  # (boxes, scores, labels) per image
    for b, s, l in zip(*preds):
        assert b.shape[0] == 4 and b.shape[1] == s.numel() == l.numel() <= 100
        if s.numel():
            assert (l >= 1).all() and (l <= 20).all()


def test_eval_end_to_end_cfg2(dev):
    """f3 on the GPU: cfg2 forward_test on a fixed synthetic batch -> BasicTester.inference
    (tester.py:25-57) -> results_to_coco (test.py:75-90) -> coco_eval.evaluate.
    The json equals the reference's conversion formula applied to the raw detections
    (xyxy2xywh with +1, / scale_factor, bbox rounded to 2, score to 3), and the summary
    equals the oracle restatement of COCOeval (oracle/coco_oracle.py) on a ground truth made
    of the batch's boxes plus jittered copies of every other detection.  Random-init
    weights give near-uniform class scores, so rcnn.min_score is lowered to 0.01."""
    import bench
    import coco_oracle
    from frcnn_amd import tester, coco_eval, utils
    model, _ = bench.make_model(dev, seed=0)
    model.test_cfg.rcnn.min_score = 0.01
    imgs, boxes, labels, metas = bench.make_batch(dev, 2, seed=4)
    names = ['000017.jpg', '004321.jpg']
    metas = [dict(m, filename='/voc/JPEGImages/' + n) for m, n in zip(metas, names)]
    seen, fwd = [], model.forward_test

    def forward_test(img, img_metas):  # keep the raw detections the tester converts
        seen.append(fwd(img, img_metas))
        return seen[-1]

    model.forward_test = forward_test
    t = tester.BasicTester(model, {}, model.test_cfg, dev)
    res = t.inference([{'img': imgs, 'img_meta': metas}])
    out = tester.results_to_coco(res)
    raw = seen[0]
    want, n = [], 0
    for i, m in enumerate(metas):
        # the reference's formula as the reference runs it on the GPU (tester.py:49 on device
        # tensors: a tensor / python-float divide, which torch implements as a multiply by the
        # reciprocal, so it is evaluated here on the device too)
        b = raw[0][i]
        xywh = (torch.stack([b[0], b[1], b[2] - b[0] + 1, b[3] - b[1] + 1]).t() / m['scale_factor']).cpu().numpy()
        s, l = raw[1][i].cpu().numpy(), raw[2][i].cpu().numpy()
        for j in range(b.shape[1]):
            want.append({'id': n, 'image_id': int(names[i][:-4]), 'file_name': names[i],
                         'bbox': [round(float(v), 2) for v in xywh[j]], 'score': round(float(s[j]), 3),
                         'category_id': int(l[j])})
            n += 1
    assert len(out) > 20, 'expected detections from the lowered threshold'
    assert out == want
    rng = np.random.default_rng(0)
    anns = []
    for i, m in enumerate(metas):
        g = (utils.xyxy2xywh(boxes[i]).t() / m['scale_factor']).cpu().numpy()
        for j, (bb, lab) in enumerate(zip(g, labels[i].cpu().numpy())):
            anns.append({'id': len(anns) + 1, 'image_id': int(names[i][:-4]), 'category_id': int(lab),
                         'bbox': [float(v) for v in bb], 'iscrowd': 0, 'area': float(bb[2] * bb[3])})
    for d in out[::2]:
        bb = np.add(d['bbox'], rng.normal(0, 0.05, 4) * np.array(d['bbox'])[[2, 3, 2, 3]]).clip(1.0)
        anns.append({'id': len(anns) + 1, 'image_id': d['image_id'], 'category_id': d['category_id'],
                     'bbox': [float(v) for v in bb], 'iscrowd': 0, 'area': float(bb[2] * bb[3])})
    gt = {'images': [{'id': int(nm[:-4])} for nm in names], 'annotations': anns,
          'categories': [{'id': c} for c in range(1, 21)]}
    s, r = coco_eval.evaluate(gt, out), coco_oracle.evaluate(gt, out)
    for k in r:
        assert s[k] == pytest.approx(r[k], abs=1e-12), k
    assert 0.0 < s['AP50'] < 1.0


def test_train_step_cfg2(dev):
    """frcnn_amd.train.TrainStep (the reference's train_one_iter: loss -> backward -> grad clip
    -> SGD, config optimizer) on cfg2 for two iterations: finite losses, trainable parameters
    move, frozen stage-1 parameters do not (backbone frozen_stages=1)."""
    import bench
    from frcnn_amd import set_sampler_mode
    from frcnn_amd.train import TrainStep
    set_sampler_mode('device', seed=5)
    model, cfg = bench.make_model(dev, seed=0)
    batch = bench.make_batch(dev, 2, seed=2)
    step = TrainStep(model, cfg.optimizer, cfg.optimizer_config.grad_clip)
    frozen = model.backbone.conv1.weight.detach().clone()
    head = model.rpn_head.conv.weight.detach().clone() if hasattr(model.rpn_head, 'conv') else None
    fc = [p for p in model.parameters() if p.requires_grad][-1].detach().clone()
    losses = [float(step(*batch)) for _ in range(2)]
    assert all(np.isfinite(losses))
    assert torch.equal(model.backbone.conv1.weight, frozen)
    assert not torch.equal([p for p in model.parameters() if p.requires_grad][-1], fc)
    if head is not None:
        assert not torch.equal(model.rpn_head.conv.weight, head)


# ----------------------------------------------------------------- backbone epilogue (frozen BN + add + ReLU)
@pytest.mark.parametrize('skip,relu,shape', [(False, True, (2, 64, 76, 128)), (True, True, (2, 256, 38, 64)),
                                             (False, False, (1, 512, 19, 32)), (True, True, (2, 2048, 19, 32))])
def test_bn_act_matches_torch(dev, skip, relu, shape):
    """frh_bn_act vs the PyTorch fp32 reference bn(x) (+ skip) (+ relu) in eval mode, forward
    and backward (f32 ulp-level tolerance: x*s+b vs (x-mean)*inv*gamma+beta)."""
    from frcnn_amd import ops
    torch.manual_seed(0)
    C = shape[1]
    bn = torch.nn.BatchNorm2d(C).to(dev).eval()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-1, 1)
        bn.running_var.uniform_(0.5, 2.0)
    x = torch.randn(*shape, device=dev, requires_grad=True)
    sk = torch.randn(*shape, device=dev, requires_grad=True) if skip else None
    y = ops.bn_act(x, bn, skip=sk, relu=relu)
    ref = bn(x) + (sk if skip else 0)
    ref = torch.relu(ref) if relu else ref
    torch.testing.assert_close(y, ref, rtol=1e-5, atol=1e-5)
    gy = torch.randn_like(y)
    grads = torch.autograd.grad(y, [x, bn.weight, bn.bias] + ([sk] if skip else []), gy)
    rgrads = torch.autograd.grad(ref, [x, bn.weight, bn.bias] + ([sk] if skip else []), gy)
    for a, b in zip(grads, rgrads):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize('shape', [(2, 64, 304, 512), (1, 8, 7, 16), (1, 4, 10, 24)])
def test_bn_act_maxpool_stem_bit_exact(dev, shape):
    """ResNet stem: frh_bn_act_maxpool (frozen BN + ReLU + max_pool2d(3, 2, 1) in one pass) equals
    frh_bn_act followed by torch's max pool bit for bit (even and odd heights, the cfg2 stem
    shape); with a gradient needed, the unfused ops run."""
    from frcnn_amd import ops
    torch.manual_seed(1)
    C = shape[1]
    bn = torch.nn.BatchNorm2d(C).to(dev).eval()
    pool = torch.nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-1, 1)
        bn.running_var.uniform_(0.5, 2.0)
        x = torch.randn(*shape, device=dev)
        y = ops.bn_act_maxpool(x, bn, pool)
        ref = pool(ops.bn_act(x, bn))
    assert y.shape == ref.shape
    assert torch.equal(y, ref)
    xg = x.clone().requires_grad_(True)
    yg = ops.bn_act_maxpool(xg, bn, pool)
    assert yg.requires_grad and torch.equal(yg.detach(), ref)


def test_graphed_trunk_matches_eager(dev):
    """frcnn_amd.graphs: backbone + neck + RPN head convs replayed as one hipGraph give the
    eager trunk's features, RPN outputs and parameter gradients, for the captured batch and
    for new data copied into the captured input; forward_train takes the graph; other shapes
    fall back to eager.  The trunk is MIOpen/Tensile (not this library), and MIOpen may pick
    another f32 solver for a captured call (measured: 5 % of P2 elements differ, by at most
    4.8e-4 absolute), so outputs compare to 1e-3 of each tensor's scale."""
    import bench
    from frcnn_amd import set_sampler_mode
    from frcnn_amd.graphs import Trunk, capture_trunk, release_trunk
    model, _ = bench.make_model(dev, seed=0)
    imgs, boxes, labels, metas = bench.make_batch(dev, 2, seed=1)
    trunk = Trunk(model.backbone, model.neck, model.rpn_head)
    params = [p for p in trunk.parameters() if p.requires_grad]

    def eager(x):
        outs = trunk(x)
        grads = torch.autograd.grad(sum(o.float().square().mean() for o in outs), params)
        return [o.detach().clone() for o in outs], [g.clone() for g in grads]

    ref = [eager(imgs), eager(imgs * 0.5)]
    set_sampler_mode('device', seed=11)
    loss_ref = {k: v.detach().clone() for k, v in model.forward_train(imgs, boxes, labels, metas).items()}
    g = capture_trunk(model, imgs)
    try:
        for x, (outs_e, grads_e) in zip([imgs, imgs * 0.5], ref):
            feats, cls_outs, reg_outs = g(x)
            outs = feats + cls_outs + reg_outs
            assert len(outs) == len(outs_e)
            grads = torch.autograd.grad(sum(o.float().square().mean() for o in outs), params)
            for a, b in zip(outs, outs_e):
                torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-3 * float(b.abs().max()))
            for a, b in zip(grads, grads_e):
                torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-3 * float(b.abs().max()))
        set_sampler_mode('device', seed=11)
        losses = model.forward_train(imgs, boxes, labels, metas)
        assert losses.keys() == loss_ref.keys()
        for k in losses:
            assert torch.isfinite(losses[k]).all(), k
        assert not g.matches(imgs[:1]) and g.matches(imgs)
        one = model.forward_train(imgs[:1], boxes[:1], labels[:1], metas[:1])  # eager fallback
        assert all(torch.isfinite(v).all() for v in one.values())

        # outputs held across the next replay: flagged stale, and a backward through them raises
        feats_n, _, _ = g(imgs)
        loss_n = feats_n[0].float().square().mean()
        n = g.replays
        assert g.is_current(feats_n[0])
        g(imgs * 0.5)
        assert g.replays == n + 1 and not g.is_current(feats_n[0])
        with pytest.raises(RuntimeError):
            loss_n.backward()
    finally:
        release_trunk(model)

    # clone_outputs: private copies survive the next replay unchanged
    g = capture_trunk(model, imgs, clone_outputs=True)
    try:
        with torch.no_grad():
            keep = g(imgs)[0][0]
            kept = keep.clone()
            g(imgs * 0.5)
        assert torch.equal(keep, kept)
        # parameters moved / replaced after capture: the graph no longer matches (eager path)
        assert g.matches(imgs)
        conv = model.rpn_head.conv if hasattr(model.rpn_head, 'conv') else None
        if conv is not None:
            old = conv.weight
            conv.weight = torch.nn.Parameter(old.detach().clone())
            assert not g.matches(imgs)
            conv.weight = old
            assert g.matches(imgs)
        model.double()
        assert not g.matches(imgs)
        model.float()
        assert not g.matches(imgs)
    finally:
        release_trunk(model)


def test_forward_train_loss_dict_vs_reference(dev):
    """The product's whole cfg2 forward_train against the loss dict the reference produced on
    the same seeded weights and inputs (tests/golden/ftrain.json; see
    test_forward_train_loss_dict_oracle_vs_reference).  The trunk (backbone + FPN + RPN head
    convs) runs on the CPU, as in the fixture, and its outputs enter forward_train through
    the graphed-trunk hook, so every detection primitive after it -- RPN targets + loss,
    proposals + NMS, RCNN targets with the numpy-RNG samplers, RoIAlign, the RCNN losses --
    runs on the HIP path with inputs identical to the reference's.  Only the RCNN FC layers'
    f32 sums (GPU GEMM vs CPU) differ in rounding: rel 1e-4."""
    import json
    import os
    from frcnn_amd import set_sampler_mode
    from test_oracle_golden import ftrain_model
    ref = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ftrain.json')))
    model, _ = ftrain_model()
    img, boxes, labels, metas = inputs.ftrain_case()
    x = torch.from_numpy(img)
    with torch.no_grad():
        feats = model.extract_feat(x)
        cls, reg = model.rpn_head(feats)
    model = model.to(dev)
    trunk = ([f.to(dev) for f in feats], [c.to(dev) for c in cls], [r.to(dev) for r in reg])

    class CpuTrunk(object):  # the graphed-trunk hook of CascadeRCNN.forward_train
        def matches(self, img_data):
            return True

        def __call__(self, img_data):
            return trunk

    model.graphed_trunk = CpuTrunk()
    set_sampler_mode('numpy')
    np.random.seed(inputs.FTRAIN_NP_SEED)
    with torch.no_grad():
        losses = model.forward_train(x.to(dev), [T(b, dev) for b in boxes], [T(l, dev) for l in labels], metas)
    assert set(losses) == set(ref['losses'])
    for k, v in ref['losses'].items():
        assert float(losses[k]) == pytest.approx(v, rel=1e-4), (k, float(losses[k]), v)


@pytest.mark.parametrize('max_props', [None, 100])
def test_sync_free_targets_match_synced(dev, max_props):
    """cfg2 forward_train with the device sampler: the sync-free RPN loss and RCNN stage
    (padded fixed-capacity targets, frh_roi_rows_dev, device avg_factor) against the synced
    path (read-back sizes, per-image split) on the same sampler stream and the same trunk
    outputs (held fixed: MIOpen may pick another conv solver from one call to the next, see
    test_graphed_trunk_matches_eager) -- same losses, and the same gradients w.r.t. the
    features, the RPN outputs and the RCNN head parameters.  max_props=100 caps the proposals
    so the RCNN buffer really carries padding rows (100 + gts < 512 per image).  Tolerances:
    the padded launches may partition the f32 sums differently (losses rtol 1e-5), the FC
    GEMMs run over more rows and RoIAlign backward accumulates with atomics."""
    import bench
    from frcnn_amd import set_sampler_mode
    model, _ = bench.make_model(dev, seed=0)
    if max_props is not None:
        model.train_cfg.rpn_proposal.max_num = max_props
    imgs, boxes, labels, metas = bench.make_batch(dev, 2, seed=1)
    with torch.no_grad():
        feats = [f.detach().clone().requires_grad_(True) for f in model.extract_feat(imgs)]
        rc, rr = model.rpn_head(feats)
    rc = [c.detach().clone().requires_grad_(True) for c in rc]
    rr = [r.detach().clone().requires_grad_(True) for r in rr]
    model.extract_feat = lambda x: feats
    model.rpn_head.forward = lambda xs: (rc, rr)
    leaves = feats + rc + rr + [p for p in model.rcnn_head.parameters() if p.requires_grad]
    calls = []
    ff = model.roi_extractors[0].forward_flat
    model.roi_extractors[0].forward_flat = lambda *a: calls.append(1) or ff(*a)

    def run():
        set_sampler_mode('device', seed=21)
        ls = model.forward_train(imgs, boxes, labels, metas)
        gr = torch.autograd.grad(sum(ls.values()), leaves, allow_unused=True)
        return {k: v.detach().clone() for k, v in ls.items()}, gr

    la, ga = run()
    assert calls, 'the sync-free RCNN stage did not run'
    model.rpn_head.sync_free = lambda *a: False
    model._sync_free_rcnn = lambda *a: False
    lb, gb = run()
    assert len(calls) == 1
    assert la.keys() == lb.keys()
    for k in la:
        a, b = float(la[k]), float(lb[k])
        assert a == pytest.approx(b, rel=1e-5, abs=1e-7), (k, a, b)
    for a, b in zip(ga, gb):
        if a is None or b is None:
            assert a is None and b is None
            continue
        torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-4 * float(b.abs().max()) + 1e-12)
