"""Guided Anchoring on the HIP path: the one-launch location / shape targets (ops.ga_targets:
frh_ga_targets, csrc/ga.hip) bit-exact against the REFERENCE's own painting loops
(tests/golden/ga_targets.npz, made by gen_ga_golden.py from lib/heads/guided_head.py:342-397 and
:195-251) and, at 200 gts where the reference loop is too slow to fixture, against the numpy
restatement of the per-cell rule (ga_inputs.cell_rule, pinned to the same fixture in
tests/test_ga_cpu.py).

Bar: equality.  The kernel performs the reference's f32 operations in its order."""
import numpy as np
import pytest
import torch

import ga_inputs
import support

pytestmark = pytest.mark.gpu


def _targets(dev, boxes, levels, img_shapes):
    from frcnn_amd import ops
    return ops.ga_targets(ga_inputs.GRIDS, [float(s) for s in ga_inputs.STRIDES],
                          [torch.from_numpy(b).to(dev) for b in boxes], [torch.from_numpy(l).to(dev) for l in levels],
                          [s[:2] for s in img_shapes], **ga_inputs.RATIOS)


def test_targets_vs_reference(dev, golden):
    """B = 3 images of different img_shape under one 96 x 160 padded size, the middle one with
    no gt; levels 0 .. 4 supplied directly (what the cases cover: ga_inputs and
    test_ga_cpu.test_target_case_covers_its_edges)."""
    z = golden('ga_targets.npz')
    loc, mask, box = _targets(dev, ga_inputs.REF_BOXES, ga_inputs.REF_LEVELS, ga_inputs.IMG_SHAPES)
    n = ga_inputs.NUM_CELLS
    assert loc.shape == (3, n) and mask.shape == (3, n) and box.shape == (3, n, 4)
    assert loc.dtype == torch.int64 and mask.dtype == torch.int64 and box.dtype == torch.float32
    for b in range(3):
        np.testing.assert_array_equal(loc[b].cpu().numpy(), z['loc_{}'.format(b)])
        np.testing.assert_array_equal(mask[b].cpu().numpy(), z['mask_{}'.format(b)])
        np.testing.assert_array_equal(box[b].cpu().numpy(), z['box_{}'.format(b)])


def test_an_image_does_not_depend_on_its_batch(dev, golden):
    """Each image alone, and the batch in reverse order (other max_gts padding, other block row)."""
    z = golden('ga_targets.npz')
    order = [2, 0, 1]
    loc, mask, box = _targets(dev, [ga_inputs.REF_BOXES[i] for i in order], [ga_inputs.REF_LEVELS[i] for i in order],
                              [ga_inputs.IMG_SHAPES[i] for i in order])
    for k, b in enumerate(order):
        np.testing.assert_array_equal(loc[k].cpu().numpy(), z['loc_{}'.format(b)])
        np.testing.assert_array_equal(box[k].cpu().numpy(), z['box_{}'.format(b)])
        one = _targets(dev, [ga_inputs.REF_BOXES[b]], [ga_inputs.REF_LEVELS[b]], [ga_inputs.IMG_SHAPES[b]])
        np.testing.assert_array_equal(one[0][0].cpu().numpy(), z['loc_{}'.format(b)])
        np.testing.assert_array_equal(one[1][0].cpu().numpy(), z['mask_{}'.format(b)])


@pytest.mark.parametrize('n', [200, 300])
def test_many_gts_vs_numpy_rule(dev, n):
    """One image of 200 (and 300: a second LDS chunk of gts) gts on random levels beside an image
    without any and the eight-gt image: heavy overlap (the later index owns a shape cell), every
    level."""
    many, lv = ga_inputs.many_case(n)
    boxes = [many, ga_inputs.EMPTY, ga_inputs.BOXES_0]
    levels = [lv, np.zeros(0, np.int64), ga_inputs.LEVELS_0]
    shapes = [ga_inputs.IMG_SHAPES[1], ga_inputs.IMG_SHAPES[2], ga_inputs.IMG_SHAPES[0]]
    loc, mask, box = _targets(dev, boxes, levels, shapes)
    for b in range(3):
        wl, wm, wb = ga_inputs.cell_rule(boxes[b], levels[b], shapes[b], **ga_inputs.RATIOS)
        np.testing.assert_array_equal(loc[b].cpu().numpy(), wl)
        np.testing.assert_array_equal(mask[b].cpu().numpy(), wm)
        np.testing.assert_array_equal(box[b].cpu().numpy(), wb)
    assert set(loc[0].cpu().tolist()) == {-1, 0, 1} and int(mask[0].sum()) > 200


def test_bad_arguments(dev):
    from frcnn_amd import ops
    with pytest.raises(AssertionError):
        ops.ga_targets(ga_inputs.GRIDS, [4.0], [torch.zeros(4, 0, device=dev)], [torch.zeros(0, device=dev)],
                       [(96, 160)], **ga_inputs.RATIOS)
    with pytest.raises(RuntimeError):
        ops.ga_targets(ga_inputs.GRIDS, [4.0] * 5, [torch.zeros(4, 0)], [torch.zeros(0)], [(96, 160)], **ga_inputs.RATIOS)


# ----------------------------------------------------------------- head losses and forward
LOSS_TOL = dict(rtol=2e-5, atol=1e-6)  # as tests/test_gpu_fcos.py
LOSS_ORDER = ('cls_loss', 'reg_loss', 'loc_loss', 'shape_loss')


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def _seeded_head(dev):
    from frcnn_amd.heads import GARPNHead
    head = GARPNHead(**ga_inputs.head_kwargs())
    sd = ga_inputs.head_state({k: tuple(v.shape) for k, v in head.state_dict().items()})
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return head.to(dev)


def _fixture_outputs(z, dev):
    return tuple([torch.from_numpy(z['{}_{}'.format(name, i)]).to(dev) for i in range(len(ga_inputs.GRIDS))]
                 for name in ('cls', 'reg', 'loc', 'shape', 'adapt'))


def test_head_losses_vs_reference(dev, golden):
    """GARPNHead.loss and GuidedAnchor.loss on the reference's own head outputs (the seeded
    8-channel head of ga_inputs.loss_case), both samplers dropping cells from the reference's
    np.random stream."""
    from frcnn_amd import set_sampler_mode
    z = golden('ga_loss.npz')
    c = ga_inputs.loss_case()
    head = _seeded_head(dev)
    outs = _fixture_outputs(z, dev)
    boxes = [torch.from_numpy(b).to(dev) for b in c['boxes']]
    labels = [torch.ones(b.shape[1], dtype=torch.long, device=dev) for b in boxes]
    cfg = _Cfg(ga_inputs.LOSS_CFG)
    set_sampler_mode('numpy')
    np.random.seed(c['np_seed'])
    with torch.no_grad():
        loss = head.loss(*(outs + (boxes, labels, c['metas'], cfg)))
    assert sorted(loss) == sorted(LOSS_ORDER)
    got = np.array([float(loss[k]) for k in LOSS_ORDER])
    print('loss', got, z['loss'])
    np.random.seed(c['np_seed'])
    with torch.no_grad():
        ga = head.guided_anchor.loss(outs[2], outs[3], outs[4], boxes, labels, c['metas'], cfg)
    ga_got = np.array([float(ga[k]) for k in LOSS_ORDER[2:]])
    print('ga_loss', ga_got, z['ga_loss'])
    np.testing.assert_allclose(got, z['loss'], **LOSS_TOL)
    np.testing.assert_allclose(ga_got, z['ga_loss'], **LOSS_TOL)
    assert (z['loss'] > 0).all()


def test_head_forward_vs_reference(dev, golden):
    """The seeded 8-channel head in eval mode on the device against the reference's CPU forward
    (8 channels do not meet the kernel's cin % 16, so its adaption layer is the restatement on
    the GPU; the 64-channel head below takes the kernel): f32 convolutions in another order, rtol
    1e-4 / atol 1e-5."""
    z = golden('ga_loss.npz')
    c = ga_inputs.loss_case()
    head = _seeded_head(dev).eval()
    with torch.no_grad():
        outs = head([torch.from_numpy(f).to(dev) for f in c['feats']])
    for name, o in zip(('cls', 'reg', 'loc', 'shape', 'adapt'), outs):
        for i, t in enumerate(o):
            np.testing.assert_allclose(t.cpu().numpy(), z['{}_{}'.format(name, i)], rtol=1e-4, atol=1e-5)


def test_guided_anchor_eval_takes_the_fused_levels_entry(dev, monkeypatch):
    """A 64-channel GuidedAnchor in eval mode: one frh_deform_conv3x3_act_levels call, equal (f32
    bar of test_gpu_deform_conv.py's dispatch test) to the same module's training path, which
    takes the restatement and back-propagates into the shape branch's offset layer."""
    from frcnn_amd.heads import GARPNHead
    torch.manual_seed(3)
    head = GARPNHead(in_channels=64, feat_channels=64, anchor_strides=list(ga_inputs.STRIDES)).to(dev)
    head.init_weights()
    feats = [torch.randn(2, 64, h, w, device=dev).contiguous(memory_format=torch.channels_last) for h, w in ga_inputs.GRIDS]
    spy = support.spy_entries(monkeypatch)
    head.eval()
    with torch.no_grad():
        ev = head.guided_anchor(feats)
    assert spy.names.count('frh_deform_conv3x3_act_levels') == 1
    spy.clear()
    head.train()
    tr = head.guided_anchor(feats)
    assert not [n for n in spy.names if 'deform' in n]
    for a, b in zip(ev[2], tr[2]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
    sum(t.sum() for t in tr[2]).backward()
    ga = head.guided_anchor
    assert ga.adapt_layer.weight.grad is not None and ga.offset_layer.weight.grad is not None
    assert ga.shape_layer.weight.grad is None  # the offsets are computed from the detached shape map


@pytest.mark.parametrize('num_anchors', [1, 3])
def test_inside_grid_mask_is_sized_by_the_grid(dev, num_anchors):
    """region.inside_grid_mask (the head's in-grid test): A * H * W flags, the first
    int(img / stride) + 1 rows and columns set, and nothing written past them (a guard tensor
    allocated right behind stays intact)."""
    from frcnn_amd import region
    gh, gw = ga_inputs.GRIDS[0]
    m = region.inside_grid_mask(num_anchors, (90, 150), (gh, gw), 4, dev)
    guard = torch.full((4096,), 7, dtype=torch.uint8, device=dev)
    m2 = region.inside_grid_mask(num_anchors, (90, 150), (gh, gw), 4, dev)
    want = np.zeros((num_anchors, gh, gw), np.float32)
    want[:, :min(gh, 90 // 4 + 1), :min(gw, 150 // 4 + 1)] = 1
    assert m.shape == (num_anchors * gh * gw,) and m.dtype == torch.float32
    np.testing.assert_array_equal(m.cpu().numpy(), want.reshape(-1))
    np.testing.assert_array_equal(m2.cpu().numpy(), want.reshape(-1))
    assert bool((guard == 7).all())
