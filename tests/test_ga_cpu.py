"""CPU checks of Guided Anchoring (no GPU).

The deformable convolution has no reference implementation to copy, so its definition (DCNv1,
include/frcnn_amd.h frh_deform_conv3x3_act) is pinned by hand-derived witnesses on the torch
restatement ops.deform_conv3x3_torch in f64: the restatement is then the numerics reference the
HIP kernel is held to in tests/test_gpu_deform_conv.py.  The targets' per-cell rule
(ga_inputs.cell_rule, what csrc/ga.hip computes) is held to the REFERENCE's own painting loops
(tests/golden/ga_targets.npz, made by gen_ga_golden.py), and BoundedIoULoss, map_gt2level and the
head's state_dict to the same fixture."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ga_inputs


def _dc(x, off, w, dg):
    from frcnn_amd.ops import deform_conv3x3_torch
    return deform_conv3x3_torch(x, off, w, dg)


def _case(n=2, cin=8, cout=6, dg=2, h=5, w=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, cin, h, w, generator=g, dtype=torch.float64),
            torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64), torch.zeros(n, 18 * dg, h, w,
                                                                                        dtype=torch.float64))


# ----------------------------------------------------------------- the restatement's witnesses
def test_zero_offsets_are_the_plain_convolution():
    x, w, off = _case()
    torch.testing.assert_close(_dc(x, off, w, 2), F.conv2d(x, w, padding=1), rtol=1e-12, atol=1e-12)


def test_dy_plus_one_shifts_the_rows():
    """Every tap one row down: row y + ky + 1, i.e. one zero row above and two below."""
    x, w, off = _case(seed=1)
    off[:, 0::2] = 1.0
    torch.testing.assert_close(_dc(x, off, w, 2), F.conv2d(F.pad(x, (1, 1, 0, 2)), w), rtol=1e-12, atol=1e-12)


def test_half_pixel_dx_is_the_two_column_average():
    """px = x + kx + 0.5 blends columns x + kx and x + kx + 1 half and half.  At the left border
    the sample at px = -0.5 is 0.5 x[0] (column -1 contributes 0), not 0; at the right border
    px = W - 0.5 is 0.5 x[W - 1]."""
    x, w, off = _case(seed=2)
    off[:, 1::2] = 0.5
    xp = F.pad(x, (1, 1))                     # columns -1 and W as zeros
    avg = 0.5 * (xp[..., :-1] + xp[..., 1:])  # avg[i] = (x[i - 1] + x[i]) / 2, i = 0 .. W
    # tap kx of output column c reads avg[c + kx + 1]; one more zero column on the right (px =
    # W + 0.5 is outside the map) and no column padding: output m reads avg[m .. m + 2]
    want = F.conv2d(F.pad(avg, (0, 1, 1, 1)), w)
    assert want.shape == x.shape[:1] + (w.shape[0],) + x.shape[2:]
    torch.testing.assert_close(_dc(x, off, w, 2), want, rtol=1e-12, atol=1e-12)
    # the border claim on its own: one input column, the tap kx = -1 of output column 0
    x1 = torch.zeros(1, 4, 1, 3, dtype=torch.float64)
    x1[..., 0] = 2.0
    w1 = torch.zeros(1, 4, 3, 3, dtype=torch.float64)
    w1[0, 0, 1, 0] = 1.0  # ky = 0, kx = -1
    o1 = torch.zeros(1, 18, 1, 3, dtype=torch.float64)
    o1[:, 1::2] = 0.5
    assert _dc(x1, o1, w1, 1)[0, 0, 0].tolist() == [1.0, 1.0, 0.0]


@pytest.mark.parametrize('far', [1e4, -1e4, 3e9, -3e9, float('inf'), float('nan')])
def test_far_offsets_give_exact_zeros(far):
    x, w, off = _case(seed=3)
    off[:] = far
    y = _dc(x, off, w, 2)
    assert (y == 0).all() and not torch.isnan(y).any()


def test_groups_are_independent():
    """Perturbing group 1's offsets moves exactly the terms of channels 4 .. 7."""
    x, w, off = _case(seed=4)
    off.copy_(torch.randint(-8, 9, off.shape, generator=torch.Generator().manual_seed(5)).double() / 4)
    off2 = off.clone()
    off2[:, 18:] += 0.75
    w0, w1 = w.clone(), w.clone()
    w0[:, 4:] = 0  # only group 0's channels
    w1[:, :4] = 0  # only group 1's
    torch.testing.assert_close(_dc(x, off, w0, 2), _dc(x, off2, w0, 2), rtol=0, atol=0)
    assert not torch.equal(_dc(x, off, w1, 2), _dc(x, off2, w1, 2))
    torch.testing.assert_close(_dc(x, off2, w, 2), _dc(x, off, w0, 2) + _dc(x, off2, w1, 2), rtol=1e-12, atol=1e-12)


def test_offset_channel_order():
    """Channel g * 18 + 2 k is dy and + 1 is dx of tap k = 3 (ky + 1) + (kx + 1): moving only the
    centre tap (k = 4) of a one-hot weight by (dy, dx) = (1, -2) reads x[y + 1, x - 2]."""
    x = torch.arange(5 * 7, dtype=torch.float64).view(1, 1, 5, 7).repeat(1, 4, 1, 1)
    w = torch.zeros(1, 4, 3, 3, dtype=torch.float64)
    w[0, 0, 1, 1] = 1.0
    off = torch.zeros(1, 18, 5, 7, dtype=torch.float64)
    off[:, 8], off[:, 9] = 1.0, -2.0
    want = F.pad(x[:, :1], (2, 0, 0, 1))[:, :, 1:, :7]
    torch.testing.assert_close(_dc(x, off, w, 1), want, rtol=0, atol=0)


def test_restatement_differentiates():
    x, w, off = _case(n=1, h=3, w=4, seed=6)
    off.copy_(torch.rand(off.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64) - 0.5)
    x.requires_grad_(True), w.requires_grad_(True), off.requires_grad_(True)
    from frcnn_amd.ops import deform_conv3x3_torch
    assert torch.autograd.gradcheck(lambda a, b, c: deform_conv3x3_torch(a, b, c, 2), (x, off, w), atol=1e-6)


# ----------------------------------------------------------------- targets
def test_cell_rule_equals_the_reference_painting(golden):
    z = golden('ga_targets.npz')
    seen = set()
    for b, meta in enumerate(ga_inputs.img_metas()):
        loc, mask, box = ga_inputs.cell_rule(ga_inputs.REF_BOXES[b], ga_inputs.REF_LEVELS[b], meta['img_shape'],
                                             **ga_inputs.RATIOS)
        np.testing.assert_array_equal(loc, z['loc_{}'.format(b)])
        np.testing.assert_array_equal(mask, z['mask_{}'.format(b)])
        np.testing.assert_array_equal(box, z['box_{}'.format(b)])
        seen |= set(loc.tolist())
    assert seen == {-1, 0, 1}


def test_target_case_covers_its_edges(golden):
    z = golden('ga_targets.npz')
    off = np.cumsum([0] + [h * w for h, w in ga_inputs.GRIDS])
    loc, box = z['loc_0'], z['box_0']
    # the 4 x 4 gt's centre region is the single cell (5, 5) of level 0
    l0 = loc[:off[1]].reshape(ga_inputs.GRIDS[0])
    assert l0[5, 5] == 1 and (l0[4:7, 4:7] == 1).sum() == 1
    # overlapping shape regions on level 0: row 11, columns 3..4 belong to the later gt (2)
    b0 = box[:off[1]].reshape(ga_inputs.GRIDS[0] + (4,))
    assert b0[11, 3].tolist() == ga_inputs.BOXES_0[:, 2].tolist() and b0[10, 3].tolist() == ga_inputs.BOXES_0[:, 1].tolist()
    # half to even on level 1: gt 3's shape region starts at column 2 and row 4
    b1 = box[off[1]:off[2]].reshape(ga_inputs.GRIDS[1] + (4,))
    g3 = ga_inputs.BOXES_0[:, 3].tolist()
    assert b1[4, 2].tolist() == g3 and b1[5, 3].tolist() == g3 and b1[6, 3].tolist() != g3
    assert sorted(set(ga_inputs.LEVELS_0.tolist())) == [0, 1, 2, 3, 4]
    assert z['loc_1'].tolist() == [0] * ga_inputs.NUM_CELLS and not z['mask_1'].any()


def test_numpy_level_map_matches_fixture(golden):
    z = golden('ga_targets.npz')
    for b in range(3):
        np.testing.assert_array_equal(
            ga_inputs.map_gt2level(ga_inputs.ANCHOR_SCALE, ga_inputs.STRIDES, ga_inputs.REF_BOXES[b]),
            z['levels_{}'.format(b)])


# ----------------------------------------------------------------- the mirror's torch pieces
def test_bounded_iou_loss_matches_reference(golden):
    from frcnn_amd.builder import build_module
    z = golden('ga_targets.npz')
    loss = build_module(dict(type='BoundedIoULoss', beta=0.2, loss_weight=1.0))
    x, y = [torch.from_numpy(v) for v in ga_inputs.bounded_iou_inputs()]
    assert float(loss(x.double(), y.double())) == pytest.approx(float(z['biou'][1]), rel=1e-12)
    assert float(loss(x, y)) == pytest.approx(float(z['biou'][0]), rel=2e-6)


def test_map_gt2level_matches_reference(golden):
    from frcnn_amd.region import map_gt2level
    z = golden('ga_targets.npz')
    for b in range(3):
        lv = map_gt2level(ga_inputs.ANCHOR_SCALE, ga_inputs.STRIDES, torch.from_numpy(ga_inputs.REF_BOXES[b]))
        assert lv.dtype == torch.int64
        np.testing.assert_array_equal(lv.numpy(), z['levels_{}'.format(b)])


def test_head_state_dict_matches_reference(golden):
    from frcnn_amd.builder import build_module
    z = golden('ga_targets.npz')
    head = build_module(dict(type='GARPNHead', **ga_inputs.head_kwargs()))
    sd = head.state_dict()
    assert list(sd.keys()) == z['keys'].tolist()
    assert [','.join(str(d) for d in v.shape) for v in sd.values()] == z['shapes'].tolist()
    head.init_weights()
    assert float(head.guided_anchor.loc_layer.bias) == pytest.approx(-np.log(99.0), rel=1e-6)


def test_builder_knows_the_ga_modules_and_config():
    import os
    from frcnn_amd.builder import MODULES, build_module
    from frcnn_amd.config import Config
    assert 'GARPNHead' in MODULES and 'BoundedIoULoss' in MODULES
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Config.fromfile(os.path.join(repo, 'pytorch-faster-rcnn_amd', 'configs', ga_inputs.WHOLE_CONFIG))
    model = build_module(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    assert type(model.rpn_head).__name__ == 'GARPNHead' and model.rpn_head.guided_anchor.deformable_groups == 4
    assert model.rpn_head.guided_anchor.adapt_layer.weight.shape == (256, 256, 3, 3)
    assert cfg.train_cfg.rpn.center_ratio == 0.2 and cfg.train_cfg.rpn.ignore_ratio == 0.5
