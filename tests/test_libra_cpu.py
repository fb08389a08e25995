"""CPU checks of the Libra R-CNN pieces: the registry and config, the balanced-L1 element and
its derivative (the HIP backward's formula) in float64, the sampler's f32 bin edges against
torch's own comparison, the quota rule against the fixtures, and the BFP mirror's CPU path."""
import math
import os

import numpy as np
import pytest
import torch

import inputs
import libra_inputs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_registry_builds_libra_modules():
    from frcnn_amd.builder import build_module
    from frcnn_amd import losses, necks, region
    assert isinstance(build_module(dict(type='BFP', in_channels=256, num_levels=5, refine_level=2, refine_type=None)),
                      necks.BFP)
    s = build_module(dict(type='IoUBalancedNegSampler', max_num=512, pos_num=128, floor_thr=-1, floor_fraction=0,
                          num_bins=3))
    assert isinstance(s, region.IoUBalancedNegSampler) and s.max_iou == 0.5
    l = build_module(dict(type='BalancedL1Loss', alpha=0.5, gamma=1.5, beta=1.0, loss_weight=1.0))
    assert isinstance(l, losses.BalancedL1Loss)
    assert not losses.fused_kinds(losses.CrossEntropyLoss(), l)  # the RCNN stage takes the synced path


def test_libra_config_builds_a_cascade_rcnn():
    from frcnn_amd.builder import build_module
    from frcnn_amd.config import Config
    from frcnn_amd import detectors, losses, necks
    cfg = Config.fromfile(os.path.join(REPO, 'pytorch-faster-rcnn_amd', 'configs', 'libra_faster_rcnn_r50_fpn.py'))
    model = build_module(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    assert isinstance(model, detectors.CascadeRCNN) and model.num_stages == 1
    assert isinstance(model.neck[0], necks.FPN) and isinstance(model.neck[1], necks.BFP)
    assert isinstance(model.rcnn_head[0].loss_bbox, losses.BalancedL1Loss)
    assert model.rcnn_head[0].reg_class_agnostic
    assert not [k for k in model.state_dict() if k.startswith('neck.1')]  # BFP has no parameters
    assert cfg.train_cfg.rcnn[0].sampler.type == 'IoUBalancedNegSampler'


def test_bfp_constructor_asserts():
    from frcnn_amd.necks import BFP
    with pytest.raises(AssertionError):
        BFP(refine_type='conv')
    with pytest.raises(AssertionError):
        BFP(num_levels=3, refine_level=3)
    m = BFP(8, 3, 1)
    m.init_weights()
    with pytest.raises(AssertionError):
        m([torch.zeros(1, 8, 4, 4)] * 2)


def test_bfp_cpu_path_skips_the_refine_level_in_the_mean():
    """Hand check: two levels, refine_level 0 -> refine = nearest(level 1) / 1."""
    from frcnn_amd.necks import BFP
    a, b = torch.zeros(1, 1, 4, 4), torch.arange(4.0).view(1, 1, 2, 2)
    o0, o1 = BFP(1, 2, 0)([a, b])
    up = b.repeat_interleave(2, 2).repeat_interleave(2, 3)
    assert torch.equal(o0, up)
    assert torch.equal(o1, b + torch.nn.functional.adaptive_max_pool2d(up, (2, 2)))


@pytest.mark.parametrize('alpha,gamma,beta', [(0.5, 1.5, 1.0), (0.3, 1.1, 0.7)])
def test_balanced_l1_element_and_slope_float64(alpha, gamma, beta):
    from frcnn_amd.losses import balanced_l1_loss, balanced_l1_slope
    b = math.e ** (gamma / alpha) - 1
    eps = 1e-9
    for d in (0.0, beta - eps, beta, beta + eps, 37.5):
        x = torch.tensor([d], dtype=torch.float64, requires_grad=True)
        y = torch.zeros(1, dtype=torch.float64)
        v = balanced_l1_loss(x, y, beta=beta, alpha=alpha, gamma=gamma)
        want = alpha / b * (b * d + 1) * math.log(b * d / beta + 1) - alpha * d if d < beta else \
            gamma * d + gamma / b - alpha * beta
        assert float(v) == pytest.approx(want, rel=1e-13, abs=1e-15)
        if d > 0:
            v.sum().backward()
            s = balanced_l1_slope(x.detach(), beta=beta, alpha=alpha, gamma=gamma)
            assert float(s) == pytest.approx(float(x.grad), rel=1e-12)
    if beta == 1.0:  # with beta = 1 the two pieces meet in value and slope (b is chosen for that)
        lo, hi = torch.tensor([beta - eps], dtype=torch.float64), torch.tensor([beta + eps], dtype=torch.float64)
        z = torch.zeros(1, dtype=torch.float64)
        assert float(balanced_l1_loss(lo, z, beta, alpha, gamma)) == pytest.approx(
            float(balanced_l1_loss(hi, z, beta, alpha, gamma)), abs=1e-8)
        assert float(balanced_l1_slope(lo, beta, alpha, gamma)) == pytest.approx(gamma, abs=1e-8)


def test_balanced_l1_module_cpu_forms():
    from frcnn_amd.losses import BalancedL1Loss, balanced_l1_loss
    x, y = (torch.from_numpy(a) for a in libra_inputs.balanced_l1_inputs(1, 12, 4))
    label = torch.tensor([0, 1, 2, 0, -1, 3, 0, 0, 1, -1, 2, 0])
    loss = BalancedL1Loss(loss_weight=2.0)
    full = balanced_l1_loss(x, y)
    assert float(loss(x, y)) == pytest.approx(2.0 * float(full.sum()), rel=1e-6)
    assert float(loss.masked(x, y, label)) == pytest.approx(2.0 * float(full[label > 0].sum()), rel=1e-6)
    reg = torch.from_numpy(np.random.default_rng(2).standard_normal((12, 4 * 5)).astype(np.float32))
    sel = reg.view(-1, 4, 5)[torch.arange(12), :, label.clamp(min=0)]
    want = balanced_l1_loss(sel, y)[label > 0].sum()
    assert float(loss.class_selected(reg, 5, y, label)) == pytest.approx(2.0 * float(want), rel=1e-6)


@pytest.mark.parametrize('num_bins,max_iou', [(3, 0.5), (1, 0.5), (8, 0.7), (5, 1.0)])
def test_f32_bin_edges_compare_as_torch_does(num_bins, max_iou):
    """x >= lo and x < hi with the mirror's f32 edges == torch's comparison of the f32 tensor with
    the reference's Python-float edges, at and one ulp beside every edge."""
    from frcnn_amd.region import IoUBalancedNegSampler
    s = IoUBalancedNegSampler(16, 4, num_bins=num_bins, max_iou=max_iou)
    starts, ends = libra_inputs.bin_edges(num_bins, max_iou)
    probe = []
    for e in starts + ends:
        f = np.float32(e)
        probe += [f, np.nextafter(f, np.float32(-1)), np.nextafter(f, np.float32(2))]
    x = torch.tensor(np.array(probe, np.float32))
    for j in range(num_bins):
        want = (x >= starts[j]) & (x < ends[j])
        got = (x.numpy() >= np.float32(s.bin_lo[j])) & (x.numpy() < np.float32(s.bin_hi[j]))
        np.testing.assert_array_equal(got, want.numpy())


def test_overlapping_bins_raise():
    """Where the reference would count a box in two bins the mirror raises, and the C entry
    refuses the edges (argument validation: no device needed)."""
    from frcnn_amd import _lib, region
    region.IoUBalancedNegSampler.check_bins([0.0, 0.25], [0.25, 0.5])
    with pytest.raises(ValueError):
        region.IoUBalancedNegSampler.check_bins([0.0, 0.2], [0.25, 0.5])
    args = (0, None, 0, None, 0, None, None, 0, 8, 4, 2)
    tail = (0, None, None, None, None)
    assert _lib.query('frh_sample_iou_balanced', *args, _lib.f32_array([0.0, 0.25]), _lib.f32_array([0.25, 0.5]),
                      *tail) == 0
    assert _lib.query('frh_sample_iou_balanced', *args, _lib.f32_array([0.0, 0.2]), _lib.f32_array([0.25, 0.5]),
                      *tail) == -1
    assert b'overlap' in _lib.load().frh_last_error()


def test_sampler_asserts():
    from frcnn_amd.region import IoUBalancedNegSampler
    for kw in (dict(max_num=4, pos_num=8), dict(max_num=8, pos_num=4, max_iou=0.0),
               dict(max_num=8, pos_num=4, max_iou=1.5), dict(max_num=8, pos_num=4, num_bins=9)):
        with pytest.raises(AssertionError):
            IoUBalancedNegSampler(**kw)


@pytest.mark.parametrize('tag', libra_inputs.SAMPLER_FIXTURE_CASES)
def test_quota_rule_matches_the_reference_fixture(tag):
    """ops.iou_bin_quotas (the host side of both sampler modes) gives the per-class counts the
    reference's sampler kept (tests/golden/libra_sampler.npz)."""
    from frcnn_amd import ops
    from frcnn_amd.region import IoUBalancedNegSampler
    c = libra_inputs.sampler_case(tag)
    z = np.load(inputs.golden_path('libra_sampler.npz'))
    s = IoUBalancedNegSampler(c['max_num'], c['pos_num'], num_bins=c['num_bins'], max_iou=c['max_iou'])
    for i, (lab, iou) in enumerate(zip(c['labels'], c['ious'])):
        kept = z['{}_labels_{}'.format(tag, i)] >= 0
        bins = [(lab == 0) & (iou >= np.float32(lo)) & (iou < np.float32(hi)) for lo, hi in zip(s.bin_lo, s.bin_hi)]
        counts = [int(b.sum()) for b in bins[::-1]]  # visiting order: highest bin first
        kp, takes = ops.iou_bin_quotas(int((lab > 0).sum()), counts, c['max_num'], c['pos_num'])
        assert kp == int((kept & (lab > 0)).sum())
        assert takes == [int((kept & b).sum()) for b in bins[::-1]]
        assert not (kept & (lab == 0) & (iou >= np.float32(c['max_iou']))).any()
