"""CPU checks of the GFL head (no GPU): losses.gfl_head_losses_torch -- the torch restatement of
the reference's FCOSHead.calc_loss with QualityFocalLoss, DistributionFocalLoss and GIoULoss
(lib/heads/fcos_head.py:419-515), the numerics reference of the fused HIP loss -- against the
REFERENCE's own outputs (tests/golden/gfl_loss.npz, made by gen_gfl_golden.py): f64 losses and
gradients at rtol 1e-10, f32 losses at the project's loss bar (rtol 2e-5, atol 1e-6, as
tests/test_gpu_losses.py).  Plus the two points where the reference raises and the
restatement (like the kernel) does not -- a target in the top bin, no positive at all -- and
the new config: it builds, with the reference model's state_dict keys and shapes."""
import json
import os

import numpy as np
import pytest
import torch

import gfl_inputs
import inputs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = sorted(gfl_inputs.LOSS_CASES)


def _run(c, dtype, grad=False):
    from frcnn_amd.losses import gfl_head_losses_torch
    cls = torch.from_numpy(c['cls']).to(dtype).requires_grad_(grad)
    reg = torch.from_numpy(c['reg']).to(dtype).requires_grad_(grad)
    out = gfl_head_losses_torch(cls, reg, torch.from_numpy(c['labels']), torch.from_numpy(c['ltrb']).to(dtype),
                                **gfl_inputs.loss_kwargs(c))
    return cls, reg, out


@pytest.mark.parametrize('tag', TAGS)
def test_restatement_f64_losses_and_gradients_vs_reference(golden, tag):
    z = golden('gfl_loss.npz')
    c = gfl_inputs.loss_case(tag)
    cls, reg, (lc, ld, lb, npos) = _run(c, torch.float64, grad=True)
    assert int(npos) == int(z[tag + '_num_pos']) == int((c['labels'] > 0).sum())
    got = np.array([float(lc), float(ld), float(lb)])
    print(tag, got, z[tag + '_f64'])
    np.testing.assert_allclose(got, z[tag + '_f64'], rtol=1e-10, atol=0)
    for loss, name, wrt in ((lc, 'cls', 0), (ld, 'dfl', 1), (lb, 'bbox', 1)):
        g = torch.autograd.grad(loss, [cls, reg], retain_graph=True, allow_unused=True)
        other = g[1 - wrt]
        assert other is None or not other.any(), name
        ref = z['{}_g{}_{}'.format(tag, 'cls' if wrt == 0 else 'reg', name)]
        np.testing.assert_allclose(g[wrt].numpy(), ref, rtol=1e-10, atol=0, err_msg=name)


@pytest.mark.parametrize('tag', TAGS)
def test_restatement_f32_losses_vs_reference(golden, tag):
    z = golden('gfl_loss.npz')
    _, _, (lc, ld, lb, _) = _run(gfl_inputs.loss_case(tag), torch.float32)
    got = np.array([float(lc), float(ld), float(lb)])
    print(tag, got, z[tag + '_f32'])
    np.testing.assert_allclose(got, z[tag + '_f32'], rtol=2e-5, atol=1e-6)


def test_top_bin_keeps_the_left_term_only():
    """y exactly (bins-1)*stride: left == bins-1, the reference indexes bin `bins` (IndexError);
    the restatement's DFL term is -((left+1)*stride - y) * logsm[left] alone, every loss finite."""
    from frcnn_amd.losses import gfl_head_losses_torch, log_softmax_with_logits
    bins, stride = 16, 0.08
    rng = np.random.default_rng(5)
    m = 6
    cls = torch.from_numpy(rng.standard_normal((20, m)))
    reg = torch.from_numpy(rng.standard_normal((4 * bins, m)))
    labels = torch.tensor([0, 0, 7, 0, -1, 0])
    ltrb = torch.full((m, 4), 0.3, dtype=torch.float64)
    top = float(np.float32((bins - 1) * stride))  # the f32 clamp bound itself
    ltrb[2] = torch.tensor([top, 0.5 * stride, top, 3.25 * stride], dtype=torch.float64)
    lc, ld, lb, npos = gfl_head_losses_torch(cls, reg, labels, ltrb, bins, stride, reg_mean=0.0, reg_std=1.0,
                                             dfl_weight=1.0, dfl_avg_factor=1.0)
    assert int(npos) == 1 and all(bool(torch.isfinite(v)) for v in (lc, ld, lb))
    logsm = log_softmax_with_logits(reg[:, 2].view(bins, 4).t())  # [side, bin]
    f32 = lambda v: float(np.float32(v))  # the reference's bin bounds are f32 (long tensor * Python float)
    want = 0.0
    for side, (y, left) in enumerate(((top, 15), (0.5 * stride, 0), (top, 15), (3.25 * stride, 3))):
        want += (f32(np.float32(left + 1) * np.float32(stride)) - y) * float(logsm[side, left])
        if left + 1 < bins:
            want += (y - f32(np.float32(left) * np.float32(stride))) * float(logsm[side, left + 1])
    assert float(ld) == pytest.approx(-want, rel=1e-12)


def test_zero_positives_divide_by_one():
    from frcnn_amd.losses import generalized_focal_loss, gfl_head_losses_torch
    rng = np.random.default_rng(6)
    cls = torch.from_numpy(rng.standard_normal((20, 9)))
    reg = torch.from_numpy(rng.standard_normal((64, 9)))
    labels = torch.tensor([0, 0, -1, 0, 0, 0, -1, 0, 0])
    lc, ld, lb, npos = gfl_head_losses_torch(cls, reg, labels, torch.ones(9, 4, dtype=torch.float64), 16, 0.08)
    assert int(npos) == 0 and float(ld) == 0.0 and float(lb) == 0.0
    pred = cls[:, labels >= 0].t()
    assert float(lc) == pytest.approx(float(generalized_focal_loss(pred, torch.zeros_like(pred)).sum()), rel=1e-12)


def test_gfl_config_builds_with_the_reference_state_dict():
    from frcnn_amd.config import Config
    from frcnn_amd.builder import build_module
    from frcnn_amd.losses import DistributionFocalLoss, GIoULoss, QualityFocalLoss
    ref = json.load(open(inputs.golden_path('whole_gfl.json')))
    cfg = Config.fromfile(os.path.join(REPO, 'pytorch-faster-rcnn_amd', 'configs', gfl_inputs.WHOLE_GFL[1]))
    assert ref['config'] == 'configs/' + gfl_inputs.WHOLE_GFL[1]
    model = build_module(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert list(got) == list(ref['state_dict_shapes'])
    assert got == ref['state_dict_shapes']
    head = model.bbox_head
    assert head.use_qfl and head.use_dfl and not head.use_centerness
    assert isinstance(head.loss_cls, QualityFocalLoss) and isinstance(head.loss_bbox, GIoULoss)
    assert isinstance(head.loss_dfl, DistributionFocalLoss)
    w = gfl_inputs.WEIGHTS
    assert (head.loss_cls.loss_weight, head.loss_dfl.loss_weight, head.loss_bbox.loss_weight) == \
        (w['cls_weight'], w['dfl_weight'], w['bbox_weight'])
    assert (head.loss_dfl.cls_channels, head.loss_dfl.stride, head.loss_dfl.norm_prob) == (16, 0.08, False)
    assert (head.reg_std, head.reg_mean) == (gfl_inputs.REG_STD, gfl_inputs.REG_MEAN)


def test_head_uses_the_restatement_on_cpu_tensors():
    """FCOSHead.calc_loss_flat off the fused path (CPU tensors): the restatement's values under the
    reference's keys, in its order."""
    from frcnn_amd.heads.fcos_head import FCOSHead
    from frcnn_amd.losses import gfl_head_losses_torch
    c = gfl_inputs.loss_case('mixed')
    w = gfl_inputs.WEIGHTS
    head = FCOSHead(num_classes=21, in_channels=8, stacked_convs=1, feat_channels=8, reg_std=c['reg_std'],
                    reg_mean=c['reg_mean'], atss_cfg=dict(topk=9, scale=8),
                    loss_cls=dict(type='QualityFocalLoss', use_sigmoid=True, loss_weight=w['cls_weight']),
                    loss_bbox=dict(type='GIoULoss', loss_weight=w['bbox_weight']),
                    loss_dfl=dict(type='DistributionFocalLoss', cls_channels=16, stride=0.08, norm_prob=False,
                                  loss_weight=w['dfl_weight']))
    t = [torch.from_numpy(c[k]) for k in ('cls', 'reg', 'labels', 'ltrb')]
    m = c['M']
    out = head.calc_loss_flat(t[0], t[1], torch.zeros(1, m), t[2], t[3], torch.zeros(m))
    want = gfl_head_losses_torch(*t, **gfl_inputs.loss_kwargs(c))
    assert list(out) == ['cls_loss', 'dfl_loss', 'bbox_loss']
    for v, r in zip(out.values(), want[:3]):
        assert float(v) == float(r)
