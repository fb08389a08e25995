"""CPU checks of plain FCOS (no GPU), against the REFERENCE's own outputs (tests/golden/
fcos_targets.npz, fcos_loss.npz, whole_fcos.json, made by gen_fcos_golden.py):
losses.fcos_head_losses_torch -- the torch restatement of the reference's FCOSHead.calc_loss
without GFL (lib/heads/fcos_head.py:419-515), the numerics reference of the fused HIP loss -- in
f64 at rtol 1e-10, in f32 at the project's loss bar (rtol 2e-5, atol 1e-6, as
tests/test_gpu_losses.py); the head's torch single_image_targets and the numpy restatement the
GPU tests use for equal areas, both exactly; and the new config: it builds, with the reference
model's state_dict keys and shapes.  These pin the semantics the kernels of csrc/fcos.hip are
held to in tests/test_gpu_fcos.py."""
import json
import os

import numpy as np
import pytest
import torch

import fcos_inputs
import inputs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_TAGS = list(fcos_inputs.REFERENCE_LOSS_CASES)


def _head(thr=None, num_classes=21, reg_std=fcos_inputs.REG_STD):
    from frcnn_amd.heads.fcos_head import FCOSHead
    w = fcos_inputs.WEIGHTS
    head = FCOSHead(num_classes=num_classes, in_channels=8, stacked_convs=1, feat_channels=8,
                    strides=list(fcos_inputs.STRIDES), reg_std=reg_std, reg_mean=fcos_inputs.REG_MEAN,
                    loss_cls=dict(type='FocalLoss', use_sigmoid=True, loss_weight=w['cls_weight']),
                    loss_bbox=dict(type='GIoULoss', loss_weight=w['bbox_weight']),
                    loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=w['ctr_weight']))
    if thr is not None:
        head.level_scale_thr = list(thr)
    return head


def _run(c, dtype, grad=False):
    from frcnn_amd.losses import fcos_head_losses_torch
    outs = [torch.from_numpy(c[k]).to(dtype).requires_grad_(grad) for k in ('cls', 'reg', 'ctr')]
    res = fcos_head_losses_torch(*outs, torch.from_numpy(c['labels']), torch.from_numpy(c['ltrb']).to(dtype),
                                 torch.from_numpy(c['ctr_t']).to(dtype), **fcos_inputs.loss_kwargs(c))
    return outs, res


def test_loss_cases_cover_the_sizes():
    ms = {t: fcos_inputs.loss_case(t)['M'] for t in fcos_inputs.LOSS_CASES}
    assert {1, 255, 257, 2 * 3412} <= set(ms.values())
    assert {c['C'] for c in fcos_inputs.LOSS_CASES.values()} == {1, 3, 20}
    assert not (fcos_inputs.loss_case('no_pos')['labels'] > 0).any()
    assert (fcos_inputs.loss_case('ignored')['labels'] == -1).all()
    c = fcos_inputs.loss_case('tie')
    pos = c['labels'] > 0
    y = c['ltrb'] / np.float32(c['reg_std'])
    tied = (c['reg'].T == y) & pos[:, None]
    assert tied[:, 0].sum() >= 10 and tied.all(1).sum() >= 5 and (pos & ~tied.any(1)).sum() >= 10
    assert np.array_equal(y.astype(np.float64), c['ltrb'].astype(np.float64) / c['reg_std'])  # a tie in f64 too


@pytest.mark.parametrize('tag', REF_TAGS)
def test_restatement_f64_losses_and_gradients_vs_reference(golden, tag):
    z = golden('fcos_loss.npz')
    c = fcos_inputs.loss_case(tag)
    outs, (lc, lb, lt, npos) = _run(c, torch.float64, grad=True)
    assert int(npos) == int(z[tag + '_num_pos']) == int((c['labels'] > 0).sum()) > 0
    got = np.array([float(lc), float(lb), float(lt)])
    print(tag, got, z[tag + '_f64'])
    np.testing.assert_allclose(got, z[tag + '_f64'], rtol=1e-10, atol=0)
    for i, (loss, key) in enumerate(zip((lc, lb, lt), ('gcls', 'greg', 'gctr'))):
        g = torch.autograd.grad(loss, outs, retain_graph=True, allow_unused=True)
        for j, other in enumerate(g):
            assert j == i or other is None or not other.any(), (key, j)
        ref = z['{}_{}'.format(tag, key)]
        np.testing.assert_allclose(g[i].numpy(), ref, rtol=1e-10, atol=1e-300, err_msg=key)


@pytest.mark.parametrize('tag', REF_TAGS)
def test_restatement_f32_losses_vs_reference(golden, tag):
    z = golden('fcos_loss.npz')
    _, (lc, lb, lt, _) = _run(fcos_inputs.loss_case(tag), torch.float32)
    got = np.array([float(lc), float(lb), float(lt)])
    print(tag, got, z[tag + '_f32'])
    np.testing.assert_allclose(got, z[tag + '_f32'], rtol=2e-5, atol=1e-6)


def test_zero_positives_divide_by_one():
    """Where the reference divides by a zero positive count: the sums over max(num_pos, 1)."""
    from frcnn_amd.losses import sigmoid_focal_loss
    c = fcos_inputs.loss_case('no_pos')
    _, (lc, lb, lt, npos) = _run(c, torch.float64)
    assert int(npos) == 0 and float(lb) == 0.0 and float(lt) == 0.0
    keep = torch.from_numpy(c['labels'] >= 0)
    want = sigmoid_focal_loss(torch.from_numpy(c['cls']).double()[:, keep].t(), torch.from_numpy(c['labels'])[keep])
    assert float(lc) == pytest.approx(float(want), rel=1e-12) and float(lc) > 0
    _, res = _run(fcos_inputs.loss_case('ignored'), torch.float64)
    assert [float(v) for v in res] == [0.0, 0.0, 0.0, 0.0]


def _torch_targets(tag):
    boxes, labels, thr = fcos_inputs.TARGET_CASES[tag]
    head = _head(thr)
    outs = [torch.from_numpy(x) for x in fcos_inputs.level_outputs()]
    res = []
    for b, meta in enumerate(fcos_inputs.img_metas()):
        cls, reg, ctr = head.single_image_targets(outs, outs, outs, torch.from_numpy(boxes[b]),
                                                  torch.from_numpy(labels[b]), meta, None)
        assert [tuple(x.shape) for x in cls] == [g + (1,) for g in fcos_inputs.GRIDS]
        assert [tuple(x.shape) for x in reg] == [g + (4,) for g in fcos_inputs.GRIDS]
        res.append((torch.cat([x.reshape(-1) for x in cls]).numpy(), torch.cat([x.reshape(-1, 4) for x in reg]).numpy(),
                    torch.cat([x.reshape(-1) for x in ctr]).numpy()))
    return res


@pytest.mark.parametrize('tag', fcos_inputs.REFERENCE_TARGET_CASES)
def test_torch_single_image_targets_vs_reference(golden, tag):
    """Labels and ltrb exactly.  The centerness to one ulp: its divisions and its product round
    correctly everywhere, but torch's CPU vector sqrt is only faithfully rounded and which values it
    rounds the other way depends on the CPU, so this torch loop may differ from
    the fixture -- whose values are the correctly rounded ones, as the generator asserts -- by the
    last bit of the square root and by nothing else."""
    z = golden('fcos_targets.npz')
    for b, (cls, reg, ctr) in enumerate(_torch_targets(tag)):
        np.testing.assert_array_equal(cls, z['{}_cls_{}'.format(tag, b)])
        np.testing.assert_array_equal(reg, z['{}_reg_{}'.format(tag, b)])
        ref = z['{}_ctr_{}'.format(tag, b)]
        np.testing.assert_array_equal(ctr[cls <= 0], ref[cls <= 0])
        np.testing.assert_array_max_ulp(ctr[cls > 0], ref[cls > 0], maxulp=1)


@pytest.mark.parametrize('tag', fcos_inputs.REFERENCE_TARGET_CASES)
def test_numpy_restatement_vs_reference(golden, tag):
    """The arg-min restatement the GPU tests check equal areas with reproduces the reference where
    the areas are distinct."""
    from test_gpu_fcos import numpy_targets
    z = golden('fcos_targets.npz')
    boxes, labels, thr = fcos_inputs.TARGET_CASES[tag]
    for b, shape in enumerate(fcos_inputs.IMG_SHAPES):
        cls, reg, ctr = numpy_targets(boxes[b], labels[b], shape, thr)
        np.testing.assert_array_equal(cls, z['{}_cls_{}'.format(tag, b)])
        np.testing.assert_array_equal(reg, z['{}_reg_{}'.format(tag, b)])
        np.testing.assert_array_equal(ctr, z['{}_ctr_{}'.format(tag, b)])


def test_target_fixtures_hold_the_planted_edges(golden):
    """What the cases were built for is in the reference's outputs."""
    z = golden('fcos_targets.npz')
    off = np.cumsum([0] + [h * w for h, w in fcos_inputs.GRIDS])
    cell = lambda lv, y, x: off[lv] + y * fcos_inputs.GRIDS[lv][1] + x
    cls, reg, ctr = z['a_cls_0'], z['a_reg_0'], z['a_ctr_0']
    # the painted area: rows <= 38 and columns <= 62 on level 0 (37.5 -> 38, 62.5 -> 62), columns <= 16
    # on level 2 (15.625 -> 16, the grid has 16)
    c0 = cls[:off[1]].reshape(40, 64)
    assert (c0[39] == -1).all() and (c0[:39, 63] == -1).all() and (c0[:39, :63] >= 0).all()
    assert (cls[off[2]:off[3]].reshape(10, 16)[:, 15] >= 0).all()
    assert (z['a_cls_1'] == 0).all() and (z['a_ctr_1'] == 0).all() and (z['a_reg_1'] == -1).all()
    assert cls[cell(0, 10, 12)] == 12                     # (100, 84): inside both nested gts, the smaller wins
    assert cls[cell(1, 3, 6)] == 3                        # level 1, (104, 56): the outer one alone
    assert cls[cell(0, 25, 25)] == 0 and cls[cell(0, 25, 26)] == 5   # x = 204 is gt 3's own edge: ltrb_l == 0
    assert cls[cell(0, 20, 45)] == 0                      # (364, 164): max(ltrb) == 64 is not level 0's
    assert cls[cell(1, 14, 8)] == 1 and reg[cell(1, 14, 8)].max() == 64.0   # (136, 232): and it is level 1's
    assert ((cls > 0) == (ctr > 0)).all() and (reg[cls > 0] > 0).all() and (reg[cls <= 0] == -1).all()
    assert [int((cls[off[i]:off[i + 1]] > 0).sum()) > 0 for i in range(5)] == [True, True, True, True, False]
    cls_b, reg_b, ctr_b = z['b_cls_0'], z['b_reg_0'], z['b_ctr_0']
    assert (cls_b[off[4]:] > 0).any()                     # the small thresholds reach the last level
    zero = (cls_b == 0) & (reg_b[:, 0] > 0)               # label 0: cls 0, the ltrb written, centerness as painted
    assert zero.sum() > 0 and (ctr_b[zero] == 0).all()


def test_fcos_config_builds_with_the_reference_state_dict():
    from frcnn_amd.config import Config
    from frcnn_amd.builder import build_module
    from frcnn_amd.losses import CrossEntropyLoss, FocalLoss, GIoULoss
    ref = json.load(open(inputs.golden_path('whole_fcos.json')))
    cfg = Config.fromfile(os.path.join(REPO, 'pytorch-faster-rcnn_amd', 'configs', fcos_inputs.WHOLE_FCOS[1]))
    assert ref['config'] == 'configs/' + fcos_inputs.WHOLE_FCOS[1]
    model = build_module(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert list(got) == list(ref['state_dict_shapes'])
    assert got == ref['state_dict_shapes']
    head = model.bbox_head
    assert not head.use_atss and not head.use_gfl and head.use_centerness
    assert head.level_scale_thr == fcos_inputs.REAL_THR and head.strides == fcos_inputs.STRIDES
    assert isinstance(head.loss_cls, FocalLoss) and isinstance(head.loss_bbox, GIoULoss)
    assert isinstance(head.loss_centerness, CrossEntropyLoss) and head.loss_centerness.use_sigmoid
    w = fcos_inputs.WEIGHTS
    assert (head.loss_cls.loss_weight, head.loss_bbox.loss_weight, head.loss_centerness.loss_weight) == \
        (w['cls_weight'], w['bbox_weight'], w['ctr_weight'])
    assert (head.loss_cls.alpha, head.loss_cls.gamma) == (w['alpha'], w['gamma'])
    assert (head.reg_std, head.reg_mean) == (fcos_inputs.REG_STD, fcos_inputs.REG_MEAN)
    assert head.reg_coef.requires_grad and tuple(head.reg_coef.shape) == (5,)
    assert dict(cfg.optimizer) == dict(type='SGD', lr=0.00125, momentum=0.9, weight_decay=0.0001)
    assert cfg.test_cfg['nms_type'] == 'strict' and cfg.test_cfg['nms_iou'] == 0.6


def test_head_uses_the_restatement_on_cpu_tensors():
    """FCOSHead.calc_loss_flat on CPU tensors: the restatement's values under the reference's keys,
    in its order; and reg_mean > 0 stays refused."""
    from frcnn_amd.losses import fcos_head_losses_torch
    c = fcos_inputs.loss_case('m255')
    head = _head(num_classes=c['C'] + 1, reg_std=c['reg_std'])
    t = [torch.from_numpy(c[k]) for k in ('cls', 'reg', 'ctr', 'labels', 'ltrb', 'ctr_t')]
    out = head.calc_loss_flat(t[0], t[1], t[2].view(1, -1), *t[3:])
    want = fcos_head_losses_torch(*t, **fcos_inputs.loss_kwargs(c))
    assert list(out) == ['cls_loss', 'ctr_loss', 'bbox_loss']
    assert [float(out[k]) for k in ('cls_loss', 'bbox_loss', 'ctr_loss')] == [float(v) for v in want[:3]]
    head.reg_mean = 1.0
    with pytest.raises(AssertionError, match='reg_mean'):
        head.calc_loss_flat(t[0], t[1], t[2].view(1, -1), *t[3:])
