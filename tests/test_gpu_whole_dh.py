"""Whole-detector parity of the Double-Head R-CNN config against the REFERENCE's own outputs
(tests/golden/whole_dh.{json,npz}, made by gen_dh_golden.gen_whole from the reference's
configs/dh_rcnn_r50_fpn.py through its lib/builder.py), shaped like tests/test_gpu_whole_libra.py:
same seeded weights, the dense convs and FCs on the CPU as in the fixture (the head's fc_layer,
fc_classifier, conv_layer, reg_fc_layer and conv_regressor included), every detection
primitive between them on the HIP path, the numpy sampler mode.  Bars as in that file: losses
rel 2e-5; detections with labels exact, scores rel 1e-6, boxes rtol 2e-6 / atol 1e-4.

The head's BatchNorm2d is live: forward_train in train mode moves its running statistics, so the
detections are taken from a freshly loaded seeded state, as the generator takes them.

Plus the eval head alone on the device through the fused conv (error against the float64 CPU
module <= 8 x the error of the head's PyTorch-on-GPU path; measured on MI355X: cls 1.0 x, reg
1.4 x), and one forward_train + backward + forward_test of the config on the GPU with the
device sampler and random init."""
import copy
import json

import numpy as np
import pytest
import torch

import dh_inputs
import inputs
import support

pytestmark = pytest.mark.gpu
HEAD_DENSE = ('fc_layer', 'fc_classifier', 'conv_layer', 'reg_fc_layer', 'conv_regressor')


def _head_on_cpu(head, dev):
    """Run the head's dense layers (HEAD_DENSE: all of its forward) on a CPU copy of the head in
    the head's own mode, outputs back on dev, as the fixture ran them."""
    from frcnn_amd.heads.bbox_head import HeadOutputs
    cpu = copy.deepcopy(head).cpu()
    assert set(n.split('.')[0] for n, _ in cpu.named_parameters()) == set(HEAD_DENSE)

    def forward(rois):
        cpu.train(head.training)
        flat = getattr(rois, 'flat', None)
        x = flat if flat is not None else torch.cat(list(rois), 0)
        sizes = [r.shape[0] for r in rois]
        with torch.no_grad(), support.fixture_threads():
            cls_out, reg_out = cpu([x.cpu().contiguous()])[0].flat
        cls_out, reg_out = cls_out.to(dev), reg_out.to(dev)
        cls_outs, reg_outs = HeadOutputs(), HeadOutputs()
        off = 0
        for s in sizes:
            cls_outs.append(cls_out[off:off + s])
            reg_outs.append(reg_out[off:off + s])
            off += s
        cls_outs.flat = (cls_out, reg_out)
        return cls_outs, reg_outs
    head.forward = forward


def _prepare(dev, training):
    """The model with the freshly loaded seeded state, in the given mode."""
    from frcnn_amd import set_sampler_mode
    _, _, over, shape = dh_inputs.WHOLE_DH
    model = support.load_seeded(support.build_whole(dh_inputs.WHOLE_DH[1], over))
    model.train(training)
    img, boxes, labels, metas = inputs.ftrain_case(shape)
    x = torch.from_numpy(img)
    with torch.no_grad(), support.fixture_threads():
        feats = [f.to(dev) for f in model.neck(model.backbone(x))]  # CPU convs, as in the fixture
    model = model.to(dev)
    model.extract_feat = lambda img_data: feats
    support.on_cpu(model.rpn_head, dev)
    for h in model.rcnn_head:
        _head_on_cpu(h, dev)
    set_sampler_mode('numpy')
    return (model, x.to(dev)) + support.gts_on(dev, boxes, labels) + (metas,)


def test_dh_forward_train_losses_vs_reference(dev):
    ref = json.load(open(inputs.golden_path('whole_dh.json')))
    model, x, boxes, labels, metas = _prepare(dev, training=True)
    support.use_cpu_trunk(model, x)
    np.random.seed(inputs.FTRAIN_NP_SEED)
    with torch.no_grad():
        losses = model.forward_train(x, boxes, labels, metas)
    support.assert_losses_match(losses, ref['losses'], rel=2e-5)


def test_dh_forward_test_detections_vs_reference(dev):
    z = np.load(inputs.golden_path('whole_dh.npz'))
    model, x, _, _, metas = _prepare(dev, training=False)
    with torch.no_grad():
        dets = model.forward_test(x, metas)
    support.assert_detections_match(dets, z, score_rtol=1e-6, box_rtol=2e-6, box_atol=1e-4)


def test_dh_head_on_the_fused_path(dev, monkeypatch):
    """The eval head on the device: seeded weights, a seeded [37, 256, 7, 7] RoI batch.  Error
    against the float64 CPU module <= 8 x the error of the same head on PyTorch's GPU ops."""
    from frcnn_amd import ops
    from frcnn_amd.builder import build_module
    cfg = support.whole_config(dh_inputs.WHOLE_DH[1], {})
    head = build_module(cfg.model.rcnn_head[0])
    pre = 'rcnn_head.0.'  # the head's keys in the detector: the whole-model tests' seeded tensors
    sd = inputs.seeded_state({pre + k: tuple(v.shape) for k, v in head.state_dict().items()})
    head.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in sd.items()})
    head.eval()
    x = torch.from_numpy(dh_inputs.head_rois())
    with torch.no_grad():
        want_cls, want_reg = copy.deepcopy(head).double()([x.double()])[0].flat
    head = head.to(dev)
    xd = x.to(dev)
    spy = support.spy_entries(monkeypatch)
    with torch.no_grad():
        cls_out, reg_out = head([xd])[0].flat
    assert spy.names.count('frh_roi_conv3x3_bn_act') == 1
    monkeypatch.setattr(ops, 'roi_conv3x3_fused_ok', lambda conv, bn, x: False)
    spy.clear()
    with torch.no_grad():
        cls_pt, reg_pt = head([xd])[0].flat
    assert 'frh_roi_conv3x3_bn_act' not in spy.names
    for tag, got, pt, want in (('cls', cls_out, cls_pt, want_cls), ('reg', reg_out, reg_pt, want_reg)):
        err = float((got.cpu().double() - want).abs().max())
        err_pt = float((pt.cpu().double() - want).abs().max())
        print(tag, 'max err', err, 'PyTorch-on-GPU max err', err_pt, 'ratio', err / err_pt)
        assert torch.isfinite(got).all() and got.shape == want.shape
        assert err <= 8.0 * err_pt, (tag, err, err_pt)


def test_dh_train_step_on_the_gpu_with_the_device_sampler(dev, monkeypatch):
    from frcnn_amd import set_sampler_mode
    torch.manual_seed(11)
    model = support.build_whole(dh_inputs.WHOLE_DH[1], {})
    model.init_weights()
    model = model.to(dev).train()
    img, boxes, labels, metas = inputs.ftrain_case(dh_inputs.WHOLE_DH[3])
    x = torch.from_numpy(img).to(dev)
    gb, gl = support.gts_on(dev, boxes, labels)
    spy = support.spy_entries(monkeypatch)
    set_sampler_mode('device', seed=5)
    try:
        losses = model.forward_train(x, gb, gl, metas)
        total = sum(losses.values())
        total.backward()
    finally:
        set_sampler_mode('numpy')
    assert 'frh_roi_conv3x3_bn_act' not in spy.names  # the head's BN is training: batch statistics
    assert set(losses) == {'rpn_cls_loss', 'rpn_reg_loss', 'rcnn_0_cls_loss', 'rcnn_0_reg_loss'}
    for k, v in losses.items():
        assert torch.isfinite(v).item(), k
    missing = [n for n, p in model.named_parameters() if p.requires_grad and p.grad is None]
    assert not missing, missing
    assert all(torch.isfinite(p.grad).all().item() for p in model.parameters() if p.grad is not None)
    head = model.rcnn_head[0]
    for p in (head.conv_layer[0].weight, head.conv_layer[1].weight, head.conv_layer[1].bias):
        assert p.grad is not None and float(p.grad.abs().sum()) > 0
    spy.clear()
    model.eval()
    with torch.no_grad():
        dets = model.forward_test(x, metas)
    assert spy.names.count('frh_roi_conv3x3_bn_act') >= 1
    assert len(dets[0]) == 1 and dets[0][0].shape[0] == 4
