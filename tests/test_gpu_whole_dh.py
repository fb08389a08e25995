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
import contextlib
import copy
import json
import os

import numpy as np
import pytest
import torch

import dh_inputs
import inputs

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_THREADS = 8
HEAD_DENSE = ('fc_layer', 'fc_classifier', 'conv_layer', 'reg_fc_layer', 'conv_regressor')


def _build(over):
    from frcnn_amd.config import Config
    from frcnn_amd.builder import build_module
    cfg = Config.fromfile(os.path.join(REPO, 'pytorch-faster-rcnn_amd', 'configs', dh_inputs.WHOLE_DH[1]))
    for k, v in over.items():
        cfg.test_cfg[k].update(v)
    return build_module(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)


def _to(x, dev):
    if torch.is_tensor(x):
        return x.to(dev)
    if isinstance(x, (list, tuple)):
        return type(x)(_to(v, dev) for v in x)
    return x


@contextlib.contextmanager
def _fixture_threads():
    """PyTorch's CPU convolutions round differently with the thread count (their reduction is
    split by it): the CPU layers run with the generator's (gen_dh_golden.main: 8)."""
    n = torch.get_num_threads()
    torch.set_num_threads(FIXTURE_THREADS)
    try:
        yield
    finally:
        torch.set_num_threads(n)


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
        with torch.no_grad(), _fixture_threads():
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


def _nchw(x):
    if torch.is_tensor(x):
        return x.contiguous()
    return type(x)(_nchw(v) for v in x) if isinstance(x, (list, tuple)) else x


def _on_cpu(module, dev):
    """Run `module` (a PyTorch conv / FC stack) on a CPU copy of itself, outputs back on dev, as
    the fixture ran it: NCHW-contiguous inputs and the generator's thread count."""
    cpu = copy.deepcopy(module).cpu()

    def forward(*args):
        with torch.no_grad(), _fixture_threads():
            return _to(cpu(*[_nchw(_to(a, 'cpu')) for a in args]), dev)
    module.forward = forward


def _prepare(dev, training):
    """The model with the freshly loaded seeded state, in the given mode."""
    from frcnn_amd import set_sampler_mode
    _, _, over, shape = dh_inputs.WHOLE_DH
    model = _build(over)
    sd = inputs.seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.train(training)
    img, boxes, labels, metas = inputs.ftrain_case(shape)
    x = torch.from_numpy(img)
    with torch.no_grad(), _fixture_threads():
        feats = [f.to(dev) for f in model.neck(model.backbone(x))]  # CPU convs, as in the fixture
    model = model.to(dev)
    model.extract_feat = lambda img_data: feats
    _on_cpu(model.rpn_head, dev)
    for h in model.rcnn_head:
        _head_on_cpu(h, dev)
    set_sampler_mode('numpy')
    return model, x.to(dev), [torch.from_numpy(b).to(dev) for b in boxes], \
        [torch.from_numpy(l).to(dev) for l in labels], metas


def test_dh_forward_train_losses_vs_reference(dev):
    ref = json.load(open(inputs.golden_path('whole_dh.json')))
    model, x, boxes, labels, metas = _prepare(dev, training=True)
    feats = model.extract_feat(x)
    rpn = model.rpn_head(feats)

    class CpuTrunk(object):
        def matches(self, img_data):
            return True

        def __call__(self, img_data):
            return feats, rpn[0], rpn[1]
    model.graphed_trunk = CpuTrunk()
    np.random.seed(inputs.FTRAIN_NP_SEED)
    with torch.no_grad():
        losses = model.forward_train(x, boxes, labels, metas)
    assert set(losses) == set(ref['losses'])
    for k, v in ref['losses'].items():
        print(k, float(losses[k]), v)
    for k, v in ref['losses'].items():
        assert float(losses[k]) == pytest.approx(v, rel=2e-5), (k, float(losses[k]), v)


def test_dh_forward_test_detections_vs_reference(dev):
    z = np.load(inputs.golden_path('whole_dh.npz'))
    model, x, _, _, metas = _prepare(dev, training=False)
    with torch.no_grad():
        dets = model.forward_test(x, metas)
    boxes, scores, labels = dets[:3]
    assert len(boxes) == int(z['n'])
    for i in range(int(z['n'])):
        rb, rs, rl = z['boxes_{}'.format(i)], z['scores_{}'.format(i)], z['labels_{}'.format(i)]
        gb = boxes[i].t().cpu().numpy()
        gs, gl = scores[i].cpu().numpy(), labels[i].cpu().numpy()
        assert len(rs) > 0 and gs.shape == rs.shape, (gs.shape, rs.shape)
        np.testing.assert_array_equal(gl, rl)
        np.testing.assert_allclose(gs, rs, rtol=1e-6, atol=0)
        np.testing.assert_allclose(gb, rb, rtol=2e-6, atol=1e-4)


def _spy(monkeypatch):
    from frcnn_amd import ops
    names = []
    real = ops._call
    monkeypatch.setattr(ops, '_call', lambda name, *a: (names.append(name), real(name, *a))[1])
    return names


def test_dh_head_on_the_fused_path(dev, monkeypatch):
    """The eval head on the device: seeded weights, a seeded [37, 256, 7, 7] RoI batch.  Error
    against the float64 CPU module <= 8 x the error of the same head on PyTorch's GPU ops."""
    from frcnn_amd import ops
    from frcnn_amd.builder import build_module
    from frcnn_amd.config import Config
    cfg = Config.fromfile(os.path.join(REPO, 'pytorch-faster-rcnn_amd', 'configs', dh_inputs.WHOLE_DH[1]))
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
    names = _spy(monkeypatch)
    with torch.no_grad():
        cls_out, reg_out = head([xd])[0].flat
    assert names.count('frh_roi_conv3x3_bn_act') == 1
    monkeypatch.setattr(ops, 'roi_conv3x3_fused_ok', lambda conv, bn, x: False)
    del names[:]
    with torch.no_grad():
        cls_pt, reg_pt = head([xd])[0].flat
    assert 'frh_roi_conv3x3_bn_act' not in names
    for tag, got, pt, want in (('cls', cls_out, cls_pt, want_cls), ('reg', reg_out, reg_pt, want_reg)):
        err = float((got.cpu().double() - want).abs().max())
        err_pt = float((pt.cpu().double() - want).abs().max())
        print(tag, 'max err', err, 'PyTorch-on-GPU max err', err_pt, 'ratio', err / err_pt)
        assert torch.isfinite(got).all() and got.shape == want.shape
        assert err <= 8.0 * err_pt, (tag, err, err_pt)


def test_dh_train_step_on_the_gpu_with_the_device_sampler(dev, monkeypatch):
    from frcnn_amd import set_sampler_mode
    torch.manual_seed(11)
    model = _build({})
    model.init_weights()
    model = model.to(dev).train()
    img, boxes, labels, metas = inputs.ftrain_case(dh_inputs.WHOLE_DH[3])
    x = torch.from_numpy(img).to(dev)
    gb = [torch.from_numpy(b).to(dev) for b in boxes]
    gl = [torch.from_numpy(l).to(dev) for l in labels]
    names = _spy(monkeypatch)
    set_sampler_mode('device', seed=5)
    try:
        losses = model.forward_train(x, gb, gl, metas)
        total = sum(losses.values())
        total.backward()
    finally:
        set_sampler_mode('numpy')
    assert 'frh_roi_conv3x3_bn_act' not in names  # the head's BN is training: batch statistics
    assert set(losses) == {'rpn_cls_loss', 'rpn_reg_loss', 'rcnn_0_cls_loss', 'rcnn_0_reg_loss'}
    for k, v in losses.items():
        assert torch.isfinite(v).item(), k
    missing = [n for n, p in model.named_parameters() if p.requires_grad and p.grad is None]
    assert not missing, missing
    assert all(torch.isfinite(p.grad).all().item() for p in model.parameters() if p.grad is not None)
    head = model.rcnn_head[0]
    for p in (head.conv_layer[0].weight, head.conv_layer[1].weight, head.conv_layer[1].bias):
        assert p.grad is not None and float(p.grad.abs().sum()) > 0
    del names[:]
    model.eval()
    with torch.no_grad():
        dets = model.forward_test(x, metas)
    assert names.count('frh_roi_conv3x3_bn_act') >= 1
    assert len(dets[0]) == 1 and dets[0][0].shape[0] == 4
