"""The VGG16 backbone on the HIP device: which entries its forward calls (inference, and a training
step with the first layers frozen), the trunk's numerics against float64, the fused forward
against the module forward, and configs/faster_rcnn_vgg16.py end to end.

The trunk input is (1, 3, 50, 70): grids 50x70, 25x35, 12x17, 6x8, 3x4, odd sizes at three depths.

Measured on MI355X (test_trunk_numerics' printed figures): max|y - y64| / max|y32 - y64| =
1.95 for the fused forward, 1.49 for the module forward (bound: 8; max|y32 - y64| = 3.6e-7 at
max|y64| = 0.66)."""
import functools
import os

import pytest
import torch

import support

pytestmark = pytest.mark.gpu

INPUT = (1, 3, 50, 70)


def _model(dev, **kw):
    from frcnn_amd.backbones import VGG16
    torch.manual_seed(21)
    m = VGG16(pretrained=False, **kw)
    m.init_weights()
    return m.to(dev)


@functools.lru_cache(maxsize=None)
def _trunk_case():
    """The CPU side, computed once: the input, the model's state, features(x) in f64 and in f32."""
    from frcnn_amd.backbones import VGG16
    torch.manual_seed(21)
    m = VGG16(pretrained=False)
    m.init_weights()
    x = torch.randn(*INPUT, generator=torch.Generator().manual_seed(22))
    with torch.no_grad():
        y32 = m.features(x)
        y64 = m.double().features(x.double())
    assert torch.isfinite(y32).all() and torch.isfinite(y64).all() and not torch.equal(y32.double(), y64)
    return x, y32, y64


def _count(names):
    return {n: names.count(n) for n in set(names)}


def test_dispatch_inference(dev, monkeypatch):
    model = _model(dev).eval()
    x = torch.randn(*INPUT, device=dev)
    spy = support.spy_entries(monkeypatch)
    with torch.no_grad():
        model(x)  # warm: allocator, the padded stem weight
        spy.clear()
        (y,) = support.no_sync(lambda: model(x))
    assert _count(spy.names) == {'frh_nchw_to_nhwc8': 1, 'frh_conv3x3_bias_act': 9, 'frh_conv3x3_bias_act_pool': 4}
    assert y.shape == (1, 512, 3, 4) and y.is_contiguous(memory_format=torch.channels_last)
    assert y.grad_fn is None and torch.isfinite(y).all()


def test_dispatch_training(dev, monkeypatch):
    """freeze_first_layers in a training step: layers 0, 2, 5, 7 take the fused entries (neither
    the image nor their weights need a gradient), the rest run the modules and train."""
    from frcnn_amd import ops
    model = _model(dev).train()
    x = torch.randn(*INPUT, device=dev)
    cl = torch.channels_last
    assert ops.vgg_conv_fused_ok(model.features[2], torch.zeros(1, 64, 50, 70, device=dev).contiguous(memory_format=cl),
                                 True)
    # its weight requires a gradient
    assert not ops.vgg_conv_fused_ok(model.features[10],
                                     torch.zeros(1, 128, 25, 35, device=dev).contiguous(memory_format=cl), False)
    spy = support.spy_entries(monkeypatch)
    (y,) = model(x)
    fused = [n for n in spy.names if n.startswith('frh_conv3x3') or n == 'frh_nchw_to_nhwc8']
    # the stem (its padding pass and its conv), conv2_1, and the two pooled layers conv1_2, conv2_2
    assert fused == ['frh_nchw_to_nhwc8', 'frh_conv3x3_bias_act', 'frh_conv3x3_bias_act_pool',
                     'frh_conv3x3_bias_act', 'frh_conv3x3_bias_act_pool']
    assert y.shape == (1, 512, 3, 4) and y.grad_fn is not None
    y.sum().backward()
    for i, layer in enumerate(model.features):
        for p in layer.parameters():
            if i < 10:
                assert p.grad is None
            else:
                assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0


def test_trunk_numerics(dev, monkeypatch):
    """max|y - y64| <= 8 max|y32 - y64| (the factor test_gpu_conv3x3.py grants a single layer), y
    the fused forward, y64 / y32 `features` in float64 / float32 on the CPU; and the module
    forward of the same model on the GPU within the same bar."""
    from frcnn_amd import ops
    x, y32, y64 = _trunk_case()
    model = _model(dev).eval()
    spy = support.spy_entries(monkeypatch)
    with torch.no_grad():
        (y,) = model(x.to(dev))
        assert spy.names.count('frh_conv3x3_bias_act_pool') == 4
        monkeypatch.setattr(ops, 'vgg_conv_fused_ok', lambda conv, x, pool: False)
        spy.clear()
        (ym,) = model(x.to(dev))
        assert not [n for n in spy.names if n.startswith('frh_conv3x3') or n == 'frh_nchw_to_nhwc8']
    err32 = float((y32.double() - y64).abs().max())
    err = float((y.cpu().double() - y64).abs().max())
    errm = float((ym.cpu().double() - y64).abs().max())
    print('max|y64|', float(y64.abs().max()), 'direct f32 err', err32, 'fused err / f32 err', err / err32,
          'modules err / f32 err', errm / err32)
    assert torch.isfinite(y).all() and y.shape == y64.shape
    assert err <= 8.0 * err32
    assert errm <= 8.0 * err32


def test_whole_config_train_and_test(dev):
    """configs/faster_rcnn_vgg16.py through the registry: forward_train (+ backward) and
    forward_test, the assertions of test_baseline_config_train_and_test at 224 x 320."""
    import bench
    from frcnn_amd import set_sampler_mode
    set_sampler_mode('device', seed=3)
    path = os.path.join(support.REPO, 'pytorch-faster-rcnn_amd', 'configs', 'faster_rcnn_vgg16.py')
    model, _ = bench.make_model(dev, seed=0, config=path)
    g = torch.Generator().manual_seed(1)
    imgs = torch.randn(2, 3, 224, 320, generator=g).to(dev)
    boxes = [torch.tensor([[20.0, 150.0], [30.0, 60.0], [140.0, 300.0], [200.0, 180.0]], device=dev),
             torch.tensor([[5.0, 100.0], [8.0, 40.0], [90.0, 250.0], [120.0, 210.0]], device=dev)]
    labels = [torch.tensor([3, 12], device=dev), torch.tensor([7, 20], device=dev)]
    metas = [{'img_shape': (224, 320, 3), 'pad_shape': (224, 320, 3), 'scale_factor': 1.0,
              'ori_shape': (224, 320, 3)} for _ in range(2)]
    losses = model.forward_train(imgs, boxes, labels, metas)
    assert len(losses) >= 2
    for k, v in losses.items():
        assert torch.isfinite(v).all(), k
    sum(losses.values()).backward()
    model.eval()
    with torch.no_grad():
        preds = model.forward_test(imgs, metas)
    assert len(preds) == 3 and len(preds[0]) == 2
    for b, s, l in zip(*preds):
        assert b.shape[0] == 4 and b.shape[1] == s.numel() == l.numel() <= 100
        if s.numel():
            assert (l >= 1).all() and (l <= 20).all()
