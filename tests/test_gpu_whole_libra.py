"""Whole-detector parity of the Libra R-CNN config against the REFERENCE's own outputs
(tests/golden/whole_libra.{json,npz}, made by gen_libra_golden.gen_whole from the reference's
configs/libra_faster_rcnn_r50_fpn.py through its lib/builder.py), shaped like
tests/test_gpu_whole.py: same seeded weights, the dense convs and FCs on the CPU as in the
fixture, every detection primitive between them on the HIP path -- here including the BFP
neck (applied to the CPU FPN's outputs after moving them to the GPU), the IoU-balanced
sampler (numpy-RNG parity mode) and the balanced-L1 loss.  Bars as in that file: losses rel
2e-5; detections with labels exact, scores rel 1e-6, boxes rtol 2e-6 / atol 1e-4.

Plus one forward_train + backward + forward_test of the config on the GPU with the device
sampler and random init: finite losses, a gradient on every parameter that takes part."""
import hashlib
import json

import numpy as np
import pytest
import torch

import inputs
import libra_inputs
import support

pytestmark = pytest.mark.gpu


def _prepare(dev):
    from frcnn_amd import necks, set_sampler_mode
    _, _, over, shape = libra_inputs.WHOLE_LIBRA
    model = support.load_seeded(support.build_whole(libra_inputs.WHOLE_LIBRA[1], over))
    model.train()
    img, boxes, labels, metas = inputs.ftrain_case(shape)
    x = torch.from_numpy(img)
    fpn, bfp = model.neck[0], model.neck[1]
    assert isinstance(bfp, necks.BFP)
    with torch.no_grad():
        with support.fixture_threads():
            fpn_outs = fpn(model.backbone(x))  # CPU convs, as in the fixture
        feats = bfp([f.to(dev) for f in fpn_outs])  # the BFP neck on the HIP path
    assert all(f.is_cuda for f in feats)
    # printed, not asserted: the levels equal the reference's bit for bit only where this host's
    # CPU convolutions round as the fixture's did (the HIP BFP itself is pinned bit-exact in test_gpu_bfp)
    ref = json.load(open(inputs.golden_path('whole_libra.json')))
    sha = [hashlib.sha256(f.contiguous().cpu().numpy().tobytes()).hexdigest() for f in feats]
    print('neck outputs bit-identical to the reference per level:', [a == b for a, b in zip(sha, ref['feat_sha256'])])
    model = model.to(dev)
    model.extract_feat = lambda img_data: feats
    support.on_cpu(model.rpn_head, dev)
    for h in model.rcnn_head:
        for name in ('shared_fcs', 'classifier', 'regressor'):
            if getattr(h, name, None) is not None:
                support.on_cpu(getattr(h, name), dev)
    set_sampler_mode('numpy')
    return (model, x.to(dev)) + support.gts_on(dev, boxes, labels) + (metas,)


def test_libra_forward_train_losses_vs_reference(dev):
    ref = json.load(open(inputs.golden_path('whole_libra.json')))
    model, x, boxes, labels, metas = _prepare(dev)
    support.use_cpu_trunk(model, x)
    np.random.seed(inputs.FTRAIN_NP_SEED)
    with torch.no_grad():
        losses = model.forward_train(x, boxes, labels, metas)
    support.assert_losses_match(losses, ref['losses'], rel=2e-5)


def test_libra_forward_test_detections_vs_reference(dev):
    z = np.load(inputs.golden_path('whole_libra.npz'))
    model, x, _, _, metas = _prepare(dev)
    model.eval()
    with torch.no_grad():
        dets = model.forward_test(x, metas)
    support.assert_detections_match(dets, z, score_rtol=1e-6, box_rtol=2e-6, box_atol=1e-4)


def test_libra_train_step_on_the_gpu_with_the_device_sampler(dev):
    from frcnn_amd import set_sampler_mode
    torch.manual_seed(11)
    model = support.build_whole(libra_inputs.WHOLE_LIBRA[1], {})
    model.init_weights()
    model = model.to(dev).train()
    img, boxes, labels, metas = inputs.ftrain_case(libra_inputs.WHOLE_LIBRA[3])
    x = torch.from_numpy(img).to(dev)
    gb, gl = support.gts_on(dev, boxes, labels)
    set_sampler_mode('device', seed=5)
    try:
        losses = model.forward_train(x, gb, gl, metas)
        total = sum(losses.values())
        total.backward()
    finally:
        set_sampler_mode('numpy')
    assert set(losses) == {'rpn_cls_loss', 'rpn_reg_loss', 'rcnn_0_cls_loss', 'rcnn_0_reg_loss'}
    for k, v in losses.items():
        assert torch.isfinite(v).item(), k
    missing = [n for n, p in model.named_parameters() if p.requires_grad and p.grad is None]
    assert not missing, missing
    assert all(torch.isfinite(p.grad).all().item() for p in model.parameters() if p.grad is not None)
    # the gradient reached the FPN through the BFP's backward
    assert float(model.neck[0].lateral_convs[0].weight.grad.abs().sum()) > 0
    model.eval()
    with torch.no_grad():
        dets = model.forward_test(x, metas)
    assert len(dets[0]) == 1 and dets[0][0].shape[0] == 4
