"""The Guided Anchoring detector's training step with GuidedAnchor.hip_grad = True: the fixture
of tests/test_gpu_whole_ga.py (same seeded weights, same inputs, the dense convs on the CPU as the
fixture ran them, here with autograd on so that the gradient reaches the adaption layer), the
adaption layer of all five levels on the HIP device -- ONE frh_deform_conv3x3_act_levels call
forward, five frh_deform_conv3x3_bwd calls backward.  The losses equal the reference's
(tests/golden/whole_ga.json) at that file's bar, rel 2e-5; every gradient is finite and those of
adapt_layer.weight and offset_layer.weight are non-zero."""
import copy
import json

import numpy as np
import pytest
import torch

import inputs
import support
import test_gpu_whole_ga as whole

pytestmark = pytest.mark.gpu


def _on_cpu_with_grad(module, dev):
    """support.on_cpu with autograd left on: a CPU copy of the conv, NCHW-contiguous input under
    the fixture's thread count, the output back on dev.  Returns the copy (it holds the gradients)."""
    cpu = copy.deepcopy(module).cpu()

    def forward(x):
        with support.fixture_threads():
            return cpu(x.cpu().contiguous()).to(dev)
    module.forward = forward
    return cpu


def test_ga_train_step_with_hip_grad(dev, monkeypatch):
    from frcnn_amd import set_sampler_mode
    ref = json.load(open(inputs.golden_path('whole_ga.json')))
    model = whole._seeded()
    model.train(True)
    img, boxes, labels, metas = inputs.ftrain_case(whole.ga_inputs.WHOLE_SHAPE)
    x = torch.from_numpy(img)
    with torch.no_grad(), support.fixture_threads():
        feats = [f.to(dev) for f in model.neck(model.backbone(x))]
    model = model.to(dev)
    model.extract_feat = lambda img_data: feats
    head, ga = model.rpn_head, model.rpn_head.guided_anchor
    copies = [_on_cpu_with_grad(m, dev) for m in (ga.loc_layer, ga.shape_layer, head.conv, head.classifier,
                                                  head.regressor)]
    for h in model.rcnn_head:
        whole._rcnn_on_cpu(h, dev)
    set_sampler_mode('numpy')
    ga.hip_grad = True
    gt_boxes, gt_labels = support.gts_on(dev, boxes, labels)
    names = support.spy_entries(monkeypatch).names
    np.random.seed(inputs.FTRAIN_NP_SEED)
    losses = model.forward_train(x.to(dev), gt_boxes, gt_labels, metas)
    support.assert_losses_match(losses, ref['losses'], rel=2e-5)
    sum(v for v in losses.values() if v.requires_grad).backward()
    deform = [k for k in names if 'deform' in k]
    assert deform == ['frh_deform_conv3x3_act_levels'] + ['frh_deform_conv3x3_bwd'] * 5, deform
    params = list(model.parameters()) + [p for c in copies for p in c.parameters()]
    grads = [p.grad for p in params if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
    for w in (ga.adapt_layer.weight, ga.offset_layer.weight):
        assert w.grad is not None and bool((w.grad != 0).any())
