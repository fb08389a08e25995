"""Whole-detector parity of the plain FCOS config against the REFERENCE's own outputs
(tests/golden/whole_fcos.{json,npz}, made by gen_fcos_golden.gen_whole from the reference's
configs/fcos_r50_fpn.py through its lib/builder.py), shaped like tests/test_gpu_whole_gfl.py: the
same seeded weights; the backbone, the FPN and the head's convolutions on the CPU as in the
fixture; the scale-range targets and the fused focal / GIoU / centerness loss (csrc/fcos.hip) and
the multiclass NMS on the HIP path.  Bars: losses rel 2e-5 (tests/test_gpu_whole.py's);
detections with labels exact and in the reference's order, scores rtol 1e-6, boxes rtol 2e-6 with
atol 1e-4 px (without DFL the decode is exp * reg_std around the cell centre: no expectation
error to allow for).

Plus one forward_train + backward + forward_test of the config on the GPU with random init:
finite losses, a gradient on every parameter, nonzero on the centerness layer, the regression
layer and the per-level scales."""
import copy
import json

import numpy as np
import pytest
import torch

import fcos_inputs
import inputs
import support

pytestmark = pytest.mark.gpu


def _build():
    return support.build_whole(fcos_inputs.WHOLE_FCOS[1], fcos_inputs.WHOLE_FCOS[2])


def _prepare(dev):
    model = support.load_seeded(_build())
    model.train()
    img, boxes, labels, metas = inputs.ftrain_case(fcos_inputs.WHOLE_FCOS[3])
    x = torch.from_numpy(img)
    with torch.no_grad(), support.fixture_threads():
        feats = model.extract_feat(x)
    cpu_head = copy.deepcopy(model.bbox_head)
    model = model.to(dev)
    dfeats = [f.to(dev) for f in feats]
    model.extract_feat = lambda img_data: dfeats
    seen = []

    def forward(xs):  # the head's convolutions on the CPU as in the fixture, their outputs on the GPU
        with torch.no_grad(), support.fixture_threads():
            out = support.to(cpu_head([f.cpu().contiguous() for f in xs]), dev)
        seen.append(all(t.is_cuda for level in out for t in level))
        return out
    model.bbox_head.forward = forward
    return (model, x.to(dev)) + support.gts_on(dev, boxes, labels) + (metas, seen)


def test_fcos_forward_train_losses_vs_reference(dev, monkeypatch):
    ref = json.load(open(inputs.golden_path('whole_fcos.json')))
    model, x, boxes, labels, metas, seen = _prepare(dev)
    count = support.count_calls(monkeypatch, ['fcos_assign', 'fcos_losses'])
    with torch.no_grad():
        losses = model.forward_train(x, boxes, labels, metas)
    assert seen == [True] and count == {'fcos_assign': 1, 'fcos_losses': 1}
    assert list(losses) == ['cls_loss', 'ctr_loss', 'bbox_loss']
    support.assert_losses_match(losses, ref['losses'], rel=2e-5, ordered=True)


def test_fcos_forward_test_detections_vs_reference(dev, monkeypatch):
    z = np.load(inputs.golden_path('whole_fcos.npz'))
    model, x, _, _, metas, seen = _prepare(dev)
    count = support.count_calls(monkeypatch, ['multiclass_nms_batched'])
    model.eval()
    with torch.no_grad():
        dets = model.forward_test(x, metas)
    assert seen == [True] and count == {'multiclass_nms_batched': 1}
    assert int(z['n']) == 1
    support.assert_detections_match(dets, z, score_rtol=1e-6, box_rtol=2e-6, box_atol=1e-4)


def test_fcos_train_step_on_the_gpu(dev):
    torch.manual_seed(13)
    model = _build()
    model.init_weights()
    model = model.to(dev).train()
    img, boxes, labels, metas = inputs.ftrain_case(fcos_inputs.WHOLE_FCOS[3])
    x = torch.from_numpy(img).to(dev)
    gb, gl = support.gts_on(dev, boxes, labels)
    losses = model.forward_train(x, gb, gl, metas)
    sum(losses.values()).backward()
    assert list(losses) == ['cls_loss', 'ctr_loss', 'bbox_loss']
    for k, v in losses.items():
        assert torch.isfinite(v).item(), k
    missing = [n for n, p in model.named_parameters() if p.requires_grad and p.grad is None]
    assert not missing, missing
    assert all(torch.isfinite(p.grad).all().item() for p in model.parameters() if p.grad is not None)
    head = model.bbox_head
    assert float(head.fcos_center.weight.grad.abs().sum()) > 0
    assert float(head.fcos_reg.weight.grad.abs().sum()) > 0
    assert float(head.reg_coef.grad.abs().sum()) > 0
    assert float(head.fcos_cls.weight.grad.abs().sum()) > 0
    model.eval()
    with torch.no_grad():
        dets = model.forward_test(x, metas)
    assert len(dets[0]) == 1 and dets[0][0].shape[0] == 4
