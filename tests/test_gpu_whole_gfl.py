"""Whole-detector parity of the GFL config against the REFERENCE's own outputs
(tests/golden/whole_gfl.{json,npz}, made by gen_gfl_golden.gen_whole from the reference's
configs/fcos_r50_fpn_atss_gfl.py through its lib/builder.py), shaped like
tests/test_gpu_whole.py for cfg5: the same seeded weights; the backbone, the FPN and the head's
convolutions on the CPU as in the fixture; ATSS targets, the fused GFL loss (csrc/gfl.hip), the
DFL decode and the multiclass NMS on the HIP path.  Bars: losses rel 2e-5 (that file's);
detections with labels exact and in the reference's order, scores rtol 1e-6, boxes rtol 2e-6
with atol = 4 * box_f32_err of the json -- the reference's own f32 expectation over the 1440 px
range is only good to box_f32_err (a few 1e-4 px), kernel and reference are two independent f32
evaluations, doubled for another expf; that file's 1e-4 px is tighter than the reference itself.

Plus one forward_train + backward + forward_test of the config on the GPU with random init:
finite losses, a gradient on every parameter that takes part (the centerness layer does not
under QFL), nonzero on the regression layer and on the per-level scales."""
import copy
import json

import numpy as np
import pytest
import torch

import gfl_inputs
import inputs
import support

pytestmark = pytest.mark.gpu


def _build():
    return support.build_whole(gfl_inputs.WHOLE_GFL[1], gfl_inputs.WHOLE_GFL[2])


def _prepare(dev):
    model = support.load_seeded(_build())
    model.train()
    img, boxes, labels, metas = inputs.ftrain_case(gfl_inputs.WHOLE_GFL[3])
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


def test_gfl_forward_train_losses_vs_reference(dev, monkeypatch):
    ref = json.load(open(inputs.golden_path('whole_gfl.json')))
    model, x, boxes, labels, metas, seen = _prepare(dev)
    count = support.count_calls(monkeypatch, ['atss_assign', 'gfl_losses'])
    with torch.no_grad():
        losses = model.forward_train(x, boxes, labels, metas)
    assert seen == [True] and count == {'atss_assign': 1, 'gfl_losses': 1}
    assert list(losses) == ['cls_loss', 'dfl_loss', 'bbox_loss']
    support.assert_losses_match(losses, ref['losses'], rel=2e-5, ordered=True)


def test_gfl_forward_test_detections_vs_reference(dev, monkeypatch):
    ref = json.load(open(inputs.golden_path('whole_gfl.json')))
    z = np.load(inputs.golden_path('whole_gfl.npz'))
    model, x, _, _, metas, seen = _prepare(dev)
    count = support.count_calls(monkeypatch, ['dfl_decode', 'multiclass_nms_batched'])
    model.eval()
    with torch.no_grad():
        dets = model.forward_test(x, metas)
    assert seen == [True] and count == {'dfl_decode': 5, 'multiclass_nms_batched': 1}
    assert int(z['n']) == 1
    atol = 4 * ref['box_f32_err']
    assert 0 < atol < 2e-3
    support.assert_detections_match(dets, z, score_rtol=1e-6, box_rtol=2e-6, box_atol=atol)


def test_gfl_train_step_on_the_gpu(dev):
    torch.manual_seed(13)
    model = _build()
    model.init_weights()
    model = model.to(dev).train()
    img, boxes, labels, metas = inputs.ftrain_case(gfl_inputs.WHOLE_GFL[3])
    x = torch.from_numpy(img).to(dev)
    gb, gl = support.gts_on(dev, boxes, labels)
    losses = model.forward_train(x, gb, gl, metas)
    sum(losses.values()).backward()
    assert list(losses) == ['cls_loss', 'dfl_loss', 'bbox_loss']
    for k, v in losses.items():
        assert torch.isfinite(v).item(), k
    # fcos_center takes no part under QFL (the reference's head carries the layer all the same)
    missing = [n for n, p in model.named_parameters()
               if p.requires_grad and p.grad is None and not n.startswith('bbox_head.fcos_center.')]
    assert not missing, missing
    assert all(torch.isfinite(p.grad).all().item() for p in model.parameters() if p.grad is not None)
    head = model.bbox_head
    assert float(head.fcos_reg.weight.grad.abs().sum()) > 0
    assert float(head.reg_coef.grad.abs().sum()) > 0
    assert float(head.fcos_cls.weight.grad.abs().sum()) > 0
    model.eval()
    with torch.no_grad():
        dets = model.forward_test(x, metas)
    assert len(dets[0]) == 1 and dets[0][0].shape[0] == 4
