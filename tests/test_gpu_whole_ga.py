"""Whole-detector parity of the Guided Anchoring config (configs/ga_faster_rcnn_r50_fpn.py, the
project's own: the reference ships none) against the REFERENCE's own outputs
(tests/golden/whole_ga.{json,npz}, made by gen_ga_golden.gen_whole from the reference's
CascadeRCNN / GARPNHead under the four repairs written out there), shaped like
tests/test_gpu_whole_dh.py: same seeded weights (ga_inputs.whole_state), the dense convs and FCs
on the CPU as in the fixture (the RPN head's forward included: its deformable convolution is then
the same torch restatement the fixture ran), every detection primitive between them on the HIP
path -- the one-launch GA targets, the samplers in numpy mode, the assigner, the box codecs, NMS --
Bars as in that file: losses rel 2e-5; detections with labels exact, scores rel 1e-6, boxes rtol
2e-6 / atol 1e-4.

The fixture's generator asserts that every cut of the proposal path -- loc_filter_thr, the top-k
boundaries and the deciding NMS IoUs -- is more than 1e-4 relative away from flipping
(whole_ga.json cut_margins) and that no two candidate scores of a level are within 2e-6 relative,
so the proposals are compared in order.

Plus the eval model wholly on the device: the adaption layer of all five levels is ONE
frh_deform_conv3x3_act_levels call, and its detections are finite."""
import copy
import json

import numpy as np
import pytest
import torch

import ga_inputs
import inputs
import support

pytestmark = pytest.mark.gpu


def _build():
    return support.build_whole(ga_inputs.WHOLE_CONFIG, ga_inputs.WHOLE_TEST_OVERRIDES)


def _rcnn_on_cpu(head, dev):
    from frcnn_amd.heads.bbox_head import HeadOutputs
    cpu = copy.deepcopy(head).cpu()

    def forward(rois):
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


def _seeded():
    return support.load_seeded(_build(), state=ga_inputs.whole_state)


def _prepare(dev, training):
    from frcnn_amd import set_sampler_mode
    model = _seeded()
    model.train(training)
    img, boxes, labels, metas = inputs.ftrain_case(ga_inputs.WHOLE_SHAPE)
    x = torch.from_numpy(img)
    with torch.no_grad(), support.fixture_threads():
        feats = [f.to(dev) for f in model.neck(model.backbone(x))]  # CPU convs, as in the fixture
    model = model.to(dev)
    model.extract_feat = lambda img_data: feats
    support.on_cpu(model.rpn_head, dev)
    for h in model.rcnn_head:
        _rcnn_on_cpu(h, dev)
    set_sampler_mode('numpy')
    return (model, x.to(dev)) + support.gts_on(dev, boxes, labels) + (metas,)


def test_config_builds_with_the_reference_keys():
    ref = json.load(open(inputs.golden_path('whole_ga.json')))
    model = _build()
    assert type(model.rpn_head).__name__ == 'GARPNHead'
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == ref['state_dict_shapes']


def test_ga_forward_train_losses_vs_reference(dev):
    ref = json.load(open(inputs.golden_path('whole_ga.json')))
    model, x, boxes, labels, metas = _prepare(dev, training=True)
    np.random.seed(inputs.FTRAIN_NP_SEED)
    with torch.no_grad():
        losses = model.forward_train(x, boxes, labels, metas)
    support.assert_losses_match(losses, ref['losses'], rel=2e-5)


def test_ga_forward_test_detections_vs_reference(dev):
    z = np.load(inputs.golden_path('whole_ga.npz'))
    model, x, _, _, metas = _prepare(dev, training=False)
    with torch.no_grad():
        props = model.rpn_head.predict_bboxes(model.extract_feat(x), metas, model.test_cfg.rpn)
        dets = model.forward_test(x, metas)
    # the proposals, scores and boxes, in order
    np.testing.assert_allclose(props[1][0].cpu().numpy(), z['prop_scores_0'], rtol=1e-6, atol=0)
    np.testing.assert_allclose(props[0][0].cpu().numpy(), z['props_0'], rtol=2e-6, atol=1e-4)
    support.assert_detections_match(dets, z, score_rtol=1e-6, box_rtol=2e-6, box_atol=1e-4)


def test_eval_forward_on_the_device_launches_the_levels_entry_once(dev, monkeypatch):
    model = _seeded().to(dev).eval()
    img, _, _, metas = inputs.ftrain_case(ga_inputs.WHOLE_SHAPE)
    names = support.spy_entries(monkeypatch).names
    with torch.no_grad():
        dets = model.forward_test(torch.from_numpy(img).to(dev), metas)
    assert names.count('frh_deform_conv3x3_act_levels') == 1 and 'frh_deform_conv3x3_act' not in names
    assert len(dets[0]) == 1 and dets[1][0].numel() > 0 and bool(torch.isfinite(dets[0][0]).all())
