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
import contextlib
import copy
import json
import os

import numpy as np
import pytest
import torch

import fcos_inputs
import inputs

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_THREADS = 8


def _build():
    from frcnn_amd.config import Config
    from frcnn_amd.builder import build_module
    cfg = Config.fromfile(os.path.join(REPO, 'pytorch-faster-rcnn_amd', 'configs', fcos_inputs.WHOLE_FCOS[1]))
    cfg.test_cfg.update(fcos_inputs.WHOLE_FCOS[2])
    return build_module(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)


def _to(x, dev):
    if torch.is_tensor(x):
        return x.to(dev)
    if isinstance(x, (list, tuple)):
        return type(x)(_to(v, dev) for v in x)
    return x


@contextlib.contextmanager
def _fixture_threads():
    """PyTorch's CPU convolutions round differently with the thread count: the CPU layers run
    with the generator's (gen_fcos_golden.main: 8)."""
    n = torch.get_num_threads()
    torch.set_num_threads(FIXTURE_THREADS)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _prepare(dev):
    model = _build()
    sd = inputs.seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.train()
    img, boxes, labels, metas = inputs.ftrain_case(fcos_inputs.WHOLE_FCOS[3])
    x = torch.from_numpy(img)
    with torch.no_grad(), _fixture_threads():
        feats = model.extract_feat(x)
    cpu_head = copy.deepcopy(model.bbox_head)
    model = model.to(dev)
    dfeats = [f.to(dev) for f in feats]
    model.extract_feat = lambda img_data: dfeats
    seen = []

    def forward(xs):  # the head's convolutions on the CPU as in the fixture, their outputs on the GPU
        with torch.no_grad(), _fixture_threads():
            out = _to(cpu_head([f.cpu().contiguous() for f in xs]), dev)
        seen.append(all(t.is_cuda for level in out for t in level))
        return out
    model.bbox_head.forward = forward
    return model, x.to(dev), [torch.from_numpy(b).to(dev) for b in boxes], \
        [torch.from_numpy(l).to(dev) for l in labels], metas, seen


def _calls(monkeypatch, names):
    from frcnn_amd import ops
    count = {n: 0 for n in names}
    for n in names:
        orig = getattr(ops, n)

        def wrapped(*a, _orig=orig, _n=n, **kw):
            count[_n] += 1
            return _orig(*a, **kw)
        monkeypatch.setattr(ops, n, wrapped)
    return count


def test_fcos_forward_train_losses_vs_reference(dev, monkeypatch):
    ref = json.load(open(inputs.golden_path('whole_fcos.json')))
    model, x, boxes, labels, metas, seen = _prepare(dev)
    count = _calls(monkeypatch, ['fcos_assign', 'fcos_losses'])
    with torch.no_grad():
        losses = model.forward_train(x, boxes, labels, metas)
    assert seen == [True] and count == {'fcos_assign': 1, 'fcos_losses': 1}
    assert list(losses) == list(ref['losses']) == ['cls_loss', 'ctr_loss', 'bbox_loss']
    for k, v in ref['losses'].items():
        print(k, float(losses[k]), v)
    for k, v in ref['losses'].items():
        assert float(losses[k]) == pytest.approx(v, rel=2e-5), (k, float(losses[k]), v)


def test_fcos_forward_test_detections_vs_reference(dev, monkeypatch):
    z = np.load(inputs.golden_path('whole_fcos.npz'))
    model, x, _, _, metas, seen = _prepare(dev)
    count = _calls(monkeypatch, ['multiclass_nms_batched'])
    model.eval()
    with torch.no_grad():
        dets = model.forward_test(x, metas)
    assert seen == [True] and count == {'multiclass_nms_batched': 1}
    boxes, scores, labels = dets[:3]
    assert len(boxes) == int(z['n']) == 1
    for i in range(int(z['n'])):
        rb, rs, rl = z['boxes_{}'.format(i)], z['scores_{}'.format(i)], z['labels_{}'.format(i)]
        gb = boxes[i].t().cpu().numpy()
        gs, gl = scores[i].cpu().numpy(), labels[i].cpu().numpy()
        assert len(rs) > 0 and gs.shape == rs.shape, (gs.shape, rs.shape)
        np.testing.assert_array_equal(gl, rl)
        np.testing.assert_allclose(gs, rs, rtol=1e-6, atol=0)
        print('largest box difference', float(np.abs(gb - rb).max()))
        np.testing.assert_allclose(gb, rb, rtol=2e-6, atol=1e-4)


def test_fcos_train_step_on_the_gpu(dev):
    torch.manual_seed(13)
    model = _build()
    model.init_weights()
    model = model.to(dev).train()
    img, boxes, labels, metas = inputs.ftrain_case(fcos_inputs.WHOLE_FCOS[3])
    x = torch.from_numpy(img).to(dev)
    gb = [torch.from_numpy(b).to(dev) for b in boxes]
    gl = [torch.from_numpy(l).to(dev) for l in labels]
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
