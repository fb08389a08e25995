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
import contextlib
import copy
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import inputs
import libra_inputs

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_THREADS = 8


def _build(over):
    from frcnn_amd.config import Config
    from frcnn_amd.builder import build_module
    cfg = Config.fromfile(os.path.join(REPO, 'pytorch-faster-rcnn_amd', 'configs', libra_inputs.WHOLE_LIBRA[1]))
    for k, v in over.items():
        cfg.test_cfg[k].update(v)
    return build_module(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)


def _to(x, dev):
    if torch.is_tensor(x):
        return x.to(dev)
    if isinstance(x, (list, tuple)):
        return type(x)(_to(v, dev) for v in x)
    return x


def _nchw(x):
    if torch.is_tensor(x):
        return x.contiguous()
    return type(x)(_nchw(v) for v in x) if isinstance(x, (list, tuple)) else x


@contextlib.contextmanager
def _fixture_threads():
    """PyTorch's CPU convolutions round differently with the thread count (their reduction is
    split by it): the CPU layers run with the generator's (gen_golden.main: 8)."""
    n = torch.get_num_threads()
    torch.set_num_threads(FIXTURE_THREADS)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _on_cpu(module, dev):
    """Run `module` (a PyTorch conv / FC stack) on a CPU copy of itself, outputs back on dev,
    as the fixture ran it: NCHW-contiguous inputs (PyTorch's CPU convolution rounds differently
    on the channels-last levels the HIP BFP writes) and the generator's thread count."""
    cpu = copy.deepcopy(module).cpu()

    def forward(*args):
        with torch.no_grad(), _fixture_threads():
            return _to(cpu(*[_nchw(_to(a, 'cpu')) for a in args]), dev)
    module.forward = forward


def _prepare(dev):
    from frcnn_amd import necks, set_sampler_mode
    _, _, over, shape = libra_inputs.WHOLE_LIBRA
    model = _build(over)
    sd = inputs.seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.train()
    img, boxes, labels, metas = inputs.ftrain_case(shape)
    x = torch.from_numpy(img)
    fpn, bfp = model.neck[0], model.neck[1]
    assert isinstance(bfp, necks.BFP)
    with torch.no_grad():
        with _fixture_threads():
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
    _on_cpu(model.rpn_head, dev)
    for h in model.rcnn_head:
        for name in ('shared_fcs', 'classifier', 'regressor'):
            if getattr(h, name, None) is not None:
                _on_cpu(getattr(h, name), dev)
    set_sampler_mode('numpy')
    return model, x.to(dev), [torch.from_numpy(b).to(dev) for b in boxes], \
        [torch.from_numpy(l).to(dev) for l in labels], metas


def test_libra_forward_train_losses_vs_reference(dev):
    ref = json.load(open(inputs.golden_path('whole_libra.json')))
    model, x, boxes, labels, metas = _prepare(dev)
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


def test_libra_forward_test_detections_vs_reference(dev):
    z = np.load(inputs.golden_path('whole_libra.npz'))
    model, x, _, _, metas = _prepare(dev)
    model.eval()
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


def test_libra_train_step_on_the_gpu_with_the_device_sampler(dev):
    from frcnn_amd import set_sampler_mode
    torch.manual_seed(11)
    model = _build({})
    model.init_weights()
    model = model.to(dev).train()
    img, boxes, labels, metas = inputs.ftrain_case(libra_inputs.WHOLE_LIBRA[3])
    x = torch.from_numpy(img).to(dev)
    gb = [torch.from_numpy(b).to(dev) for b in boxes]
    gl = [torch.from_numpy(l).to(dev) for l in labels]
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
