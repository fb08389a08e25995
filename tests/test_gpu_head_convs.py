"""The one-stage heads' towers and output convs on the fused HIP entries at inference
(RetinaHead.forward, FCOSHead.forward through ops.head_convs_fused_ok): each tower layer one
frh_conv3x3_bias_act_levels call over the levels, each output group one frh_conv3x3_out_levels
launch; training, gradients and small heads keep the module expressions bit for bit.

Heads: 21 classes, 64 input and tower channels, two tower layers, PyTorch's default init; two
images, channels-last seeded-normal levels of (12, 20), (6, 10), (3, 5), (2, 3), (1, 2)."""
import pytest
import torch

import head_convs_cases as hc
import support

pytestmark = pytest.mark.gpu


def _head(mode, dev, **kw):
    return hc.make_head(mode, **kw).to(dev)


def _modules_only(monkeypatch):
    from frcnn_amd import ops
    monkeypatch.setattr(ops, 'head_convs_fused_ok', lambda *a, **k: False)


@pytest.mark.parametrize('mode', hc.MODES)
def test_fused_forward_matches_the_modules(dev, mode, monkeypatch):
    """Every tensor of the fused forward against the module path, within the tolerance
    test_fpn_and_rpn_head_match_the_unfused_path grants a Winograd layer stack; the modules'
    shapes and dtypes, channels-last."""
    head, xs = _head(mode, dev), hc.make_levels(dev)
    spy = support.spy_entries(monkeypatch)
    with torch.no_grad():
        got = head(xs)
        assert 'frh_conv3x3_out_levels' in spy.names
        with monkeypatch.context() as m:
            _modules_only(m)
            spy.clear()
            want = head(xs)
            assert not [n for n in spy.names if n.startswith('frh_conv3x3')]
    assert len(got) == len(want) == (2 if mode == 'retina' else 3)
    for g_l, w_l in zip(got, want):
        assert len(g_l) == len(w_l) == len(xs)
        for g, w in zip(g_l, w_l):
            assert g.shape == w.shape and g.dtype == w.dtype and g.grad_fn is None
            assert g.permute(0, 2, 3, 1).is_contiguous()
            print(mode, tuple(g.shape), 'max |diff|', float((g - w).abs().max()), 'max |ref|', float(w.abs().max()))
            torch.testing.assert_close(g, w, rtol=1e-3, atol=1e-3 * float(w.abs().max()))


@pytest.mark.parametrize('mode', hc.MODES)
def test_entry_counts(dev, mode, monkeypatch):
    """One fused forward: 2 towers x stacked_convs Winograd calls, two output-conv launches."""
    head, xs = _head(mode, dev), hc.make_levels(dev)
    names = support.spy_entries(monkeypatch).names
    with torch.no_grad():
        head(xs)
    assert names.count('frh_conv3x3_bias_act_levels') == 2 * head.stacked_convs
    assert names.count('frh_conv3x3_out_levels') == 2


@pytest.fixture
def deterministic_convs(monkeypatch):
    """MIOpen's default solver for the 64 -> 64 conv of the (6, 10) level does not repeat its own
    bits from call to call (measured: the module expressions alone differ between two runs at
    that level, and only there); under torch.backends.cudnn.deterministic they do.  The fallback
    tests compare the modules with themselves bit for bit, so they run under it."""
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)


def _assert_module_bits(head, xs, names):
    hc.module_forward(head, xs)  # MIOpen's first call of a shape may take another solver than the later ones
    del names[:]
    got = hc.flat(head(xs))
    assert not [n for n in names if n.startswith('frh_conv3x3')]
    for g, w in zip(got, hc.flat(hc.module_forward(head, xs))):
        assert g.shape == w.shape and g.stride() == w.stride() and torch.equal(g, w)
    return got


@pytest.mark.parametrize('mode', hc.MODES)
def test_parameters_that_need_a_gradient_keep_the_modules(dev, mode, monkeypatch, deterministic_convs):
    head, xs = _head(mode, dev), hc.make_levels(dev)
    names = support.spy_entries(monkeypatch).names
    with torch.enable_grad():
        for p in head.parameters():
            p.requires_grad_(False)
        last = (head.retina_reg if mode == 'retina' else head.fcos_center).bias
        for p in (head.cls_convs[0].weight, last) + (() if mode == 'retina' else (head.reg_coef,)):
            p.requires_grad_(True)
            got = _assert_module_bits(head, xs, names)
            assert any(t.grad_fn is not None for t in got)
            p.requires_grad_(False)


@pytest.mark.parametrize('mode', ('retina', 'gfl'))
def test_an_input_that_needs_a_gradient_keeps_the_modules(dev, mode, monkeypatch, deterministic_convs):
    head, xs = _head(mode, dev), hc.make_levels(dev)
    for p in head.parameters():
        p.requires_grad_(False)
    xs[2].requires_grad_(True)
    names = support.spy_entries(monkeypatch).names
    with torch.enable_grad():
        got = _assert_module_bits(head, xs, names)
        assert got[2].grad_fn is not None


@pytest.mark.parametrize('mode', hc.MODES)
def test_a_small_head_keeps_the_modules(dev, mode, monkeypatch, deterministic_convs):
    head, xs = _head(mode, dev, feat=8), hc.make_levels(dev, cin=8)
    names = support.spy_entries(monkeypatch).names
    with torch.no_grad():
        _assert_module_bits(head, xs, names)


@pytest.mark.parametrize('mode', ('retina', 'fcos', 'gfl'))
def test_graph_capture(dev, mode):
    """One fused forward captured after a warm-up and replayed equals the eager one bit for bit:
    the entries capture and keep no state."""
    head, xs = _head(mode, dev), hc.make_levels(dev)
    with torch.no_grad():
        eager = hc.flat(head(xs))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            head(xs)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = hc.flat(head(xs))
        for t in captured:
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
    for g, w in zip(captured, eager):
        assert torch.equal(g, w)


def test_predict_bboxes_end_to_end(dev, monkeypatch):
    """FCOS-ATSS predict_bboxes on the fused forward: finite boxes, the module path's shapes."""
    from frcnn_amd.config import ConfigDict
    head, xs = _head('atss', dev), hc.make_levels(dev)
    h, w = hc.LEVELS[0][0] * hc.STRIDES[0], hc.LEVELS[0][1] * hc.STRIDES[0]
    metas = [{'img_shape': (h, w, 3), 'pad_shape': (h, w, 3), 'scale_factor': 1.0, 'ori_shape': (h, w, 3)}] * 2
    cfg = ConfigDict(dict(pre_nms=1000, min_bbox_size=0, min_score=0.05, nms_iou=0.6, nms_type='strict', max_per_img=100))
    names = support.spy_entries(monkeypatch).names
    with torch.no_grad():
        got = head.predict_bboxes(xs, metas, cfg)
        assert names.count('frh_conv3x3_out_levels') == 2
        with monkeypatch.context() as m:
            _modules_only(m)
            want = head.predict_bboxes(xs, metas, cfg)
    for b in range(2):
        assert got[0][b].numel() > 0 and torch.isfinite(got[0][b]).all() and torch.isfinite(got[1][b]).all()
        for k in range(3):
            assert got[k][b].shape == want[k][b].shape and got[k][b].dtype == want[k][b].dtype
