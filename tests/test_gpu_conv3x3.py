"""frh_conv3x3_bias_act: the FPN output convs and the RPN head's shared conv (3x3, stride 1,
padding 1, channels-last f32) as Winograd F(2x2, 3x3) on the f32 MFMA with the bias (+ ReLU)
epilogue on the accumulators (csrc/conv3x3_wino_kernels.h), its multi-level form, the Python
dispatch (ops.conv3x3_bias_act, ops.conv3x3_bias_act_levels) and the FPN / RPNHead that call it.

Shapes are (n, cin, cout, h, w).  A workgroup owns 8 x 8 tiles (16 x 16 outputs) x 64 output
channels and walks cin in chunks of 8; cin % 8 == 0, cout % 64 == 0.

Measured on MI355X (test_accuracy_against_float64's printed ratios over the four shapes and
flag pairs): max error / bound 3.6e-4 .. 1.0e-2; max error / the CPU direct f32 conv's max error
0.55 .. 2.5 (bound: 8)."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import support

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 8, 64, 3, 5),       # smaller than one tile block, odd h and w, one cin chunk
    (2, 64, 64, 19, 32),    # P5's grid: half-empty last tile row, batch stride
    (2, 256, 128, 10, 16),  # the workload's full cin loop, two cout blocks
    (1, 32, 192, 17, 34),   # ragged tile block on both sides, three cout blocks
]
FLAGS = [(b, r) for b in (False, True) for r in (False, True)]

@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs (CPU f32) and the references of one shape, computed once."""
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(3000 + cin + 7 * cout + h * w)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g)
    bias = torch.randn(cout, generator=g)
    y64 = F.conv2d(x.double(), wt.double(), None, padding=1)
    y32 = F.conv2d(x, wt, None, padding=1)
    return dict(x=x, w=wt, bias=bias, y64=y64, y32=y32, mag=support.wino_magnitude(x, wt))


@functools.lru_cache(maxsize=None)
def _on_dev(shape, dev):
    c = _case(shape)
    cl = torch.channels_last
    return dict(x=c['x'].to(dev).contiguous(memory_format=cl), w=c['w'].to(dev).contiguous(memory_format=cl),
                bias=c['bias'].to(dev))


def _fused(x, w, bias, relu):
    """frh_conv3x3_bias_act on x (any NCHW-shaped view with channel stride 1) and a channels-last w."""
    from frcnn_amd import _lib
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    assert x.stride(1) == 1 and w.is_contiguous(memory_format=torch.channels_last)
    y = torch.empty(n, cout, h, wd, dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    ws = torch.empty(16 * cin * cout, dtype=torch.float32, device=x.device)
    p = _lib.ptr
    _lib.call('frh_conv3x3_bias_act', p(x), p(w), p(bias), p(y), p(ws), n, cin, cout, h, wd, x.stride(0),
              x.stride(2), x.stride(3), int(relu), _lib.stream_of(x))
    return y


def _fused_case(d, bias, relu):
    return _fused(d['x'], d['w'], d['bias'] if bias else None, relu)


@pytest.mark.parametrize('relu', (False, True))
@pytest.mark.parametrize('shape', SHAPES)
def test_exact_borders(dev, shape, relu):
    """x = 1, w = 1, no bias: every Winograd intermediate is a multiple of 1/4 below 2^24, so the
    result is exactly cin x (number of valid taps): 4, 6 or 9 x cin."""
    n, cin, cout, h, w = shape
    cl = torch.channels_last
    x = torch.ones(n, cin, h, w, device=dev).contiguous(memory_format=cl)
    wt = torch.ones(cout, cin, 3, 3, device=dev).contiguous(memory_format=cl)
    taps = F.conv2d(torch.ones(1, 1, h, w), torch.ones(1, 1, 3, 3), padding=1)
    want = (taps * cin).expand(n, cout, h, w)
    assert set(taps.unique().tolist()) <= {4.0, 6.0, 9.0}
    assert torch.equal(_fused(x, wt, None, relu).cpu(), want)


@pytest.mark.parametrize('bias,relu', FLAGS)
@pytest.mark.parametrize('shape', SHAPES)
def test_accuracy_against_float64(dev, shape, bias, relu):
    """|y - y64| <= 2 (cin + 16) 2^-24 magW for every element, magW the forward bound of the
    algorithm's own sums (cin multiply-adds plus 4 roundings in each of the three transforms,
    plus the bias); and max|y - y64| <= 8 max|y32 - y64|, y32 torch's CPU f32 direct conv."""
    c, d = _case(shape), _on_dev(shape, dev)
    cin = shape[1]
    y = _fused_case(d, bias, relu).cpu().double()
    y64, y32, mag = c['y64'], c['y32'], c['mag']
    if bias:
        b = c['bias'].view(1, -1, 1, 1)
        y64, y32, mag = y64 + b.double(), y32 + b, mag + b.double().abs()
    if relu:
        y64, y32 = y64.clamp_min(0.0), y32.clamp_min(0.0)
    bound = 2.0 * (cin + 16) * 2.0 ** -24 * mag
    err = (y - y64).abs()
    err32 = (y32.double() - y64).abs()
    print('shape', shape, 'bias', bias, 'relu', relu, 'max err / bound', float((err / bound).max()),
          'max err / max direct-f32 err', float(err.max() / err32.max()))
    assert torch.isfinite(y).all()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float(err.max()) <= 8.0 * float(err32.max())


@pytest.mark.parametrize('bias,relu', FLAGS)
@pytest.mark.parametrize('shape', SHAPES)
def test_epilogue_bits_equal_bias_act(dev, shape, bias, relu):
    """fused(bias, relu) == frh_bias_act_nhwc(fused(no bias, no relu)) (a zero bias where the
    fused call has none)."""
    from frcnn_amd import _lib
    d = _on_dev(shape, dev)
    y = _fused_case(d, bias, relu)
    ref = _fused_case(d, False, False)
    n, cout, h, w = ref.shape
    b = d['bias'] if bias else torch.zeros_like(d['bias'])
    _lib.call('frh_bias_act_nhwc', _lib.ptr(ref), _lib.ptr(b), n * h * w, cout, int(relu), _lib.stream_of(ref))
    assert torch.equal(y, ref)


@pytest.mark.parametrize('shape', SHAPES)
def test_two_launches_give_the_same_bits(dev, shape):
    d = _on_dev(shape, dev)
    assert torch.equal(_fused_case(d, True, True), _fused_case(d, True, True))


@pytest.mark.parametrize('bias,relu', FLAGS)
def test_strided_view_equals_its_copy(dev, bias, relu):
    """The P6 form: x[:, :, ::2, ::2] of a channels-last level runs without a copy and gives the
    bits of the same call on its contiguous copy."""
    torch.manual_seed(5)
    cl = torch.channels_last
    p5 = torch.randn(2, 64, 19, 32, device=dev).contiguous(memory_format=cl)
    w = torch.randn(64, 64, 3, 3, device=dev).contiguous(memory_format=cl)
    b = torch.randn(64, device=dev) if bias else None
    view = p5[:, :, ::2, ::2]
    assert view.shape == (2, 64, 10, 16) and not view.is_contiguous(memory_format=cl)
    copy = view.contiguous(memory_format=cl)
    y = _fused(view, w, b, relu)
    assert torch.equal(y, _fused(copy, w, b, relu))
    ref = F.conv2d(copy, w, b, padding=1)
    ref = ref.relu() if relu else ref
    torch.testing.assert_close(y, ref, rtol=1e-3, atol=1e-3 * float(ref.abs().max()))


def test_entry_refuses_what_it_cannot_run(dev):
    from frcnn_amd import _lib
    cl = torch.channels_last
    p = _lib.ptr

    def run(x, w, y, cin, cout, ws=None):
        ws = torch.empty(16 * cin * cout, device=dev) if ws is None else ws
        _lib.call('frh_conv3x3_bias_act', x, p(w), None, y, p(ws), 1, cin, cout, 4, 4, 16 * cin, 4 * cin, cin, 0,
                  _lib.stream_of(w))

    x12 = torch.zeros(1, 12, 4, 4, device=dev).contiguous(memory_format=cl)
    w12 = torch.zeros(64, 12, 3, 3, device=dev).contiguous(memory_format=cl)
    x64 = torch.zeros(1, 64, 4, 4, device=dev).contiguous(memory_format=cl)
    w64 = torch.zeros(64, 64, 3, 3, device=dev).contiguous(memory_format=cl)
    w32 = torch.zeros(32, 64, 3, 3, device=dev).contiguous(memory_format=cl)
    y64 = torch.zeros(1, 64, 4, 4, device=dev).contiguous(memory_format=cl)
    with pytest.raises(RuntimeError, match='multiple'):
        run(p(x12), w12, p(y64), 12, 64)
    with pytest.raises(RuntimeError, match='multiple'):
        run(p(x64), w32, p(y64), 64, 32)
    with pytest.raises(RuntimeError, match='alias'):
        run(p(x64), w64, p(x64), 64, 64)
    with pytest.raises(RuntimeError, match='alias'):
        run(p(x64), w64, p(y64), 64, 64, ws=y64)
    with pytest.raises(RuntimeError, match='aligned'):
        run(ctypes.c_void_p(x64.data_ptr() + 4), w64, p(y64), 64, 64)
    with pytest.raises(RuntimeError, match='aligned'):
        run(p(x64), w64, ctypes.c_void_p(y64.data_ptr() + 8), 64, 64)


@pytest.mark.parametrize('shared', (True, False))
@pytest.mark.parametrize('bias,relu', [(True, True), (False, False)])
def test_levels_launch_equals_per_level_launches(dev, bias, relu, shared):
    """One launch over three levels, with shared weights (one transform) or one weight per level,
    gives each level the bits of its own launch."""
    from frcnn_amd import _lib
    torch.manual_seed(7)
    cl = torch.channels_last
    cin, cout, n = 32, 128, 2
    xs = [torch.randn(n, cin, h, w, device=dev).contiguous(memory_format=cl) for h, w in ((6, 10), (3, 5), (2, 3))]
    ws_ = [torch.randn(cout, cin, 3, 3, device=dev).contiguous(memory_format=cl) for _ in range(1 if shared else 3)]
    ws_ = ws_ * 3 if shared else ws_
    bs = [torch.randn(cout, device=dev) if bias else None for _ in range(3)]
    ys = [torch.empty(n, cout, x.shape[2], x.shape[3], device=dev).contiguous(memory_format=cl) for x in xs]
    work = torch.empty((1 if shared else 3) * 16 * cin * cout, device=dev)
    nul = (_lib.c_vp * 3)(*[None if b is None else b.data_ptr() for b in bs])
    args = [len(xs), _lib.ptr_array(xs), _lib.ptr_array(ws_), nul, _lib.ptr_array(ys), _lib.ptr(work),
            work.numel() * 4, n, cin, cout, _lib.i32_array([v for x in xs for v in x.shape[2:]]),
            _lib.i64_array([v for x in xs for v in (x.stride(0), x.stride(2), x.stride(3))]), int(relu),
            _lib.stream_of(work)]
    _lib.call('frh_conv3x3_bias_act_levels', *args)
    for x, w, b, y in zip(xs, ws_, bs, ys):
        assert torch.equal(y, _fused(x, w, b, relu))
    if not shared:
        args[6] = 2 * 16 * cin * cout * 4
        with pytest.raises(RuntimeError, match='workspace'):
            _lib.call('frh_conv3x3_bias_act_levels', *args)


def _conv(dev, cin, cout, seed, **kw):
    from frcnn_amd.utils import conv_layout
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1, **kw).to(dev)
    conv_layout(conv)
    return conv


def test_dispatch(dev, monkeypatch):
    """Under no_grad the op is the fused entry; with a gradient needed, on CPU tensors, at an
    excluded level size and for a stride-2 conv it is what ran before (conv_bias_relu when relu
    is set, the module when not)."""
    from frcnn_amd import ops
    conv = _conv(dev, 64, 128, 3)
    x = torch.randn(2, 64, 8, 12, device=dev).contiguous(memory_format=torch.channels_last)
    ran = support.spy_entries(monkeypatch).ran

    with torch.enable_grad():
        assert conv.weight.requires_grad and not ops.conv3x3_fused_ok(conv, x)
        y, got = ran(lambda: ops.conv3x3_bias_act(conv, x, relu=True))
        assert got == ['frh_bias_act_nhwc'] and y.grad_fn is not None
        y, got = ran(lambda: ops.conv3x3_bias_act(conv, x))
        assert got == [] and y.grad_fn is not None
        ref = conv(x).detach()
    with torch.no_grad():
        assert ops.conv3x3_fused_ok(conv, x)
        y, got = ran(lambda: ops.conv3x3_bias_act(conv, x))
        assert got == ['frh_conv3x3_bias_act'] and y.grad_fn is None
        assert torch.equal(y, _fused(x, conv.weight, conv.bias, False))
        assert y.is_contiguous(memory_format=torch.channels_last)
        torch.testing.assert_close(y, ref, rtol=1e-3, atol=1e-3 * float(ref.abs().max()))
        y, got = ran(lambda: ops.conv3x3_bias_act(conv, x, relu=True))
        assert got == ['frh_conv3x3_bias_act']
        torch.testing.assert_close(y, ref.relu(), rtol=1e-3, atol=1e-3 * float(ref.abs().max()))
        # all levels of a shared conv: one call
        xs = [x, x[:, :, ::2, ::2]]
        ys, got = ran(lambda: ops.conv3x3_bias_act_levels(conv, xs, relu=True))
        assert got == ['frh_conv3x3_bias_act_levels']
        for xi, yi in zip(xs, ys):
            assert torch.equal(yi, _fused(xi, conv.weight, conv.bias, True))

        # CPU tensors
        cpu_conv = torch.nn.Conv2d(64, 128, 3, padding=1)
        x_cpu = x.cpu()
        assert not ops.conv3x3_fused_ok(cpu_conv, x_cpu)
        y, got = ran(lambda: ops.conv3x3_bias_act(cpu_conv, x_cpu, relu=True))
        assert got == [] and torch.equal(y, cpu_conv(x_cpu).relu())
        # a stride-2 conv, an NCHW input
        strided = _conv(dev, 64, 128, 4, stride=2)
        assert not ops.conv3x3_fused_ok(strided, x)
        y, got = ran(lambda: ops.conv3x3_bias_act(strided, x, relu=True))
        assert got == ['frh_bias_act_nhwc'] and y.shape == (2, 128, 4, 6)
        assert not ops.conv3x3_fused_ok(conv, x.contiguous())
        # an excluded level size keeps the old path alone and rides along in a multi-level launch
        monkeypatch.setattr(ops, '_CONV3X3_EXCLUDED', frozenset([(8, 12)]))
        assert not ops.conv3x3_fused_ok(conv, x) and ops.conv3x3_fused_ok(conv, x, alone=False)
        y, got = ran(lambda: ops.conv3x3_bias_act(conv, x, relu=True))
        assert got == ['frh_bias_act_nhwc']
        y, got = ran(lambda: ops.conv3x3_bias_act(conv, x))
        assert got == []
        ys, got = ran(lambda: ops.conv3x3_bias_act_levels(conv, xs, relu=True))
        assert got == ['frh_conv3x3_bias_act_levels']
        monkeypatch.setattr(ops, '_CONV3X3_EXCLUDED', frozenset([(8, 12), (4, 6)]))
        ys, got = ran(lambda: ops.conv3x3_bias_act_levels(conv, xs, relu=True))
        assert got == ['frh_bias_act_nhwc']  # the strided view takes conv_bias_relu's module ops
        # one conv per level
        other = _conv(dev, 64, 128, 6)
        monkeypatch.setattr(ops, '_CONV3X3_EXCLUDED', frozenset())
        ys, got = ran(lambda: ops.conv3x3_bias_act_levels([conv, other], xs))
        assert got == ['frh_conv3x3_bias_act_levels']
        for ci, xi, yi in zip((conv, other), xs, ys):
            assert torch.equal(yi, _fused(xi, ci.weight, ci.bias, False))


def test_fpn_and_rpn_head_match_the_unfused_path(dev, monkeypatch):
    """FPN + RPNHead forward on a small pyramid under no_grad (fused 3x3 convs) against the same
    modules forced onto the path that ran before, to the tolerance the trunk parity test grants
    solver differences."""
    from frcnn_amd import ops
    from frcnn_amd.necks import FPN
    from frcnn_amd.heads.rpn_head import RPNHead
    torch.manual_seed(13)
    fpn = FPN([32, 64, 128, 256], 64, 5).to(dev)
    head = RPNHead(64, 64, loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True),
                   loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0)).to(dev)
    with torch.no_grad():
        for m in list(fpn.modules()) + list(head.modules()):
            if isinstance(m, torch.nn.Conv2d):
                m.weight.normal_(0.0, 0.05)
                m.bias.uniform_(-0.5, 0.5)
        feats = [torch.randn(2, c, h, w, device=dev) for c, (h, w) in
                 zip((32, 64, 128, 256), ((38, 52), (19, 26), (10, 13), (5, 7)))]
        spy = support.spy_entries(monkeypatch)
        levels = fpn(feats)
        cls, reg = head(levels)
        # the FPN's four output convs, the head's five levels
        assert spy.names.count('frh_conv3x3_bias_act_levels') == 2
        monkeypatch.setattr(ops, 'conv3x3_fused_ok', lambda conv, x, alone=True: False)
        spy.clear()
        ref_levels = fpn(feats)
        ref_cls, ref_reg = head(ref_levels)
        assert not [n for n in spy.names if n.startswith('frh_conv3x3')]
    for got, want in zip(levels + cls + reg, ref_levels + ref_cls + ref_reg):
        assert got.shape == want.shape
        torch.testing.assert_close(got, want, rtol=1e-3, atol=1e-3 * float(want.abs().max()))
