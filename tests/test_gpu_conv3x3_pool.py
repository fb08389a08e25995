"""frh_conv3x3_bias_act_pool: frh_conv3x3_bias_act (Winograd F(2x2, 3x3) on the f32 MFMA,
csrc/conv3x3_wino_kernels.h) with the 2 x 2 / stride-2 max pool that follows a VGG16 conv taken
in the epilogue, where every lane holds a whole pool window; frh_nchw_to_nhwc8, which pads the
first layer's 3 input channels to the kernel's chunk of 8; and ops.vgg_stem on both.

Shapes are (n, cin, cout, h, w).  A workgroup owns 8 x 8 tiles (16 x 16 outputs, 8 x 8 pooled)
x 64 output channels; an odd last row / column is a neighbour of the convolution only.

Measured on MI355X (test_accuracy_against_float64's printed ratios over the four shapes and flag
pairs): max error / pooled bound 1.3e-3 .. 3.6e-3; ops.vgg_stem (cin = 3): 1.8e-2."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import support

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 8, 64, 3, 5),      # under one block, odd both ways, one cin chunk
    (2, 64, 64, 19, 32),   # odd h, half-empty last tile row, batch stride
    (1, 32, 192, 17, 34),  # ragged block on both sides, three cout blocks
    (2, 16, 128, 16, 16),  # exactly one block, even
]
FLAGS = [(b, r) for b in (False, True) for r in (False, True)]
CL = torch.channels_last


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs (CPU f32) and the float64 references of one shape, computed once."""
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(5000 + cin + 7 * cout + h * w)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g)
    bias = torch.randn(cout, generator=g)
    return dict(x=x, w=wt, bias=bias, y64=F.conv2d(x.double(), wt.double(), None, padding=1),
                mag=support.wino_magnitude(x, wt))


@functools.lru_cache(maxsize=None)
def _on_dev(shape, dev):
    c = _case(shape)
    return dict(x=c['x'].to(dev).contiguous(memory_format=CL), w=c['w'].to(dev).contiguous(memory_format=CL),
                bias=c['bias'].to(dev))


def _call(entry, x, w, bias, relu, y):
    from frcnn_amd import _lib
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    assert x.stride(1) == 1 and w.is_contiguous(memory_format=CL)
    ws = torch.empty(16 * cin * cout, dtype=torch.float32, device=x.device)
    p = _lib.ptr
    _lib.call(entry, p(x), p(w), p(bias), p(y), p(ws), n, cin, cout, h, wd, x.stride(0), x.stride(2), x.stride(3),
              int(relu), _lib.stream_of(x))
    return y


def _unpooled(x, w, bias, relu):
    n, _, h, wd = x.shape
    return _call('frh_conv3x3_bias_act', x, w, bias, relu,
                 torch.empty(n, w.shape[0], h, wd, device=x.device).contiguous(memory_format=CL))


def _pooled(x, w, bias, relu):
    n, _, h, wd = x.shape
    return _call('frh_conv3x3_bias_act_pool', x, w, bias, relu,
                 torch.empty(n, w.shape[0], h // 2, wd // 2, device=x.device).contiguous(memory_format=CL))


@pytest.mark.parametrize('bias,relu', FLAGS)
@pytest.mark.parametrize('shape', SHAPES)
def test_bits_equal_max_pool_of_the_unpooled_entry(dev, shape, bias, relu):
    d = _on_dev(shape, dev)
    b = d['bias'] if bias else None
    y = _pooled(d['x'], d['w'], b, relu)
    n, _, cout, h, w = shape
    assert y.shape == (n, cout, h // 2, w // 2)
    assert torch.equal(y, F.max_pool2d(_unpooled(d['x'], d['w'], b, relu), 2))


@pytest.mark.parametrize('bias,relu', FLAGS)
def test_strided_view_bits(dev, bias, relu):
    """x[:, :, ::2, ::2] of a larger channels-last map runs without a copy."""
    torch.manual_seed(5)
    big = torch.randn(2, 64, 19, 32, device=dev).contiguous(memory_format=CL)
    w = torch.randn(64, 64, 3, 3, device=dev).contiguous(memory_format=CL)
    b = torch.randn(64, device=dev) if bias else None
    view = big[:, :, ::2, ::2]
    assert view.shape == (2, 64, 10, 16) and not view.is_contiguous(memory_format=CL)
    y = _pooled(view, w, b, relu)
    assert torch.equal(y, F.max_pool2d(_unpooled(view, w, b, relu), 2))
    assert torch.equal(y, _pooled(view.contiguous(memory_format=CL), w, b, relu))


@pytest.mark.parametrize('relu', (False, True))
@pytest.mark.parametrize('shape', SHAPES)
def test_exact_integers(dev, shape, relu):
    """x = 1, w = 1, no bias: every Winograd intermediate is a multiple of 1/4 below 2^24, so a
    pooled value is exactly cin x the largest tap count of its window (4, 6 or 9)."""
    n, cin, cout, h, w = shape
    x = torch.ones(n, cin, h, w, device=dev).contiguous(memory_format=CL)
    wt = torch.ones(cout, cin, 3, 3, device=dev).contiguous(memory_format=CL)
    taps = F.max_pool2d(F.conv2d(torch.ones(1, 1, h, w), torch.ones(1, 1, 3, 3), padding=1), 2)
    assert set(taps.unique().tolist()) <= {4.0, 6.0, 9.0}
    assert torch.equal(_pooled(x, wt, None, relu).cpu(), (taps * cin).expand(n, cout, h // 2, w // 2))


def _bounded(y, y64, mag, cin, bias, relu):
    """(max |y - pool(act(y64 + b))| / pool(bound)) with test_gpu_conv3x3.py's bound
    2 (cin + 16) 2^-24 magW; the max of a window is 1-Lipschitz in the sup norm, so the window's
    largest bound bounds the pooled value's error."""
    if bias is not None:
        b = bias.view(1, -1, 1, 1).double()
        y64, mag = y64 + b, mag + b.abs()
    if relu:
        y64 = y64.clamp_min(0.0)
    bound = F.max_pool2d(2.0 * (cin + 16) * 2.0 ** -24 * mag, 2)
    err = (y.cpu().double() - F.max_pool2d(y64, 2)).abs()
    assert torch.isfinite(y).all()
    return float((err / bound).max()), bool((err <= bound).all())


@pytest.mark.parametrize('bias,relu', FLAGS)
@pytest.mark.parametrize('shape', SHAPES)
def test_accuracy_against_float64(dev, shape, bias, relu):
    c, d = _case(shape), _on_dev(shape, dev)
    y = _pooled(d['x'], d['w'], d['bias'] if bias else None, relu)
    ratio, ok = _bounded(y, c['y64'], c['mag'], shape[1], c['bias'] if bias else None, relu)
    print('shape', shape, 'bias', bias, 'relu', relu, 'max err / pooled bound', ratio)
    assert ok, ratio


@pytest.mark.parametrize('shape', SHAPES)
def test_stores_stay_inside_the_output(dev, shape):
    """y is a 16-byte-aligned slice in the middle of a NaN-filled buffer: the guards stay NaN and
    every output element is written (finite)."""
    d = _on_dev(shape, dev)
    n, _, cout, h, w = shape
    numel, guard = n * cout * (h // 2) * (w // 2), 4096
    buf = torch.full((numel + 2 * guard,), float('nan'), device=dev)
    y = buf[guard:guard + numel].view(n, h // 2, w // 2, cout).permute(0, 3, 1, 2)
    assert y.data_ptr() % 16 == 0 and y.is_contiguous(memory_format=CL)
    _call('frh_conv3x3_bias_act_pool', d['x'], d['w'], d['bias'], False, y)
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + numel:]).all()
    assert torch.isfinite(buf[guard:guard + numel]).all()
    assert torch.equal(y, _pooled(d['x'], d['w'], d['bias'], False))


@pytest.mark.parametrize('h,w', [(1, 6), (6, 1), (1, 1)])
def test_degenerate_sizes_write_nothing(dev, h, w):
    x = torch.randn(2, 8, h, w, device=dev).contiguous(memory_format=CL)
    wt = torch.randn(64, 8, 3, 3, device=dev).contiguous(memory_format=CL)
    buf = torch.full((4096,), float('nan'), device=dev)
    _call('frh_conv3x3_bias_act_pool', x, wt, None, True, buf)  # FRH_OK: call raises otherwise
    assert torch.isnan(buf).all()


def test_entry_refuses_what_it_cannot_run(dev):
    from frcnn_amd import _lib
    p = _lib.ptr

    def run(x, w, y, cin, cout, ws=None):
        ws = torch.empty(16 * cin * cout, device=dev) if ws is None else ws
        _lib.call('frh_conv3x3_bias_act_pool', x, p(w), None, y, p(ws), 1, cin, cout, 4, 4, 16 * cin, 4 * cin, cin,
                  0, _lib.stream_of(w))

    def zeros(*shape):
        return torch.zeros(*shape, device=dev).contiguous(memory_format=CL)
    x12, w12 = zeros(1, 12, 4, 4), zeros(64, 12, 3, 3)
    x64, w64, w32 = zeros(1, 64, 4, 4), zeros(64, 64, 3, 3), zeros(32, 64, 3, 3)
    y64 = zeros(1, 64, 2, 2)
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


def test_alias_check_uses_the_pooled_extent(dev):
    """A y of the pooled size that ends exactly where x begins is accepted: the check does not
    take y for a full-resolution map."""
    cin, cout = 8, 64
    pooled = 1 * 2 * 2 * cout
    buf = torch.randn(pooled + 4 * 4 * cin, device=dev)
    y = buf[:pooled].view(1, 2, 2, cout).permute(0, 3, 1, 2)
    x = buf[pooled:].view(1, 4, 4, cin).permute(0, 3, 1, 2)
    w = torch.randn(cout, cin, 3, 3, device=dev).contiguous(memory_format=CL)
    want = _pooled(x.contiguous(memory_format=CL), w, None, False)
    assert torch.equal(_call('frh_conv3x3_bias_act_pool', x, w, None, False, y), want)


@pytest.mark.parametrize('shape', SHAPES)
def test_two_launches_give_the_same_bits(dev, shape):
    d = _on_dev(shape, dev)
    assert torch.equal(_pooled(d['x'], d['w'], d['bias'], True), _pooled(d['x'], d['w'], d['bias'], True))


# ----------------------------------------------------------------- frh_nchw_to_nhwc8
def _pad8(x):
    """The torch construction: NHWC with the channels zero-padded to 8, as an NCHW-shaped view."""
    return F.pad(x.permute(0, 2, 3, 1), (0, 8 - x.shape[1])).contiguous().permute(0, 3, 1, 2)


@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (1, 1, 4, 4), (1, 8, 3, 2)])
def test_nchw_to_nhwc8(dev, shape):
    from frcnn_amd import _lib
    n, c, h, w = shape
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(c)).to(dev)
    guard = 64
    buf = torch.full((n * h * w * 8 + 2 * guard,), float('nan'), device=dev)
    _lib.call('frh_nchw_to_nhwc8', _lib.ptr(x), ctypes.c_void_p(buf.data_ptr() + guard * 4), n, c, h, w,
              _lib.stream_of(x))
    y = buf[guard:-guard].view(n, h, w, 8).permute(0, 3, 1, 2)
    assert torch.equal(y, _pad8(x))
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[-guard:]).all()


def test_nchw_to_nhwc8_refusals_and_empty(dev):
    from frcnn_amd import _lib
    x, y = torch.zeros(1, 3, 4, 4, device=dev), torch.full((1, 4, 4, 8), float('nan'), device=dev)
    p, s = _lib.ptr, _lib.stream_of(x)
    _lib.call('frh_nchw_to_nhwc8', p(x), p(y), 1, 3, 0, 4, s)
    _lib.call('frh_nchw_to_nhwc8', p(x), p(y), 0, 3, 4, 4, s)
    assert torch.isnan(y).all()
    with pytest.raises(RuntimeError, match='channels'):
        _lib.call('frh_nchw_to_nhwc8', p(x), p(y), 1, 9, 4, 4, s)
    with pytest.raises(RuntimeError, match='aligned'):
        _lib.call('frh_nchw_to_nhwc8', ctypes.c_void_p(x.data_ptr() + 4), p(y), 1, 3, 4, 4, s)
    with pytest.raises(RuntimeError, match='alias'):
        _lib.call('frh_nchw_to_nhwc8', p(y), p(y), 1, 3, 4, 4, s)


# ----------------------------------------------------------------- ops.vgg_stem
def test_vgg_stem(dev, monkeypatch):
    """The stem on a (2, 3, 19, 32) image: one padding pass and one fused conv call, the bits of
    frh_conv3x3_bias_act on the hand-padded tensors, within the float64 bound at cin = 3."""
    from frcnn_amd import ops
    from frcnn_amd.utils import conv_layout
    g = torch.Generator().manual_seed(77)
    x, wt = torch.randn(2, 3, 19, 32, generator=g), torch.randn(64, 3, 3, 3, generator=g)
    bias = torch.randn(64, generator=g)
    conv = torch.nn.Conv2d(3, 64, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(wt)
        conv.bias.copy_(bias)
    conv = conv.to(dev)
    conv_layout(conv)
    img = x.to(dev)
    spy = support.spy_entries(monkeypatch)
    with torch.no_grad():
        y, names = spy.ran(lambda: ops.vgg_stem(conv, img))
        assert names == ['frh_nchw_to_nhwc8', 'frh_conv3x3_bias_act']
        w8 = F.pad(conv.weight, (0, 0, 0, 0, 0, 5)).contiguous(memory_format=CL)
        assert torch.equal(y, _unpooled(_pad8(img), w8, conv.bias, True))
        # the padded weight is made once per weight version
        a = ops._stem_weight8(conv)
        assert ops._stem_weight8(conv) is a and torch.equal(a, w8)
        conv.weight.mul_(2.0)
        assert ops._stem_weight8(conv) is not a and torch.equal(ops._stem_weight8(conv), 2.0 * w8)
    with torch.enable_grad():  # the weight needs a gradient: the module
        y2, names = spy.ran(lambda: ops.vgg_stem(conv, img))
        assert names == [] and y2.grad_fn is not None
    y64 = F.conv2d(x.double(), wt.double(), bias.double(), padding=1).clamp_min(0.0)
    mag = support.wino_magnitude(x, wt) + bias.view(1, -1, 1, 1).double().abs()
    bound = 2.0 * (3 + 16) * 2.0 ** -24 * mag
    err = (y.cpu().double() - y64).abs()
    print('vgg_stem max err / bound', float((err / bound).max()))
    assert torch.isfinite(y).all() and bool((err <= bound).all())
