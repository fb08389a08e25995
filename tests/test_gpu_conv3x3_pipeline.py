"""The staging pipeline of frh_conv3x3_bias_act (csrc/conv3x3_wino_kernels.h): U by LDS-DMA, two
sets of patch registers, one loop body for every chunk count.

Exact-integer inputs (x in [-3, 3], w = 4 x [-2, 2], integer bias): every Winograd intermediate
is an integer below 2^24 (|V| <= 12, |U| <= 18, sums <= 256 * 216), so the output must equal the
float64 convolution exactly -- and, unlike all-ones inputs, a chunk's V meeting another chunk's
U, a stale stage or a dropped or doubled chunk changes it.  The recorded-bits test pins the
output of random inputs to the bits the kernel gave before the pipeline was rebuilt
(tests/golden/conv3x3_bits.json, written by tools/record_conv3x3_bits.py)."""
import functools
import hashlib
import json
import os

import pytest
import torch
import torch.nn.functional as F

import support

pytestmark = pytest.mark.gpu

CL = torch.channels_last
# (n, cin, cout, h, w): every chunk count from 1 to 8 (the pipeline's prologue, both halves of its
# loop body and both exits, and fewer chunks than it is deep), the workload's 32 chunks, a ragged
# tile block with three cout blocks
INT_SHAPES = [(1, cin, 64, 5, 7) for cin in (8, 16, 24, 32, 40, 48, 56, 64)] + [(2, 256, 128, 4, 4),
                                                                              (1, 40, 192, 17, 34)]
FLAGS = [(b, r) for b in (False, True) for r in (False, True)]
BIT_SHAPES = [(2, 64, 64, 19, 32), (2, 256, 128, 10, 16), (1, 32, 192, 17, 34)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv3x3_bits.json')


@functools.lru_cache(maxsize=None)
def _int_case(shape):
    """Integer inputs (CPU f32) and the float64 convolution without bias, computed once."""
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(7000 + cin + 7 * cout + h * w)
    x = support.ints(g, -3, 3, n, cin, h, w)
    wt = 4.0 * support.ints(g, -2, 2, cout, cin, 3, 3)
    bias = support.ints(g, -5, 5, cout)
    return dict(x=x, w=wt, bias=bias, y64=F.conv2d(x.double(), wt.double(), None, padding=1))


@functools.lru_cache(maxsize=None)
def _int_on_dev(shape, dev):
    c = _int_case(shape)
    return dict(x=c['x'].to(dev).contiguous(memory_format=CL), w=c['w'].to(dev).contiguous(memory_format=CL),
                bias=c['bias'].to(dev))


def _want(c, bias, relu):
    y = c['y64'] + c['bias'].double().view(1, -1, 1, 1) if bias else c['y64']
    return y.clamp_min(0.0) if relu else y


def _fused(x, w, bias, relu):
    from frcnn_amd import _lib
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    y = torch.empty(n, cout, h, wd, dtype=torch.float32, device=x.device, memory_format=CL)
    ws = torch.empty(16 * cin * cout, dtype=torch.float32, device=x.device)
    p = _lib.ptr
    _lib.call('frh_conv3x3_bias_act', p(x), p(w), p(bias), p(y), p(ws), n, cin, cout, h, wd, x.stride(0),
              x.stride(2), x.stride(3), int(relu), _lib.stream_of(x))
    return y


@pytest.mark.parametrize('bias,relu', FLAGS)
@pytest.mark.parametrize('shape', INT_SHAPES)
def test_integer_convolution_is_exact(dev, shape, bias, relu):
    c, d = _int_case(shape), _int_on_dev(shape, dev)
    y = _fused(d['x'], d['w'], d['bias'] if bias else None, relu)
    assert torch.equal(y.cpu().double(), _want(c, bias, relu))


@pytest.mark.parametrize('shape', INT_SHAPES)
def test_two_launches_give_the_same_bits(dev, shape):
    """Also a race between a DMA landing and an operand read: it would not repeat."""
    d = _int_on_dev(shape, dev)
    first = _fused(d['x'], d['w'], d['bias'], True)
    assert torch.equal(first, _fused(d['x'], d['w'], d['bias'], True))


@pytest.mark.parametrize('shared', (True, False))
@pytest.mark.parametrize('bias,relu', [(True, True), (False, False)])
def test_levels_launch_is_exact_and_equals_single_launches(dev, bias, relu, shared):
    """Three levels of integer inputs, cin 40 (five chunks), in one launch with shared or per-level
    weights: each level equals its own launch and the float64 convolution."""
    from frcnn_amd import _lib
    n, cin, cout = 2, 40, 128
    g = torch.Generator().manual_seed(7100 + shared)
    xs_c = [support.ints(g, -3, 3, n, cin, h, w) for h, w in ((6, 10), (3, 5), (2, 3))]
    ws_c = [4.0 * support.ints(g, -2, 2, cout, cin, 3, 3) for _ in range(1 if shared else 3)]
    ws_c = ws_c * 3 if shared else ws_c
    bs_c = [support.ints(g, -5, 5, cout) for _ in range(3)]
    xs = [x.to(dev).contiguous(memory_format=CL) for x in xs_c]
    wd = [w.to(dev).contiguous(memory_format=CL) for w in (ws_c[:1] if shared else ws_c)]
    wd = wd * 3 if shared else wd
    bs = [b.to(dev) if bias else None for b in bs_c]
    ys = [torch.empty(n, cout, x.shape[2], x.shape[3], device=dev).contiguous(memory_format=CL) for x in xs]
    work = torch.empty((1 if shared else 3) * 16 * cin * cout, device=dev)
    nul = (_lib.c_vp * 3)(*[None if b is None else b.data_ptr() for b in bs])
    _lib.call('frh_conv3x3_bias_act_levels', len(xs), _lib.ptr_array(xs), _lib.ptr_array(wd), nul,
              _lib.ptr_array(ys), _lib.ptr(work), work.numel() * 4, n, cin, cout,
              _lib.i32_array([v for x in xs for v in x.shape[2:]]),
              _lib.i64_array([v for x in xs for v in (x.stride(0), x.stride(2), x.stride(3))]), int(relu),
              _lib.stream_of(work))
    for xc, wc, bc, x, w, b, y in zip(xs_c, ws_c, bs_c, xs, wd, bs, ys):
        assert torch.equal(y, _fused(x, w, b, relu))
        want = _want(dict(y64=F.conv2d(xc.double(), wc.double(), None, padding=1), bias=bc), bias, relu)
        assert torch.equal(y.cpu().double(), want)


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return {tuple(c['shape']): c for c in json.load(f)['cases']}


@pytest.mark.parametrize('shape', BIT_SHAPES)
def test_recorded_bits(dev, shape):
    """Seeded CPU torch.randn inputs (tools/record_conv3x3_bits.py's randn_case), bias and ReLU:
    the SHA-256 of the output's bytes in NHWC order is the recorded one.  Skips only if this
    torch's CPU generator does not reproduce the recorded inputs."""
    n, cin, cout, h, w = shape
    want = _golden()[shape]
    g = torch.Generator().manual_seed(9000 + cin + 7 * cout + h * w)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g)
    bias = torch.randn(cout, generator=g)
    if (_sha(x), _sha(wt), _sha(bias)) != (want['x'], want['w'], want['bias']):
        pytest.skip('torch.randn on this CPU does not reproduce the recorded inputs')
    y = _fused(x.to(dev).contiguous(memory_format=CL), wt.to(dev).contiguous(memory_format=CL), bias.to(dev), True)
    assert _sha(y.permute(0, 2, 3, 1)) == want['y_nhwc']
