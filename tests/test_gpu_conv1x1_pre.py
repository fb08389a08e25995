"""The input-side forms of the fused 1x1 convolution (csrc/conv1x1_kernels.h):
frh_conv1x1_bn_act_pre (the BN + ReLU in front of the convolution applied to the X tile) and
frh_conv1x1_s2_bn_act (the X tile gathered from x[:, :, ::2, ::2]), their Python dispatch
(ops.conv1x1_bn_act(pre_bn=...), ops.conv1x1_s2_bn_act) and the Bottleneck that calls them.

Both are pinned by bit equality to the chain they replace, so the accuracy bounds of
test_gpu_conv1x1.py carry over."""
import functools

import pytest
import torch

import support

pytestmark = pytest.mark.gpu

# (n, cin, cout, h, w): the shapes of test_gpu_conv1x1.py
SHAPES = [
    (2, 64, 256, 4, 12),     # less than one pixel tile; batch stride; step 16
    (2, 256, 64, 19, 32),    # 608 pixels: ragged last pixel tile; step 32
    (1, 512, 128, 10, 10),   # hw % 4 == 0 but not a multiple of 32; long K loop
    (2, 128, 512, 6, 20),    # cout spanning several row tiles; hw = 120
    (1, 48, 64, 6, 22),      # cin % 32 != 0: step 16 with three steps; hw = 132
]
FLAGS = [(s, r) for s in (False, True) for r in (False, True)]
S2_PLANES = [(8, 12), (6, 8), (2, 4)]  # output planes
S2_CHANNELS = [(64, 128), (256, 512)]
EPS = 1e-5


@functools.lru_cache(maxsize=None)
def _case(n, cin, cout, h, w, dev):
    """x [n, cin, h, w], the weight, a skip for the plane (h, w) and for its stride-2 output, the
    output BN and the input BN (signed gammas), on the device."""
    g = torch.Generator().manual_seed(2000 + cin + 7 * cout + h * w)
    d = dict(x=torch.randn(n, cin, h, w, generator=g), w=torch.randn(cout, cin, generator=g),
             skip=torch.randn(n, cout, h, w, generator=g),
             skip2=torch.randn(n, cout, (h + 1) // 2, w // 2, generator=g))
    d['gamma'], d['beta'], d['mean'], d['var'] = support.bn_params(cout, g)
    d['pgamma'], d['pbeta'], d['pmean'], d['pvar'] = support.bn_params(cin, g)
    return {k: v.to(dev) for k, v in d.items()}


def _bn_ptrs(d, prefix=''):
    from frcnn_amd import _lib
    return [_lib.ptr(d[prefix + k]) for k in ('gamma', 'beta', 'mean', 'var')]


def _plain(d, x, skip, relu):
    from frcnn_amd import _lib
    n, cin, h, w = x.shape
    cout = d['w'].shape[0]
    y = torch.empty(n, cout, h, w, device=x.device)
    _lib.call('frh_conv1x1_bn_act', _lib.ptr(x), _lib.ptr(d['w']), _lib.ptr(skip), _lib.ptr(y), *_bn_ptrs(d), EPS, n,
              cin, cout, h * w, int(relu), _lib.stream_of(x))
    return y


def _nan(shape, dev):
    return torch.full(shape, float('nan'), device=dev)


def _pre(d, x, skip, relu, alloc=_nan):
    """frh_conv1x1_bn_act_pre on the raw input; alloc(shape, device) makes the output (NaN-filled
    here; tests/test_gpu_guarded_convs.py passes torch.empty under its allocator)."""
    from frcnn_amd import _lib
    n, cin, h, w = x.shape
    cout = d['w'].shape[0]
    y = alloc((n, cout, h, w), x.device)
    _lib.call('frh_conv1x1_bn_act_pre', _lib.ptr(x), _lib.ptr(d['w']), _lib.ptr(skip), _lib.ptr(y), *_bn_ptrs(d), EPS,
              *_bn_ptrs(d, 'p'), EPS, 1, n, cin, cout, h * w, int(relu), _lib.stream_of(x))
    return y


@pytest.mark.parametrize('skip,relu', FLAGS)
@pytest.mark.parametrize('shape', SHAPES)
def test_pre_bn_bits_equal_bn_act_then_conv(dev, shape, skip, relu):
    """frh_conv1x1_bn_act_pre on the raw input == frh_bn_act (BN + ReLU) then frh_conv1x1_bn_act."""
    from frcnn_amd import _lib
    d = _case(*shape, dev)
    x = d['x']
    n, cin, h, w = x.shape
    cout = d['w'].shape[0]
    sk = d['skip'] if skip else None
    p = _lib.ptr
    mid = torch.empty_like(x)
    _lib.call('frh_bn_act', p(x), None, p(mid), *_bn_ptrs(d, 'p'), EPS, n, cin, h * w, 1, _lib.stream_of(x))
    ref = _plain(d, mid, sk, relu)
    y = _pre(d, x, sk, relu)
    assert y.shape == (n, cout, h, w)
    assert torch.isfinite(y).all()
    assert torch.equal(y, ref)


def _s2(d, x, skip, relu, alloc=_nan):
    from frcnn_amd import _lib
    n, cin, h, w = x.shape
    cout = d['w'].shape[0]
    y = alloc((n, cout, (h + 1) // 2, w // 2), x.device)
    _lib.call('frh_conv1x1_s2_bn_act', _lib.ptr(x), _lib.ptr(d['w']), _lib.ptr(skip), _lib.ptr(y), *_bn_ptrs(d), EPS, n,
              cin, cout, h, w, int(relu), _lib.stream_of(x))
    return y


@pytest.mark.parametrize('channels', S2_CHANNELS)
@pytest.mark.parametrize('plane', S2_PLANES)
def test_stride2_bits_equal_stride1_on_the_subsampled_copy(dev, plane, channels):
    """frh_conv1x1_s2_bn_act(x) == frh_conv1x1_bn_act(x[:, :, ::2, ::2].contiguous()); the (6, 8)
    plane comes from an input with an odd number of rows."""
    oh, ow = plane
    h = 2 * oh - 1 if plane == (6, 8) else 2 * oh
    d = _case(2, channels[0], channels[1], h, 2 * ow, dev)
    sub = d['x'][:, :, ::2, ::2].contiguous()
    assert sub.shape[2:] == plane
    for skip, relu in FLAGS:
        sk = d['skip2'] if skip else None
        y = _s2(d, d['x'], sk, relu)
        assert torch.isfinite(y).all()
        assert torch.equal(y, _plain(d, sub, sk, relu))


def _conv_bn(dev, cin, cout, seed, **kw):
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, 1, bias=False, **kw).to(dev)
    bn = torch.nn.BatchNorm2d(cout).to(dev).eval()
    _randomise_bn(bn)
    return conv, bn


def _randomise_bn(bn):
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-1, 1)
        bn.running_var.uniform_(0.5, 2.0)


def test_stride2_refuses_an_output_width_off_4(dev):
    from frcnn_amd import ops
    conv, bn = _conv_bn(dev, 64, 128, 3, stride=2)
    d = _case(1, 64, 128, 4, 12, dev)  # output width 6
    with pytest.raises(RuntimeError, match='multiple'):
        _s2(d, d['x'], None, False)
    with torch.no_grad():
        assert not ops.conv1x1_s2_fused_ok(conv, bn, d['x'])
        assert ops.conv1x1_s2_fused_ok(conv, bn, torch.randn(1, 64, 4, 16, device=dev))
        got = ops.conv1x1_s2_bn_act(conv, bn, d['x'])  # the fallback
        want = ops.bn_act(conv(d['x']), bn, relu=False)
    torch.testing.assert_close(got, want, rtol=1e-3, atol=1e-3 * float(want.abs().max()))


BLOCKS = [(256, 256), (256, 512, True)]


@pytest.mark.parametrize('args', BLOCKS)
def test_bottleneck_launches_and_values(dev, args, monkeypatch):
    """Under no_grad no frh_bn_act pass is left where both fused paths hold (conv3 reads conv2's
    raw output through the input-side BN, the stride-2 projection is one launch), and the block's
    output is within the tolerance the trunk parity tests grant of the unfused chain."""
    blk, x = support.block(dev, args, _randomise_bn)
    with torch.no_grad():
        ref = support.bottleneck_unfused(blk, x)
        names = support.spy_entries(monkeypatch).names
        y = blk(x)
    assert 'frh_bn_act' not in names
    assert names.count('frh_conv1x1_bn_act_pre') == 1
    assert names.count('frh_conv1x1_s2_bn_act') == (1 if len(args) == 3 else 0)
    torch.testing.assert_close(y, ref, rtol=1e-3, atol=1e-3 * float(ref.abs().max()))


@pytest.mark.parametrize('args', BLOCKS)
def test_bottleneck_under_grad_keeps_the_old_path(dev, args, monkeypatch):
    blk, x = support.block(dev, args, _randomise_bn)
    names = support.spy_entries(monkeypatch).names
    with torch.enable_grad():
        y = blk(x)
        ref = support.bottleneck_unfused(blk, x)
    assert y.grad_fn is not None
    assert set(names) == {'frh_bn_act'}
    torch.testing.assert_close(y, ref, rtol=1e-3, atol=1e-3 * float(ref.abs().max()))
