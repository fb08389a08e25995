"""frh_conv1x1_bn_act: the bottleneck's 1x1 / stride-1 convolution with the frozen-BN
(+ residual) (+ ReLU) epilogue on the GEMM accumulator (csrc/conv1x1_kernels.h), its Python
dispatch (ops.conv1x1_bn_act) and the Bottleneck that calls it.

Shapes are (n, cin, cout, h, w).  The kernel has one workgroup tile (64 channels x 64
pixels) and two cin steps per barrier: 16 for cin < 128 or cin % 32 != 0, 32 otherwise."""
import functools

import pytest
import torch

import support

pytestmark = pytest.mark.gpu

SHAPES = [
    (2, 64, 256, 4, 12),     # less than one pixel tile; batch stride; step 16
    (2, 256, 64, 19, 32),    # 608 pixels: stage 4's plane, ragged last pixel tile; 20 workgroups over 8 XCDs
    (1, 512, 128, 10, 10),   # hw % 4 == 0 but not a multiple of 32; long K loop
    (2, 128, 512, 6, 20),    # cout spanning several row tiles; hw = 120
    (1, 48, 64, 6, 22),      # cin % 32 != 0: step 16 with three steps; hw = 132
]
FLAGS = [(s, r) for s in (False, True) for r in (False, True)]
EPS = 1e-5


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs (CPU f32) and the float64 references of one shape, computed once."""
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(1000 + cin + 7 * cout + h * w)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, generator=g)
    skip = torch.randn(n, cout, h, w, generator=g)
    gamma = (torch.rand(cout, generator=g) + 0.5) * torch.where(torch.rand(cout, generator=g) < 0.5, -1.0, 1.0)
    beta = torch.rand(cout, generator=g) - 0.5
    mean = torch.rand(cout, generator=g) * 2 - 1
    var = torch.rand(cout, generator=g) * 1.5 + 0.5
    # frh_bn_act's expressions in f32 (divide and sqrt are correctly rounded on both sides)
    s32 = gamma / torch.sqrt(var + torch.tensor(EPS, dtype=torch.float32))
    b32 = beta - mean * s32
    x64, w64 = x.double().reshape(n, cin, h * w), wt.double()
    acc64 = torch.einsum('oc,ncp->nop', w64, x64).reshape(n, cout, h, w)
    absacc = torch.einsum('oc,ncp->nop', w64.abs(), x64.abs()).reshape(n, cout, h, w)
    return dict(x=x, w=wt, skip=skip, gamma=gamma, beta=beta, mean=mean, var=var, s32=s32, b32=b32, acc64=acc64,
                absacc=absacc)


@functools.lru_cache(maxsize=None)
def _on_dev(shape, dev):
    c = _case(shape)
    return {k: c[k].to(dev) for k in ('x', 'w', 'skip', 'gamma', 'beta', 'mean', 'var')}


def _fused(d, skip, relu, bn=True):
    from frcnn_amd import _lib
    x = d['x']
    n, cin, h, w = x.shape
    cout = d['w'].shape[0]
    y = torch.empty(n, cout, h, w, dtype=torch.float32, device=x.device)
    p = _lib.ptr
    _lib.call('frh_conv1x1_bn_act', p(x), p(d['w']), p(d['skip']) if skip else None, p(y),
              p(d['gamma']) if bn else None, p(d['beta']) if bn else None, p(d['mean']) if bn else None,
              p(d['var']) if bn else None, EPS, n, cin, cout, h * w, int(relu), _lib.stream_of(x))
    return y


@pytest.mark.parametrize('skip,relu', FLAGS)
@pytest.mark.parametrize('shape', SHAPES)
def test_accuracy_against_float64(dev, shape, skip, relu):
    """|y - y64| <= 2 (cin + 3) 2^-24 (|s| sum_k |w_k x_k| + |b| + |skip|) for every element:
    the forward bound of cin f32 multiply-adds in any order plus the three epilogue roundings."""
    c, d = _case(shape), _on_dev(shape, dev)
    cin = shape[1]
    y = _fused(d, skip, relu).cpu().double()
    s, b = c['s32'].double().view(1, -1, 1, 1), c['b32'].double().view(1, -1, 1, 1)
    y64 = c['acc64'] * s + b
    mag = s.abs() * c['absacc'] + b.abs()
    if skip:
        y64 = y64 + c['skip'].double()
        mag = mag + c['skip'].double().abs()
    if relu:
        y64 = y64.clamp_min(0.0)
    bound = 2.0 * (cin + 3) * 2.0 ** -24 * mag
    err = (y - y64).abs()
    print('shape', shape, 'skip', skip, 'relu', relu, 'max err / bound', float((err / bound).max()))
    assert torch.isfinite(y).all()
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize('skip,relu', FLAGS)
@pytest.mark.parametrize('shape', SHAPES)
def test_epilogue_bits_equal_bn_act(dev, shape, skip, relu):
    """The fused epilogue gives frh_bn_act's bits on the same accumulator: fused(BN, skip, relu)
    == frh_bn_act(fused(no BN, no skip, no relu), skip, BN, relu)."""
    from frcnn_amd import _lib
    d = _on_dev(shape, dev)
    y = _fused(d, skip, relu)
    raw = _fused(d, False, False, bn=False)
    n, cout, h, w = raw.shape
    ref = torch.empty_like(raw)
    p = _lib.ptr
    _lib.call('frh_bn_act', p(raw), p(d['skip']) if skip else None, p(ref), p(d['gamma']), p(d['beta']), p(d['mean']),
              p(d['var']), EPS, n, cout, h * w, int(relu), _lib.stream_of(raw))
    assert torch.equal(y, ref)


@pytest.mark.parametrize('shape', SHAPES)
def test_two_launches_give_the_same_bits(dev, shape):
    d = _on_dev(shape, dev)
    assert torch.equal(_fused(d, True, True), _fused(d, True, True))


def test_entry_refuses_what_it_cannot_run(dev):
    from frcnn_amd import _lib
    x = torch.zeros(1, 24, 4, 4, device=dev)
    w = torch.zeros(64, 24, device=dev)
    y = torch.zeros(1, 64, 4, 4, device=dev)
    p = _lib.ptr
    with pytest.raises(RuntimeError, match='multiple'):
        _lib.call('frh_conv1x1_bn_act', p(x), p(w), None, p(y), None, None, None, None, EPS, 1, 24, 64, 16, 1,
                  _lib.stream_of(x))
    with pytest.raises(RuntimeError, match='alias'):
        _lib.call('frh_conv1x1_bn_act', p(y), p(w), None, p(y), None, None, None, None, EPS, 1, 64, 64, 16, 1,
                  _lib.stream_of(x))


def test_entry_refuses_partial_overlap(dev):
    """y must not share a byte with skip or x (n = 1, cin = 16, cout = 64, hw = 4, the smallest
    shape the entry takes): refused by range, not by pointer equality, and before any launch, so
    the buffer keeps its contents."""
    from frcnn_amd import _lib
    buf = torch.arange(1.0, 385.0, device=dev)
    before = buf.clone()
    w = torch.ones(64, 16, device=dev)
    x = torch.ones(1, 16, 2, 2, device=dev)
    y = buf[:256]
    p = _lib.ptr

    def run(x, skip):
        _lib.call('frh_conv1x1_bn_act', p(x), p(w), p(skip) if skip is not None else None, p(y), None, None, None,
                  None, EPS, 1, 16, 64, 4, 0, _lib.stream_of(buf))
    with pytest.raises(RuntimeError, match='alias'):
        run(x, buf[64:320])      # skip starts 256 bytes into y
    with pytest.raises(RuntimeError, match='alias'):
        run(buf[224:288], None)  # x starts in y's last 128 bytes
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


def test_bn_without_running_statistics_takes_the_modules(dev, monkeypatch):
    """An eval-mode BatchNorm2d(track_running_stats=False) normalises with the batch's statistics:
    ops.conv1x1_bn_act and ops.bn_act call no library entry for it (read off ops.call) and return
    relu(bn(conv(x))), to test_dispatch's tolerance for two calls of one MIOpen conv."""
    from frcnn_amd import ops
    torch.manual_seed(7)
    conv = torch.nn.Conv2d(16, 64, 1, bias=False).to(dev)
    bn = torch.nn.BatchNorm2d(64, track_running_stats=False).to(dev).eval()
    x = torch.randn(1, 16, 2, 2, device=dev)
    names = support.spy_entries(monkeypatch).names
    with torch.no_grad():
        ref = torch.relu(bn(conv(x)))
        assert not ops.conv1x1_fused_ok(conv, bn, x)
        got = ops.conv1x1_bn_act(conv, bn, x)
        got_bn = ops.bn_act(conv(x), bn)
    assert [n for n in names if n.startswith('frh_')] == []
    tol = dict(rtol=1e-3, atol=1e-3 * float(ref.abs().max()))
    torch.testing.assert_close(got, ref, **tol)
    torch.testing.assert_close(got_bn, ref, **tol)


def _conv_bn(dev, cin, cout, seed, **kw):
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, 1, bias=kw.pop('bias', False), **kw).to(dev)
    bn = torch.nn.BatchNorm2d(cout).to(dev).eval()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5).mul_(torch.where(torch.rand(cout, device=dev) < 0.5, -1.0, 1.0))
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-1, 1)
        bn.running_var.uniform_(0.5, 2.0)
    return conv, bn


def test_dispatch(dev, monkeypatch):
    """With a gradient needed the op is conv + bn_act (same values, same gradients); under
    no_grad it is the fused entry; stride 2, a bias or a channels-last input keep the old path."""
    from frcnn_amd import _lib, ops
    conv, bn = _conv_bn(dev, 64, 128, 3)
    x = torch.randn(2, 64, 8, 12, device=dev)
    skip = torch.randn(2, 128, 8, 12, device=dev)
    gy = torch.randn(2, 128, 8, 12, device=dev)
    with torch.enable_grad():
        conv(x)  # MIOpen's first call of a shape may take another solver than the later ones
        assert not ops.conv1x1_fused_ok(conv, bn, x, skip)
        y = ops.conv1x1_bn_act(conv, bn, x, skip=skip)
        assert y.grad_fn is not None
        ref = ops.bn_act(conv(x), bn, skip=skip)
        assert torch.equal(y, ref)
        params = [conv.weight, bn.weight, bn.bias]
        for a, b in zip(torch.autograd.grad(y, params, gy), torch.autograd.grad(ref, params, gy)):
            assert torch.equal(a, b)
    with torch.no_grad():
        assert ops.conv1x1_fused_ok(conv, bn, x, skip)
        y = ops.conv1x1_bn_act(conv, bn, x, skip=skip)
        direct = torch.empty_like(y)
        p = _lib.ptr
        _lib.call('frh_conv1x1_bn_act', p(x), p(conv.weight), p(skip), p(direct), p(bn.weight), p(bn.bias),
                  p(bn.running_mean), p(bn.running_var), bn.eps, 2, 64, 128, 96, 1, _lib.stream_of(x))
        assert y.grad_fn is None and torch.equal(y, direct)
        torch.testing.assert_close(y, ref.detach(), rtol=1e-3, atol=1e-3 * float(ref.abs().max()))

        strided, bn_s = _conv_bn(dev, 64, 128, 4, stride=2)
        biased, bn_b = _conv_bn(dev, 64, 128, 5, bias=True)
        x_cl = x.contiguous(memory_format=torch.channels_last)
        # which entries run is read off ops.call; the values are MIOpen's, and two calls of one
        # MIOpen conv need not agree bit for bit (the first call of a shape may take another solver)
        spy = support.spy_entries(monkeypatch)
        for c, b, xi in ((strided, bn_s, x), (biased, bn_b, x), (conv, bn, x_cl)):
            assert not ops.conv1x1_fused_ok(c, b, xi)
            spy.clear()
            got = ops.conv1x1_bn_act(c, b, xi, relu=False)
            assert spy.names == ['frh_bn_act']
            want = ops.bn_act(c(xi), b, relu=False)
            torch.testing.assert_close(got, want, rtol=1e-3, atol=1e-3 * float(want.abs().max()))
        spy.clear()
        ops.conv1x1_bn_act(conv, bn, x, skip=skip)
        assert spy.names == ['frh_conv1x1_bn_act']


@pytest.mark.parametrize('args', [(256, 256), (64, 256, True)])
def test_bottleneck_matches_unfused(dev, args):
    """A Bottleneck under no_grad (fused 1x1 convs) against the same block through conv +
    bn_act, to the tolerance the trunk parity test grants MIOpen's own solver differences."""
    from frcnn_amd import ops
    from frcnn_amd.backbones import Bottleneck
    torch.manual_seed(11)
    blk = Bottleneck(*args).to(dev).eval()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.5, 0.5)
                m.running_mean.uniform_(-1, 1)
                m.running_var.uniform_(0.5, 2.0)
        x = torch.randn(2, args[0], 8, 12, device=dev)
        assert ops.conv1x1_fused_ok(blk.conv1, blk.bn1, x)
        y = blk(x)
        ref = support.bottleneck_unfused(blk, x)
    torch.testing.assert_close(y, ref, rtol=1e-3, atol=1e-3 * float(ref.abs().max()))
