"""frh_roi_conv3x3_bn_act: the Double-Head regression branch's 3x3 / stride-1 / padding-1 conv
over RoI tiles [r, cin, 7, 7] -> [r, cout, 7, 7] (NCHW f32 both sides) with the eval-mode BN
(+ ReLU) epilogue on the f32-MFMA accumulators (csrc/roi_conv3x3_kernels.h), and its Python
dispatch ops.roi_conv3x3_bn_act.

Shapes are (r, cin, cout).  A workgroup owns 4 RoIs (196 columns in 7 blocks of 32) x 128 output
channels (64 when cout % 128 != 0) and walks cin in chunks of 8; cin % 16 == 0, cout % 64 == 0.

Measured on MI355X (test_accuracy_against_float64's printed ratios over the four shapes and
flag pairs): max error / bound 9.5e-4 .. 9.7e-3; max error / the CPU f32 path's max error
1.2 .. 6.5 (bound: 8; the largest at cin = 256, where the CPU conv sums in blocks and this
kernel in one 2304-term chain)."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import support

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 16, 64),     # one RoI, the smallest legal channels, two K chunks
    (5, 32, 64),     # r not a multiple of the RoI group; column blocks straddle RoIs; the 64-channel form
    (33, 64, 128),   # several workgroups of RoIs plus a ragged tail; the 128-channel (four-wave) form
    (7, 256, 256),   # the workload's full K loop, two cout blocks
]
FLAGS = [(b, r) for b in (False, True) for r in (False, True)]
EPS = 1e-5


def _fused(x, w, bn, relu, eps=EPS, r=None, y=None, ws=None, xp=None):
    """frh_roi_conv3x3_bn_act on device tensors; bn = (gamma, beta, mean, var) or None."""
    from frcnn_amd import _lib
    cout, cin = w.shape[:2]
    r = x.shape[0] if r is None else r
    if y is None:
        y = torch.empty(r, cout, 7, 7, dtype=torch.float32, device=x.device)
    if ws is None:
        ws = torch.empty(max(_lib.query('frh_roi_conv3x3_workspace', cin, cout) // 4, 1), dtype=torch.float32,
                         device=x.device)
    p = _lib.ptr
    g, b, m, v = bn if bn is not None else (None, None, None, None)
    _lib.call('frh_roi_conv3x3_bn_act', xp if xp is not None else p(x), p(w), p(y), p(g), p(b), p(m), p(v),
              float(eps), r, cin, cout, int(relu), p(ws), _lib.stream_of(x))
    return y


def _gen(shape):
    r, cin, cout = shape
    return torch.Generator().manual_seed(5000 + r + 3 * cin + 11 * cout)


@functools.lru_cache(maxsize=None)
def _int_case(shape):
    """Integer-valued inputs (CPU f32) and the exact results for the four flag pairs."""
    r, cin, cout = shape
    g = _gen(shape)
    x = torch.randint(-2, 3, (r, cin, 7, 7), generator=g).float()
    w = torch.randint(-1, 2, (cout, cin, 3, 3), generator=g).float()
    gamma = 2.0 ** torch.randint(-1, 3, (cout,), generator=g).float()
    beta = torch.randint(-3, 4, (cout,), generator=g).float()
    mean = torch.randint(-3, 4, (cout,), generator=g).float()
    var = torch.full((cout,), 4.0)
    acc = F.conv2d(x.double(), w.double(), None, padding=1)
    assert float(acc.abs().max()) * 4 + 64 < 2 ** 24
    s = gamma.double() / 2.0
    b = beta.double() - mean.double() * s
    want = {}
    for bn, relu in FLAGS:
        v = acc * s.view(1, -1, 1, 1) + b.view(1, -1, 1, 1) if bn else acc
        want[(bn, relu)] = (v.clamp_min(0.0) if relu else v).float()
    return dict(x=x, w=w, bn=(gamma, beta, mean, var), want=want)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Random inputs (CPU f32) and the float64 / CPU-f32 references, computed once."""
    r, cin, cout = shape
    g = _gen(shape)
    x = torch.randn(r, cin, 7, 7, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g)
    gamma = torch.randn(cout, generator=g)
    beta = torch.randn(cout, generator=g)
    mean = torch.randn(cout, generator=g)
    var = torch.rand(cout, generator=g) * 1.5 + 0.5
    acc64 = F.conv2d(x.double(), w.double(), None, padding=1)
    mag = F.conv2d(x.double().abs(), w.double().abs(), None, padding=1)
    acc32 = F.conv2d(x, w, None, padding=1)
    s = (gamma.double() / torch.sqrt(var.double() + EPS)).view(1, -1, 1, 1)
    b = beta.double().view(1, -1, 1, 1) - mean.double().view(1, -1, 1, 1) * s
    bn32 = F.batch_norm(acc32, mean, var, gamma, beta, False, 0.0, EPS)
    return dict(x=x, w=w, bn=(gamma, beta, mean, var), acc64=acc64, mag=mag, acc32=acc32, s=s, b=b, bn32=bn32)


@functools.lru_cache(maxsize=None)
def _on_dev(kind, shape, dev):
    c = _int_case(shape) if kind == 'int' else _case(shape)
    return dict(x=c['x'].to(dev), w=c['w'].to(dev), bn=tuple(t.to(dev) for t in c['bn']))


@pytest.mark.parametrize('bn,relu', FLAGS)
@pytest.mark.parametrize('shape', SHAPES)
def test_exact_integers(dev, shape, bn, relu):
    """Integer x in [-2, 2], w in {-1, 0, 1}, gamma a power of two, var = 4, eps = 0, integer mean
    and beta: every intermediate is a multiple of 1/4 below 2^24, so the result is exact in any
    summation order and must equal the CPU computation bit for bit."""
    c, d = _int_case(shape), _on_dev('int', shape, dev)
    y = _fused(d['x'], d['w'], d['bn'] if bn else None, relu, eps=0.0)
    assert torch.equal(y.cpu(), c['want'][(bn, relu)])


@pytest.mark.parametrize('shape', SHAPES)
def test_no_leak_between_rois(dev, shape):
    """RoI i filled with i + 1, w = 1, no BN: exactly (i + 1) x cin x (valid taps: 4, 6 or 9)."""
    r, cin, cout = shape
    x = (torch.arange(r, dtype=torch.float32) + 1).view(r, 1, 1, 1).expand(r, cin, 7, 7).contiguous().to(dev)
    w = torch.ones(cout, cin, 3, 3, device=dev)
    taps = F.conv2d(torch.ones(1, 1, 7, 7), torch.ones(1, 1, 3, 3), padding=1)
    assert set(taps.unique().tolist()) == {4.0, 6.0, 9.0}
    want = (torch.arange(r, dtype=torch.float32) + 1).view(r, 1, 1, 1) * cin * taps.expand(r, cout, 7, 7)
    assert torch.equal(_fused(x, w, None, False).cpu(), want)


@pytest.mark.parametrize('bn,relu', FLAGS)
@pytest.mark.parametrize('shape', SHAPES)
def test_accuracy_against_float64(dev, shape, bn, relu):
    """|y - y64| <= 2 (9 cin + 8) 2^-24 mag for every element, mag the float64 conv of |x|, |w|
    pushed through |s| and + |b|: the forward bound of a 9 cin-term fmaf chain plus the
    epilogue's roundings (three in s, two in b, two on the accumulator), doubled; and
    max|y - y64| <= 8 max|y32 - y64|, y32 torch's CPU f32 conv + BN + ReLU."""
    c, d = _case(shape), _on_dev('rand', shape, dev)
    cin = shape[1]
    y = _fused(d['x'], d['w'], d['bn'] if bn else None, relu).cpu().double()
    y64, y32, mag = c['acc64'], c['acc32'], c['mag']
    if bn:
        y64, y32, mag = y64 * c['s'] + c['b'], c['bn32'], mag * c['s'].abs() + c['b'].abs()
    if relu:
        y64, y32 = y64.clamp_min(0.0), y32.clamp_min(0.0)
    bound = 2.0 * (9 * cin + 8) * 2.0 ** -24 * mag
    err = (y - y64).abs()
    err32 = (y32.double() - y64).abs()
    print('shape', shape, 'bn', bn, 'relu', relu, 'max err / bound', float((err / bound).max()),
          'max err / max cpu-f32 err', float(err.max() / err32.max()))
    assert torch.isfinite(y).all()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float(err.max()) <= 8.0 * float(err32.max())


@pytest.mark.parametrize('a,b', [(0, 1), (3, 20), (32, 33)])
def test_position_independence(dev, a, b):
    """A call on x[a:b] gives the bits of rows a:b of the full call: a RoI's result depends
    neither on r nor on its index (its place in a workgroup's group of four)."""
    shape = SHAPES[2]
    d = _on_dev('rand', shape, dev)
    full = _fused(d['x'], d['w'], d['bn'], True)
    part = _fused(d['x'][a:b].contiguous(), d['w'], d['bn'], True)
    assert torch.equal(part, full[a:b])


@pytest.mark.parametrize('shape', SHAPES)
def test_repeat_launches_same_bits(dev, shape):
    d = _on_dev('rand', shape, dev)
    assert torch.equal(_fused(d['x'], d['w'], d['bn'], True), _fused(d['x'], d['w'], d['bn'], True))


def test_bad_arguments(dev):
    """FRH_EINVAL (-1) with a message for cin = 8, cout = 32, a misaligned pointer and y aliasing
    x; r = 0 is OK and leaves y untouched."""
    x = torch.zeros(2, 64, 7, 7, device=dev)
    w = torch.zeros(64, 64, 3, 3, device=dev)
    with pytest.raises(RuntimeError, match=r'\(-1\).*cin'):
        _fused(torch.zeros(2, 8, 7, 7, device=dev), torch.zeros(64, 8, 3, 3, device=dev), None, False)
    with pytest.raises(RuntimeError, match=r'\(-1\).*cout'):
        _fused(torch.zeros(2, 16, 7, 7, device=dev), torch.zeros(32, 16, 3, 3, device=dev), None, False)
    big = torch.zeros(2 * 64 * 49 + 4, device=dev)
    with pytest.raises(RuntimeError, match=r'\(-1\).*aligned'):
        _fused(x, w, None, False, xp=ctypes.c_void_p(big.data_ptr() + 4))
    with pytest.raises(RuntimeError, match=r'\(-1\).*overlap'):
        _fused(x, w, None, False, y=x)
    y = torch.full((2, 64, 7, 7), 7.0, device=dev)
    _fused(x, w, None, False, r=0, y=y)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


def _conv_bn(dev, cin, cout, stride=1, bias=False, seed=9):
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, 3, stride=stride, padding=1, bias=bias).to(dev)
    bn = torch.nn.BatchNorm2d(cout).to(dev)
    with torch.no_grad():
        bn.weight.normal_()
        bn.bias.normal_()
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
    return conv, bn


def test_dispatch(dev, monkeypatch):
    """An eval head under no_grad takes the fused entry; a training BN, a gradient needed, stride 2
    and a biased conv take relu(bn(conv(x))) with no library call, and give PyTorch's result."""
    from frcnn_amd import ops
    spy = support.spy_entries(monkeypatch)
    x = torch.randn(9, 32, 7, 7, device=dev)

    conv, bn = _conv_bn(dev, 32, 64)
    bn.eval()
    with torch.no_grad():
        assert ops.roi_conv3x3_fused_ok(conv, bn, x)
        got = ops.roi_conv3x3_bn_act(conv, bn, x)
        assert spy.names == ['frh_roi_conv3x3_bn_act']
        want = torch.relu(bn(conv(x)))
        # MIOpen's own sum order differs: close, not equal
        assert torch.allclose(got, want, rtol=1e-4, atol=1e-4)

    def falls_back(conv, bn, xi, grad):
        spy.clear()
        ctx = torch.enable_grad() if grad else torch.no_grad()
        with ctx:
            assert not ops.roi_conv3x3_fused_ok(conv, bn, xi)
            torch.relu(bn(conv(xi)))  # MIOpen settles on its solver for this shape
            got = ops.roi_conv3x3_bn_act(conv, bn, xi)
            want = torch.relu(bn(conv(xi)))
        assert spy.names == []
        assert torch.equal(got, want)
        return got

    # eval BN, but a gradient is needed (trainable weights, grad mode on)
    got = falls_back(conv, bn, x, grad=True)
    assert got.requires_grad
    xg = x.clone().requires_grad_(True)
    for p in list(conv.parameters()) + list(bn.parameters()):
        p.requires_grad_(False)
    falls_back(conv, bn, xg, grad=True)
    with torch.no_grad():  # the same frozen modules and input, nothing to differentiate: fused
        assert ops.roi_conv3x3_fused_ok(conv, bn, xg)
    # training-mode BN: batch statistics (the output does not depend on the running ones)
    conv_t, bn_t = _conv_bn(dev, 32, 64)
    bn_t.train()
    falls_back(conv_t, bn_t, x, grad=False)
    # stride 2, a biased conv
    conv_s, bn_s = _conv_bn(dev, 32, 64, stride=2)
    falls_back(conv_s, bn_s.eval(), x, grad=False)
    conv_b, bn_b = _conv_bn(dev, 32, 64, bias=True)
    falls_back(conv_b, bn_b.eval(), x, grad=False)
