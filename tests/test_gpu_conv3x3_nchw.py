"""frh_conv3x3_nchw_bn_act: the bottlenecks' 3x3 / stride-1 / padding-1 convs on contiguous NCHW
f32 as Winograd F(2x2, 3x3) on the f32 MFMA with the frozen-BN (+ ReLU) epilogue on the
accumulators (csrc/conv3x3_nchw_kernels.h), its Python dispatch (ops.conv3x3_nchw_bn_act) and
the Bottleneck that calls it.

Shapes are (n, cin, cout, h, w).  A wave owns 16 tiles along w x NT tile rows x NC blocks of 16
output channels and walks cin in steps of 4; cin % 4 == 0, cout % 16 == 0 (% 32 for NC = 2),
w % 2 == 0.  Every kernel form (NT, NC) = (2, 1), (1, 2), (1, 1) is reached at every
shape through the tools library's frh_conv3x3_nchw_bn_act_form; form None is the product entry
with its own choice.

Measured on MI355X (test_accuracy_against_float64's printed ratios over the four shapes and
forms; every form gives the same ratios): max error / bound 7.7e-4 .. 3.5e-3; max error / the
CPU direct f32 conv's max error 0.50 .. 1.7 (bound: 8).

The entry takes no strides, so a non-contiguous x cannot reach it: that case is refused by the
predicate (test_noncontiguous_x_takes_the_module), the others by the entry itself."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import support

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 16, 64, 3, 8),       # smaller than one tile block, odd h, four cin steps
    (2, 64, 64, 19, 32),     # stage 4's plane: half-empty last tile row, batch stride
    (2, 128, 128, 10, 16),   # many cin steps, several channel blocks, half-empty tile run
    (1, 32, 192, 17, 36),    # ragged tile block in both directions, an odd count of 32-channel blocks
]
FORMS = [None, 0, 1, 2]
EPS = 1e-5

@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs (CPU f32) and the references of one shape, computed once."""
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(4000 + cin + 7 * cout + h * w)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g)
    bn = support.bn_params(cout, g)
    y64 = F.conv2d(x.double(), wt.double(), None, padding=1)
    y32 = F.conv2d(x, wt, None, padding=1)
    return dict(x=x, w=wt, bn=bn, y64=y64, y32=y32, mag=support.wino_magnitude(x, wt))


@functools.lru_cache(maxsize=None)
def _on_dev(shape, dev):
    c = _case(shape)
    return dict(x=c['x'].to(dev), w=c['w'].to(dev), bn=[t.to(dev) for t in c['bn']])


def _fused(x, w, bn=None, relu=False, form=None, y=None, ws=None, n=None):
    """frh_conv3x3_nchw_bn_act (form None) or the tools library's _form entry on contiguous x, w."""
    from frcnn_amd import _lib
    cin, h, wd = x.shape[1:]
    n = x.shape[0] if n is None else n
    cout = w.shape[0]
    assert x.is_contiguous() and w.is_contiguous()
    y = torch.empty(n, cout, h, wd, dtype=torch.float32, device=x.device) if y is None else y
    ws = torch.empty(16 * cin * cout, dtype=torch.float32, device=x.device) if ws is None else ws
    p = _lib.ptr
    bnp = [p(t) for t in bn] + [EPS] if bn is not None else [None, None, None, None, 0.0]
    a = [p(x), p(w)] + bnp + [p(y), p(ws), n, cin, cout, h, wd, int(relu), _lib.stream_of(x)]
    if form is None:
        _lib.call('frh_conv3x3_nchw_bn_act', *a)
    else:
        st = support.tools().frh_conv3x3_nchw_bn_act_form(form, *a)
        assert st == 0, _lib.load().frh_last_error()
    return y


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', SHAPES)
def test_exact_borders(dev, shape, form):
    """x = 1, w = 1, no BN: every Winograd intermediate is a multiple of 1/4 below 2^24, so the
    result is exactly cin x (number of valid taps): 4, 6 or 9 x cin."""
    n, cin, cout, h, w = shape
    x = torch.ones(n, cin, h, w, device=dev)
    wt = torch.ones(cout, cin, 3, 3, device=dev)
    taps = F.conv2d(torch.ones(1, 1, h, w), torch.ones(1, 1, 3, 3), padding=1)
    want = (taps * cin).expand(n, cout, h, w)
    assert set(taps.unique().tolist()) <= {4.0, 6.0, 9.0}
    assert torch.equal(_fused(x, wt, form=form).cpu(), want)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', SHAPES)
def test_accuracy_against_float64(dev, shape, form):
    """On the raw output: |y - y64| <= 2 (cin + 16) 2^-24 magW for every element, magW the forward
    bound of the algorithm's own sums (cin multiply-adds plus 4 roundings in each of the three
    transforms); and max|y - y64| <= 8 max|y32 - y64|, y32 torch's CPU f32 direct conv."""
    c, d = _case(shape), _on_dev(shape, dev)
    cin = shape[1]
    y = _fused(d['x'], d['w'], form=form).cpu().double()
    y64, y32, mag = c['y64'], c['y32'], c['mag']
    bound = 2.0 * (cin + 16) * 2.0 ** -24 * mag
    err = (y - y64).abs()
    err32 = (y32.double() - y64).abs()
    print('shape', shape, 'form', form, 'max err / bound', float((err / bound).max()),
          'max err / max direct-f32 err', float(err.max() / err32.max()))
    assert torch.isfinite(y).all()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float(err.max()) <= 8.0 * float(err32.max())


@pytest.mark.parametrize('relu', (False, True))
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', SHAPES)
def test_epilogue_bits_equal_bn_act(dev, shape, form, relu):
    """fused(BN with signed gammas, relu) == frh_bn_act(fused raw output of the same entry)."""
    from frcnn_amd import _lib
    d = _on_dev(shape, dev)
    y = _fused(d['x'], d['w'], d['bn'], relu, form)
    raw = _fused(d['x'], d['w'], form=form)
    n, cout, h, w = raw.shape
    ref = torch.empty_like(raw)
    p = _lib.ptr
    _lib.call('frh_bn_act', p(raw), None, p(ref), *[p(t) for t in d['bn']], EPS, n, cout, h * w, int(relu),
              _lib.stream_of(raw))
    assert torch.equal(y, ref)
    if relu:  # the ReLU alone, without a BN
        assert torch.equal(_fused(d['x'], d['w'], None, True, form), raw.clamp_min(0.0))


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', SHAPES)
def test_repeatability(dev, shape, form):
    """Two launches give equal bits; image i of the whole batch equals the n = 1 call on it."""
    d = _on_dev(shape, dev)
    y = _fused(d['x'], d['w'], d['bn'], True, form)
    assert torch.equal(y, _fused(d['x'], d['w'], d['bn'], True, form))
    for i in range(shape[0]):
        assert torch.equal(y[i:i + 1], _fused(d['x'][i:i + 1].contiguous(), d['w'], d['bn'], True, form))


def test_entry_refuses_what_it_cannot_run(dev):
    """Each refusal is an error and no launch: the sentinel-filled output is unchanged."""
    x = torch.zeros(1, 16, 4, 8, device=dev)
    w = torch.zeros(32, 16, 3, 3, device=dev)
    bn = [torch.ones(32, device=dev) for _ in range(4)]
    y = torch.full((1, 32, 4, 8), 7.0, device=dev)
    big = torch.zeros(2 * 16 * 16 * 32, device=dev)

    def refused(match, *a, **kw):
        with pytest.raises(RuntimeError, match=match):
            _fused(*a, **kw)
        torch.cuda.synchronize()
        assert bool((y == 7.0).all())

    wide = torch.zeros(1, 16, 4, 16, device=dev)
    refused('contiguous|even', wide[:, :, :, :7].contiguous(), w, y=y)        # w = 7
    refused('multiple', torch.zeros(1, 6, 4, 8, device=dev), torch.zeros(32, 6, 3, 3, device=dev), y=y)
    refused('multiple', x, torch.zeros(24, 16, 3, 3, device=dev), y=y)        # cout = 24
    refused('alias', x, w, y=x)                                              # y over x (cin = cout planes overlap)
    refused('alias', x, w, y=y, ws=y)                                        # workspace over y
    refused('alias', x, w, y=y, ws=x.view(-1))                               # workspace over x
    refused('alias', x, w, y=y, ws=w.view(-1))                               # workspace over w
    refused('mean and var', x, w, [bn[0], bn[1], bn[2], None], y=y)
    refused('mean and var', x, w, [bn[0], bn[1], None, bn[3]], y=y)
    from frcnn_amd import _lib
    p = _lib.ptr
    ws = torch.empty(16 * 16 * 32, device=dev)
    for xa, ya in ((ctypes.c_void_p(big.data_ptr() + 4), p(y)), (p(x), ctypes.c_void_p(y.data_ptr() + 8))):
        with pytest.raises(RuntimeError, match='aligned'):
            _lib.call('frh_conv3x3_nchw_bn_act', xa, p(w), None, None, None, None, 0.0, ya, p(ws), 1, 16, 32, 4, 8, 0,
                      _lib.stream_of(x))
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    # the form with two channel blocks needs cout % 32 == 0
    w48 = torch.zeros(48, 16, 3, 3, device=dev)
    y48 = torch.full((1, 48, 4, 8), 7.0, device=dev)
    form1 = support.tools().frh_conv3x3_nchw_bn_act_form
    assert form1(1, p(x), p(w48), None, None, None, None, 0.0, p(y48), p(big), 1, 16, 48, 4, 8, 0,
                 _lib.stream_of(x)) != 0
    assert bool((y48 == 7.0).all())
    assert torch.equal(_fused(x, w48, y=y48), torch.zeros_like(y48))  # the product entry picks a form that fits


def test_noncontiguous_x_takes_the_module(dev, monkeypatch):
    """A non-contiguous x never reaches the entry (the entry takes no strides): the op runs the
    module on it."""
    from frcnn_amd import ops
    monkeypatch.setattr(ops, '_CONV3X3_NCHW_EXCLUDED', frozenset())
    conv = torch.nn.Conv2d(16, 32, 3, padding=1, bias=False).to(dev)
    x = torch.randn(2, 16, 8, 16, device=dev)[:, :, :, ::2]
    with torch.no_grad():
        assert not ops.conv3x3_nchw_fused_ok(conv, x)
        assert torch.equal(ops.conv3x3_nchw_bn_act(conv, x), conv(x))


def _randomise_bn(bn):
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5).mul_(torch.where(torch.rand_like(bn.weight) < 0.5, -1.0, 1.0))
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-1, 1)
        bn.running_var.uniform_(0.5, 2.0)


def test_dispatch(dev, monkeypatch):
    """With the table empty the op is the fused entry under no_grad; with the table full, with
    grad mode on (whether or not a gradient is needed), for a stride-2 conv, a biased conv, a training-mode BN and CPU tensors it is
    what ran before."""
    from frcnn_amd import ops
    torch.manual_seed(21)
    conv = torch.nn.Conv2d(64, 64, 3, padding=1, bias=False).to(dev)
    bn = torch.nn.BatchNorm2d(64).to(dev).eval()
    _randomise_bn(bn)
    x = torch.randn(2, 64, 8, 12, device=dev)
    ran = support.spy_entries(monkeypatch).ran
    bnp = [bn.weight, bn.bias, bn.running_mean, bn.running_var]
    full = frozenset([(64, 64), (128, 128), (256, 256), (512, 512)])

    monkeypatch.setattr(ops, '_CONV3X3_NCHW_EXCLUDED', frozenset())
    with torch.enable_grad():
        assert conv.weight.requires_grad and not ops.conv3x3_nchw_fused_ok(conv, x, bn)
        y, got = ran(lambda: ops.conv3x3_nchw_bn_act(conv, x, bn, relu=True))
        assert got == ['frh_bn_act'] and y.grad_fn is not None
        y, got = ran(lambda: ops.conv3x3_nchw_bn_act(conv, x))
        assert got == [] and y.grad_fn is not None
        xg = x.clone().requires_grad_()
        for prm in list(conv.parameters()) + list(bn.parameters()):
            prm.requires_grad_(False)
        assert not ops.conv3x3_nchw_fused_ok(conv, xg, bn)
        # a frozen stage inside a training step (grad mode on, nothing here needing a gradient)
        # keeps the module too: training steps compute what they computed before
        assert not ops.conv3x3_nchw_fused_ok(conv, x, bn)
        y, got = ran(lambda: ops.conv3x3_nchw_bn_act(conv, x, bn, relu=True))
        assert got == ['frh_bn_act'] and y.grad_fn is None
        for prm in list(conv.parameters()) + list(bn.parameters()):
            prm.requires_grad_(True)
    with torch.no_grad():
        ref = conv(x)
        assert ops.conv3x3_nchw_fused_ok(conv, x, bn) and ops.conv3x3_nchw_fused_ok(conv, x)
        y, got = ran(lambda: ops.conv3x3_nchw_bn_act(conv, x))
        assert got == ['frh_conv3x3_nchw_bn_act'] and torch.equal(y, _fused(x, conv.weight))
        torch.testing.assert_close(y, ref, rtol=1e-3, atol=1e-3 * float(ref.abs().max()))
        y, got = ran(lambda: ops.conv3x3_nchw_bn_act(conv, x, bn, relu=True))
        assert got == ['frh_conv3x3_nchw_bn_act']
        bn.eps = EPS
        assert torch.equal(y, _fused(x, conv.weight, bnp, True))
        refb = ops.bn_act(ref, bn)
        torch.testing.assert_close(y, refb, rtol=1e-3, atol=1e-3 * float(refb.abs().max()))

        # the table full: the module, then frh_bn_act where there is a BN
        monkeypatch.setattr(ops, '_CONV3X3_NCHW_EXCLUDED', full)
        assert not ops.conv3x3_nchw_fused_ok(conv, x, bn)
        y, got = ran(lambda: ops.conv3x3_nchw_bn_act(conv, x, bn, relu=True))
        assert got == ['frh_bn_act'] and torch.equal(y, refb)
        y, got = ran(lambda: ops.conv3x3_nchw_bn_act(conv, x))
        assert got == [] and torch.equal(y, ref)
        monkeypatch.setattr(ops, '_CONV3X3_NCHW_EXCLUDED', frozenset())

        strided = torch.nn.Conv2d(64, 64, 3, stride=2, padding=1, bias=False).to(dev)
        assert not ops.conv3x3_nchw_fused_ok(strided, x, bn)
        y, got = ran(lambda: ops.conv3x3_nchw_bn_act(strided, x, bn, relu=True))
        assert got == ['frh_bn_act'] and y.shape == (2, 64, 4, 6)
        biased = torch.nn.Conv2d(64, 64, 3, padding=1).to(dev)
        assert not ops.conv3x3_nchw_fused_ok(biased, x)
        y, got = ran(lambda: ops.conv3x3_nchw_bn_act(biased, x))
        assert got == [] and torch.equal(y, biased(x))
        training = torch.nn.BatchNorm2d(64).to(dev)
        assert not ops.conv3x3_nchw_fused_ok(conv, x, training)
        y, got = ran(lambda: ops.conv3x3_nchw_bn_act(conv, x, training, relu=True))
        assert got == []
        cpu_conv, x_cpu = torch.nn.Conv2d(64, 64, 3, padding=1, bias=False), x.cpu()
        assert not ops.conv3x3_nchw_fused_ok(cpu_conv, x_cpu)
        y, got = ran(lambda: ops.conv3x3_nchw_bn_act(cpu_conv, x_cpu, relu=True))
        assert got == [] and torch.equal(y, cpu_conv(x_cpu).relu())


@pytest.mark.parametrize('args', [(256, 256), (2048, 2048)])
def test_bottleneck_with_conv2_dispatched(dev, args, monkeypatch):
    """With conv2's class dispatched, Bottleneck(256, 256) (conv3 takes bn2 on its input side:
    conv2 writes its raw output) and the stage-4-like Bottleneck(2048, 2048) (conv3's input-side
    form is excluded: bn2 + ReLU in conv2's epilogue) match the unfused chain to the tolerance the
    trunk parity tests grant, and no separate bn2 pass is left.  The stage-4 block's conv1 class
    (2048 -> 512) is one of the 1x1 kernel's own exclusions and would record its frh_bn_act, so
    that table is emptied here: then the block records no frh_bn_act at all."""
    from frcnn_amd import ops
    blk, x = support.block(dev, args, _randomise_bn)
    monkeypatch.setattr(ops, '_CONV3X3_NCHW_EXCLUDED', frozenset())
    monkeypatch.setattr(ops, '_CONV1X1_EXCLUDED', frozenset())
    ran = support.spy_entries(monkeypatch).ran
    with torch.no_grad():
        ref = support.bottleneck_unfused(blk, x)
        y, names = ran(lambda: blk(x))
    assert names.count('frh_conv3x3_nchw_bn_act') == 1 and 'frh_bn_act' not in names
    assert names.count('frh_conv1x1_bn_act_pre') == (1 if args[0] == 256 else 0)
    torch.testing.assert_close(y, ref, rtol=1e-3, atol=1e-3 * float(ref.abs().max()))
    # the table full: the block is what it was
    monkeypatch.setattr(ops, '_CONV3X3_NCHW_EXCLUDED', frozenset([(64, 64), (128, 128), (256, 256), (512, 512)]))
    with torch.no_grad():
        y, names = ran(lambda: blk(x))
    assert 'frh_conv3x3_nchw_bn_act' not in names
    assert names.count('frh_conv1x1_bn_act_pre') == (1 if args[0] == 256 else 0)
    assert names.count('frh_bn_act') == (0 if args[0] == 256 else 1)
    torch.testing.assert_close(y, ref, rtol=1e-3, atol=1e-3 * float(ref.abs().max()))
