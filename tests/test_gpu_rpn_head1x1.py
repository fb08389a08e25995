"""frh_rpn_head1x1_levels: the RPN head's classifier and regressor (two 1x1 convolutions) over
every pyramid level in one launch (csrc/rpn_head1x1_kernels.h), its Python dispatch
(ops.rpn_head1x1_levels) and the RPNHead that calls it.

Cases are (n, cin, c_cls, c_reg, levels, index of the level that is a [:, :, ::2, ::2] view).
A tile is 64 pixels of a level's flattened [n, h, w] index and cin is staged in chunks of 128
channels, 16 per MFMA group: the cases cover ragged tiles, a one-pixel level, two chunks, and a
cin that is neither a multiple of 16 nor of the chunk."""
import functools

import pytest
import torch

import support

pytestmark = pytest.mark.gpu

CASES = [
    (2, 256, 3, 12, ((5, 7), (3, 4), (1, 1)), 1),  # the cfg2 channels; the second level a strided view
    (1, 64, 2, 8, ((9, 6),), None),                # a single level, other channel counts
    (2, 40, 3, 12, ((4, 4), (2, 2)), None),        # cin % 8 == 0, not a multiple of 16 or 32
]


def _channels_last_level(n, cin, h, w, fill, view):
    """A channels-last [n, cin, h, w] level; view: cut as [:, :, ::2, ::2] from one twice the size."""
    if not view:
        return fill(n, cin, h, w).contiguous(memory_format=torch.channels_last)
    big = fill(n, cin, 2 * h, 2 * w).contiguous(memory_format=torch.channels_last)
    return big[:, :, ::2, ::2]


@functools.lru_cache(maxsize=None)
def _case(case, kind):
    """Inputs (CPU f32) and the float64 references of one case, computed once.
    kind 'int': integers in [-4, 4] (every partial sum exact in f32); 'randn': seeded normals."""
    n, cin, cc, cr, levels, view = case
    g = torch.Generator().manual_seed(77 + cin + 5 * cc + len(levels))
    if kind == 'int':
        fill = lambda *s: torch.randint(-4, 5, s, generator=g).float()
    else:
        fill = lambda *s: torch.randn(*s, generator=g)
    xs = [_channels_last_level(n, cin, h, w, fill, i == view) for i, (h, w) in enumerate(levels)]
    wc, wr = fill(cc, cin), fill(cr, cin)
    bc, br = fill(cc), fill(cr)
    ref, mag = [], []
    for x in xs:
        x64 = x.double()
        for wt, b in ((wc, bc), (wr, br)):
            ref.append(torch.einsum('oc,nchw->nohw', wt.double(), x64) + b.double().view(1, -1, 1, 1))
            mag.append(torch.einsum('oc,nchw->nohw', wt.double().abs(), x64.abs()) + b.double().abs().view(1, -1, 1, 1))
    return dict(xs=xs, wc=wc, wr=wr, bc=bc, br=br, ref=ref, mag=mag)


def _to_dev(x, dev):
    """x on the device with its strides kept (a strided view stays a view of a larger tensor)."""
    if x.is_contiguous(memory_format=torch.channels_last):
        return x.to(dev)
    n, c, h, w = x.shape
    big = torch.zeros(n, c, 2 * h, 2 * w, device=dev).contiguous(memory_format=torch.channels_last)
    v = big[:, :, ::2, ::2]
    v.copy_(x.to(dev))
    assert v.stride() == x.stride()
    return v


@functools.lru_cache(maxsize=None)
def _on_dev(case, kind, dev):
    c = _case(case, kind)
    d = {k: c[k].to(dev) for k in ('wc', 'wr', 'bc', 'br')}
    d['xs'] = [_to_dev(x, dev) for x in c['xs']]
    return d


def _nan_level(n, c, x):
    return torch.full((n, c, x.shape[2], x.shape[3]), float('nan'), device=x.device).contiguous(
        memory_format=torch.channels_last)


def _entry(xs, wc, bc, wr, br, mk=_nan_level):
    """One frh_rpn_head1x1_levels launch; returns the outputs interleaved (cls_0, reg_0, cls_1, ...).
    mk(n, c, x) makes the channels-last output of c channels for the level x (NaN-filled here;
    tests/test_gpu_guarded_convs.py passes a torch.empty one under its allocator)."""
    from frcnn_amd import _lib
    n, cin = xs[0].shape[:2]
    cc, cr = wc.shape[0], wr.shape[0]
    mk = functools.partial(mk, n)
    cls, reg = [mk(cc, x) for x in xs], [mk(cr, x) for x in xs]
    p = _lib.ptr
    _lib.call('frh_rpn_head1x1_levels', len(xs), _lib.ptr_array(xs), _lib.ptr_array(cls), _lib.ptr_array(reg), p(wc),
              p(bc), p(wr), p(br), n, cin, cc, cr, _lib.i32_array([v for x in xs for v in x.shape[2:]]),
              _lib.i64_array([v for x in xs for v in (x.stride(0), x.stride(2), x.stride(3))]),
              _lib.stream_of(xs[0]))
    return [t for pair in zip(cls, reg) for t in pair]


def _run(d):
    return _entry(d['xs'], d['wc'], d['bc'], d['wr'], d['br'])


@pytest.mark.parametrize('case', CASES)
def test_exact_on_integers(dev, case):
    """Integer inputs in [-4, 4]: every partial sum is below 2^24, so the f32 result is the
    float64 one bit for bit, whatever the order (this pins the MFMA operand and result maps)."""
    c, d = _case(case, 'int'), _on_dev(case, 'int', dev)
    for y, y64 in zip(_run(d), c['ref']):
        assert torch.equal(y.cpu().double(), y64)


@pytest.mark.parametrize('case', CASES)
def test_accuracy_against_float64(dev, case):
    """|y - y64| <= 2 (cin + 1) 2^-24 (sum_k |w_k x_k| + |b|) for every element: the forward bound
    of cin f32 multiply-adds in any order plus the bias add."""
    c, d = _case(case, 'randn'), _on_dev(case, 'randn', dev)
    cin = case[1]
    for y, y64, mag in zip(_run(d), c['ref'], c['mag']):
        y = y.cpu().double()
        bound = 2.0 * (cin + 1) * 2.0 ** -24 * mag
        err = (y - y64).abs()
        print('case', case[:4], tuple(y.shape), 'max err / bound', float((err / bound).max()))
        assert torch.isfinite(y).all()
        assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize('case', CASES)
def test_two_launches_give_the_same_bits(dev, case):
    d = _on_dev(case, 'randn', dev)
    for a, b in zip(_run(d), _run(d)):
        assert torch.equal(a, b)


@pytest.mark.parametrize('case', CASES)
def test_levels_do_not_depend_on_each_other(dev, case):
    """One multi-level launch equals the per-level launches bit for bit."""
    d = _on_dev(case, 'randn', dev)
    together = _run(d)
    for i, x in enumerate(d['xs']):
        alone = _entry([x], d['wc'], d['bc'], d['wr'], d['br'])
        assert torch.equal(alone[0], together[2 * i]) and torch.equal(alone[1], together[2 * i + 1])


def _modules(dev, case, d=None):
    n, cin, cc, cr = case[:4]
    torch.manual_seed(5)
    classifier = torch.nn.Conv2d(cin, cc, 1).to(dev)
    regressor = torch.nn.Conv2d(cin, cr, 1).to(dev)
    if d is not None:
        with torch.no_grad():
            classifier.weight.copy_(d['wc'].view(cc, cin, 1, 1)), classifier.bias.copy_(d['bc'])
            regressor.weight.copy_(d['wr'].view(cr, cin, 1, 1)), regressor.bias.copy_(d['br'])
    return classifier, regressor


@pytest.mark.parametrize('case', CASES)
def test_shape_and_strides_are_the_modules(dev, case):
    from frcnn_amd import ops
    d = _on_dev(case, 'randn', dev)
    classifier, regressor = _modules(dev, case, d)
    with torch.no_grad():
        assert ops.rpn_head1x1_fused_ok(classifier, regressor, d['xs'])
        cls, reg = ops.rpn_head1x1_levels(classifier, regressor, d['xs'])
        for x, c, r in zip(d['xs'], cls, reg):
            for got, want in ((c, classifier(x)), (r, regressor(x))):
                assert got.shape == want.shape and got.stride() == want.stride(), (got.stride(), want.stride())


def test_dispatch_with_gradients(dev, monkeypatch):
    """Parameters that need a gradient keep the module path: grad_fn is set, no fused launch,
    the modules' values."""
    from frcnn_amd import ops
    case = CASES[1]
    d = _on_dev(case, 'randn', dev)
    classifier, regressor = _modules(dev, case, d)
    names = support.spy_entries(monkeypatch).names
    with torch.enable_grad():
        for x in d['xs']:  # MIOpen's first call of a shape may take another solver than the later ones
            classifier(x), regressor(x)
        assert not ops.rpn_head1x1_fused_ok(classifier, regressor, d['xs'])
        cls, reg = ops.rpn_head1x1_levels(classifier, regressor, d['xs'])
        assert names == []
        for x, c, r in zip(d['xs'], cls, reg):
            assert c.grad_fn is not None and r.grad_fn is not None
            assert torch.equal(c, classifier(x)) and torch.equal(r, regressor(x))


@pytest.mark.parametrize('case', CASES)
def test_dispatch_under_no_grad(dev, case, monkeypatch):
    """Under no_grad the head is exactly one fused launch, within the tolerance the trunk parity
    tests grant MIOpen's solver differences of the modules."""
    from frcnn_amd import ops
    d = _on_dev(case, 'randn', dev)
    classifier, regressor = _modules(dev, case, d)
    names = support.spy_entries(monkeypatch).names
    with torch.no_grad():
        cls, reg = ops.rpn_head1x1_levels(classifier, regressor, d['xs'])
        assert names == ['frh_rpn_head1x1_levels']
        for x, c, r in zip(d['xs'], cls, reg):
            for got, want in ((c, classifier(x)), (r, regressor(x))):
                assert got.grad_fn is None
                torch.testing.assert_close(got, want, rtol=1e-3, atol=1e-3 * float(want.abs().max()))


def test_rpn_head_forward_takes_it(dev, monkeypatch):
    """RPNHead.forward under no_grad: its two 1x1 convs are the one launch."""
    from frcnn_amd.heads.rpn_head import RPNHead
    torch.manual_seed(2)
    head = RPNHead(64, 64, loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True),
                   loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0)).to(dev)
    head = head.to(memory_format=torch.channels_last)
    xs = [torch.randn(2, 64, h, w, device=dev).contiguous(memory_format=torch.channels_last)
          for h, w in ((6, 8), (3, 4))]
    names = support.spy_entries(monkeypatch).names
    with torch.no_grad():
        cls, reg = head(xs)
        assert names.count('frh_rpn_head1x1_levels') == 1
        hidden = [torch.relu(head.conv(x)) for x in xs]
        for h, c, r in zip(hidden, cls, reg):
            for got, want in ((c, head.classifier(h)), (r, head.regressor(h))):
                assert got.shape == want.shape
                torch.testing.assert_close(got, want, rtol=1e-3, atol=1e-3 * float(want.abs().max()))


def test_entry_refuses_what_it_cannot_run(dev):
    x = [torch.zeros(1, 64, 2, 2, device=dev).contiguous(memory_format=torch.channels_last)]
    w = lambda c, cin: torch.zeros(c, cin, device=dev)
    with pytest.raises(RuntimeError, match='at most 16'):
        _entry(x, w(5, 64), None, w(12, 64), None)
    x36 = [torch.zeros(1, 36, 2, 2, device=dev).contiguous(memory_format=torch.channels_last)]
    with pytest.raises(RuntimeError, match='multiple of 8'):
        _entry(x36, w(3, 36), None, w(12, 36), None)
