"""frh_deform_conv3x3_bwd (csrc/deform_conv3x3_bwd.hip) behind ops.deform_conv3x3(...,
hip_grad=True), against the f64 autograd of the torch restatement ops.deform_conv3x3_torch on the
host (whose offset gradient tests/test_deform_bwd_cpu.py pins by hand).  The upstream gradient is
random.

Bar, per gradient element: |err| <= (n_terms + 8) 2^-24 sum |terms| -- the forward bound of an f32
sum of n_terms terms added in any order, with 8 more roundings for the products and the blend
inside a term.  sum |terms| comes from deform_bwd_ref.abs_terms (checked against scalar loops in
test_deform_bwd_cpu.py); n_terms is cout + the most samples that touch one input element for gx,
cout + 4 cin / dg for goff, n h w for gw.  The offsets are multiples of 1/8, so coordinates and
blend weights are exact in f32.  Where the forward applied ReLU the reference takes the mask
y > 0 from the forward's own output: the definition of the entry."""
import ctypes

import pytest
import torch

import deform_bwd_ref as ref
import ga_inputs
import support

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def _case(n, cin, cout, dg, h, w, kind='eighths', seed=0):
    host = [torch.from_numpy(a) for a in ga_inputs.deform_case(n, cin, cout, dg, h, w, kind, seed)]
    gy = torch.randn(n, cout, h, w, generator=torch.Generator().manual_seed(seed + 1000))
    return host, gy


def _device_grads(dev, host, gy, dg, relu=False, view=None, need=(True, True, True)):
    """y and (gx, goff, gw) of the hip_grad path; view: the stride-2 view of a larger base, whose
    gradient is returned for x."""
    from frcnn_amd import ops
    x, off, wt = host
    xd = x.to(dev).contiguous(memory_format=CL).requires_grad_(need[0])
    offd = off.to(dev).requires_grad_(need[1])
    wd = wt.to(dev).requires_grad_(need[2])
    y = ops.deform_conv3x3(xd[:, :, ::2, ::2] if view else xd, offd, wd, dg, relu=relu, hip_grad=True)
    y.backward(gy.to(dev))
    return y.detach(), (xd.grad, offd.grad, wd.grad)


def _check_all(host, gy_eff, dg, grads, which=(True, True, True)):
    x, off, wt = host
    n, cin, h, w = x.shape
    cout = wt.shape[0]
    _, gx, goff, gw = ref.reference(x, off, wt, dg, gy_eff)
    ax, aoff, aw, touch = ref.abs_terms(x, off, wt, dg, gy_eff)
    if which[0]:
        ref.check('gx', grads[0], gx, ax, cout + touch)
    if which[1]:
        ref.check('goff', grads[1], goff, aoff, cout + 4 * cin // dg)
    if which[2]:
        ref.check('gw', grads[2], gw, aw, n * h * w)
    return gx, goff, gw


@pytest.mark.parametrize('cout', [64, 128])
@pytest.mark.parametrize('hw', [(1, 1), (5, 7), (19, 32)])
def test_vs_restatement(dev, hw, cout):
    """The forward test's shapes: n = 2, cin = 32, dg = 4 (two channel quads of a chunk share a
    group, two chunks a tap); 70 positions: a partial second tile across the image boundary; 1216
    positions: 19 tiles, so the weight launch has 19 splits.  1 x 1: a channels-last one-pixel map
    has column stride 1 < cin, which the entries refuse, so the call falls back to the restatement
    on the device and is held to the same bar."""
    host, gy = _case(2, 32, cout, 4, hw[0], hw[1], seed=hw[0] + cout)
    _, grads = _device_grads(dev, host, gy, 4)
    _check_all(host, gy, 4, grads)


@pytest.mark.parametrize('relu', [False, True])
def test_256_channels(dev, relu):
    """256 -> 256, dg = 4 (a group spans four chunks; four row tiles a wave) at 6 x 6."""
    host, gy = _case(2, 256, 256, 4, 6, 6, seed=21)
    y, grads = _device_grads(dev, host, gy, 4, relu=relu)
    mask = (y > 0).cpu() if relu else torch.ones_like(gy, dtype=torch.bool)
    assert not relu or (bool(mask.any()) and not bool(mask.all()))
    _check_all(host, gy * mask, 4, grads)


def test_one_group_and_odd_cout(dev):
    host, gy = _case(2, 32, 192, 1, 5, 7, seed=22)
    _, grads = _device_grads(dev, host, gy, 1)
    _check_all(host, gy, 1, grads)


def test_strided_view_gradient_reaches_the_base(dev):
    """x = base[:, :, ::2, ::2] (9 x 13 -> 5 x 7): gx is the view's, autograd scatters it into the
    base, zeros at the skipped cells."""
    (xb, _, _), _ = _case(2, 32, 64, 4, 9, 13, seed=23)
    (_, off, wt), gy = _case(2, 32, 64, 4, 5, 7, seed=24)
    _, grads = _device_grads(dev, [xb, off, wt], gy, 4, view=True)
    gbase = grads[0]
    assert gbase.shape == xb.shape
    keep = torch.zeros(9, 13, dtype=torch.bool)
    keep[::2, ::2] = True
    assert bool((gbase[:, :, ~keep] == 0).all())
    _check_all([xb[:, :, ::2, ::2].contiguous(), off, wt], gy, 4, (gbase[:, :, ::2, ::2], grads[1], grads[2]))


def test_zero_offsets_against_conv2d(dev):
    host, gy = _case(2, 32, 64, 4, 5, 7, 'zero', seed=25)
    _, grads = _device_grads(dev, host, gy, 4)
    gx, _, gw = _check_all(host, gy, 4, grads)
    x, wt = host[0].double().requires_grad_(True), host[2].double().requires_grad_(True)
    torch.nn.functional.conv2d(x, wt, padding=1).backward(gy.double())
    torch.testing.assert_close(gx, x.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(gw, wt.grad, rtol=1e-12, atol=1e-12)


def test_integer_offsets_one_sided_derivative(dev):
    """Every sample sits on a grid point: lx = ly = 0, and goff is the one-sided difference
    towards +1 the formula gives (the restatement's autograd, pinned on the CPU by hand)."""
    host, gy = _case(2, 32, 64, 4, 5, 7, 'integer', seed=26)
    _, grads = _device_grads(dev, host, gy, 4)
    _, goff, _ = _check_all(host, gy, 4, grads)
    assert bool((goff != 0).any())


def test_far_offsets_give_exact_zeros(dev):
    host, gy = _case(2, 32, 64, 4, 5, 7, 'far', seed=27)
    _, grads = _device_grads(dev, host, gy, 4)
    for g in grads:
        assert bool((g == 0).all())
    host[1][0, ::3] = float('nan')
    host[1][1, 1::3] = float('inf')
    host[1][1, 2::3] = float('-inf')
    _, grads = _device_grads(dev, host, gy, 4)
    for g in grads:
        assert bool((g == 0).all())


def test_collision(dev):
    """Every tap of every position samples the one point (2.5, 3.5): 2 x 9 x 35 adds per channel
    land on each of four cells (atomics on one address from every workgroup), same bar."""
    host, gy = _case(2, 32, 64, 4, 5, 7, seed=28)
    off = torch.zeros(2, 4, 9, 2, 5, 7)
    k = torch.arange(9)
    off[:, :, :, 0] = 2.5 - (torch.arange(5.0).view(1, 1, 1, 5, 1) + (k // 3 - 1).float().view(1, 1, 9, 1, 1))
    off[:, :, :, 1] = 3.5 - (torch.arange(7.0).view(1, 1, 1, 1, 7) + (k % 3 - 1).float().view(1, 1, 9, 1, 1))
    host[1] = off.reshape(2, 72, 5, 7)
    _, grads = _device_grads(dev, host, gy, 4)
    _check_all(host, gy, 4, grads)
    hit = torch.zeros(5, 7, dtype=torch.bool)
    hit[2:4, 3:5] = True
    assert bool((grads[0][:, :, ~hit] == 0).all()) and bool((grads[0][:, :, hit] != 0).all())


def test_needs_input_grad_subsets(dev, monkeypatch):
    host, gy = _case(2, 32, 64, 4, 5, 7, seed=29)
    spy = support.spy_entries(monkeypatch)
    _, grads = _device_grads(dev, host, gy, 4, need=(False, False, True))
    name, args = spy.calls[-1]
    assert spy.names == ['frh_deform_conv3x3_act', 'frh_deform_conv3x3_bwd']
    assert args[6] is None and args[7] is None and args[8] is not None
    _check_all(host, gy, 4, grads, which=(False, False, True))
    _, grads = _device_grads(dev, host, gy, 4, need=(True, False, False))
    name, args = spy.calls[-1]
    assert name == 'frh_deform_conv3x3_bwd' and args[6] is not None and args[7] is None and args[8] is None
    _check_all(host, gy, 4, grads, which=(True, False, False))


def _guided_case(seed=30, dg=4, cin=32, cout=64, h=5, w=7):
    """Dyadic shape values and offset weights (multiples of 1/4): the offsets are exact."""
    g = torch.Generator().manual_seed(seed)
    ow = torch.randint(-4, 5, (18 * dg, 2), generator=g).float() / 4
    s = torch.randint(-6, 7, (2, 2, h, w), generator=g).float() / 4
    x = torch.randn(2, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.05
    gy = torch.randn(2, cout, h, w, generator=g)
    return x, s, ow, wt, gy


def test_guided_mode(dev):
    from frcnn_amd import ops
    x, s, ow, wt, gy = _guided_case()
    xd = x.to(dev).contiguous(memory_format=CL).requires_grad_(True)
    sd, owd, wd = [t.to(dev).requires_grad_(True) for t in (s, ow.view(72, 2, 1, 1), wt)]
    ops.deform_conv3x3(xd, sd, wd, 4, offset_weight=owd, hip_grad=True).backward(gy.to(dev))
    # f64 reference: the restatement behind conv2d
    s6, ow6 = s.double().requires_grad_(True), ow.double().requires_grad_(True)
    off6 = torch.nn.functional.conv2d(s6, ow6.view(72, 2, 1, 1))
    off = off6.detach().float()
    assert torch.equal(off.double(), off6.detach())  # exact in f32
    _, gx, goff, gw = ref.reference(x, off, wt, 4, gy)
    off6.backward(goff)
    ax, aoff, aw, touch = ref.abs_terms(x, off, wt, 4, gy)
    ref.check('gx', xd.grad, gx, ax, 64 + touch)
    ref.check('gw', wd.grad, gw, aw, 2 * 5 * 7)
    # the two contractions of goff add n h w (offset weight) or 18 dg (shape) terms of |goff| |factor|
    a_ow = torch.einsum('nchw,njhw->cj', aoff, s.double().abs())
    a_s = torch.einsum('cj,nchw->njhw', ow.double().abs(), aoff)
    ref.check('g_offset_w', owd.grad.view(72, 2), ow6.grad, a_ow, 64 + 4 * 8 + 70)
    ref.check('g_shape', sd.grad, s6.grad, a_s, 64 + 4 * 8 + 72)
    # goff itself, through explicit offsets on that map
    offd = off.to(dev).requires_grad_(True)
    ops.deform_conv3x3(xd.detach(), offd, wd.detach(), 4, hip_grad=True).backward(gy.to(dev))
    ref.check('goff', offd.grad, goff, aoff, 64 + 4 * 8)


def _raw(x, off, wt, gy, gx=None, goff=None, gw=None, dg=4, xp=None, n=None, ow=None):
    from frcnn_amd import _lib
    n_, cin, h, w = x.shape
    cout = wt.shape[0]
    ws = torch.empty(max(_lib.query('frh_deform_conv3x3_bwd_workspace', n_, cin, cout, h, w), 16) // 4, device=x.device)
    sn, _, sy, sx = x.stride()
    _lib.call('frh_deform_conv3x3_bwd', xp or _lib.ptr(x), _lib.ptr(off), _lib.ptr(ow), _lib.ptr(wt), None, _lib.ptr(gy),
              _lib.ptr(gx), _lib.ptr(goff), _lib.ptr(gw), _lib.ptr(ws), n_ if n is None else n, cin, cout, dg, h, w,
              sn, sy, sx, _lib.i64_array(off.stride()), _lib.stream_of(x))


def test_guided_goff_equals_explicit_goff_and_launches_repeat(dev):
    """The raw entry: goff of the guided mode is that of the explicit mode on the same map bit for
    bit; goff and gw are bit-identical across two launches."""
    x, s, ow, wt, gy = _guided_case(seed=31, h=19, w=32)
    xd = x.to(dev).contiguous(memory_format=CL)
    sd, owd, wd = s.to(dev), ow.to(dev), wt.to(dev)
    gyd = gy.to(dev).contiguous(memory_format=CL)
    offd = (owd[:, 0].view(1, -1, 1, 1) * sd[:, :1]) + (owd[:, 1].view(1, -1, 1, 1) * sd[:, 1:])
    out = []
    for mode in ('guided', 'explicit', 'explicit'):
        gx = torch.zeros_like(xd)
        goff, gw = torch.full((2, 72, 19, 32), 7.0, device=dev), torch.full_like(wd, 7.0)
        if mode == 'guided':
            _raw(xd, sd, wd, gyd, gx, goff, gw, ow=owd)
        else:
            _raw(xd, offd, wd, gyd, gx, goff, gw)
        out.append((gx, goff, gw))
    for a, b in ((0, 1), (1, 2)):
        assert torch.equal(out[a][1], out[b][1]) and torch.equal(out[a][2], out[b][2])
        torch.testing.assert_close(out[a][0], out[b][0], rtol=1e-4, atol=1e-5)
    assert bool((out[0][1] != 7.0).all()) and bool((out[0][2] != 7.0).all())


def test_deterministic_mode_takes_the_restatement(dev, monkeypatch):
    from frcnn_amd import ops
    host, gy = _case(2, 32, 64, 4, 5, 7, seed=32)
    names = support.spy_entries(monkeypatch).names
    torch.use_deterministic_algorithms(True, warn_only=True)  # the restatement's gather backward only warns
    try:
        _, grads = _device_grads(dev, host, gy, 4)
    finally:
        torch.use_deterministic_algorithms(False)
    assert names == [] and all(g is not None for g in grads)
    ops.set_deterministic_backward(True)
    try:
        _device_grads(dev, host, gy, 4)
    finally:
        ops.set_deterministic_backward(False)
    assert names == []
    _device_grads(dev, host, gy, 4)
    assert names == ['frh_deform_conv3x3_act', 'frh_deform_conv3x3_bwd']


def test_double_backward_raises(dev):
    from frcnn_amd import ops
    host, gy = _case(1, 32, 64, 4, 3, 3, seed=33)
    x = host[0].to(dev).contiguous(memory_format=CL).requires_grad_(True)
    y = ops.deform_conv3x3(x, host[1].to(dev), host[2].to(dev), 4, hip_grad=True)
    gx, = torch.autograd.grad(y, x, gy.to(dev), create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


def test_bad_arguments(dev):
    """As the forward's: FRH_EINVAL (-1) with a message and no launch for cin = 24, a misaligned
    pointer and gx overlapping x; n = 0 is OK and leaves the outputs untouched."""
    x = torch.zeros(2, 32, 5, 7, device=dev).contiguous(memory_format=CL)
    off = torch.zeros(2, 72, 5, 7, device=dev)
    wt = torch.zeros(64, 32, 3, 3, device=dev)
    gy = torch.zeros(2, 64, 5, 7, device=dev).contiguous(memory_format=CL)
    gx = torch.full((2, 32, 5, 7), 7.0, device=dev).contiguous(memory_format=CL)
    goff, gw = torch.full_like(off, 7.0), torch.full_like(wt, 7.0)
    with pytest.raises(RuntimeError, match=r'\(-1\).*cin'):
        _raw(torch.zeros(2, 24, 5, 7, device=dev).contiguous(memory_format=CL), off[:, :54],
             torch.zeros(64, 24, 3, 3, device=dev), gy, gw=gw, dg=3)
    with pytest.raises(RuntimeError, match=r'\(-1\).*groups'):
        _raw(x, off, wt, gy, gx, goff, gw, dg=16)
    big = torch.zeros(x.numel() + 4, device=dev)
    with pytest.raises(RuntimeError, match=r'\(-1\).*aligned'):
        _raw(x, off, wt, gy, gx, goff, gw, xp=ctypes.c_void_p(big.data_ptr() + 4))
    with pytest.raises(RuntimeError, match=r'\(-1\).*overlap'):
        _raw(x, off, wt, gy, gx=x)
    with pytest.raises(RuntimeError, match=r'\(-1\).*overlap'):
        _raw(x, off, wt, gy, goff=goff, gw=goff)
    _raw(x, off, wt, gy, gx, goff, gw, n=0)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (gx, goff, gw))


def _param_and_input_grads(run):
    out = run()
    g = torch.Generator().manual_seed(9)
    outs = out if isinstance(out, (list, tuple)) else [out]
    sum((o * torch.randn(o.shape, generator=g).to(o.device)).sum() for o in outs).backward()


def _close(a, b):
    torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5 * float(b.abs().max()))


def test_deform_conv_module(dev, monkeypatch):
    from frcnn_amd.dcn import DeformConv
    host, _ = _case(2, 32, 64, 4, 5, 7, seed=34)
    m = DeformConv(32, 64, 3, padding=1, deformable_groups=4).to(dev)
    names = support.spy_entries(monkeypatch).names
    grads = []
    for flag in (False, True):
        m.hip_grad = flag
        m.zero_grad()
        x = host[0].to(dev).contiguous(memory_format=CL).requires_grad_(True)
        off = host[1].to(dev).requires_grad_(True)
        _param_and_input_grads(lambda: m(x, off, relu=True))
        grads.append((m.weight.grad.clone(), x.grad, off.grad))
        assert names == (['frh_deform_conv3x3_act', 'frh_deform_conv3x3_bwd'] if flag else [])
    for a, b in zip(grads[1], grads[0]):
        _close(a, b)


def test_guided_anchor_module(dev, monkeypatch):
    """A 64-channel GuidedAnchor on three small levels: hip_grad = True is one _levels forward and
    one backward call per level; parameter and input gradients match the default path."""
    from frcnn_amd.heads.guided_head import GuidedAnchor
    torch.manual_seed(3)
    ga = GuidedAnchor(64, 64, anchor_scales=[8.0], anchor_ratios=[0.5, 1.0, 2.0], anchor_strides=[8, 16, 32],
                      deformable_groups=4, loss_loc=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25,
                                                         loss_weight=1.0),
                      loss_shape=dict(type='BoundedIoULoss', beta=0.2, loss_weight=1.0)).to(dev)
    with torch.no_grad():
        ga.offset_layer.weight.normal_(0, 0.5)
        ga.adapt_layer.weight.normal_(0, 0.05)
        ga.shape_layer.weight.normal_(0, 0.1)
    g = torch.Generator().manual_seed(4)
    shapes = [(19, 32), (10, 16), (5, 8)]
    names = support.spy_entries(monkeypatch).names
    grads = []
    assert GuidedAnchor.hip_grad is False
    for flag in (False, True):
        ga.hip_grad = flag
        ga.zero_grad()
        g.manual_seed(4)
        feats = [torch.randn(2, 64, h, w, generator=g).to(dev).contiguous(memory_format=CL).requires_grad_(True)
                 for h, w in shapes]
        del names[:]
        _param_and_input_grads(lambda: ga(feats)[2])
        deform = [k for k in names if 'deform' in k]
        assert deform == (['frh_deform_conv3x3_act_levels'] + ['frh_deform_conv3x3_bwd'] * 3 if flag else [])
        grads.append([ga.adapt_layer.weight.grad.clone(), ga.offset_layer.weight.grad.clone()] + [f.grad for f in feats])
    assert bool((grads[1][1] != 0).any())
    for a, b in zip(grads[1], grads[0]):
        _close(a, b)
