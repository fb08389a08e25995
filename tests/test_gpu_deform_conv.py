"""The fused HIP deformable 3x3 convolution (csrc/deform_conv3x3.hip: frh_deform_conv3x3_act and
_levels, explicit and guided offsets) against the f64 torch restatement
ops.deform_conv3x3_torch, whose definition tests/test_ga_cpu.py pins with hand-derived witnesses.

Bar: per output |err| <= (9 cin + 8) 2^-24 sum |w| |sample| -- the standard forward bound of an
f32 dot product of 9 cin terms summed in any order (gamma_n <= n u), with 8 more roundings for
the blend of each term's four corners; the right-hand side is the restatement on |x| and |w|.
The offsets are multiples of 1/8 (or integers, or zero), so every sample coordinate and
bilinear weight is exact in f32 and the kernel and the reference blend the same numbers.  Far
and non-finite offsets must give exact zeros.  The equalities (guided = explicit, _levels =
per-level, launch = launch, batch = single images, ReLU = clamp) are bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import ga_inputs
import support

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _inputs(dev, n, cin, cout, dg, h, w, kind='eighths', seed=0):
    x, off, wt = ga_inputs.deform_case(n, cin, cout, dg, h, w, kind, seed)
    t = [torch.from_numpy(a) for a in (x, off, wt)]
    return t, [t[0].to(dev).contiguous(memory_format=torch.channels_last), t[1].to(dev), t[2].to(dev)]


def _check(y, host, dg, relu=False):
    """y (device) against the f64 restatement of the host tensors at the bar of the module docstring."""
    from frcnn_amd.ops import deform_conv3x3_torch
    x, off, wt = [t.double() for t in host]
    want = deform_conv3x3_torch(x, off, wt, dg, relu)
    bound = (9 * x.shape[1] + 8) * U * deform_conv3x3_torch(x.abs(), off, wt.abs(), dg)
    err = (y.double().cpu() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print('max err / bound = {:.4f}'.format(ratio))
    assert y.shape == want.shape and bool((err <= bound).all()), ratio
    return want


@pytest.mark.parametrize('cout', [64, 128])
@pytest.mark.parametrize('hw', [(1, 1), (5, 7), (19, 32)])
def test_vs_restatement(dev, hw, cout):
    """n = 2, cin = 32, dg = 4 (8 channels a group: two channel quads of a chunk share a group,
    two chunks a tap); 19 x 32 x 2 = 1216 positions = 19 tiles; 5 x 7 x 2 = 70: a partial
    second tile that crosses the image boundary; cout 64 / 128: two of the three wave layouts."""
    from frcnn_amd import ops
    host, (x, off, wt) = _inputs(dev, 2, 32, cout, 4, hw[0], hw[1], seed=hw[0] + cout)
    y = ops.deform_conv3x3(x, off, wt, 4)
    assert y.is_contiguous(memory_format=torch.channels_last) or hw == (1, 1)
    _check(y, host, 4)


def test_256_channels(dev):
    """The head's own channel counts (256 -> 256, dg = 4: 64 channels a group, the 256-row wave
    layout) at 6 x 6."""
    from frcnn_amd import ops
    host, (x, off, wt) = _inputs(dev, 2, 256, 256, 4, 6, 6, seed=21)
    _check(ops.deform_conv3x3(x, off, wt, 4), host, 4)
    _check(ops.deform_conv3x3(x, off, wt, 4, relu=True), host, 4, relu=True)


def test_one_group_and_odd_cout(dev):
    """dg = 1 (a group spans both chunks), cout = 192 (three 64-row blocks)."""
    from frcnn_amd import ops
    host, (x, off, wt) = _inputs(dev, 2, 32, 192, 1, 5, 7, seed=22)
    _check(ops.deform_conv3x3(x, off, wt, 1), host, 1)


def test_strided_view_runs_without_a_copy(dev, monkeypatch):
    """x[..., ::2, ::2] of a channels-last tensor (P6 of P5): the entry reads it in place."""
    from frcnn_amd import ops
    (xh, _, _), (xb, _, _) = _inputs(dev, 2, 32, 64, 4, 9, 13, seed=23)
    host, (_, off, wt) = _inputs(dev, 2, 32, 64, 4, 5, 7, seed=24)
    spy = support.spy_entries(monkeypatch)
    view = xb[:, :, ::2, ::2]
    y = ops.deform_conv3x3(view, off, wt, 4)
    assert [(name, a[0].value) for name, a in spy.calls] == [('frh_deform_conv3x3_act', xb.data_ptr())]
    _check(y, [xh[:, :, ::2, ::2], host[1], host[2]], 4)
    assert torch.equal(y, ops.deform_conv3x3(view.contiguous(memory_format=torch.channels_last), off, wt, 4))


@pytest.mark.parametrize('kind', ['zero', 'integer'])
def test_offset_kinds(dev, kind):
    from frcnn_amd import ops
    host, (x, off, wt) = _inputs(dev, 2, 32, 64, 4, 5, 7, kind, seed=25)
    want = _check(ops.deform_conv3x3(x, off, wt, 4), host, 4)
    if kind == 'zero':
        torch.testing.assert_close(want, torch.nn.functional.conv2d(host[0].double(), host[2].double(), padding=1),
                                   rtol=1e-12, atol=1e-12)


def test_far_and_non_finite_offsets_give_exact_zeros(dev):
    from frcnn_amd import ops
    _, (x, off, wt) = _inputs(dev, 2, 32, 64, 4, 5, 7, 'far', seed=26)
    y = ops.deform_conv3x3(x, off, wt, 4)
    assert bool((y == 0).all())
    off[0, ::3] = float('nan')
    off[1, 1::3] = float('inf')
    off[1, 2::3] = float('-inf')
    y = ops.deform_conv3x3(x, off, wt, 4)
    assert bool((y == 0).all())


def _guided(dev, shapes, dg=4, cin=32, cout=64, seed=30):
    """Per level: x, the 2-channel shape map (multiples of 1/4) and the explicit offsets
    (w0 s0) + (w1 s1) formed with torch f32 ops; offset-layer weights multiples of 1/4."""
    g = torch.Generator().manual_seed(seed)
    ow = (torch.randint(-4, 5, (18 * dg, 2), generator=g).float() / 4).to(dev)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) * 0.05).to(dev)
    xs, ss, offs = [], [], []
    for h, w in shapes:
        xs.append(torch.randn(2, cin, h, w, generator=g).to(dev).contiguous(memory_format=torch.channels_last))
        s = (torch.randint(-6, 7, (2, 2, h, w), generator=g).float() / 4).to(dev)
        ss.append(s)
        offs.append((ow[:, 0].view(1, -1, 1, 1) * s[:, :1]) + (ow[:, 1].view(1, -1, 1, 1) * s[:, 1:]))
    return xs, ss, offs, ow, wt


def test_guided_equals_explicit_bit_for_bit(dev):
    from frcnn_amd import ops
    xs, ss, offs, ow, wt = _guided(dev, [(5, 7), (19, 32)])
    for x, s, off in zip(xs, ss, offs):
        a = ops.deform_conv3x3(x, s, wt, 4, relu=True, offset_weight=ow.view(72, 2, 1, 1))
        b = ops.deform_conv3x3(x, off, wt, 4, relu=True)
        assert torch.equal(a, b) and bool((a != 0).any())
        # a channels-last shape map (what a 1x1 conv on a channels-last level returns)
        c = ops.deform_conv3x3(x, s.contiguous(memory_format=torch.channels_last), wt, 4, relu=True, offset_weight=ow)
        assert torch.equal(a, c)


def test_guided_with_general_weights_vs_restatement(dev):
    """Non-dyadic offset weights and shapes: the offsets are whatever f32 the two products and
    the sum give; the reference takes the same f32 offsets, so the bar holds where the sample
    coordinates round equally (they are formed by one f32 add from the same offsets)."""
    from frcnn_amd import ops
    g = torch.Generator().manual_seed(31)
    ow = torch.randn(72, 2, generator=g) * 0.3
    s = torch.randn(2, 2, 5, 7, generator=g)
    x = torch.randn(2, 32, 5, 7, generator=g)
    wt = torch.randn(64, 32, 3, 3, generator=g) * 0.05
    off = (ow[:, 0].view(1, -1, 1, 1) * s[:, :1]) + (ow[:, 1].view(1, -1, 1, 1) * s[:, 1:])
    y = ops.deform_conv3x3(x.to(dev), s.to(dev), wt.to(dev), 4, offset_weight=ow.to(dev))
    # the f32 sample coordinates the kernel forms, as f64 offsets for the reference
    ky = (torch.arange(9) // 3 - 1).float().view(1, 1, 9, 1, 1)
    kx = (torch.arange(9) % 3 - 1).float().view(1, 1, 9, 1, 1)
    o6 = off.view(2, 4, 9, 2, 5, 7)
    py = (torch.arange(5).float().view(1, 1, 1, 5, 1) + ky) + o6[:, :, :, 0]
    px = (torch.arange(7).float().view(1, 1, 1, 1, 7) + kx) + o6[:, :, :, 1]
    exact = torch.stack([py.double() - (torch.arange(5).double().view(1, 1, 1, 5, 1) + ky.double()),
                         px.double() - (torch.arange(7).double().view(1, 1, 1, 1, 7) + kx.double())], 3)
    _check(y, [x, exact.reshape(2, 72, 5, 7), wt], 4)


def test_levels_equal_the_per_level_calls(dev, monkeypatch):
    from frcnn_amd import ops
    shapes = [(19, 32), (10, 16), (5, 8), (3, 4), (2, 2)]
    xs, ss, offs, ow, wt = _guided(dev, shapes, seed=32)
    big = torch.randn(2, 32, 3, 3, generator=torch.Generator().manual_seed(33)).to(dev) \
        .contiguous(memory_format=torch.channels_last)
    xs[4] = big[:, :, ::2, ::2]  # the last level as a stride-2 view
    names = support.spy_entries(monkeypatch).names
    ge = ops.deform_conv3x3_levels(xs, ss, wt, 4, relu=True, offset_weight=ow)
    ex = ops.deform_conv3x3_levels(xs, offs, wt, 4, relu=True)
    assert names == ['frh_deform_conv3x3_act_levels'] * 2
    for x, s, off, a, b in zip(xs, ss, offs, ge, ex):
        one = ops.deform_conv3x3(x, off, wt, 4, relu=True)
        assert a.shape == one.shape and torch.equal(a, one) and torch.equal(b, one)
        assert torch.equal(ops.deform_conv3x3(x, s, wt, 4, relu=True, offset_weight=ow), one)


def test_launches_batches_and_relu(dev):
    from frcnn_amd import ops
    host, (x, off, wt) = _inputs(dev, 2, 32, 128, 4, 5, 7, seed=34)
    y = ops.deform_conv3x3(x, off, wt, 4)
    assert torch.equal(y, ops.deform_conv3x3(x, off, wt, 4))
    for b in range(2):  # 35 positions alone, positions 35 .. 69 of the batch: other tiles and lanes
        assert torch.equal(y[b:b + 1], ops.deform_conv3x3(x[b:b + 1], off[b:b + 1], wt, 4))
    r = ops.deform_conv3x3(x, off, wt, 4, relu=True)
    assert torch.equal(r, y.clamp_min(0)) and bool((y < 0).any())


def _raw(x, off, wt, y, dg=4, xp=None, n=None):
    from frcnn_amd import _lib
    n_, cin, h, w = x.shape
    cout = wt.shape[0]
    ws = torch.empty(9 * cin * cout, device=x.device)
    sn, _, sy, sx = x.stride()
    _lib.call('frh_deform_conv3x3_act', xp or _lib.ptr(x), _lib.ptr(off), None, _lib.ptr(wt), _lib.ptr(y), _lib.ptr(ws),
              n_ if n is None else n, cin, cout, dg, h, w, sn, sy, sx, _lib.i64_array(off.stride()), 0,
              _lib.stream_of(x))


def test_bad_arguments(dev):
    """FRH_EINVAL (-1) with a message and no launch for cin = 24, a misaligned pointer and y
    overlapping x; n = 0 is OK and leaves y untouched."""
    cl = torch.channels_last
    x = torch.zeros(2, 32, 5, 7, device=dev).contiguous(memory_format=cl)
    off = torch.zeros(2, 72, 5, 7, device=dev)
    wt = torch.zeros(64, 32, 3, 3, device=dev)
    y = torch.full((2, 64, 5, 7), 7.0, device=dev).contiguous(memory_format=cl)
    with pytest.raises(RuntimeError, match=r'\(-1\).*cin'):
        _raw(torch.zeros(2, 24, 5, 7, device=dev).contiguous(memory_format=cl), off[:, :54], torch.zeros(64, 24, 3, 3, device=dev),
             y, dg=3)
    with pytest.raises(RuntimeError, match=r'\(-1\).*groups'):
        _raw(x, off, wt, y, dg=16)
    big = torch.zeros(x.numel() + 4, device=dev)
    with pytest.raises(RuntimeError, match=r'\(-1\).*aligned'):
        _raw(x, off, wt, y, xp=ctypes.c_void_p(big.data_ptr() + 4))
    x64 = torch.zeros(2, 64, 5, 7, device=dev).contiguous(memory_format=cl)
    with pytest.raises(RuntimeError, match=r'\(-1\).*overlap'):
        _raw(x64, torch.zeros(2, 72, 5, 7, device=dev), torch.zeros(64, 64, 3, 3, device=dev), x64)
    _raw(x, off, wt, y, n=0)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


def test_dispatch(dev, monkeypatch):
    """Inference takes the HIP entry; a gradient needed, or cin = 24, takes the restatement with
    no library call, and gives its result; the module's backward runs."""
    from frcnn_amd import ops
    from frcnn_amd.dcn import DeformConv
    names = support.spy_entries(monkeypatch).names
    host, (x, off, wt) = _inputs(dev, 2, 32, 64, 4, 5, 7, seed=35)
    m = DeformConv(32, 64, 3, padding=1, deformable_groups=4).to(dev)
    assert [k for k, _ in m.named_parameters()] == ['weight'] and m.weight.shape == (64, 32, 3, 3)
    with torch.no_grad():
        m.weight.copy_(wt)
        y = m(x, off)
    assert names == ['frh_deform_conv3x3_act']
    y2 = m(x, off)  # the weight needs a gradient
    assert names == ['frh_deform_conv3x3_act'] and y2.requires_grad
    torch.testing.assert_close(y2, y, rtol=1e-4, atol=1e-5)
    y2.sum().backward()
    assert m.weight.grad is not None and bool(m.weight.grad.abs().sum() > 0)
    _, (x24, off24, wt24) = _inputs(dev, 1, 24, 64, 3, 3, 3, seed=36)
    with torch.no_grad():
        y24 = ops.deform_conv3x3(x24, off24, wt24, 3)
    assert names == ['frh_deform_conv3x3_act']
    torch.testing.assert_close(y24, ops.deform_conv3x3_torch(x24, off24, wt24, 3), rtol=0, atol=0)
