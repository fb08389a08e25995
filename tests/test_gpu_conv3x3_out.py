"""frh_conv3x3_out_levels: the prediction convs of a one-stage head (3x3 / stride 1 / padding 1,
1 to 192 output channels, one conv or two that read the same input) over every pyramid level in
one launch (csrc/conv3x3_out_kernels.h): a direct convolution on the exact-f32 16x16x4 MFMA with
the bias, the per-level scale and the exp on the accumulators.

Cases are (n, cin, c0, c1, levels, index of the level that is a [:, :, ::2, ::2] view).  A tile is
4 rows x 16 columns of one image, the output columns go in 16-column blocks (at most 4 per
workgroup, then a second column group) and cin is staged in chunks of 32 (one or two blocks) or 16
channels: the cases cover levels smaller than a tile, ragged tiles on both sides, a one-pixel
level, every kernel instance (1, 2, 3 and 4 blocks; 2 and 3 column groups), a cin that is not a
multiple of the chunk, and the second conv starting inside and at the edge of a block.

Measured on an MI355X (max over the elements of a case; cases in the order of CASES):
  accuracy, bias epilogue, max err / bound:   0.0064, 0.0018, 0.00072, 0.0057, 0.0026, 0.016
  max err / max direct-f32 err (bar 8):       1.17, 2.25, 7.00, 1.74, 1.70, 1.06
    (7.00 at cin = 256: one 2304-term chain against the CPU library's blocked partial sums)
  accuracy, scale epilogue, max err / bound:  0.0063, 0.0018, 0.00072, 0.0056, 0.0027, 0.015
  exp epilogue, max relative difference to torch.exp of the same argument: 0.0 in every case
    (bar 2^-21)
"""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CASES = [
    (1, 8, 1, 0, ((3, 5),), None),                  # one cin chunk, one output column, smaller than a tile
    (2, 64, 4, 1, ((5, 8), (3, 4), (1, 1)), 1),     # FCOS's reg + centerness pair, a strided view, one pixel
    (1, 256, 20, 0, ((10, 16),), None),             # the workload's full cin loop and cls width
    (2, 40, 36, 0, ((17, 34),), None),              # cin % 16 != 0, width across column 32, ragged tiles
    (1, 64, 64, 1, ((9, 6), (4, 4)), None),         # GFL's pair: the second output starts at column 64
    (1, 16, 180, 0, ((6, 7),), None),               # Retina's classifier width, the last block partly masked
]
FRH_EINVAL = -1


def _channels_last_level(n, cin, h, w, fill, view):
    """A channels-last [n, cin, h, w] level; view: cut as [:, :, ::2, ::2] from one twice the size."""
    if not view:
        return fill(n, cin, h, w).contiguous(memory_format=torch.channels_last)
    return fill(n, cin, 2 * h, 2 * w).contiguous(memory_format=torch.channels_last)[:, :, ::2, ::2]


@functools.lru_cache(maxsize=None)
def _case(case, kind):
    """Inputs (CPU f32) and the float64 references of one case, computed once.  kind 'int': integers
    in [-4, 4] (every partial sum exact in f32); 'randn': seeded normals; 'exp': normals with the
    weights scaled by 1 / sqrt(9 cin).  Per level and conv: y64 the bias-free float64 convolution,
    mag = conv(|x|, |w|), y32 torch's CPU f32 direct convolution."""
    n, cin, c0, c1, levels, view = case
    g = torch.Generator().manual_seed(131 + cin + 7 * c0 + c1 + len(levels))
    if kind == 'int':
        fill = lambda *s: torch.randint(-4, 5, s, generator=g).float()
    else:
        fill = lambda *s: torch.randn(*s, generator=g)
    xs = [_channels_last_level(n, cin, h, w, fill, i == view) for i, (h, w) in enumerate(levels)]
    ws = [fill(c, cin, 3, 3) for c in (c0, c1)]
    if kind == 'exp':
        ws = [w / math.sqrt(9 * cin) for w in ws]
    bs = [fill(c) for c in (c0, c1)]
    gs = torch.Generator().manual_seed(977 + cin)
    scales = [[torch.rand(c, generator=gs) + 0.5 for _ in levels] for c in (c0, c1)]
    convs = _convs(case)
    y64 = {k: [F.conv2d(x.double(), ws[k].double(), None, padding=1) for x in xs] for k in convs}
    mag = {k: [F.conv2d(x.double().abs(), ws[k].double().abs(), None, padding=1) for x in xs] for k in convs}
    y32 = {k: [F.conv2d(x.contiguous(), ws[k], None, padding=1) for x in xs] for k in convs} if kind == 'randn' else None
    return dict(xs=xs, ws=ws, bs=bs, scales=scales, y64=y64, mag=mag, y32=y32)


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
    return dict(xs=[_to_dev(x, dev) for x in c['xs']],
                # [c][3][3][cin]: the channels-last Conv2d weight as it lies in memory
                ws=[w.permute(0, 2, 3, 1).contiguous().to(dev) for w in c['ws']],
                bs=[b.to(dev) for b in c['bs']],
                scales=[[s.to(dev) for s in sk] for sk in c['scales']])


def _ptrs(ts):
    from frcnn_amd import _lib
    return (_lib.c_vp * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _nan_level(n, c, x):
    return torch.full((n, c, x.shape[2], x.shape[3]), float('nan'), device=x.device).contiguous(
        memory_format=torch.channels_last)


def _entry(xs, ws, bs=(None, None), scales=(None, None), exps=(False, False), mk=_nan_level):
    """One frh_conv3x3_out_levels launch over the levels xs with the convs ws ([c][3][3][cin]
    tensors; the second may be empty or None); returns [ys0, ys1] (ys1 empty for one conv).
    mk(n, c, x) makes the channels-last output of c channels for the level x (NaN-filled here;
    tests/test_gpu_guarded_convs.py passes a torch.empty one under its allocator)."""
    from frcnn_amd import _lib
    n, cin = xs[0].shape[:2]
    two = len(ws) > 1 and ws[1] is not None and ws[1].shape[0] > 0
    c0, c1 = ws[0].shape[0], ws[1].shape[0] if two else 0
    mk = functools.partial(mk, n)
    ys0, ys1 = [mk(c0, x) for x in xs], [mk(c1, x) for x in xs] if two else []
    p = _lib.ptr
    _lib.call('frh_conv3x3_out_levels', len(xs), _lib.ptr_array(xs), _lib.ptr_array(ys0),
              _lib.ptr_array(ys1) if two else None, p(ws[0]), p(bs[0]), p(ws[1]) if two else None,
              p(bs[1]) if two else None, _ptrs(scales[0]) if scales[0] is not None else None,
              _ptrs(scales[1]) if two and scales[1] is not None else None, int(exps[0]), int(exps[1]), n, cin, c0, c1,
              _lib.i32_array([v for x in xs for v in x.shape[2:]]),
              _lib.i64_array([v for x in xs for v in (x.stride(0), x.stride(2), x.stride(3))]),
              _lib.stream_of(xs[0]))
    return [ys0, ys1]


def _convs(case):
    return (0, 1) if case[3] else (0,)


@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('case', CASES)
def test_exact_on_integers(dev, case, bias):
    """Integer inputs in [-4, 4]: every partial sum is below 9 * 256 * 16 < 2^24, so the f32 result
    is the float64 one bit for bit, whatever the order: borders, padding, masking, column splits
    and strides with no tolerance at all."""
    c, d = _case(case, 'int'), _on_dev(case, 'int', dev)
    ys = _entry(d['xs'], d['ws'], d['bs'] if bias else (None, None))
    for k in _convs(case):
        for y, y64 in zip(ys[k], c['y64'][k]):
            if bias:
                y64 = y64 + c['bs'][k].double().view(1, -1, 1, 1)
            assert y.shape == y64.shape and y.is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(y.cpu().double(), y64)


def _check_bound(case, ys, refs, mags, roundings):
    """max over the case of err / bound, bound = 2 * roundings * 2^-24 * mag elementwise."""
    worst, errs = 0.0, []
    for k in _convs(case):
        for y, y64, mag in zip(ys[k], refs[k], mags[k]):
            y = y.cpu().double()
            assert torch.isfinite(y).all()
            err, bound = (y - y64).abs(), 2.0 * roundings * 2.0 ** -24 * mag
            worst = max(worst, float((err / bound).max()))
            errs.append(err)
            assert bool((err <= bound).all()), float((err / bound).max())
    return worst, errs


@pytest.mark.parametrize('case', CASES)
def test_accuracy_against_float64(dev, case):
    """|y - y64| <= 2 (9 cin + 2) 2^-24 mag for every element, mag = conv(|x|, |w|) + |bias|: the
    forward bound of a 9 cin + 1-term f32 sum in any order; and, over the case,
    max|y - y64| <= 8 max|y32 - y64|, y32 torch's CPU f32 direct conv."""
    c, d = _case(case, 'randn'), _on_dev(case, 'randn', dev)
    cin = case[1]
    b64 = [b.double().view(1, -1, 1, 1) for b in c['bs']]
    refs = {k: [y + b64[k] for y in c['y64'][k]] for k in _convs(case)}
    mags = {k: [m + b64[k].abs() for m in c['mag'][k]] for k in _convs(case)}
    worst, errs = _check_bound(case, _entry(d['xs'], d['ws'], d['bs']), refs, mags, 9 * cin + 2)
    err = max(float(e.max()) for e in errs)
    err32 = max(float(((y32 + c['bs'][k].view(1, -1, 1, 1)).double() - y64).abs().max())
                for k in _convs(case) for y32, y64 in zip(c['y32'][k], refs[k]))
    print('case', case[:4], 'max err / bound', worst, 'max err / max direct-f32 err', err / err32)
    assert err <= 8.0 * err32


@pytest.mark.parametrize('case', CASES)
def test_scale_epilogue(dev, case):
    """(acc + bias) * scale[level][c] against (y64 + b) * s: one more rounding, 9 cin + 3."""
    c, d = _case(case, 'randn'), _on_dev(case, 'randn', dev)
    cin = case[1]
    b64 = [b.double().view(1, -1, 1, 1) for b in c['bs']]
    s64 = [[s.double().view(1, -1, 1, 1) for s in sk] for sk in c['scales']]
    refs = {k: [(y + b64[k]) * s for y, s in zip(c['y64'][k], s64[k])] for k in _convs(case)}
    mags = {k: [(m + b64[k].abs()) * s for m, s in zip(c['mag'][k], s64[k])] for k in _convs(case)}
    worst, _ = _check_bound(case, _entry(d['xs'], d['ws'], d['bs'], d['scales']), refs, mags, 9 * cin + 3)
    print('case', case[:4], 'scale epilogue: max err / bound', worst)
    # a NULL entry of the array is no scale for that level
    some = [[None] + sk[1:] for sk in d['scales']]
    ys, plain = _entry(d['xs'], d['ws'], d['bs'], some), _entry(d['xs'], d['ws'], d['bs'])
    for k in _convs(case):
        assert torch.equal(ys[k][0], plain[k][0])


@pytest.mark.parametrize('case', CASES)
def test_exp_epilogue(dev, case):
    """expf((acc + bias) * scale) against torch.exp, on the device, of the entry's own scale-mode
    output: both an f32 exp of the same f32 argument, each within 1 ulp of the exact value, so at
    most 2 ulp = 2^-22 apart relatively; the bar is twice that."""
    d = _on_dev(case, 'exp', dev)
    arg = _entry(d['xs'], d['ws'], d['bs'], d['scales'])
    got = _entry(d['xs'], d['ws'], d['bs'], d['scales'], (True, True))
    worst = 0.0
    for k in _convs(case):
        for a, y in zip(arg[k], got[k]):
            want = torch.exp(a)
            assert torch.isfinite(y).all() and float(a.abs().max()) < 20.0
            worst = max(worst, float(((y - want).abs() / want).max()))
    print('case', case[:4], 'exp epilogue: max relative difference', worst)
    assert worst <= 2.0 ** -21
    # the flags are per conv
    if case[3]:
        one = _entry(d['xs'], d['ws'], d['bs'], d['scales'], (True, False))
        for i in range(len(d['xs'])):
            assert torch.equal(one[0][i], got[0][i]) and torch.equal(one[1][i], arg[1][i])


def _full(d, xs=None):
    return _entry(d['xs'] if xs is None else xs, d['ws'], d['bs'], d['scales'])


@pytest.mark.parametrize('case', CASES)
def test_same_bits_across_launch_shapes(dev, case):
    """Two launches; a multi-level launch and each level's own; a pair launch and the two
    single-conv launches; a strided view and its contiguous copy: equal bits throughout."""
    d = _on_dev(case, 'randn', dev)
    together = _full(d)
    again = _full(d)
    for k in _convs(case):
        for a, b in zip(together[k], again[k]):
            assert torch.equal(a, b)
    for i, x in enumerate(d['xs']):
        alone = _entry([x], d['ws'], d['bs'], [[sk[i]] for sk in d['scales']])
        for k in _convs(case):
            assert torch.equal(alone[k][0], together[k][i])
    if case[3]:
        for k in (0, 1):
            single = _entry(d['xs'], [d['ws'][k]], [d['bs'][k], None], [d['scales'][k], None])
            for a, b in zip(single[0], together[k]):
                assert torch.equal(a, b)
    if case[5] is not None:
        copies = [x.contiguous(memory_format=torch.channels_last) for x in d['xs']]
        assert copies[case[5]].stride() != d['xs'][case[5]].stride()
        for k in _convs(case):
            for a, b in zip(_full(d, copies)[k], together[k]):
                assert torch.equal(a, b)


def test_entry_refuses_what_it_cannot_run(dev):
    """FRH_EINVAL and a message, with no launch: only the return code is looked at (the pointers of
    the refused calls are never followed)."""
    from frcnn_amd import _lib
    lib = _lib.load()
    x = torch.zeros(1, 16, 4, 4, device=dev).contiguous(memory_format=torch.channels_last)
    w = torch.zeros(200, 3, 3, 16, device=dev)
    y = torch.zeros(1, 200, 4, 4, device=dev).contiguous(memory_format=torch.channels_last)
    y1 = torch.zeros_like(y)

    def status(levels=1, xp=None, wp=None, cin=16, c0=4, c1=0, strides=None):
        xp = x.data_ptr() if xp is None else xp
        n = max(levels, 1)
        st = lib.frh_conv3x3_out_levels(
            levels, (_lib.c_vp * n)(*[xp] * n), (_lib.c_vp * n)(*[y.data_ptr()] * n),
            (_lib.c_vp * n)(*[y1.data_ptr()] * n), ctypes.c_void_p(w.data_ptr() if wp is None else wp), None,
            ctypes.c_void_p(w.data_ptr()) if c1 else None, None, None, None, 0, 0, 1, cin, c0, c1,
            _lib.i32_array([4, 4] * n), _lib.i64_array((strides or [256, 64, 16]) * n), _lib.stream_of(x))
        return st, lib.frh_last_error().decode(errors='replace')

    for kw in (dict(cin=12), dict(c0=0), dict(c0=192, c1=1), dict(c0=100, c1=93), dict(levels=0), dict(levels=9),
               dict(strides=[256, 64, 18]), dict(strides=[256, 66, 16]), dict(xp=x.data_ptr() + 4),
               dict(wp=w.data_ptr() + 8)):
        st, msg = status(**kw)
        assert st == FRH_EINVAL and msg, (kw, st, msg)
    torch.cuda.synchronize()
    assert status()[0] == 0 and status(c0=100, c1=92)[0] == 0  # the same calls within the limits run
    torch.cuda.synchronize()
