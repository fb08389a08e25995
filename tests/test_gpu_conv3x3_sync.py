"""The chunk step's synchronisation in frh_conv3x3_bias_act (csrc/conv3x3_wino_kernels.h): the U
DMA issued in pieces over the step, the barrier in mid-step with the last positions' operands in
registers, the next step's first operands read right behind it.

The ordering arguments are in the kernel's comments; this is a screen for what they could have
missed.  Integer inputs drawn as tests/test_gpu_conv3x3_pipeline.py draws them (x in [-3, 3],
w = 4 x [-2, 2], integer bias): every Winograd intermediate and every partial sum is an integer
below 2^24 (cases_bound below, checked without a GPU in tests/test_conv3x3_sync_cases.py), so the
output must equal the float64 convolution exactly.  Two such sets, each with its own weights and
workspace, alternate over back-to-back launches with no host synchronisation in between: a DMA
that lands late (in the LDS of the workgroup that follows on the CU), an operand read before its
stage is complete, or a stage overwritten before its last read changes some launch's output."""
import functools

import pytest
import torch
import torch.nn.functional as F

import support

pytestmark = pytest.mark.gpu

CL = torch.channels_last
# (n, cin, cout, h, w).  The first: 1056 workgroups, more than four rounds on 256 CUs, so
# workgroups follow each other on a CU; three chunks.  The second: seven chunks, ragged on
# both sides, two cout blocks.
ALTERNATING_SHAPES = [(1, 24, 64, 512, 528), (2, 56, 128, 35, 50)]
ALTERNATING_LAUNCHES = 24
# P2..P6-shaped levels at 1/4 scale; the last is the ::2 view of the 5 x 8 level
LEVEL_HW = [(38, 64), (19, 32), (10, 16), (5, 8)]
LEVELS_N, LEVELS_CIN, LEVELS_COUT, LEVELS_LAUNCHES = 2, 40, 64, 12
# one and two chunks, a single partial tile block: every prefetch past the end is a clamped repeat
PROLOGUE_SHAPES = [(1, 8, 64, 3, 5), (1, 16, 64, 3, 5)]
FLAGS = [(b, r) for b in (False, True) for r in (False, True)]
X_MAX, W_MAX, BIAS_MAX = 3, 8, 5


def cases_bound(cin):
    """Largest magnitude any sum of products (in any order) plus the bias can reach."""
    return X_MAX * W_MAX * 9 * cin + BIAS_MAX


def _draw(g, n, cin, cout, hws):
    xs = [support.ints(g, -X_MAX, X_MAX, n, cin, h, w) for h, w in hws]
    wt = 4.0 * support.ints(g, -2, 2, cout, cin, 3, 3)
    bias = support.ints(g, -BIAS_MAX, BIAS_MAX, cout)
    return xs, wt, bias


def _exact(x, wt, bias, relu):
    """The float64 convolution, + bias, ReLU, as f32 (exact: integers below 2^24)."""
    y = F.conv2d(x.double(), wt.double(), None if bias is None else bias.double(), padding=1)
    return (y.clamp_min(0.0) if relu else y).float()


@functools.lru_cache(maxsize=None)
def _alternating_case(shape):
    n, cin, cout, h, w = shape
    sets = []
    for k in range(2):
        g = torch.Generator().manual_seed(7300 + 1000 * k + cin + 7 * cout + h * w)
        (x,), wt, bias = _draw(g, n, cin, cout, [(h, w)])
        sets.append(dict(x=x, w=wt, bias=bias, want=_exact(x, wt, bias, True)))
    return sets


@functools.lru_cache(maxsize=None)
def _levels_case():
    sets = []
    for k in range(2):
        g = torch.Generator().manual_seed(7400 + k)
        xs, wt, bias = _draw(g, LEVELS_N, LEVELS_CIN, LEVELS_COUT, LEVEL_HW)
        xs.append(xs[-1][:, :, ::2, ::2])
        sets.append(dict(xs=xs, w=wt, bias=bias, want=[_exact(x, wt, bias, True) for x in xs]))
    return sets


def _launch(xs, wt, bias, ys, work, relu):
    """One frh_conv3x3_bias_act_levels call (shared weights), no synchronisation."""
    from frcnn_amd import _lib
    n, cin = xs[0].shape[:2]
    cout = wt.shape[0]
    bs = (_lib.c_vp * len(xs))(*[None if bias is None else bias.data_ptr()] * len(xs))
    _lib.call('frh_conv3x3_bias_act_levels', len(xs), _lib.ptr_array(xs), _lib.ptr_array([wt] * len(xs)), bs,
              _lib.ptr_array(ys), _lib.ptr(work), work.numel() * 4, n, cin, cout,
              _lib.i32_array([v for x in xs for v in x.shape[2:]]),
              _lib.i64_array([v for x in xs for v in (x.stride(0), x.stride(2), x.stride(3))]), int(relu),
              _lib.stream_of(work))


def _empty_like_out(x, cout):
    return torch.empty(x.shape[0], cout, x.shape[2], x.shape[3], dtype=torch.float32, device=x.device,
                       memory_format=CL)


@pytest.mark.parametrize('shape', ALTERNATING_SHAPES)
def test_alternating_back_to_back_launches_are_exact(dev, shape):
    n, cin, cout, h, w = shape
    sets = []
    for c in _alternating_case(shape):
        sets.append(dict(x=c['x'].to(dev).contiguous(memory_format=CL), w=c['w'].to(dev).contiguous(memory_format=CL),
                         bias=c['bias'].to(dev), want=c['want'].to(dev),
                         work=torch.empty(16 * cin * cout, device=dev)))
    outs = [_empty_like_out(sets[0]['x'], cout) for _ in range(ALTERNATING_LAUNCHES)]
    for o in outs:
        o.fill_(float('nan'))
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        s = sets[i % 2]
        _launch([s['x']], s['w'], s['bias'], [o], s['work'], True)
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert torch.equal(o, sets[i % 2]['want']), 'launch {} of {}'.format(i, ALTERNATING_LAUNCHES)


def test_alternating_multi_level_launches_are_exact(dev):
    sets = []
    for c in _levels_case():
        xs = [x.to(dev).contiguous(memory_format=CL) for x in c['xs'][:-1]]
        xs.append(xs[-1][:, :, ::2, ::2])
        sets.append(dict(xs=xs, w=c['w'].to(dev).contiguous(memory_format=CL), bias=c['bias'].to(dev),
                         want=[t.to(dev) for t in c['want']],
                         work=torch.empty(16 * LEVELS_CIN * LEVELS_COUT, device=dev)))
    outs = [[_empty_like_out(x, LEVELS_COUT) for x in sets[0]['xs']] for _ in range(LEVELS_LAUNCHES)]
    for ys in outs:
        for o in ys:
            o.fill_(float('nan'))
    torch.cuda.synchronize()
    for i, ys in enumerate(outs):
        s = sets[i % 2]
        _launch(s['xs'], s['w'], s['bias'], ys, s['work'], True)
    torch.cuda.synchronize()
    for i, ys in enumerate(outs):
        for lv, (o, want) in enumerate(zip(ys, sets[i % 2]['want'])):
            assert torch.equal(o, want), 'launch {} of {}, level {}'.format(i, LEVELS_LAUNCHES, lv)


@pytest.mark.parametrize('bias,relu', FLAGS)
@pytest.mark.parametrize('shape', PROLOGUE_SHAPES)
def test_one_and_two_chunks_on_a_partial_tile_block(dev, shape, bias, relu):
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(7500 + cin)
    (x,), wt, b = _draw(g, n, cin, cout, [(h, w)])
    want = _exact(x, wt, b if bias else None, relu)
    xd = x.to(dev).contiguous(memory_format=CL)
    y = _empty_like_out(xd, cout)
    y.fill_(float('nan'))
    _launch([xd], wt.to(dev).contiguous(memory_format=CL), b.to(dev) if bias else None, [y],
            torch.empty(16 * cin * cout, device=dev), relu)
    assert torch.equal(y.cpu(), want)
