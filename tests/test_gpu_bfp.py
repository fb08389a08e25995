"""BFP neck on the HIP path (csrc/bfp.hip through ops.bfp / necks.BFP) against the torch-CPU
reference ops (necks.BFP's CPU branch: the reference's lib/necks.py:116-141 expressions).

Forward: bit-exact (assert_array_equal).  Max pooling and nearest resampling select values,
the mean is the reference's adds in its order and one f32 divide by 4 (or 1), and the build
has no FMA contraction.  Backward: against torch-CPU autograd of the same module in float64,
within 1e-4 of the largest gradient magnitude (the project's gradient bar; a gradient routed
to the wrong cell is an O(1) error).  The kernels' sums run in a fixed order, so two runs
agree bit for bit."""
import numpy as np
import pytest
import torch

import libra_inputs
from frcnn_amd.necks import BFP, FPN

pytestmark = pytest.mark.gpu


def _layout(a, how, dev, last):
    t = torch.from_numpy(a).to(dev)
    if how == 'nhwc':
        return t.contiguous(memory_format=torch.channels_last)
    if how == 'view' and last:  # the FPN's extra level: a [::2, ::2] view of a larger channels-last map
        b, c, h, w = t.shape
        big = torch.full((b, c, 2 * h, 2 * w), 7.0, device=dev).contiguous(memory_format=torch.channels_last)
        big[:, :, ::2, ::2] = t
        return big[:, :, ::2, ::2]
    if how == 'view':
        return t.contiguous(memory_format=torch.channels_last)
    return t.contiguous()  # nchw


FWD_CASES = [
    ('ragged', libra_inputs.BFP_RAGGED, 8, 2, 'nhwc'),
    ('ragged_nchw', libra_inputs.BFP_RAGGED, 8, 2, 'nchw'),
    ('ragged_view', libra_inputs.BFP_RAGGED, 8, 2, 'view'),
    ('divisible', libra_inputs.BFP_DIVISIBLE, 8, 2, 'nhwc'),
    ('scalar_c3', libra_inputs.BFP_RAGGED, 3, 2, 'nhwc'),
    ('scalar_c3_nchw', libra_inputs.BFP_RAGGED, 3, 1, 'nchw'),
    ('refine0', libra_inputs.BFP_RAGGED, 8, 0, 'nhwc'),
    ('refine_last', libra_inputs.BFP_RAGGED, 8, 4, 'view'),
    ('two_levels', libra_inputs.BFP_RAGGED[1:3], 8, 1, 'nhwc'),
    ('two_levels_r0', libra_inputs.BFP_RAGGED[:2], 4, 0, 'nchw'),
    ('multi_block', [(37, 41), (19, 21), (10, 11)], 260, 1, 'nhwc'),  # rows wider than one workgroup
]


@pytest.mark.parametrize('case', FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_bfp_forward_bit_exact(dev, case):
    _, sizes, channels, r, how = case
    feats = libra_inputs.bfp_levels(50, sizes, channels)
    m = BFP(channels, len(sizes), r)
    ref = m([torch.from_numpy(a) for a in feats])
    with torch.no_grad():
        out = m([_layout(a, how, dev, i == len(sizes) - 1) for i, a in enumerate(feats)])
    assert len(out) == len(ref)
    for o, e in zip(out, ref):
        assert o.shape == e.shape and o.is_contiguous(memory_format=torch.channels_last)
        np.testing.assert_array_equal(o.cpu().numpy(), e.numpy())


def test_bfp_forward_with_nan_and_inf(dev):
    """torch's max scan: a NaN in a window wins it; -inf windows stay -inf."""
    feats = libra_inputs.bfp_levels(51, libra_inputs.BFP_RAGGED, 4)
    feats[0][0, 1, 3, 4] = np.nan
    feats[0][1, 2, :, :] = -np.inf
    feats[3][0, 0, 1, 1] = np.inf
    m = BFP(4, 5, 2)
    ref = m([torch.from_numpy(a) for a in feats])
    with torch.no_grad():
        out = m([_layout(a, 'nhwc', dev, False) for a in feats])
    for o, e in zip(out, ref):
        np.testing.assert_array_equal(o.cpu().numpy(), e.numpy())


def _backward_case(dev, sizes, channels, r, how, quantise, seed):
    feats = libra_inputs.bfp_levels(seed, sizes, channels, quantise=quantise)
    rng = np.random.default_rng(seed + 1)
    gouts = [rng.standard_normal(a.shape).astype(np.float32) for a in feats]
    m = BFP(channels, len(sizes), r)
    x64 = [torch.from_numpy(a).double().requires_grad_(True) for a in feats]
    ref = m(x64)
    torch.autograd.backward(ref, [torch.from_numpy(g).double() for g in gouts])
    xg = [_layout(a, how, dev, i == len(sizes) - 1).requires_grad_(True) for i, a in enumerate(feats)]
    out = m(xg)
    torch.autograd.backward(out, [torch.from_numpy(g).to(dev) for g in gouts])
    for i, (a, e) in enumerate(zip(xg, x64)):
        got, want = a.grad.cpu().numpy().astype(np.float64), e.grad.numpy()
        bar = 1e-4 * np.abs(want).max()
        err = np.abs(got - want).max()
        print('level {}: max |grad| {:.4g}, max err {:.3g}, bar {:.3g}'.format(i, np.abs(want).max(), err, bar))
        assert err <= bar, (i, err, bar)
    return [a.grad.clone() for a in xg]


BWD_CASES = [
    ('ragged', libra_inputs.BFP_RAGGED, 8, 2, 'nhwc', 0),
    ('ragged_view', libra_inputs.BFP_RAGGED, 8, 2, 'view', 0),
    ('divisible_nchw', libra_inputs.BFP_DIVISIBLE, 8, 2, 'nchw', 0),
    ('scalar_c3', libra_inputs.BFP_RAGGED, 3, 2, 'nhwc', 0),
    ('refine0', libra_inputs.BFP_RAGGED, 8, 0, 'nhwc', 0),
    ('refine_last', libra_inputs.BFP_RAGGED, 8, 4, 'nhwc', 0),
    ('two_levels', libra_inputs.BFP_RAGGED[1:3], 8, 1, 'nhwc', 0),
    # inputs quantised to 3 / 5 values: most windows tie and the gradient must land on torch's
    # first-in-scan cell
    ('tied', libra_inputs.BFP_RAGGED, 8, 2, 'nhwc', 3),
    ('tied_refine0', libra_inputs.BFP_RAGGED, 4, 0, 'nhwc', 5),
    ('tied_refine_last', libra_inputs.BFP_RAGGED, 4, 4, 'nchw', 3),
]


@pytest.mark.parametrize('case', BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_bfp_backward_vs_float64_autograd(dev, case):
    _, sizes, channels, r, how, q = case
    _backward_case(dev, sizes, channels, r, how, q, 60)


def test_bfp_backward_cell_is_argmax_of_two_windows(dev):
    """13 -> 7 rows: windows [0,2) [1,4) [3,6) .. overlap in rows 1, 3, 5, ..; a large value
    there is the argmax of both windows that hold it and receives both gradients."""
    sizes = [(13, 11), (7, 6)]
    feats = libra_inputs.bfp_levels(70, sizes, 4)
    feats[0][:, :, 1, 1] = 50.0  # row 1 lies in row-windows 0 and 1, column 1 in column-windows 0 and 1
    m = BFP(4, 2, 1)
    x64 = [torch.from_numpy(a).double().requires_grad_(True) for a in feats]
    g = [np.ones(a.shape, np.float32) for a in feats]
    torch.autograd.backward(m(x64), [torch.from_numpy(v).double() for v in g])
    want = x64[0].grad.numpy()
    assert want[0, 0, 1, 1] > 3.5  # its own + four windows' gradients (mean over 1 level: / 1)
    xg = [torch.from_numpy(a).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
          for a in feats]
    torch.autograd.backward(m(xg), [torch.from_numpy(v).to(dev) for v in g])
    for a, e in zip(xg, x64):
        assert np.abs(a.grad.cpu().numpy() - e.grad.numpy()).max() <= 1e-4 * np.abs(e.grad.numpy()).max()


def test_bfp_backward_is_deterministic(dev):
    a = _backward_case(dev, libra_inputs.BFP_RAGGED, 8, 2, 'nhwc', 3, 80)
    b = _backward_case(dev, libra_inputs.BFP_RAGGED, 8, 2, 'nhwc', 3, 80)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_fpn_then_bfp_under_graph_capture(dev):
    """FPN -> BFP captured in a torch.cuda.graph (as graphs.capture_trunk captures the neck)
    and replayed with changed input contents equals the eager call bit for bit: the BFP
    launches take no host synchronisation and no table built at run time."""
    torch.manual_seed(3)
    fpn = FPN([8, 16, 32], 8, 5).to(dev)
    bfp = BFP(8, 5, 2)
    sizes = [(27, 35), (14, 18), (7, 9)]
    xs = [torch.randn(2, c, h, w, device=dev) for c, (h, w) in zip((8, 16, 32), sizes)]
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            bfp(fpn(xs))
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        static_out = bfp(fpn(xs))
    for k in range(2):
        new = [torch.randn_like(x) * (k + 2) for x in xs]
        for x, n in zip(xs, new):
            x.copy_(n)
        graph.replay()
        torch.cuda.synchronize(dev)
        with torch.no_grad():
            eager = bfp(fpn(xs))
        for o, e in zip(static_out, eager):
            assert torch.equal(o, e)
            assert o.shape[2] > 0 and o.is_contiguous(memory_format=torch.channels_last)


def test_bfp_rejects_bad_inputs(dev):
    from frcnn_amd import ops
    a = torch.zeros(1, 4, 4, 4, device=dev)
    with pytest.raises(AssertionError):
        ops.bfp([a], 0)
    with pytest.raises(AssertionError):
        ops.bfp([a, torch.zeros(1, 8, 2, 2, device=dev)], 0)
    with pytest.raises(RuntimeError):
        ops.bfp([a, torch.zeros(1, 4, 2, 2)], 0)
