"""RoIPool (csrc/roi_pool.hip, ops._RoIPoolFn): the argmax, the backward scatter, the feature
strides and the extractor's per-level path, on an input with the edges the C4 config really
feeds it.

One 2 x 8 x 38 x 64 map in two forms -- continuous, and quantised to round(max(f, 0) * 2) / 2, a
post-ReLU map full of equal values -- and 64 RoIs (border, outside, degenerate, sub-pixel and random
ones, all with x2 >= x1 and y2 >= y1), scale 1/16, 7 x 7 bins.  On the quantised map a bin's
maximum usually occurs in several cells, and then the tie rule (the first cell in row-major order:
strict `>`) decides the argmax and with it where the gradient goes.

* forward: `out` AND `argmax` equal the oracle's (same rule, restated in C) for contiguous NCHW,
  channels_last and a strided view; the argmax is y * W + x of the logical map whatever the strides.
* backward: against a float64 scatter of grad_out into the oracle's argmax cells.  A cell with m
  contributions g_i is the sum of m f32 additions in the order the atomics happen to run, so
  |got - ref| <= (m - 1) * 2^-24 * sum|g_i| * (1 + 2^-20) (the standard bound of recursive f32
  summation in any order; the first addition, to 0, is exact); cells with one contribution are
  exact and cells with none exactly 0.
* no RoIs: a [0, C, 7, 7] output whose backward is an all-zero gradient.
* BasicRoIExtractor with a RoIPool layer (the C4 config's form, _forward_per_level).

The CPU guard test asserts from the oracle and the map alone that the input still has its edges
(empty bins, tied maxima, cells hit by several bins), so the GPU tests cannot pass on an input that
lost them."""
import functools

import numpy as np
import pytest
import torch

import inputs
import oracle
import support

H, W, C, B = 38, 64, 8, 2
PH, PW = 7, 7
SCALE = 1.0 / 16.0


@functools.lru_cache(maxsize=None)
def _case():
    """The inputs and the oracle's results, computed once and shared (treated as read-only)."""
    f = inputs.feature_maps(70, [(H, W)], C, B)[0]
    fq = (np.round(np.maximum(f, 0) * 2) / 2).astype(np.float32)
    rois = support.rois(71, 64, B)
    assert np.all(rois[:, 3] >= rois[:, 1]) and np.all(rois[:, 4] >= rois[:, 2])
    d = dict(rois=rois, cont=f, quant=fq)
    for name in ('cont', 'quant'):
        d[name + '_out'], d[name + '_arg'] = oracle.roi_pool(d[name], rois, (PH, PW), SCALE)
    for v in d.values():
        v.setflags(write=False)
    return d


def _bin_edges(rois):
    """The bins' cell ranges [hs, he) x [ws, we), restated in numpy f32 (torchvision's RoIPool:
    round-half-away of the scaled corners, floor / ceil bin edges, clipped to the map)."""
    f32 = np.float32

    def rnd(v):  # roundf
        v = v.astype(np.float64)
        return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)
    sw, sh = rnd(rois[:, 1] * f32(SCALE)), rnd(rois[:, 2] * f32(SCALE))
    ew, eh = rnd(rois[:, 3] * f32(SCALE)), rnd(rois[:, 4] * f32(SCALE))
    rw, rh = np.maximum(ew - sw + 1, 1), np.maximum(eh - sh + 1, 1)
    bh, bw = rh.astype(f32) / f32(PH), rw.astype(f32) / f32(PW)
    py, px = np.arange(PH, dtype=f32), np.arange(PW, dtype=f32)
    hs = np.clip(np.floor(py[None] * bh[:, None]).astype(np.int64) + sh[:, None], 0, H)
    he = np.clip(np.ceil((py[None] + f32(1)) * bh[:, None]).astype(np.int64) + sh[:, None], 0, H)
    ws = np.clip(np.floor(px[None] * bw[:, None]).astype(np.int64) + sw[:, None], 0, W)
    we = np.clip(np.ceil((px[None] + f32(1)) * bw[:, None]).astype(np.int64) + sw[:, None], 0, W)
    return hs, he, ws, we


def _scatter(rois, arg, g):
    """float64 scatter of g into the argmax cells: (sum, sum of |g|, contributions) per cell."""
    K = len(rois)
    img = rois[:, 0].astype(np.int64)
    plane = (img[:, None] * C + np.arange(C)[None]) * (H * W)  # [K, C]
    idx = plane[:, :, None, None] + arg.astype(np.int64)
    hit = arg >= 0
    ref, mag, cnt = (np.zeros(B * C * H * W, t) for t in (np.float64, np.float64, np.int64))
    g64 = g.astype(np.float64)
    np.add.at(ref, idx[hit], g64[hit])
    np.add.at(mag, idx[hit], np.abs(g64[hit]))
    np.add.at(cnt, idx[hit], 1)
    assert idx.shape == (K, C, PH, PW)
    return (a.reshape(B, C, H, W) for a in (ref, mag, cnt))


def test_inputs_keep_their_edges():
    """From the oracle and the map alone: the quantised case has empty bins, non-empty bins whose
    maximum occurs in more than one of their cells (counted from the map, not from the argmax) and
    cells that receive several gradient contributions."""
    d = _case()
    arg, fq, rois = d['quant_arg'], d['quant'], d['rois']
    empty = int((arg < 0).sum())
    hs, he, ws, we = _bin_edges(rois)
    tied = n_empty_geom = 0
    for k in range(len(rois)):
        b = int(rois[k, 0])
        for py in range(PH):
            for px in range(PW):
                win = fq[b, :, hs[k, py]:he[k, py], ws[k, px]:we[k, px]].reshape(C, -1)
                if win.shape[1] == 0:
                    n_empty_geom += C
                    continue
                tied += int(((win == win.max(1, keepdims=True)).sum(1) > 1).sum())
    _, _, cnt = _scatter(rois, arg, np.ones(arg.shape, np.float32))
    multi = int((cnt >= 2).sum())
    print('roi_pool inputs: {} empty bins of {}, {} bins with a tied maximum, {} cells with >= 2 contributions '
          '(at most {})'.format(empty, arg.size, tied, multi, int(cnt.max())))
    assert n_empty_geom == empty  # the restated bin edges agree with the oracle's on which bins are empty
    assert empty >= 500
    assert tied >= 1000
    assert multi >= 1000
    # the two forms differ, and the continuous one has (next to) no ties: they are two cases
    assert not np.array_equal(d['cont_arg'], arg)


def _layout(f, dev, layout):
    """f on the device in the asked layout; every layout is the same logical [B, C, H, W] map."""
    t = torch.from_numpy(np.array(f)).to(dev)
    if layout == 'nhwc':
        t = t.contiguous(memory_format=torch.channels_last)
        assert t.stride(1) == 1
    elif layout == 'strided':
        big = np.random.default_rng(72).standard_normal((B, C, 2 * H, 2 * W)).astype(np.float32) + 20.0
        big = torch.from_numpy(big).to(dev)  # the cells between are larger than any of f's: a wrong stride shows
        big[:, :, ::2, ::2] = t
        t = big[:, :, ::2, ::2]
        assert not t.is_contiguous() and t.shape == (B, C, H, W)
    return t


@pytest.mark.gpu
@pytest.mark.parametrize('layout', ['nchw', 'nhwc', 'strided'])
@pytest.mark.parametrize('form', ['cont', 'quant'])
def test_forward_and_argmax_equal_oracle(dev, form, layout):
    """frh_roi_pool_fwd through the C entry: out and argmax, bit for bit, for three stride sets."""
    from frcnn_amd import _lib
    d = _case()
    f = _layout(d[form], dev, layout)
    rois = torch.from_numpy(np.array(d['rois'])).to(dev)
    K = rois.shape[0]
    out = torch.full((K, C, PH, PW), float('nan'), dtype=torch.float32, device=dev)
    arg = torch.full((K, C, PH, PW), -7, dtype=torch.int32, device=dev)
    p = _lib.ptr
    _lib.call('frh_roi_pool_fwd', p(f), _lib.i64_array(f.stride()), H, W, C, SCALE, p(rois), K, PH, PW, p(out),
              p(arg), _lib.stream_of(out))
    np.testing.assert_array_equal(out.cpu().numpy(), d[form + '_out'])
    np.testing.assert_array_equal(arg.cpu().numpy(), d[form + '_arg'])


@pytest.mark.gpu
@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
def test_backward_against_float64_scatter(dev, layout):
    """ops.roi_pool under autograd on the quantised map: each cell within the f32 summation bound
    of the float64 scatter, exact where one bin or none contributes."""
    from frcnn_amd import ops
    d = _case()
    rois = d['rois']
    g = np.random.default_rng(73).standard_normal((len(rois), C, PH, PW)).astype(np.float32)
    ref, mag, cnt = _scatter(rois, d['quant_arg'], g)
    f = _layout(d['quant'], dev, layout).requires_grad_(True)
    out = ops.roi_pool(f, torch.from_numpy(np.array(rois)).to(dev), (PH, PW), SCALE)
    out.backward(torch.from_numpy(g).to(dev))
    got = f.grad.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    bound = np.maximum(cnt - 1, 0) * 2.0 ** -24 * mag * (1 + 2.0 ** -20)
    many = cnt >= 2
    print('roi_pool backward [{}]: {} cells with >= 2 contributions (at most {}), largest error / bound = {:.4f}'
          .format(layout, int(many.sum()), int(cnt.max()), float((err[many] / bound[many]).max())))
    np.testing.assert_array_equal(got[cnt == 0], 0.0)
    np.testing.assert_array_equal(got[cnt == 1], ref[cnt == 1])
    assert many.sum() >= 1000
    bad = err > bound
    assert not bad.any(), 'cells outside the bound: {} (first at {})'.format(int(bad.sum()), np.argwhere(bad)[0])


@pytest.mark.gpu
def test_no_rois(dev):
    """K = 0: a [0, C, 7, 7] output, and its backward an all-zero gradient of the feature's shape."""
    from frcnn_amd import ops
    f = torch.from_numpy(np.array(_case()['quant'])).to(dev).requires_grad_(True)
    out = ops.roi_pool(f, torch.zeros(0, 5, device=dev), (PH, PW), SCALE)
    assert out.shape == (0, C, PH, PW) and out.dtype == torch.float32
    out.backward(torch.zeros_like(out))
    assert f.grad is not None and f.grad.shape == f.shape
    assert torch.count_nonzero(f.grad).item() == 0


@pytest.mark.gpu
def test_extractor_per_level_path(dev):
    """BasicRoIExtractor with one RoIPool layer (the C4 config: _forward_per_level), two per-image
    proposal lists: the concatenated rows equal oracle.roi_pool's."""
    from frcnn_amd.region import BasicRoIExtractor
    d = _case()
    ex = BasicRoIExtractor([dict(type='RoIPool', spatial_scale=SCALE, sampling_ratio=2)], output_size=(PH, PW))
    rois = d['rois']
    props = [np.ascontiguousarray(rois[rois[:, 0] == b, 1:].T) for b in range(B)]
    assert all(p.shape[1] > 8 for p in props)
    outs = ex([torch.from_numpy(np.array(d['quant'])).to(dev)], [torch.from_numpy(p).to(dev) for p in props])
    r5 = np.concatenate([np.concatenate([np.full((p.shape[1], 1), b, np.float32), p.T], 1)
                         for b, p in enumerate(props)], 0)
    ref, _ = oracle.roi_pool(d['quant'], r5, (PH, PW), SCALE)
    np.testing.assert_array_equal(outs.flat.cpu().numpy(), ref)
    off = 0
    for b, p in enumerate(props):
        np.testing.assert_array_equal(outs[b].cpu().numpy(), ref[off:off + p.shape[1]])
        off += p.shape[1]
