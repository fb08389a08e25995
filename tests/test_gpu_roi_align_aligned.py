"""RoIAlign with aligned=True (torchvision's half-pixel form: the box shifted by 0.5 after scaling,
no clamp of the RoI's width and height to 1) on every forward and backward kernel.

Every kernel takes its geometry from roi_geom* (csrc/roi_common.h); the staged kernels derive tap
windows, tap lists, band heights and slab layouts from it.  With aligned=True a RoI may have zero
size: all samples of a row / column coincide, windows of 1 x 1 and 2 x 2 cells appear, and the
adaptive grid (sampling_ratio 0) is 0 x 0.  The forward is compared bit for bit with the oracle
(oracle.roi_align(..., aligned=True), same operation order), the backward at the tolerance the
legacy (aligned=False) kernels are held to.

Two levels, 19 x 32 at scale 1/32 and 10 x 30 at scale 1/4, 2 images; border / outside /
degenerate / sub-pixel and random RoIs, wide RoIs, RoIs far larger than the 10 x 30 level, and
whole-map RoIs on the 19 x 32 level.  All RoIs have x2 >= x1 and y2 >= y1: inverted RoIs are out of
scope (torchvision rejects them for aligned=True: the box size would be negative).

The CPU guard test restates make_tap / roi_geom in numpy f32 and asserts that the set still holds
the cases the kernels branch on."""
import functools

import numpy as np
import pytest
import torch

import inputs
import oracle
import support

GRIDS = [(19, 32), (10, 30)]
SCALES = [1 / 32, 1 / 4]
B = 2


@functools.lru_cache(maxsize=None)
def _set():
    """(rois [K, 5], levels [K]): read-only, shared by every test."""
    wide = np.array([[1, 0, 0, 119, 39], [0, 2, 1, 110, 38], [1, 30, 20, 1000, 500]], np.float32)
    # whole-map RoIs on the 19 x 32 level: windows of 19 rows x 28 tap-list columns (> 480 cells)
    large = np.array([[0, -10, -10, 1100, 650], [1, 0, 0, 1023, 607], [0, 5, 3, 1015, 600]], np.float32)
    rois = np.concatenate([large, support.rois(61, 64, B), wide[2:], support.pathological_rois(B), wide[:2]], 0)
    levels = np.zeros(len(rois), np.int64)
    levels[-13:] = 1  # the pathological and the first two wide RoIs on the 10 x 30 level
    assert np.all(rois[:, 3] >= rois[:, 1]) and np.all(rois[:, 4] >= rois[:, 2])
    rois.setflags(write=False)
    levels.setflags(write=False)
    return rois, levels


@functools.lru_cache(maxsize=None)
def _feats(C, seed=90):
    fs = tuple(inputs.feature_maps(seed, GRIDS, C, B))
    for f in fs:
        f.setflags(write=False)
    return fs


@functools.lru_cache(maxsize=None)
def _ref_fwd(C, pooled, sampling):
    rois, levels = _set()
    ref = oracle.roi_align(list(_feats(C)), rois, levels, SCALES, pooled, sampling, aligned=True)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _grad_out(C, pooled):
    g = np.random.default_rng(91).standard_normal((len(_set()[0]), C) + pooled).astype(np.float32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _ref_bwd(C, pooled, sampling):
    rois, levels = _set()
    ref = oracle.roi_align_bwd([f.shape for f in _feats(C)], rois, levels, SCALES, _grad_out(C, pooled), sampling,
                               aligned=True)
    return tuple(ref)


# ----------------------------------------------------------------- the geometry, restated
def _axis_taps(lo_px, hi_px, scale, size, bins, aligned):
    """make_tap of the 2 * bins sample positions of one axis (sampling 2), in f32 as roi_geom and
    sample_y / sample_x compute them: (valid, lo, hi) arrays and the RoI's extent on the axis."""
    f32 = np.float32
    off = f32(0.5) if aligned else f32(0.0)
    s = f32(lo_px) * f32(scale) - off
    e = f32(hi_px) * f32(scale) - off
    ext = e - s
    if not aligned:
        ext = max(ext, f32(1.0))
    bin_ = ext / f32(bins)
    valid, lo, hi = [], [], []
    for p in range(bins):
        for i in range(2):
            v = s + f32(p) * bin_ + (f32(i) + f32(0.5)) * bin_ / f32(2)
            assert isinstance(v, np.float32)
            ok = not (v < f32(-1.0) or v > f32(size))
            v = max(v, f32(0.0))
            a = int(v)
            if a >= size - 1:
                a = b = size - 1
            else:
                b = a + 1
            valid.append(ok), lo.append(a), hi.append(b)
    return np.array(valid), np.array(lo), np.array(hi), ext


def _window(roi, level, ph=7, pw=7, aligned=True):
    """The RoI's tap window as the staged forward kernels lay it out (pair_setup in
    csrc/roi_kernels.h): rows / columns are the dense range [min lo, max hi] of the valid samples
    when that is at most the 4 * bins tap-list entries, else the tap list; the slab's row stride
    is the column count made odd.  None without a valid sample."""
    H, W = GRIDS[level]
    vy, ylo, yhi, rh = _axis_taps(roi[2], roi[4], SCALES[level], H, ph, aligned)
    vx, xlo, xhi, rw = _axis_taps(roi[1], roi[3], SCALES[level], W, pw, aligned)
    d = dict(zero_size=bool(rw == 0 and rh == 0), cells=None, single=False)
    if not vy.any() or not vx.any():
        return d
    ny, nx = yhi[vy].max() - ylo[vy].min() + 1, xhi[vx].max() - xlo[vx].min() + 1
    d['single'] = bool(ny == 1 and nx == 1)
    R, Cs = (ny if ny <= 4 * ph else 4 * ph), (nx if nx <= 4 * pw else 4 * pw)
    d['cells'] = int(R * (Cs | 1))
    # for the band kernel: is the row range dense, the most rows one bin's two samples span in
    # it, and the rows of this width that one band of its 240-cell slab holds
    d['dense_rows'] = bool(ny <= 4 * ph)
    d['bin_rows'] = max([int(yhi[2 * p + 1] - ylo[2 * p] + 1) for p in range(ph) if vy[2 * p] and vy[2 * p + 1]] or [0])
    d['band_rows'] = 240 // (Cs | 1)
    return d


def test_set_holds_the_cases_the_kernels_branch_on():
    rois, levels = _set()
    w = [_window(r, int(l)) for r, l in zip(rois, levels)]
    zero = sum(x['zero_size'] for x in w)
    single = sum(x['single'] for x in w)
    empty = sum(x['cells'] is None for x in w)
    cells = np.array([x['cells'] for x in w if x['cells'] is not None])
    small, mid, big = int((cells <= 192).sum()), int(((cells > 192) & (cells <= 480)).sum()), int((cells > 480).sum())
    print('aligned RoI set: {} RoIs, {} of zero size, {} with a one-cell window, {} without a valid sample; '
          'band-kernel window classes <= 192 / <= 480 / larger: {} / {} / {}'
          .format(len(rois), zero, single, empty, small, mid, big))
    assert zero >= 2
    assert single >= 1
    assert small >= 3 and mid >= 3 and big >= 3
    assert empty >= 1
    # the legacy form of the same set differs: the half pixel and the missing clamp are both in play
    legacy = [_window(r, int(l), aligned=False) for r, l in zip(rois, levels)]
    assert not any(x['zero_size'] for x in legacy)
    a = _ref_fwd(16, (7, 7), 2)
    b = oracle.roi_align(list(_feats(16)), rois, levels, SCALES, (7, 7), 2, aligned=False)
    share = float((a != b).mean())
    print('aligned=True differs from aligned=False on {:.1%} of the outputs'.format(share))
    assert share > 0.2
    # adaptive sampling: a zero-size RoI has a 0 x 0 grid, its rows are exactly 0
    z = np.array([x['zero_size'] for x in w])
    assert not _ref_fwd(16, (7, 7), 0)[z].any()


# ----------------------------------------------------------------- forward
def _dev_feats(C, dev, layout):
    ft = [torch.from_numpy(np.array(f)).to(dev) for f in _feats(C)]
    if layout == 'nhwc':
        ft = [f.contiguous(memory_format=torch.channels_last) for f in ft]
    return ft


FWD_CASES = {
    # name: (layout, C, pooled, sampling)
    'cg': ('nhwc', 64, (7, 7), 2),
    'cg_1x1': ('nhwc', 64, (1, 1), 2),
    'band_c16': ('nhwc', 16, (7, 7), 2),
    'band_c40': ('nhwc', 40, (7, 7), 2),
    'quad': ('nhwc', 16, (4, 12), 2),
    'pair': ('nchw', 16, (7, 7), 2),
    'lds_odd_c': ('nchw', 15, (7, 7), 2),
    'lds_9x7': ('nchw', 16, (9, 7), 2),
    'direct_9x8': ('nchw', 16, (9, 8), 2),
    'direct_adaptive': ('nchw', 16, (7, 7), 0),
    'direct_adaptive_nhwc': ('nhwc', 16, (7, 7), 0),
}


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(FWD_CASES))
def test_forward_bit_identical_to_oracle(dev, case):
    """One case per forward kernel, by roi_fwd's dispatch (csrc/roi_align.hip):

    * cg, cg_1x1 -- roi_align_fwd_cg_kernel: channels-last, C % 64 == 0 (quad_ok and cg_ok).
    * band_c16, band_c40 -- roi_align_fwd_band_kernel: channels-last, C % 4 == 0 but not % 64,
      7 x 7 bins (band_fits); one 16-channel chunk, and two plus a partial third.  The set's windows
      take all three of its paths (quad stages, interleaved stages, row bands: see the guard test).
    * quad -- roi_align_fwd_quad_kernel: channels-last, 4 x 12 bins (a 5-row band of the 49-column
      window exceeds the band kernel's slab).
    * pair -- roi_align_fwd_pair_kernel: NCHW (channel stride != 1), even C, 7 x 7 bins.
    * lds_odd_c -- roi_align_fwd_lds_kernel: NCHW, odd C (pair_ok fails); windows above 256 floats
      take its buffer-gather path.
    * lds_9x7 -- roi_align_fwd_lds_kernel as well: 4 * 9 * 29 = 1044 cells exceed the pair kernel's
      832-cell slab, and 63 bins still fit the per-RoI LDS kernel's 64.
    * direct_9x8 -- roi_align_fwd_kernel (direct gather): 72 bins exceed every staged kernel.
    * direct_adaptive, direct_adaptive_nhwc -- roi_align_fwd_kernel: sampling_ratio 0 (every staged
      kernel needs sampling 2).  A zero-size RoI has a 0 x 0 grid here: its rows are exactly 0.
    """
    from frcnn_amd import ops
    layout, C, pooled, sampling = FWD_CASES[case]
    rois, levels = _set()
    ref = _ref_fwd(C, pooled, sampling)
    out = ops.roi_align_multilevel(_dev_feats(C, dev, layout), torch.from_numpy(np.array(rois)).to(dev),
                                   torch.from_numpy(np.array(levels)).to(dev), SCALES, pooled, sampling,
                                   aligned=True).cpu().numpy()
    np.testing.assert_array_equal(out, ref)
    if sampling == 0:
        zero = np.array([_window(r, int(l))['zero_size'] for r, l in zip(rois, levels)])
        assert zero.sum() >= 2 and not out[zero].any()


@pytest.mark.gpu
def test_module_on_a_strided_view(dev):
    """ops.RoIAlign(..., aligned=True) on a non-contiguous view P[:, :, ::2, ::2] (the pair kernel
    through explicit element strides); a 20 x 30 map at scale 1/32, so that the RoIs lie on it."""
    from frcnn_amd.ops import RoIAlign
    f = inputs.feature_maps(92, [(40, 60)], 32, B)[0]
    ft = torch.from_numpy(f).to(dev)[:, :, ::2, ::2]
    assert not ft.is_contiguous()
    rois = support.rois(93, 64, B)
    out = RoIAlign((7, 7), 1 / 32, 2, aligned=True)(ft, torch.from_numpy(rois).to(dev)).cpu().numpy()
    ref = oracle.roi_align([np.ascontiguousarray(f[:, :, ::2, ::2])], rois, None, [1 / 32], (7, 7), 2, aligned=True)
    np.testing.assert_array_equal(out, ref)
    legacy = oracle.roi_align([np.ascontiguousarray(f[:, :, ::2, ::2])], rois, None, [1 / 32], (7, 7), 2)
    assert (ref != legacy).mean() > 0.2


# ----------------------------------------------------------------- backward
BWD_CASES = {
    # name: (layout, C, pooled, sampling)
    'sep': ('nchw', 16, (7, 7), 2),
    'nhwc_c16': ('nhwc', 16, (7, 7), 2),
    'nhwc_c80': ('nhwc', 80, (7, 7), 2),
    'lds_9x7': ('nchw', 16, (9, 7), 2),
    'direct_adaptive': ('nchw', 16, (7, 7), 0),
}


def _backward(dev, layout, C, pooled, sampling, order=None):
    from frcnn_amd import ops
    rois, levels = _set()
    g = _grad_out(C, pooled)
    order = np.arange(len(rois)) if order is None else order
    ft = [f.requires_grad_(True) for f in _dev_feats(C, dev, layout)]
    out = ops.roi_align_multilevel(ft, torch.from_numpy(rois[order]).to(dev), torch.from_numpy(levels[order]).to(dev),
                                   SCALES, pooled, sampling, aligned=True)
    out.backward(torch.from_numpy(g[order]).to(dev))
    if layout == 'nhwc':
        assert all(f.grad.stride(1) == 1 for f in ft)  # the gradient keeps the features' format
    return [f.grad.clone() for f in ft]


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(BWD_CASES))
def test_backward_vs_oracle(dev, case):
    """One case per backward kernel (frh_roi_align_bwd_strided's dispatch): sep --
    roi_align_bwd_sep_kernel (NCHW gradients, sampling 2, up to 8 x 8 bins); nhwc_c16, nhwc_c80 --
    roi_align_bwd_nhwc_kernel (channels-last gradients; 80 channels = one full and one partial
    64-channel group); lds_9x7 -- roi_align_bwd_lds_kernel (36 tap entries exceed the separable
    kernels' 32, 63 bins fit); direct_adaptive -- roi_align_bwd_kernel (per-tap atomics, sampling 0).
    Float atomics reorder the sums: the legacy kernels' f32-accumulation tolerance."""
    layout, C, pooled, sampling = BWD_CASES[case]
    got = _backward(dev, layout, C, pooled, sampling)
    for a, r in zip(got, _ref_bwd(C, pooled, sampling)):
        np.testing.assert_allclose(a.cpu().numpy(), r, rtol=1e-4, atol=2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
def test_backward_deterministic(dev, layout):
    """frh_roi_align_bwd_fixed (the fixed-point forms of the sep and nhwc kernels) with
    aligned=True: bit-identical across two runs and under a permutation of the RoIs, and within the
    same tolerance of the oracle."""
    from frcnn_amd import ops
    C, pooled = 16, (7, 7)
    ops.set_deterministic_backward(True)
    try:
        a = _backward(dev, layout, C, pooled, 2)
        b = _backward(dev, layout, C, pooled, 2)
        c = _backward(dev, layout, C, pooled, 2, order=np.random.default_rng(94).permutation(len(_set()[0])))
    finally:
        ops.set_deterministic_backward(False)
    for x, y, z, r in zip(a, b, c, _ref_bwd(C, pooled, 2)):
        assert torch.equal(x, y) and torch.equal(x, z)
        np.testing.assert_allclose(x.cpu().numpy(), r, rtol=1e-4, atol=2e-5)


# ----------------------------------------------------------------- RoIs several times taller than their level
# Few of such a RoI's samples are valid, and they lie many rows apart, so the window is still a
# dense row range (at most 28 rows) in which ONE bin's two samples span more rows than a band of
# the band kernel's slab holds (8 rows of the 29-column stride): pair_setup<16, kBandCells> lays
# such a window out as tap-list rows (4 rows per bin), as the channel-group kernel does.  Not
# specific to aligned=True: both forms run.
TALL_ROIS = np.array([[0, 0, -1280, 1023, 2220], [1, 0, -1024, 1023, 2976], [0, 0, -608, 1023, 2892],
                      [1, -5, -352, 1030, 3148]], np.float32)


@pytest.mark.parametrize('aligned', [False, True])
def test_tall_rois_exceed_a_band(aligned):
    w = [_window(r, 0, aligned=aligned) for r in TALL_ROIS]
    over = [x for x in w if x['cells'] > 480 and x['dense_rows'] and x['bin_rows'] > x['band_rows']]
    print('aligned={}: bin rows / band rows {}'.format(aligned, [(x['bin_rows'], x['band_rows']) for x in over]))
    assert len(over) >= 3
    # nothing of the kind in the main set (its band-path bins fit their bands)
    rois, levels = _set()
    main = [_window(r, int(l), aligned=aligned) for r, l in zip(rois, levels)]
    assert all(x['bin_rows'] <= x['band_rows'] for x in main if x['cells'] is not None and x['cells'] > 480)


@pytest.mark.gpu
@pytest.mark.parametrize('aligned', [False, True])
@pytest.mark.parametrize('kernel,layout,C', [('band', 'nhwc', 16), ('cg', 'nhwc', 64), ('pair', 'nchw', 16)])
def test_tall_rois_forward_bit_identical(dev, kernel, layout, C, aligned):
    """The band kernel (dense window -> tap-list rows), the channel-group kernel (list-row bands)
    and the pair kernel (whole window in one slab) on the tall RoIs, 19 x 32 level, 7 x 7 bins."""
    from frcnn_amd import ops
    feats = _feats(C)[:1]
    ref = oracle.roi_align(list(feats), TALL_ROIS, None, SCALES[:1], (7, 7), 2, aligned=aligned)
    assert np.count_nonzero(ref) > ref.size // 8
    ft = _dev_feats(C, dev, layout)[:1]
    out = ops.roi_align_multilevel(ft, torch.from_numpy(TALL_ROIS).to(dev), None, SCALES[:1], (7, 7), 2,
                                   aligned=aligned).cpu().numpy()
    np.testing.assert_array_equal(out, ref)
