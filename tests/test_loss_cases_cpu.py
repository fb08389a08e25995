"""The cases of tests/loss_cases.py, checked without a GPU: every builder hits the edge it is
named for, and the float64 reference and its f32 CPU restatement (the yardstick of
test_gpu_losses_f64.py's gradient bound) are finite for every case.  These are conditions on the
inputs, not measurements; no GPU test may skip an element."""
import math

import pytest
import torch

import loss_cases as lc

CLS_PARAMS = [('focal', a, g) for a, g in lc.FOCAL_PARAMS] + [('bce', 0.25, 2.0), ('softmax', 0.25, 2.0)]
COUNTS = [(k, n, c) for k in ('focal', 'bce') for n, c in lc.SIGMOID_COUNTS] + \
         [('softmax', n, c) for n, c in lc.SOFTMAX_COUNTS]
L1_CASES = [(b, rd, v) for b in lc.L1_BETAS for rd in (0, 1) for v in lc.L1_VARIANTS
            if not (v == 'class_select' and rd == 1)]


def _finite_references(case):
    assert math.isfinite(case['loss64']) and math.isfinite(case['loss32'])
    assert set(case['grads']) == set(lc.SCALES)
    for g64, g32, e32 in case['grads'].values():
        assert g64.dtype == torch.float64 and g32.dtype == torch.float32 and g64.shape == case['x'].shape
        assert bool(torch.isfinite(g64).all()) and bool(torch.isfinite(g32).all()) and math.isfinite(e32)


def test_the_case_tables_are_the_listed_ones():
    assert {n * c for n, c in lc.SIGMOID_COUNTS if c == 1} == {1, 255, 256, 257, 65535, 65536, 65537, 131075}
    assert {(n, c) for n, c in lc.SIGMOID_COUNTS if c > 1} == {(16384, 4), (16385, 4), (21846, 3)}
    # at and just past the capped grid of 256 workgroups x 256 threads; 21 846 x 3 = 65 538 ends in
    # the middle of a row's channels
    assert 16384 * 4 == 65536 and 16385 * 4 == 65540 and 21846 * 3 == 65538
    assert set(lc.SOFTMAX_COUNTS) == {(1, 3), (257, 3), (65536, 3), (65537, 3)}
    assert sorted(m for ms in lc.MAGNITUDES.values() for m in ms) == [0.0, 1e-4, 1.0, 5.0, 10.0, 16.0, 17.0, 20.0,
                                                                      30.0, 87.0, 88.8, 100.0, 1e4]
    assert set(lc.FOCAL_PARAMS) == {(0.25, 2.0), (0.5, 0.0), (0.5, 1.0), (0.25, 1.5)}
    assert set(lc.SCALES) == {0.37, 1e-8, 1e4} and set(lc.L1_BETAS) == {1.0 / 9.0, 0.5, 1.0}
    assert all(not 0.0 < g < 1.0 for _, g in lc.FOCAL_PARAMS)  # the supported gamma domain


@pytest.mark.parametrize('mag', list(lc.MAGNITUDES))
@pytest.mark.parametrize('kind,alpha,gamma', CLS_PARAMS)
def test_magnitude_case_crosses_signs_and_targets(kind, alpha, gamma, mag):
    case = lc.magnitude_case(kind, mag, alpha, gamma)
    x, lab = case['x'], case['lab']
    assert x.shape[1] == 3 and x.dtype == torch.float32 and lab.dtype == torch.int64
    assert bool((lab == -1).any())
    kept = lab >= 0
    if kind == 'softmax':
        assert int(lab.max()) == 2
        xs = x[kept]
        row_min, row_max = xs.min(1).values, xs.max(1).values
        at_label = xs[torch.arange(len(xs)), lab[kept]]
        mixed = (row_min < 0) & (row_max > 0)  # both signs within a row ...
        # ... labelled at its minimum logit, and at its maximum
        assert bool((mixed & (at_label == row_min)).any()) and bool((mixed & (at_label == row_max)).any())
        for m in lc.MAGNITUDES[mag]:
            for v in (m, -m):
                assert bool((xs == torch.tensor(v, dtype=torch.float32)).any())
    else:
        assert int(lab.max()) == 3
        target = (lab.view(-1, 1) == torch.arange(1, 4).view(1, -1))[kept]
        xs = x[kept]
        for m in lc.MAGNITUDES[mag]:
            for v in (m, -m):
                at = xs == torch.tensor(v, dtype=torch.float32)
                assert bool((at & target).any()) and bool((at & ~target).any()), (v, 'needs target 0 and 1')
    _finite_references(case)


@pytest.mark.parametrize('kind,n,c', COUNTS)
def test_count_case_labels(kind, n, c):
    case = lc.count_case(kind, n, c)
    x, lab = case['x'], case['lab']
    assert tuple(x.shape) == (n, c) and tuple(lab.shape) == (n,)
    hi = c - 1 if kind == 'softmax' else c
    assert int(lab.min()) >= -1 and int(lab.max()) <= hi
    if n in (257, 65537):
        assert int(lab[-1]) == -1
    if n == 1:
        assert int(lab[0]) == 1
    else:
        pos, ign = float((lab > 0).float().mean()), float((lab == -1).float().mean())
        assert 0.15 < pos < 0.35 and 0.1 < ign < 0.3
        # scattered: both halves of the tensor carry ignored and positive rows
        for half in (lab[:n // 2], lab[n // 2:]):
            assert bool((half == -1).any()) and bool((half > 0).any())
    _finite_references(case)
    # the ignored rows' reference gradient is exactly zero
    assert not bool(case['grads'][0.37][0][lab < 0].any())


@pytest.mark.parametrize('layout', lc.LAYOUTS)
@pytest.mark.parametrize('c', [1, 3, 4])
def test_layouts_hold_the_values_and_the_named_strides(layout, c):
    n = 6
    x = torch.arange(n * c, dtype=torch.float32).view(n, c)
    buf = lc.place(x, layout)
    v = lc.view_of(buf, c, layout)
    assert torch.equal(v, x) and tuple(buf.shape) == lc.buffer_shape(n, c, layout)
    sr, sc = v.stride()
    wide = c + lc.PAD_COLS
    want = {'rows': (c, 1), 'channel_major': (1, n), 'row_slice': (wide, 1), 'col_stride': (wide, 2)}
    assert (sr, sc) == want[layout]
    assert int(torch.isnan(buf).sum()) == buf.numel() - n * c
    # the largest offset a kernel forms stays inside the buffer
    assert (n - 1) * sr + (c - 1) * sc < buf.numel()
    if c > 1:
        assert (sr < sc) == (layout == 'channel_major')  # the traversal-order switch of make_cls


@pytest.mark.parametrize('beta,rows_dim,variant', L1_CASES)
def test_l1_case_hits_its_edges(beta, rows_dim, variant):
    case = lc.l1_case(beta, rows_dim, variant)
    b32 = lc.f32_scale(beta)
    n = case['n']
    assert n * 4 > 4 * 256 and (n * 4) % 256 != 0
    lab = case['lab']
    if variant == 'no_pos':
        assert int(lab.max()) == 0 and bool((lab == -1).any())
        assert case['loss64'] == 0.0 and not bool(case['grads'][0.37][0].any())
    else:
        assert bool((lab[:5] > 0).all()) and int(lab[-1]) == -1 and bool((lab == 0).any())
        assert lc.l1_diff(case, 0, 0) == b32 and lc.l1_diff(case, 1, 1) == -b32 and lc.l1_diff(case, 2, 2) == 0.0
        g64 = case['grads'][0.37][0]
        s = lc.f32_scale(0.37)
        xi = lambda i, j: lc._l1_element(case, i, j)[0]  # noqa: E731
        # d == beta takes the linear branch (slope 1), diff == 0 has sign 0
        assert float(g64[xi(0, 0)]) == s and float(g64[xi(1, 1)]) == -s and float(g64[xi(2, 2)]) == 0.0
    if variant == 'large':
        assert lc.l1_diff(case, 3, 3) == 1e4 and lc.l1_diff(case, 4, 0) == -1e4
    if variant == 'class_select':
        assert case['classes'] == 21 and tuple(case['x'].shape) == (n, 84)
        assert int(lab[0]) == 20 and int(lab.max()) == 20
    else:
        assert case['classes'] == 0 and tuple(case['x'].shape) == tuple(case['y'].shape)
    assert tuple(case['y'].shape) == ((n, 4) if rows_dim == 0 else (4, n))
    _finite_references(case)
    mask = lc.l1_selected_mask(case)
    assert int(mask.sum()) == 4 * int((lab > 0).sum())
    assert not bool(case['grads'][0.37][0][~mask].any())


def test_l1_bad_label_case():
    case = lc.l1_bad_label_case()
    assert int(case['lab'][3]) == case['classes'] == 21 and int((case['lab'] >= 21).sum()) == 1
    # the largest offset the class select may form for the other rows is in bounds
    assert int(case['lab'][case['lab'] < 21].max()) == 20
    _finite_references(case)
    mask = lc.l1_selected_mask(case)
    assert not bool(mask[3].any()) and int(mask.sum()) == 4 * (int((case['lab'] > 0).sum()) - 1)
    assert not bool(case['grads'][0.37][0][3].any())


@pytest.mark.parametrize('kind,n,c', [(k, n, c) for k in lc.KINDS for n, c in ((257, 1), (65537, 1), (16385, 4))])
def test_written_case_ends_on_an_ignored_row(kind, n, c):
    case = lc.written_case(kind, n, c)
    lab = case['lab']
    assert int(lab[-1]) == -1 and bool((lab >= 0).any())
    assert int(lab.max()) <= (c - 1 if kind == 'softmax' else c) and int(lab.min()) == -1
    for layout in ('row_slice', 'col_stride'):  # the gradient buffers of that test: the view fits
        rows, cols = lc.buffer_shape(n, c, layout)
        sr, sc = (cols, 1) if layout == 'row_slice' else (cols, 2)
        assert (n - 1) * sr + (c - 1) * sc < rows * cols
