"""The fused detection losses (csrc/losses.hip: frh_cls_loss_fwd/bwd, frh_smooth_l1_fwd/bwd,
frh_det_loss_fwd) against float64 at their edges, on the cases of tests/loss_cases.py: saturated
logits up to and past expf overflow, every focal (alpha, gamma) pair, element counts around one
workgroup and around the capped grid, strided views, ignored (-1) rows, smooth-L1 at d == beta,
diff == 0 and |diff| = 1e4, class select at the last class.

Forward: the sum is finite and within the project's rtol 2e-5 (header of test_gpu_losses.py) of
the float64 sum.  Backward, elementwise: |g - g64| <= 8 E32 + 2^-22 |g64|, E32 = max |g32 - g64|
of the f32 CPU restatement over the case (the reference's own f32 error; 8 is the margin
test_accuracy_against_float64 of the conv tests grants over torch's f32 error).  Every forward
and backward runs twice and gives the same bits.

Measured on MI355X (the printed max |g - g64| / E32, largest over each kind's cases, layouts and
upstream scales 0.37, 1e-8, 1e4; the bound grants 8 plus the relative term): focal 1.72 (all
four (alpha, gamma) pairs; 1.0 at gamma 0 and 1), sigmoid BCE 1.26, softmax 4.99, smooth L1 2.58;
0 where the gradient is exactly representable (gradient 0, or +-scale).  The two above 2 are
single roundings measured against a small E32, not a loss of accuracy: softmax at the one-row
case (E32 over three elements, scale 1e4; 1.9 at the other scales, at most 1.08 in every larger
case), where `(k == l ? -g : 0) + sm * g` rounds the product sm * g at |g| = 1e4 before the
cancelling add (0.6 ulp of g); smooth L1 at beta = 1/9, where `g * ((2 d) / (2 beta)) * sgn`
rounds the quotient and then the product (0.8 ulp of the result).  Forward sums: at most 1.4e-7
relative to float64.  Before the gamma == 0 guard in focal_elem (loss_common.h) the focal
gradient at (alpha, gamma) = (0.5, 0) was NaN for every |x| >= 17 (the classes round_to_one,
tail, exp_overflow and huge): gamma * powf(q, gamma - 1) = 0 * inf at q == 0."""
import pytest
import torch

import loss_cases as lc

pytestmark = pytest.mark.gpu

RTOL = 2e-5
CLS_PARAMS = [('focal', a, g) for a, g in lc.FOCAL_PARAMS] + [('bce', 0.25, 2.0), ('softmax', 0.25, 2.0)]
COUNTS = [(k, n, c) for k in ('focal', 'bce') for n, c in lc.SIGMOID_COUNTS] + \
         [('softmax', n, c) for n, c in lc.SOFTMAX_COUNTS]
L1_CASES = [(b, rd, v) for b in lc.L1_BETAS for rd in (0, 1) for v in lc.L1_VARIANTS
            if not (v == 'class_select' and rd == 1)]


def _scalar(v, dev, dtype=torch.float32):
    return torch.tensor([v], dtype=dtype, device=dev)


def _close_to_f64(got, want64, what):
    """finite and within rtol 2e-5 of the float64 value"""
    got = float(got)
    print(what, 'loss', got, 'f64', want64, 'rel err', abs(got - want64) / abs(want64) if want64 else abs(got))
    assert got == got and abs(got) != float('inf'), (what, got)
    assert abs(got - want64) <= RTOL * abs(want64), (what, got, want64)


def _check_grad(what, g, ref):
    """|g - g64| <= 8 E32 + 2^-22 |g64| for every element; prints max |g - g64| / E32."""
    g64, _, e32 = ref
    g = g.detach().cpu().double()
    assert g.shape == g64.shape and bool(torch.isfinite(g).all()), (what, 'non-finite gradient',
                                                                    int((~torch.isfinite(g)).sum()))
    err = (g - g64).abs()
    worst = float(err.max())
    print(what, 'max |g - g64|', worst, 'E32', e32, 'ratio', worst / e32 if e32 else (0.0 if worst == 0.0 else 'inf'))
    over = err - (8.0 * e32 + 2.0 ** -22 * g64.abs())
    at = int(over.argmax())
    assert float(over.max()) <= 0.0, (what, 'element', at, 'got', float(g.view(-1)[at]), 'f64', float(g64.view(-1)[at]),
                                      'E32', e32)


def _cls_on_dev(case, layout, dev):
    """(buffer leaf, [n, C] view, labels) of a classification case on the device"""
    c = case['x'].shape[1]
    buf = lc.place(case['x'], layout).to(dev).requires_grad_(True)
    return buf, lc.view_of(buf, c, layout), case['lab'].to(dev)


def _cls_loss(case, view, lab):
    from frcnn_amd import ops
    return ops.cls_loss(view, lab, lc.KIND_ID[case['kind']], case['alpha'], case['gamma'])


def _forward_cls(case, dev, what):
    for layout in lc.LAYOUTS:
        _, view, lab = _cls_on_dev(case, layout, dev)
        with torch.no_grad():
            a, b = _cls_loss(case, view, lab), _cls_loss(case, view, lab)
        _close_to_f64(a, case['loss64'], '{} {}'.format(what, layout))
        assert torch.equal(a, b), (what, layout, 'two launches differ')


def _backward_cls(case, dev, what):
    c = case['x'].shape[1]
    for layout in lc.LAYOUTS:
        buf, view, lab = _cls_on_dev(case, layout, dev)
        loss = _cls_loss(case, view, lab)
        for s in lc.SCALES:
            up = torch.tensor(s, dtype=torch.float32, device=dev)
            ga, = torch.autograd.grad(loss, buf, up, retain_graph=True)
            gb, = torch.autograd.grad(loss, buf, up, retain_graph=True)
            _check_grad('{} {} scale {}'.format(what, layout, s), lc.view_of(ga, c, layout), case['grads'][s])
            assert torch.equal(ga, gb), (what, layout, s, 'two launches differ')


# ---------------------------------------------------------------- forward / backward vs float64
@pytest.mark.parametrize('mag', list(lc.MAGNITUDES))
@pytest.mark.parametrize('kind,alpha,gamma', CLS_PARAMS)
def test_forward_magnitudes_vs_reference_f64(dev, kind, alpha, gamma, mag):
    _forward_cls(lc.magnitude_case(kind, mag, alpha, gamma), dev, '{} a{} g{} {}'.format(kind, alpha, gamma, mag))


@pytest.mark.parametrize('kind,n,c', COUNTS)
def test_forward_counts_vs_reference_f64(dev, kind, n, c):
    _forward_cls(lc.count_case(kind, n, c), dev, '{} n{} c{}'.format(kind, n, c))


@pytest.mark.parametrize('mag', list(lc.MAGNITUDES))
@pytest.mark.parametrize('kind,alpha,gamma', CLS_PARAMS)
def test_backward_magnitudes_vs_reference_f64(dev, kind, alpha, gamma, mag):
    _backward_cls(lc.magnitude_case(kind, mag, alpha, gamma), dev, '{} a{} g{} {}'.format(kind, alpha, gamma, mag))


@pytest.mark.parametrize('kind,n,c', COUNTS)
def test_backward_counts_vs_reference_f64(dev, kind, n, c):
    _backward_cls(lc.count_case(kind, n, c), dev, '{} n{} c{}'.format(kind, n, c))


def _l1_loss(case, x, y, lab):
    from frcnn_amd import ops
    if case['classes']:
        return ops.smooth_l1_class_select(x, case['classes'], y, lab, case['beta'])
    return ops.smooth_l1_loss(x, y, case['beta'], lab, case['rows_dim'])


@pytest.mark.parametrize('beta,rows_dim,variant', L1_CASES)
def test_smooth_l1_vs_reference_f64(dev, beta, rows_dim, variant):
    case = lc.l1_case(beta, rows_dim, variant)
    what = 'smooth_l1 beta {:.3f} rows_dim {} {}'.format(beta, rows_dim, variant)
    x = case['x'].to(dev).requires_grad_(True)
    y, lab = case['y'].to(dev), case['lab'].to(dev)
    loss = _l1_loss(case, x, y, lab)
    _close_to_f64(loss, case['loss64'], what)
    assert torch.equal(loss, _l1_loss(case, x, y, lab)), (what, 'two launches differ')
    for s in lc.SCALES:
        up = torch.tensor(s, dtype=torch.float32, device=dev)
        ga, = torch.autograd.grad(loss, x, up, retain_graph=True)
        gb, = torch.autograd.grad(loss, x, up, retain_graph=True)
        _check_grad('{} scale {}'.format(what, s), ga, case['grads'][s])
        assert torch.equal(ga, gb), (what, s, 'two launches differ')
        assert not bool(ga.cpu()[~lc.l1_selected_mask(case)].any())


# ---------------------------------------------------------------- raw entries
def _raw_cls_args(case, view, lab):
    from frcnn_amd import _lib
    n, c = view.shape
    return (lc.KIND_ID[case['kind']], _lib.ptr(view), n, c, view.stride(0), view.stride(1), _lib.ptr(lab), 0,
            case['alpha'], case['gamma'])


def _raw_cls_fwd(case, view, lab, ws, status):
    from frcnn_amd import _lib
    out = torch.full((1,), 7.0, device=view.device)
    _lib.call('frh_cls_loss_fwd', *_raw_cls_args(case, view, lab), _lib.ptr(status), _lib.ptr(out), _lib.ptr(ws),
              ws.numel(), _lib.stream_of(view))
    return out


def _raw_l1_args(case, x, y, lab):
    """frh_smooth_l1_*'s leading arguments, through the product's own stride helpers"""
    from frcnn_amd import _lib, ops
    if case['classes']:
        x, y, lab, xs, ys, n, m, n_sel = ops._l1_class_select_args(x, case['classes'], y, lab)
    else:
        x, y, lab, xs, ys, n, m, n_sel = ops._l1_args(x, y, lab, case['rows_dim'])
    return (_lib.ptr(x), xs[0], xs[1], xs[2], _lib.ptr(y), ys[0], ys[1], _lib.ptr(lab), n, m, n_sel, case['beta']), xs


def _raw_l1_fwd(case, x, y, lab, ws, status):
    from frcnn_amd import _lib
    out = torch.full((1,), 7.0, device=x.device)
    _lib.call('frh_smooth_l1_fwd', *_raw_l1_args(case, x, y, lab)[0], _lib.ptr(status), _lib.ptr(out), _lib.ptr(ws),
              ws.numel(), _lib.stream_of(x))
    return out


def _raw_det_fwd(case, view, lab, reg, rx, ry, rlab, wc, dc, wr, dr, dcount, ws, status):
    from frcnn_amd import _lib
    out = torch.full((2,), 7.0, device=view.device)
    _lib.call('frh_det_loss_fwd', *_raw_cls_args(case, view, lab), wc, dc, *_raw_l1_args(reg, rx, ry, rlab)[0], wr, dr,
              _lib.ptr(dcount), _lib.ptr(status), _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_of(view))
    return out


def _fresh(dev):
    """(zeroed workspace, zero status word) of the test's own"""
    from frcnn_amd import _lib
    return (torch.zeros(int(_lib.query('frh_loss_workspace')), dtype=torch.uint8, device=dev),
            torch.zeros(1, dtype=torch.int32, device=dev))


@pytest.mark.parametrize('layout', ['row_slice', 'col_stride'])
@pytest.mark.parametrize('n,c', [(257, 1), (65537, 1), (16385, 4)])
@pytest.mark.parametrize('kind', lc.KINDS)
def test_cls_bwd_writes_every_element_and_nothing_else(dev, kind, n, c, layout):
    """_ClsLoss.backward hands the kernel torch.empty_like: on a NaN-filled gradient buffer wider
    than the view, no NaN is left inside the view, the ignored rows are exactly 0 and every
    element outside the view is still NaN."""
    from frcnn_amd import _lib
    case = lc.written_case(kind, n, c)
    _, view, lab = _cls_on_dev(case, layout, dev)
    view = view.detach()
    gbuf = torch.full(lc.buffer_shape(n, c, layout), float('nan'), device=dev)
    gview = lc.view_of(gbuf, c, layout)
    up = _scalar(0.37, dev)
    _lib.call('frh_cls_loss_bwd', *_raw_cls_args(case, view, lab), _lib.ptr(up), _lib.ptr(gbuf), gview.stride(0),
              gview.stride(1), _lib.stream_of(view))
    inside = torch.zeros(gbuf.shape, dtype=torch.bool, device=dev)
    lc.view_of(inside, c, layout).fill_(True)
    assert not bool(torch.isnan(gview).any())
    assert bool(torch.isnan(gbuf[~inside]).all()) and int((~inside).sum()) == gbuf.numel() - n * c
    assert bool((lab < 0).any()) and not bool(gview[lab < 0].any())
    if c > 1 or kind != 'softmax':  # softmax over one channel has gradient 0 everywhere
        assert bool(gview[lab >= 0].any())
    again = torch.full_like(gbuf, float('nan'))
    _lib.call('frh_cls_loss_bwd', *_raw_cls_args(case, view, lab), _lib.ptr(up), _lib.ptr(again), gview.stride(0),
              gview.stride(1), _lib.stream_of(view))
    assert torch.equal(lc.view_of(again, c, layout), gview)


def test_smooth_l1_bwd_writes_the_selected_elements_only(dev):
    """The converse contract: on a zero-filled buffer only the selected class's four elements of
    the positive rows become nonzero.  A row labelled n_sel makes the forward NaN and is left
    alone by the backward (a marker written into its row survives)."""
    from frcnn_amd import _lib
    case = lc.l1_bad_label_case()
    x, y, lab = case['x'].to(dev), case['y'].to(dev), case['lab'].to(dev)
    ws, status = _fresh(dev)
    assert bool(torch.isnan(_raw_l1_fwd(case, x, y, lab, ws, status)).all())
    assert not bool(ws[:256].any())
    args, xs = _raw_l1_args(case, x, y, lab)
    gx = torch.zeros_like(x)
    gx[3] = 5.0
    up = _scalar(0.37, dev)
    _lib.call('frh_smooth_l1_bwd', *args, _lib.ptr(up), _lib.ptr(gx), xs[0], xs[1], xs[2], _lib.stream_of(x))
    g = gx.cpu()
    assert bool((g[3] == 5.0).all())
    g[3] = 0.0
    mask = lc.l1_selected_mask(case)
    assert bool((g[mask] != 0).all()) and not bool(g[~mask].any())
    _check_grad('smooth_l1 bad label', g, case['grads'][0.37])


DET_CASES = {
    'cls_256_reg_1': (('bce', 65537, 1), 1),       # nbc = 256 (capped), nbr = 1
    'cls_1_reg_256': (('bce', 1, 1), 20000),       # nbc = 1, nbr = 256 (capped: 80 000 elements)
    'focal_c4_reg_1': (('focal', 16385, 4), 3),
    'softmax_256_reg_1': (('softmax', 65537, 3), 1),  # softmax rows at the capped stride nbc = 256
}


def _det_inputs(name, dev):
    cls_key, rn = DET_CASES[name]
    case, reg = lc.count_case(*cls_key), lc.l1_rows_case(rn)
    _, view, lab = _cls_on_dev(case, 'rows', dev)
    return case, view.detach(), lab, reg, reg['x'].to(dev), reg['y'].to(dev), reg['lab'].to(dev)


@pytest.mark.parametrize('name', list(DET_CASES))
def test_det_loss_unequal_halves(dev, name):
    """frh_det_loss_fwd with one half at the grid cap and the other in one workgroup: both outputs
    have the bits of the separate entries' sums scaled (sum * w) / div in f32, are within rtol
    2e-5 of float64, and a device count of 0 gives exact zeros."""
    case, view, lab, reg, rx, ry, rlab = _det_inputs(name, dev)
    wc, wr, div = 0.7, 1.3, 517.0
    ws, status = _fresh(dev)
    sep_c = _raw_cls_fwd(case, view, lab, ws, status).cpu()
    sep_r = _raw_l1_fwd(reg, rx, ry, rlab, ws, status).cpu()
    out = _raw_det_fwd(case, view, lab, reg, rx, ry, rlab, wc, div, wr, div, None, ws, status)
    assert torch.equal(out, _raw_det_fwd(case, view, lab, reg, rx, ry, rlab, wc, div, wr, div, None, ws, status))
    assert not bool(ws[:256].any())
    f32 = lambda v: torch.tensor([v], dtype=torch.float32)  # noqa: E731
    want = torch.cat([(sep_c * f32(wc)) / f32(div), (sep_r * f32(wr)) / f32(div)])
    assert torch.equal(out.cpu(), want), (out.tolist(), want.tolist())
    _close_to_f64(out[0], case['loss64'] * float(f32(wc)) / div, name + ' cls')
    _close_to_f64(out[1], reg['loss64'] * float(f32(wr)) / div, name + ' reg')
    count = _scalar(517, dev, torch.int32)
    by_count = _raw_det_fwd(case, view, lab, reg, rx, ry, rlab, wc, 1.0, wr, 1.0, count, ws, status)
    assert torch.equal(by_count, out)
    zero = _raw_det_fwd(case, view, lab, reg, rx, ry, rlab, wc, 1.0, wr, 1.0, count.zero_(), ws, status)
    assert zero.tolist() == [0.0, 0.0] and not bool(torch.signbit(zero).any())
    assert not bool(ws[:256].any())


def test_workspace_counter_is_zero_after_every_call_and_status_gives_nan(dev):
    """One workspace, one stream: a 256-workgroup focal, a 1-workgroup BCE, a det loss (256, 1), a
    1-workgroup smooth L1 and a 256-workgroup softmax in a row.  Each gives the bits of the same
    call made first on a freshly zeroed workspace and leaves the first 256 bytes zero.  With the
    status word set, the cls, smooth-L1 and det forwards give NaN and still reset the counter:
    after clearing the word the next calls have the fresh bits again."""
    focal = lc.count_case('focal', 16385, 4)
    bce = lc.count_case('bce', 255, 1)
    softmax = lc.count_case('softmax', 65537, 3)
    small = lc.l1_rows_case(3)
    on = {id(c): _cls_on_dev(c, 'rows', dev)[1:] for c in (focal, bce, softmax)}
    sx, sy, slab = small['x'].to(dev), small['y'].to(dev), small['lab'].to(dev)
    det = _det_inputs('cls_256_reg_1', dev)
    calls = [
        lambda ws, st: _raw_cls_fwd(focal, on[id(focal)][0].detach(), on[id(focal)][1], ws, st),
        lambda ws, st: _raw_cls_fwd(bce, on[id(bce)][0].detach(), on[id(bce)][1], ws, st),
        lambda ws, st: _raw_det_fwd(*det, 0.7, 517.0, 1.3, 517.0, None, ws, st),
        lambda ws, st: _raw_l1_fwd(small, sx, sy, slab, ws, st),
        lambda ws, st: _raw_cls_fwd(softmax, on[id(softmax)][0].detach(), on[id(softmax)][1], ws, st),
    ]
    fresh = [call(*_fresh(dev)) for call in calls]
    assert all(bool(torch.isfinite(f).all()) for f in fresh)
    ws, status = _fresh(dev)
    for rounds in range(2):
        for call, want in zip(calls, fresh):
            assert torch.equal(call(ws, status), want)
            assert not bool(ws[:256].any())
    for i in (0, 3, 2):  # cls, smooth L1, det
        status.fill_(8)  # no one-launch kernel's bit: only the loss's NaN is under test
        assert bool(torch.isnan(calls[i](ws, status)).all())
        assert not bool(ws[:256].any())
        status.zero_()
        for j in (i, 4):
            assert torch.equal(calls[j](ws, status), fresh[j])
            assert not bool(ws[:256].any())
