"""The fused GFL head loss (ops.gfl_losses: frh_gfl_loss_fwd / _bwd) and the DFL box decode
(ops.dfl_decode: frh_dfl_decode), csrc/gfl.hip, against the REFERENCE's own f64 outputs
(tests/golden/gfl_loss.npz / gfl_decode.npz, made by gen_gfl_golden.py from
lib/heads/fcos_head.py:419-515 and :579-600) and, where there is no fixture, against the torch
restatement losses.gfl_head_losses_torch in f64 on the CPU (pinned to the reference in
tests/test_gfl_cpu.py).

Bars: fused sums rtol 2e-5 / atol 1e-6 and gradients rtol 1e-4 / atol 1e-6, as
tests/test_gpu_losses.py; each loss is back-propagated on its own with the upstream gradient
num_pos, so the gradients are O(1).  The decode's largest error against the reference's f64 boxes
may be at most 4 E, E the largest |reference f32 - reference f64| of the fixture: kernel and
reference are two independent f32 evaluations, each good to about E, doubled for another expf."""
import numpy as np
import pytest
import torch

import gfl_inputs
import support

pytestmark = pytest.mark.gpu
TAGS = sorted(gfl_inputs.LOSS_CASES)
LOSS_TOL = dict(rtol=2e-5, atol=1e-6)
GRAD_TOL = dict(rtol=1e-4, atol=1e-6)


def _dev_case(c, dev, grad=False):
    cls = torch.from_numpy(c['cls']).to(dev).requires_grad_(grad)
    reg = torch.from_numpy(c['reg']).to(dev).requires_grad_(grad)
    return cls, reg, torch.from_numpy(c['labels']).to(dev), torch.from_numpy(c['ltrb']).to(dev)


def _grads(out, cls, reg, scale):
    """(d cls_loss / d cls, d dfl_loss / d reg, d bbox_loss / d reg), each loss on its own with the
    upstream gradient `scale`; the three other pairs must be exactly zero."""
    res = []
    up = torch.tensor(float(scale), device=cls.device)
    for i, wrt in ((0, 0), (1, 1), (2, 1)):
        g = torch.autograd.grad(out[i], [cls, reg], grad_outputs=up, retain_graph=True)
        assert not g[1 - wrt].any()
        res.append(g[wrt])
    return res


def _cpu_reference(c):
    """The restatement in f64 on the CPU: losses, num_pos and the three gradients scaled by num_pos."""
    from frcnn_amd.losses import gfl_head_losses_torch
    cls = torch.from_numpy(c['cls']).double().requires_grad_(True)
    reg = torch.from_numpy(c['reg']).double().requires_grad_(True)
    out = gfl_head_losses_torch(cls, reg, torch.from_numpy(c['labels']), torch.from_numpy(c['ltrb']).double(),
                                **gfl_inputs.loss_kwargs(c))
    n = max(int(out[3]), 1)
    grads = []
    for i, wrt in ((0, 0), (1, 1), (2, 1)):
        leaf = (cls, reg)[wrt]
        g = torch.autograd.grad(out[i], leaf, retain_graph=True, allow_unused=True)[0]
        grads.append((torch.zeros_like(leaf) if g is None else g).numpy() * n)
    return support.loss_values(out), int(out[3]), grads


@pytest.mark.parametrize('tag', TAGS)
def test_forward_vs_reference_f64(dev, golden, tag):
    from frcnn_amd import ops
    z = golden('gfl_loss.npz')
    c = gfl_inputs.loss_case(tag)
    out = ops.gfl_losses(*_dev_case(c, dev), **gfl_inputs.loss_kwargs(c))
    assert all(o.dim() == 0 and o.is_cuda for o in out)
    print(tag, support.loss_values(out), z[tag + '_f64'])
    assert int(out[3]) == int(z[tag + '_num_pos'])
    np.testing.assert_allclose(support.loss_values(out), z[tag + '_f64'], **LOSS_TOL)


@pytest.mark.parametrize('tag', TAGS)
def test_backward_vs_reference_f64(dev, golden, tag):
    from frcnn_amd import ops
    z = golden('gfl_loss.npz')
    c = gfl_inputs.loss_case(tag)
    cls, reg, labels, ltrb = _dev_case(c, dev, grad=True)
    out = ops.gfl_losses(cls, reg, labels, ltrb, **gfl_inputs.loss_kwargs(c))
    n = int(z[tag + '_num_pos'])
    got = _grads(out, cls, reg, n)
    for g, key in zip(got, ('gcls_cls', 'greg_dfl', 'greg_bbox')):
        ref = z['{}_{}'.format(tag, key)] * n
        print(tag, key, 'largest |grad|', float(np.abs(ref).max()), 'largest error', float(np.abs(g.cpu().numpy() - ref).max()))
        np.testing.assert_allclose(g.cpu().numpy(), ref, err_msg=key, **GRAD_TOL)
    assert not got[0][:, labels < 0].any()       # ignored positions: class gradients exactly 0
    assert not got[1][:, labels <= 0].any() and not got[2][:, labels <= 0].any()  # non-positives: regression 0


def test_strided_views_are_bit_identical(dev):
    """The logits as transposed views, as views of a channels-last map and as every second column
    of a wider buffer: the same losses and gradients, bit for bit, as the contiguous tensors."""
    from frcnn_amd import ops
    c = gfl_inputs.loss_case('first_last')  # one image, one level (17, 19)
    kw = gfl_inputs.loss_kwargs(c)
    cls, reg, labels, ltrb = _dev_case(c, dev)
    h, w = c['grids'][0]

    def transposed(t):
        return t.t().contiguous().t()

    def channels_last(t):
        x = t.reshape(1, t.shape[0], h, w).contiguous(memory_format=torch.channels_last)
        return x[0].reshape(t.shape[0], -1)

    def every_second(t):
        big = torch.full((t.shape[0], 2 * t.shape[1]), float('nan'), device=dev)
        big[:, ::2] = t
        return big[:, ::2]

    def run(f):
        a, b = f(cls).detach().requires_grad_(True), f(reg).detach().requires_grad_(True)
        out = ops.gfl_losses(a, b, labels, ltrb, **kw)
        sum(out[:3]).backward()
        return [o.detach() for o in out], a.grad, b.grad, a.stride()
    base = run(lambda t: t.clone())
    for f in (transposed, channels_last, every_second):
        got = run(f)
        assert got[3] != base[3], f.__name__
        for x, y in zip(base[0], got[0]):
            assert torch.equal(x, y), f.__name__
        assert torch.equal(base[1], got[1]) and torch.equal(base[2], got[2]), f.__name__


def test_two_calls_are_bit_identical(dev):
    from frcnn_amd import ops
    c = gfl_inputs.loss_case('mixed')
    outs = []
    for _ in range(2):
        cls, reg, labels, ltrb = _dev_case(c, dev, grad=True)
        out = ops.gfl_losses(cls, reg, labels, ltrb, **gfl_inputs.loss_kwargs(c))
        sum(out[:3]).backward()
        outs.append([o.detach() for o in out] + [cls.grad, reg.grad])
    for x, y in zip(*outs):
        assert torch.equal(x, y)


@pytest.fixture(scope='module')
def large_case():
    """One level of (200, 336), one image: 67 200 positions, more than one pass of the forward's
    256-workgroup grid (65 536); about 1 % positives, 5 % ignored.  With its f64 CPU reference."""
    rng = np.random.default_rng(7300)
    m, C, bins = 200 * 336, 20, 16
    labels = np.zeros(m, np.int64)
    u = rng.random(m)
    labels[u < 0.05] = -1
    pos = u > 0.99
    labels[pos] = rng.integers(1, C + 1, int(pos.sum()))
    c = dict(gfl_inputs.LOSS_CASES['mixed'], labels=labels, M=m, reg_std=gfl_inputs.REG_STD,
             reg_mean=gfl_inputs.REG_MEAN, cls=rng.standard_normal((C, m)).astype(np.float32),
             reg=rng.standard_normal((4 * bins, m)).astype(np.float32),
             ltrb=rng.uniform(0.5, 1400.0, (m, 4)).astype(np.float32))
    return c, _cpu_reference(c)


def test_large_forward_and_backward_vs_restatement_f64(dev, large_case):
    from frcnn_amd import ops
    c, (ref_losses, ref_n, ref_grads) = large_case
    assert c['M'] > 256 * 256 and 400 < ref_n < 1000
    cls, reg, labels, ltrb = _dev_case(c, dev, grad=True)
    out = ops.gfl_losses(cls, reg, labels, ltrb, **gfl_inputs.loss_kwargs(c))
    print(support.loss_values(out), ref_losses, int(out[3]), ref_n)
    assert int(out[3]) == ref_n
    np.testing.assert_allclose(support.loss_values(out), ref_losses, **LOSS_TOL)
    for g, ref, key in zip(_grads(out, cls, reg, ref_n), ref_grads, ('cls', 'dfl', 'bbox')):
        np.testing.assert_allclose(g.cpu().numpy(), ref, err_msg=key, **GRAD_TOL)


def test_zero_positives(dev):
    from frcnn_amd import ops
    c = gfl_inputs.loss_case('mixed')
    c['labels'] = np.where(c['labels'] > 0, 0, c['labels'])
    ref_losses, ref_n, ref_grads = _cpu_reference(c)
    assert ref_n == 0
    cls, reg, labels, ltrb = _dev_case(c, dev, grad=True)
    out = ops.gfl_losses(cls, reg, labels, ltrb, **gfl_inputs.loss_kwargs(c))
    got = support.loss_values(out)
    assert int(out[3]) == 0 and np.isfinite(got).all() and got[1] == 0.0 and got[2] == 0.0
    np.testing.assert_allclose(got[0], ref_losses[0], **LOSS_TOL)  # divided by max(num_pos, 1)
    g = _grads(out, cls, reg, 1.0)
    np.testing.assert_allclose(g[0].cpu().numpy(), ref_grads[0], **GRAD_TOL)
    assert not g[1].any() and not g[2].any()


def test_top_bin_target(dev):
    """One positive whose first and third sides sit exactly on (bins-1)*stride (left == bins-1:
    the reference raises there, include/frcnn_amd.h): finite, and equal to the restatement.  The
    regression tensor has exactly 4*bins rows; a plain run on legal memory."""
    from frcnn_amd import ops
    bins, stride = 16, 0.08
    rng = np.random.default_rng(7400)
    m = 70
    top = np.float32((bins - 1) * stride)
    c = dict(gfl_inputs.LOSS_CASES['mixed'], M=m, reg_std=1.0, reg_mean=0.0,
             labels=np.zeros(m, np.int64), cls=rng.standard_normal((20, m)).astype(np.float32),
             reg=rng.standard_normal((4 * bins, m)).astype(np.float32),
             ltrb=np.full((m, 4), 0.3, np.float32))
    c['labels'][[3, 66]] = (5, 9)
    c['ltrb'][66] = (top, 0.04, top, 0.26)
    ref_losses, ref_n, ref_grads = _cpu_reference(c)
    assert ref_n == 2 and np.isfinite(ref_losses).all()
    cls, reg, labels, ltrb = _dev_case(c, dev, grad=True)
    assert reg.shape[0] == 4 * bins and reg.is_contiguous()
    out = ops.gfl_losses(cls, reg, labels, ltrb, **gfl_inputs.loss_kwargs(c))
    assert int(out[3]) == 2 and np.isfinite(support.loss_values(out)).all()
    np.testing.assert_allclose(support.loss_values(out), ref_losses, **LOSS_TOL)
    for g, ref, key in zip(_grads(out, cls, reg, ref_n), ref_grads, ('cls', 'dfl', 'bbox')):
        assert torch.isfinite(g).all(), key
        np.testing.assert_allclose(g.cpu().numpy(), ref, err_msg=key, **GRAD_TOL)


def test_more_than_16_bins_is_refused(dev):
    from frcnn_amd import ops
    m = 8
    with pytest.raises(RuntimeError, match='exceeds one wave'):
        ops.gfl_losses(torch.zeros(20, m, device=dev), torch.zeros(4 * 17, m, device=dev),
                       torch.zeros(m, dtype=torch.int64, device=dev), torch.ones(m, 4, device=dev), 17, 0.08)


def test_status_word_gives_nan_losses(dev):
    from frcnn_amd import ops
    c = gfl_inputs.loss_case('mixed')
    args = _dev_case(c, dev)
    word = ops.status_word(dev)
    assert int(word.item()) == 0
    try:
        word.fill_(4)
        out = ops.gfl_losses(*args, **gfl_inputs.loss_kwargs(c))
        assert np.isnan(support.loss_values(out)).all()
    finally:
        word.zero_()
    out = ops.gfl_losses(*args, **gfl_inputs.loss_kwargs(c))
    assert np.isfinite(support.loss_values(out)).all()
    ops.check_device_status(dev)


@pytest.mark.parametrize('layout', ['nchw', 'channels_last'])
def test_decode_vs_reference_f64(dev, golden, layout):
    from frcnn_amd import ops
    z = golden('gfl_decode.npz')
    n = len(gfl_inputs.DECODE_LEVELS)
    E = max(float(np.abs(z['boxes_f32_{}'.format(i)].astype(np.float64) - z['boxes_f64_{}'.format(i)]).max())
            for i in range(n))
    err, inside = 0.0, 0
    for i, (cell, reg) in enumerate(gfl_inputs.decode_case()):
        r = torch.from_numpy(reg).to(dev)
        if layout == 'channels_last':
            r = r.contiguous(memory_format=torch.channels_last)
            assert r.stride(1) == 1
        got = ops.dfl_decode(r, gfl_inputs.DECODE_BINS, gfl_inputs.DECODE_STRIDE, gfl_inputs.REG_STD,
                             gfl_inputs.REG_MEAN, cell, gfl_inputs.DECODE_IMG)
        ref = z['boxes_f64_{}'.format(i)]
        assert tuple(got.shape) == ref.shape
        err = max(err, float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max()))
        hi = np.array([gfl_inputs.DECODE_IMG[1] - 1, gfl_inputs.DECODE_IMG[0] - 1] * 2).reshape(1, 4, 1)
        inside += int(((ref > 0) & (ref < hi)).sum())
    print('decode {}: largest |kernel - reference f64| = {:.3e} px, E = largest |reference f32 - reference f64| '
          '= {:.3e} px'.format(layout, err, E))
    assert inside > 200  # coordinates the clamp does not decide
    assert E > 0 and err <= 4 * E, (err, E)


def test_no_host_sync(dev):
    """ops.gfl_losses (forward and backward) and the fused FCOSHead.calc_loss_flat read nothing
    back to the host; the mode itself is checked to catch the read the old path made."""
    from frcnn_amd import ops
    from frcnn_amd.heads.fcos_head import FCOSHead
    c = gfl_inputs.loss_case('mixed')
    kw, w = gfl_inputs.loss_kwargs(c), gfl_inputs.WEIGHTS
    cls, reg, labels, ltrb = _dev_case(c, dev, grad=True)
    ops.gfl_losses(cls, reg, labels, ltrb, **kw)  # workspace and status word exist from here on
    with pytest.raises(RuntimeError):
        support.no_sync(lambda: int((labels > 0).sum()))

    def fused():
        out = ops.gfl_losses(cls, reg, labels, ltrb, **kw)
        sum(out[:3]).backward()
        return out
    out = support.no_sync(fused)
    head = FCOSHead(num_classes=21, in_channels=8, stacked_convs=1, feat_channels=8, reg_std=c['reg_std'],
                    reg_mean=c['reg_mean'], atss_cfg=dict(topk=9, scale=8),
                    loss_cls=dict(type='QualityFocalLoss', use_sigmoid=True, loss_weight=w['cls_weight']),
                    loss_bbox=dict(type='GIoULoss', loss_weight=w['bbox_weight']),
                    loss_dfl=dict(type='DistributionFocalLoss', cls_channels=16, stride=0.08, norm_prob=False,
                                  loss_weight=w['dfl_weight']))
    m = c['M']
    zeros1, zeros = torch.zeros(1, m, device=dev), torch.zeros(m, device=dev)
    res = support.no_sync(lambda: head.calc_loss_flat(cls, reg, zeros1, labels, ltrb, zeros))
    assert list(res) == ['cls_loss', 'dfl_loss', 'bbox_loss']
    for v, r in zip(res.values(), out[:3]):
        assert torch.equal(v.detach(), r.detach())
