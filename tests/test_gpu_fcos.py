"""Plain FCOS on the HIP path (csrc/fcos.hip): the one-launch scale-range target assignment
(ops.fcos_assign: frh_fcos_assign) and the fused focal / GIoU / centerness head loss
(ops.fcos_losses: frh_fcos_loss_fwd / _bwd), against the REFERENCE's own outputs
(tests/golden/fcos_targets.npz / fcos_loss.npz, made by gen_fcos_golden.py from
lib/heads/fcos_head.py:371-416 and :419-515) and, where the reference cannot run (one position,
no positive) or does not define the answer (equal areas), against the torch restatement
losses.fcos_head_losses_torch in f64 and the numpy restatement below (both pinned to the
reference in tests/test_fcos_cpu.py).

Bars: the targets are bit-exact (the kernel performs the reference's f32 operations in its
order); fused loss sums rtol 2e-5 / atol 1e-6 and gradients rtol 1e-4 / atol 1e-6, as
tests/test_gpu_losses.py; each loss is back-propagated on its own with the upstream gradient
num_pos, so the gradients are O(1).  Disjoint boxes are not tested: the predicted and the target
box both contain the origin ((-l, -t, r, b) with positive distances), so they always intersect."""
import numpy as np
import pytest
import torch

import fcos_inputs
import support

pytestmark = pytest.mark.gpu
TAGS = sorted(fcos_inputs.LOSS_CASES)
REF_TAGS = list(fcos_inputs.REFERENCE_LOSS_CASES)
LOSS_TOL = dict(rtol=2e-5, atol=1e-6)
GRAD_TOL = dict(rtol=1e-4, atol=1e-6)
KEYS = ('gcls', 'greg', 'gctr')


# ----------------------------------------------------------------- targets
def numpy_targets(boxes, labels, img_shape, thr, grids=fcos_inputs.GRIDS, strides=fcos_inputs.STRIDES):
    """FCOSHead.single_image_targets restated in numpy f32 as a per-cell arg-min: the matching gt
    of smallest area owns the cell, the later of equal areas (what painting in descending-area
    order behind a stable sort leaves).  (cls [N] i64, reg [N, 4] f32, ctr [N] f32), levels
    concatenated."""
    f = np.float32
    boxes = boxes.astype(f)
    area = (boxes[2] - boxes[0] + f(1)) * (boxes[3] - boxes[1] + f(1))
    out = []
    for lv, ((h, w), s) in enumerate(zip(grids, strides)):
        sc = f(1.0 / s)
        y2, x2 = int(np.rint(f(img_shape[0]) * sc)), int(np.rint(f(img_shape[1]) * sc))  # half to even
        ys, xs = np.mgrid[0:h, 0:w]
        inside = (ys <= y2) & (xs <= x2)
        cls = np.where(inside, 0, -1).astype(np.int64)
        ctr = np.where(inside, 0, -1).astype(f)
        reg = np.full((h, w, 4), -1, f)
        cx, cy = xs.astype(f) * f(s) + f(s / 2.0), ys.astype(f) * f(s) + f(s / 2.0)
        best = np.full((h, w), np.inf, f)
        for g in range(boxes.shape[1]):
            b = boxes[:, g]
            lt = np.stack([cx - b[0], cy - b[1], b[2] - cx, b[3] - cy], -1)
            mx = lt.max(-1)
            m = (lt > 0).all(-1) & (mx >= f(thr[lv])) & (mx < f(thr[lv + 1])) & (area[g] <= best)
            cls[m], reg[m], best[m] = labels[g], lt[m], area[g]
        v = reg + f(1e-6)
        c = np.sqrt((np.minimum(v[..., 0], v[..., 2]) / np.maximum(v[..., 0], v[..., 2])) *
                    (np.minimum(v[..., 1], v[..., 3]) / np.maximum(v[..., 1], v[..., 3])))
        ctr[cls > 0] = c[cls > 0]
        out.append((cls.reshape(-1), reg.reshape(-1, 4), ctr.reshape(-1)))
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


def _assign(tag, dev):
    from frcnn_amd import ops
    boxes, labels, thr = fcos_inputs.TARGET_CASES[tag]
    return ops.fcos_assign(fcos_inputs.GRIDS, [float(s) for s in fcos_inputs.STRIDES],
                           [torch.from_numpy(b).to(dev) for b in boxes], [torch.from_numpy(l).to(dev) for l in labels],
                           [s[:2] for s in fcos_inputs.IMG_SHAPES], thr)


@pytest.mark.parametrize('tag', fcos_inputs.REFERENCE_TARGET_CASES)
def test_assign_vs_reference(dev, golden, tag):
    z = golden('fcos_targets.npz')
    cls, reg, ctr = _assign(tag, dev)
    n = fcos_inputs.NUM_CELLS
    assert cls.shape == (2, n) and reg.shape == (2, n, 4) and ctr.shape == (2, n)
    assert cls.dtype == torch.int64 and reg.dtype == torch.float32 and ctr.dtype == torch.float32
    for b in range(2):
        np.testing.assert_array_equal(cls[b].cpu().numpy(), z['{}_cls_{}'.format(tag, b)])
        np.testing.assert_array_equal(reg[b].cpu().numpy(), z['{}_reg_{}'.format(tag, b)])
        np.testing.assert_array_equal(ctr[b].cpu().numpy(), z['{}_ctr_{}'.format(tag, b)])


def test_assign_equal_areas_vs_numpy(dev):
    """Two gts of one area: the larger index owns the overlap, in either order of the pair."""
    boxes, labels, thr = fcos_inputs.TARGET_CASES['tie']
    cls, reg, ctr = _assign('tie', dev)
    owners = []
    for b, shape in enumerate(fcos_inputs.IMG_SHAPES):
        rc, rr, rt = numpy_targets(boxes[b], labels[b], shape, thr)
        np.testing.assert_array_equal(cls[b].cpu().numpy(), rc)
        np.testing.assert_array_equal(reg[b].cpu().numpy(), rr)
        np.testing.assert_array_equal(ctr[b].cpu().numpy(), rt)
        owners.append(int(rc[16 * 64 + 17]))  # level 0, centre (140, 132): inside both equal-area gts
    assert owners == [int(labels[0][1]), int(labels[1][2])] and owners[0] != owners[1]


def test_assign_many_gts_and_no_gts(dev):
    """More gts than one LDS chunk (256), and a batch without any gt (through ops, which pads the
    gt buffers to one column, and through the entry with max_gts == 0)."""
    from frcnn_amd import ops
    rng = np.random.default_rng(7600)
    g = 300
    xy = (rng.uniform(0, 1, (2, g)) * [[400], [250]]).astype(np.float32)
    wh = rng.uniform(8, 120, (2, g)).astype(np.float32)
    boxes = np.concatenate([xy, np.minimum(xy + wh, np.float32([[511], [319]]))]).astype(np.float32)
    labels = rng.integers(1, 21, g)
    strides = [float(s) for s in fcos_inputs.STRIDES]
    shapes = [s[:2] for s in fcos_inputs.IMG_SHAPES]
    cls, reg, ctr = ops.fcos_assign(fcos_inputs.GRIDS, strides, [torch.from_numpy(boxes).to(dev)] * 2,
                                    [torch.from_numpy(labels).to(dev)] * 2, shapes, fcos_inputs.REAL_THR)
    for b in range(2):
        rc, rr, rt = numpy_targets(boxes, labels, shapes[b], fcos_inputs.REAL_THR)
        assert (rc > 0).sum() > 500
        np.testing.assert_array_equal(cls[b].cpu().numpy(), rc)
        np.testing.assert_array_equal(reg[b].cpu().numpy(), rr)
        np.testing.assert_array_equal(ctr[b].cpu().numpy(), rt)
    none, nolab = [torch.zeros(4, 0, device=dev)] * 2, [torch.zeros(0, dtype=torch.int64, device=dev)] * 2
    cls, reg, ctr = ops.fcos_assign(fcos_inputs.GRIDS, strides, none, nolab, shapes, fcos_inputs.REAL_THR)
    for b in range(2):
        rc, rr, rt = numpy_targets(np.zeros((4, 0), np.float32), np.zeros(0, np.int64), shapes[b], fcos_inputs.REAL_THR)
        np.testing.assert_array_equal(cls[b].cpu().numpy(), rc)
        assert (reg[b] == -1).all() and torch.equal(ctr[b].cpu(), torch.from_numpy(rt))
    # the entry itself with max_gts == 0 and no gt buffers: the same painted background
    from frcnn_amd import _lib
    c0, r0, t0 = torch.empty_like(cls), torch.empty_like(reg), torch.empty_like(ctr)
    count = torch.zeros(2, dtype=torch.int32, device=dev)
    img_hw = torch.tensor([list(s) for s in shapes], dtype=torch.int32, device=dev)
    _lib.call('frh_fcos_assign', 2, len(strides), _lib.i32_array([v for g in fcos_inputs.GRIDS for v in g]),
              _lib.f32_array(strides), _lib.f32_array(fcos_inputs.REAL_THR), None, 0, _lib.ptr(count), None, 0,
              _lib.ptr(img_hw), _lib.ptr(c0), _lib.ptr(r0), _lib.ptr(t0), _lib.stream_of(c0))
    assert torch.equal(c0, cls) and torch.equal(r0, reg) and torch.equal(t0, ctr)


def _head(dev, thr=None, num_classes=21, reg_std=fcos_inputs.REG_STD, reg_coef_trainable=False):
    from frcnn_amd.heads.fcos_head import FCOSHead
    w = fcos_inputs.WEIGHTS
    head = FCOSHead(num_classes=num_classes, in_channels=8, stacked_convs=1, feat_channels=8,
                    strides=list(fcos_inputs.STRIDES), reg_std=reg_std, reg_mean=fcos_inputs.REG_MEAN,
                    reg_coef_trainable=reg_coef_trainable,
                    loss_cls=dict(type='FocalLoss', use_sigmoid=True, loss_weight=w['cls_weight']),
                    loss_bbox=dict(type='GIoULoss', loss_weight=w['bbox_weight']),
                    loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=w['ctr_weight']))
    if thr is not None:
        head.level_scale_thr = list(thr)
    return head.to(dev)


def test_single_image_targets_on_gpu_tensors(dev, golden):
    """The reference's signature and per-level [H, W, k] return, as views of the batched call."""
    z = golden('fcos_targets.npz')
    boxes, labels, thr = fcos_inputs.TARGET_CASES['a']
    head = _head(dev, thr)
    outs = [torch.from_numpy(x).to(dev) for x in fcos_inputs.level_outputs()]
    cls, reg, ctr = head.single_image_targets(outs, outs, outs, torch.from_numpy(boxes[0]).to(dev),
                                              torch.from_numpy(labels[0]).to(dev), fcos_inputs.img_metas()[0], None)
    assert [tuple(x.shape) for x in cls] == [g + (1,) for g in fcos_inputs.GRIDS]
    assert [tuple(x.shape) for x in reg] == [g + (4,) for g in fcos_inputs.GRIDS]
    assert [tuple(x.shape) for x in ctr] == [g + (1,) for g in fcos_inputs.GRIDS]
    assert cls[0].dtype == torch.int64 and all(x.is_cuda for x in cls + reg + ctr)
    np.testing.assert_array_equal(torch.cat([x.reshape(-1) for x in cls]).cpu().numpy(), z['a_cls_0'])
    np.testing.assert_array_equal(torch.cat([x.reshape(-1, 4) for x in reg]).cpu().numpy(), z['a_reg_0'])
    np.testing.assert_array_equal(torch.cat([x.reshape(-1) for x in ctr]).cpu().numpy(), z['a_ctr_0'])


# ----------------------------------------------------------------- losses
def _dev_case(c, dev, grad=False):
    outs = [torch.from_numpy(c[k]).to(dev).requires_grad_(grad) for k in ('cls', 'reg', 'ctr')]
    return outs + [torch.from_numpy(c[k]).to(dev) for k in ('labels', 'ltrb', 'ctr_t')]


def _grads(out, leaves, scale):
    """(d cls_loss / d cls, d bbox_loss / d reg, d ctr_loss / d ctr), each loss on its own with the
    upstream gradient `scale`; the six other pairs must be exactly zero."""
    res = []
    up = torch.tensor(float(scale), device=leaves[0].device)
    for i in range(3):
        g = torch.autograd.grad(out[i], leaves, grad_outputs=up, retain_graph=True)
        assert all(not g[j].any() for j in range(3) if j != i)
        res.append(g[i])
    return res


_CPU_REF = {}


def _cpu_reference(tag):
    """The restatement in f64 on the CPU, once per case: losses, num_pos and the three gradients
    scaled by max(num_pos, 1)."""
    if tag not in _CPU_REF:
        from frcnn_amd.losses import fcos_head_losses_torch
        c = fcos_inputs.loss_case(tag)
        outs = [torch.from_numpy(c[k]).double().requires_grad_(True) for k in ('cls', 'reg', 'ctr')]
        out = fcos_head_losses_torch(*outs, torch.from_numpy(c['labels']), torch.from_numpy(c['ltrb']).double(),
                                     torch.from_numpy(c['ctr_t']).double(), **fcos_inputs.loss_kwargs(c))
        n = max(int(out[3]), 1)
        grads = []
        for i in range(3):
            g = torch.autograd.grad(out[i], outs[i], retain_graph=True, allow_unused=True)[0]
            grads.append((torch.zeros_like(outs[i]) if g is None else g).numpy() * n)
        _CPU_REF[tag] = (support.loss_values(out), int(out[3]), grads)
    return _CPU_REF[tag]


@pytest.mark.parametrize('tag', REF_TAGS)
def test_forward_vs_reference_f64(dev, golden, tag):
    from frcnn_amd import ops
    z = golden('fcos_loss.npz')
    c = fcos_inputs.loss_case(tag)
    out = ops.fcos_losses(*_dev_case(c, dev), **fcos_inputs.loss_kwargs(c))
    assert all(o.dim() == 0 and o.is_cuda for o in out)
    print(tag, support.loss_values(out), z[tag + '_f64'])
    assert int(out[3]) == int(z[tag + '_num_pos'])
    np.testing.assert_allclose(support.loss_values(out), z[tag + '_f64'], **LOSS_TOL)


@pytest.mark.parametrize('tag', REF_TAGS)
def test_backward_vs_reference_f64(dev, golden, tag):
    from frcnn_amd import ops
    z = golden('fcos_loss.npz')
    c = fcos_inputs.loss_case(tag)
    t = _dev_case(c, dev, grad=True)
    out = ops.fcos_losses(*t, **fcos_inputs.loss_kwargs(c))
    n = int(z[tag + '_num_pos'])
    got = _grads(out, t[:3], n)
    labels = t[3]
    for g, key in zip(got, KEYS):
        ref = z['{}_{}'.format(tag, key)] * n
        print(tag, key, 'largest |grad|', float(np.abs(ref).max()), 'largest error',
              float(np.abs(g.cpu().numpy() - ref).max()))
        np.testing.assert_allclose(g.cpu().numpy(), ref, err_msg=key, **GRAD_TOL)
    assert not got[0][:, labels < 0].any()                                   # ignored: class gradients exactly 0
    assert not got[1][:, labels <= 0].any() and not got[2][labels <= 0].any()  # non-positives: box, centerness 0


@pytest.mark.parametrize('tag', ['one', 'no_pos', 'ignored'])
def test_cases_the_reference_cannot_run_vs_restatement_f64(dev, tag):
    """One position (the reference squeezes its mask to 0-d), no positive and every label -1 (it
    divides by zero): finite, out[3] the count, sums over max(num_pos, 1)."""
    from frcnn_amd import ops
    ref_losses, ref_n, ref_grads = _cpu_reference(tag)
    c = fcos_inputs.loss_case(tag)
    t = _dev_case(c, dev, grad=True)
    out = ops.fcos_losses(*t, **fcos_inputs.loss_kwargs(c))
    got = support.loss_values(out)
    print(tag, got, ref_losses, int(out[3]), ref_n)
    assert int(out[3]) == ref_n == {'one': 1, 'no_pos': 0, 'ignored': 0}[tag] and np.isfinite(got).all()
    np.testing.assert_allclose(got, ref_losses, **LOSS_TOL)
    if ref_n == 0:
        assert got[1] == 0.0 and got[2] == 0.0
    if tag == 'ignored':
        assert got[0] == 0.0
    for g, ref, key in zip(_grads(out, t[:3], max(ref_n, 1)), ref_grads, KEYS):
        assert torch.isfinite(g).all(), key
        np.testing.assert_allclose(g.cpu().numpy(), ref, err_msg=key, **GRAD_TOL)


def test_giou_ties_split_the_gradient(dev, golden):
    """Prediction side == target side: torch gives each operand of the min / max a half, and so
    does the kernel (the fixture's gradients are torch's).  With the l and r sides tied the
    gradient of those sides is far from zero, so a 1 / 0 split would show; with all four tied the
    two boxes are equal and the halves cancel to zero."""
    from frcnn_amd import ops
    c = fcos_inputs.loss_case('tie')
    t = _dev_case(c, dev, grad=True)
    out = ops.fcos_losses(*t, **fcos_inputs.loss_kwargs(c))
    g = _grads(out, t[:3], int(out[3]))[1].cpu().numpy()
    y = c['ltrb'] / np.float32(c['reg_std'])
    tied = (c['reg'].T == y) & (c['labels'] > 0)[:, None]
    equal, part = tied.all(1), tied[:, 0] & tied[:, 2] & ~tied.all(1)
    assert equal.sum() >= 5 and part.sum() >= 5
    ref = golden('fcos_loss.npz')['tie_greg'] * int(out[3])
    assert np.abs(ref[0][part]).min() > 1e-3 and np.abs(ref[2][part]).min() > 1e-3
    np.testing.assert_allclose(g[:, part], ref[:, part], **GRAD_TOL)
    assert np.abs(ref[:, equal]).max() < 1e-12
    np.testing.assert_allclose(g[:, equal], ref[:, equal], **GRAD_TOL)


def test_two_calls_are_bit_identical(dev):
    from frcnn_amd import ops
    c = fcos_inputs.loss_case('full')
    outs = []
    for _ in range(2):
        t = _dev_case(c, dev, grad=True)
        out = ops.fcos_losses(*t, **fcos_inputs.loss_kwargs(c))
        sum(out[:3]).backward()
        outs.append([o.detach() for o in out] + [x.grad for x in t[:3]])
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_strided_views_are_bit_identical(dev):
    """Channels-last class logits (sk = 1, si = C), transposed regression, every second centerness
    element of a wider buffer: the same losses and gradients, bit for bit, as the contiguous tensors."""
    from frcnn_amd import ops
    c = fcos_inputs.loss_case('m255')
    kw = fcos_inputs.loss_kwargs(c)
    cls, reg, ctr, labels, ltrb, ctr_t = _dev_case(c, dev)

    def transposed(x):
        return x.t().contiguous().t()

    def every_second(x):
        big = torch.full((2 * x.shape[0],), float('nan'), device=dev)
        big[::2] = x
        return big[::2]

    def run(fc, fr, ft):
        a, b, d = [f(x).detach().requires_grad_(True) for f, x in ((fc, cls), (fr, reg), (ft, ctr))]
        out = ops.fcos_losses(a, b, d, labels, ltrb, ctr_t, **kw)
        sum(out[:3]).backward()
        return [o.detach() for o in out] + [a.grad, b.grad, d.grad], (a.stride(), b.stride(), d.stride())
    clone = lambda x: x.clone()
    base, s0 = run(clone, clone, clone)
    got, s1 = run(transposed, transposed, every_second)
    assert s0 == ((c['M'], 1), (c['M'], 1), (1,)) and s1 == ((1, c['C']), (1, 4), (2,))
    for x, y in zip(base, got):
        assert torch.equal(x, y)


def test_status_word_gives_nan_losses(dev):
    from frcnn_amd import ops
    c = fcos_inputs.loss_case('m257')
    args = _dev_case(c, dev)
    word = ops.status_word(dev)
    assert int(word.item()) == 0
    try:
        word.fill_(4)
        out = ops.fcos_losses(*args, **fcos_inputs.loss_kwargs(c))
        assert np.isnan(support.loss_values(out)).all()
    finally:
        word.zero_()
    out = ops.fcos_losses(*args, **fcos_inputs.loss_kwargs(c))
    assert np.isfinite(support.loss_values(out)).all()
    ops.check_device_status(dev)


def test_head_routes_both_samplers_to_the_fused_loss(dev, monkeypatch):
    """calc_loss_flat of a head without GFL -- plain FCOS and ATSS alike -- is one ops.fcos_losses
    call, under the reference's keys in its order."""
    from frcnn_amd import ops
    from frcnn_amd.heads.fcos_head import FCOSHead
    c = fcos_inputs.loss_case('m255')
    t = _dev_case(c, dev)
    want = ops.fcos_losses(*t, **fcos_inputs.loss_kwargs(c))
    calls = []
    orig = ops.fcos_losses
    monkeypatch.setattr(ops, 'fcos_losses', lambda *a, **k: calls.append(1) or orig(*a, **k))
    w = fcos_inputs.WEIGHTS
    for atss in (None, dict(topk=9, scale=8)):
        head = FCOSHead(num_classes=c['C'] + 1, in_channels=8, stacked_convs=1, feat_channels=8, reg_std=c['reg_std'],
                        reg_mean=c['reg_mean'], atss_cfg=atss,
                        loss_cls=dict(type='FocalLoss', use_sigmoid=True, loss_weight=w['cls_weight']),
                        loss_bbox=dict(type='GIoULoss', loss_weight=w['bbox_weight']),
                        loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=w['ctr_weight']))
        res = head.calc_loss_flat(t[0], t[1], t[2].view(1, -1), *t[3:])
        assert list(res) == ['cls_loss', 'ctr_loss', 'bbox_loss']
        for k, r in zip(('cls_loss', 'bbox_loss', 'ctr_loss'), want[:3]):
            assert torch.equal(res[k], r)
    assert calls == [1, 1]


def test_no_host_sync(dev):
    """ops.fcos_assign, ops.fcos_losses (forward and backward) and the head's fused forward_train
    read nothing back to the host; the mode itself is checked to catch the read the old path made."""
    from frcnn_amd import ops
    c = fcos_inputs.loss_case('m257')
    kw = fcos_inputs.loss_kwargs(c)
    t = _dev_case(c, dev, grad=True)
    ops.fcos_losses(*t, **kw)  # workspace and status word exist from here on
    with pytest.raises(RuntimeError):
        support.no_sync(lambda: int((t[3] > 0).sum()))

    def fused():
        out = ops.fcos_losses(*t, **kw)
        sum(out[:3]).backward()
        return out
    support.no_sync(fused)

    torch.manual_seed(3)
    head = _head(dev, reg_coef_trainable=True)
    head.init_weights()
    feats = [torch.randn(2, 8, h, w, device=dev) for h, w in fcos_inputs.GRIDS]
    boxes, labels, _ = fcos_inputs.TARGET_CASES['a']
    gb = [torch.from_numpy(b).to(dev) for b in boxes]
    gl = [torch.from_numpy(l).to(dev) for l in labels]
    metas = fcos_inputs.img_metas()

    def step():
        head.zero_grad()
        losses = head.forward_train(feats, gb, gl, metas, None)
        sum(losses.values()).backward()
        return losses
    step()  # the convolutions choose their algorithms on the first call
    losses = support.no_sync(step)
    assert list(losses) == ['cls_loss', 'ctr_loss', 'bbox_loss']
    assert all(torch.isfinite(v).item() for v in losses.values())
    assert float(head.reg_coef.grad.abs().sum()) > 0 and float(head.fcos_center.weight.grad.abs().sum()) > 0
