"""Balanced-L1 HIP loss (csrc/losses.hip, frh_balanced_l1_fwd / _bwd) against the torch
restatement of lib/losses.py:158-180 (frcnn_amd.losses.balanced_l1_loss) run on the CPU copy
of the same f32 tensors: forward sums within rtol 2e-5 and gradients within rtol 1e-4 / atol
1e-6 (the bars of tests/test_gpu_losses.py), for the plain, masked and class-selected forms,
strided inputs, padding rows (label -1) and the status-word NaN.  Each test prints the sum's
relative deviation from the CPU float32 restatement and that restatement's own deviation
from float64."""
import pytest
import torch

import libra_inputs
from frcnn_amd import losses, ops

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
CFGS = [dict(alpha=0.5, gamma=1.5, beta=1.0), dict(alpha=0.3, gamma=1.1, beta=0.7)]


def _ref(x, y, mask, kw):
    """Summed restatement over the rows of `mask` (CPU, x's dtype)."""
    e = losses.balanced_l1_loss(x, y, **kw)
    return (e if mask is None else e * mask.to(e.dtype)).sum()


def _check(hip_fn, x0, y0, mask, kw, scale=0.37):
    xa = x0.clone().to(DEV).requires_grad_(True)
    la = hip_fn(xa)
    xb = x0.clone().requires_grad_(True)
    lb = _ref(xb, y0, mask, kw)
    l64 = _ref(x0.double(), y0.double(), mask, kw)
    print('sum hip {:.9g} cpu32 {:.9g} cpu64 {:.12g}: hip-cpu32 rel {:.3g}, cpu32-cpu64 rel {:.3g}'.format(
        float(la), float(lb), float(l64), abs(float(la) - float(lb)) / abs(float(lb)),
        abs(float(lb) - float(l64)) / abs(float(l64))))
    torch.testing.assert_close(la.cpu(), lb.detach(), rtol=2e-5, atol=1e-6)
    (la * scale).backward()
    (lb * scale).backward()
    torch.testing.assert_close(xa.grad.cpu(), xb.grad, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize('kw', CFGS)
def test_balanced_l1_plain(kw):
    x, y = (torch.from_numpy(a) for a in libra_inputs.balanced_l1_inputs(21, 1037, 4))  # > one workgroup, odd
    loss = losses.BalancedL1Loss(**kw)
    yd = y.to(DEV)
    _check(lambda t: loss(t, yd), x, y, None, kw)


@pytest.mark.parametrize('rows_dim', [0, 1])
def test_balanced_l1_masked_with_padding_rows(rows_dim):
    """label > 0 rows only; label -1 (padding) and 0 rows add nothing, forward or backward."""
    kw = CFGS[0]
    x, y = (torch.from_numpy(a) for a in libra_inputs.balanced_l1_inputs(22, 771, 4))
    gen = torch.Generator().manual_seed(5)
    label = torch.randint(-1, 4, (771,), generator=gen)
    mask = (label > 0).view(-1, 1)
    if rows_dim == 1:  # the channel-major [4, n] views the target gathers produce
        x, y, mask = x.t().contiguous(), y.t().contiguous(), mask.view(1, -1)
    loss = losses.BalancedL1Loss(**kw)
    yd, ld = y.to(DEV), label.to(DEV)
    _check(lambda t: loss.masked(t, yd, ld, rows_dim), x, y, mask, kw)


def test_balanced_l1_strided_inputs():
    """x a transposed view and y a column slice of a wider buffer: read through their strides."""
    kw = CFGS[1]
    x, y = (torch.from_numpy(a) for a in libra_inputs.balanced_l1_inputs(23, 515, 4))
    label = torch.randint(0, 3, (515,), generator=torch.Generator().manual_seed(6))
    wide = torch.zeros(515, 9)
    wide[:, 2:6] = y
    wd, ld = wide.to(DEV), label.to(DEV)
    loss = losses.BalancedL1Loss(**kw)

    def hip(t):
        xt = t.t().contiguous().t()  # [n, 4] with strides (1, n)
        assert xt.stride() == (1, 515)
        return loss.masked(xt, wd[:, 2:6], ld, 0)
    _check(hip, x, y, (label > 0).view(-1, 1), kw)


def test_balanced_l1_class_selected():
    kw = CFGS[0]
    n, ncls = 389, 7
    gen = torch.Generator().manual_seed(7)
    reg = torch.randn(n, 4 * ncls, generator=gen)
    y = torch.randn(n, 4, generator=gen) * 1.3
    label = torch.randint(-1, ncls, (n,), generator=gen)
    loss = losses.BalancedL1Loss(loss_weight=1.0, **kw)
    yd, ld = y.to(DEV), label.to(DEV)
    xa = reg.clone().to(DEV).requires_grad_(True)
    la = loss.class_selected(xa, ncls, yd, ld)
    xb = reg.clone().requires_grad_(True)
    sel = xb.view(-1, 4, ncls)[torch.arange(n), :, label.clamp(min=0)]
    lb = _ref(sel, y, (label > 0).view(-1, 1), kw)
    print('sum hip {:.9g} cpu32 {:.9g}'.format(float(la), float(lb)))
    torch.testing.assert_close(la.cpu(), lb.detach(), rtol=2e-5, atol=1e-6)
    la.backward()
    lb.backward()
    torch.testing.assert_close(xa.grad.cpu(), xb.grad, rtol=1e-4, atol=1e-6)


def test_balanced_l1_status_word_gives_nan():
    x, y = (torch.from_numpy(a).to(DEV) for a in libra_inputs.balanced_l1_inputs(24, 64, 4))
    loss = losses.BalancedL1Loss()
    w = ops.status_word(DEV)
    assert int(w.item()) == 0
    try:
        w.fill_(8)  # no one-launch kernel's bit: only the loss's NaN is under test
        assert torch.isnan(loss(x, y)).item()
    finally:
        w.zero_()
    assert torch.isfinite(loss(x, y)).item()


def test_rcnn_head_loss_uses_the_hip_balanced_l1():
    """BBoxHead.calc_loss_all with BalancedL1Loss (class-agnostic, sampled avg_factor): the
    regression loss is the masked HIP sum over avg_factor."""
    from frcnn_amd.heads.bbox_head import BBoxHead
    from frcnn_amd.config import wrap
    head = BBoxHead(21, reg_class_agnostic=True, loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False),
                    loss_bbox=dict(type='BalancedL1Loss'))
    gen = torch.Generator().manual_seed(8)
    n = 200
    cls_out, reg_out = torch.randn(n, 21, generator=gen), torch.randn(n, 4, generator=gen)
    label = torch.randint(0, 21, (n,), generator=gen)
    label[torch.rand(n, generator=gen) > 0.3] = 0
    param = torch.randn(4, n, generator=gen)
    c, r = head.calc_loss_all(cls_out.to(DEV), reg_out.to(DEV), label.to(DEV), param.to(DEV),
                              wrap(dict(sampler=dict(type='IoUBalancedNegSampler'))))
    want = _ref(reg_out, param.t(), (label > 0).view(-1, 1), CFGS[0]) / n
    torch.testing.assert_close(r.cpu(), want, rtol=2e-5, atol=1e-6)
    torch.testing.assert_close(c.cpu(), torch.nn.functional.cross_entropy(cls_out, label, reduction='sum') / n,
                               rtol=2e-5, atol=1e-6)
