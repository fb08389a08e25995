"""The workgroup forms of frh_conv3x3_nchw_bn_act: cin split across the waves of a workgroup
(csrc/conv3x3_nchw_kernels.h, forms 3 and 4, the ones the product's table picks), and the
laboratory forms that share U through LDS, with and without the split (forms 5 to 7,
tools/csrc/conv3x3_nchw_lab.hip).

Every new form runs through the tools library's frh_conv3x3_nchw_bn_act_form, the product
entry (form None) with its own choice beside them, and is held to the four properties of
test_gpu_conv3x3_nchw.py with that file's definitions: exact borders, the float64 error bound
2 (cin + 16) 2^-24 magW (the at most three extra roundings of a split fit inside the 16), the
epilogue's bits against frh_bn_act, and repeatability.  Shapes are (n, cin, cout, h, w), the
smallest that reach each way a workgroup form can go wrong; a form that cannot run a shape
(two channel blocks per wave at cout = 48) must refuse it and leave the output untouched.

A test here that runs into a time limit has hung at a barrier: every wave of a workgroup must
reach every barrier, so look for a wave-dependent exit in the kernel, do not run it again."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import support  # noqa: E402
from test_gpu_conv3x3_nchw import EPS, _case, _fused, _on_dev  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 4, 16, 3, 8),        # one cin step: fewer steps than S waves or ring stages; workgroup mostly empty
    (1, 20, 32, 5, 34),      # cin no multiple of the chunk or of 4 S; a run of one valid tile column past a full run
    (2, 64, 64, 19, 32),     # stage 4's plane: odd h, batch stride
    (1, 32, 48, 17, 36),     # cout that only the 16-wide block fits; ragged in both directions
    (2, 48, 192, 2, 2),      # one tile per image; many channel blocks; work items no multiple of the workgroup
]
# channel blocks per wave of each new form: 3 (cin in 4), 4 (cin in 2, two tile runs); the lab's
# 5 (LDS, NC = 2, four runs), 6 (LDS, cin in 2, two runs), 7 (LDS, four runs)
NEW_FORMS = {3: 1, 4: 1, 5: 2, 6: 1, 7: 1}
FORMS = [None] + sorted(NEW_FORMS)


def _fits(shape, form):
    return form is None or shape[2] % (16 * NEW_FORMS[form]) == 0


def _refused(shape, form, dev):
    """The form entry returns an error and launches nothing: the sentinel stays."""
    from frcnn_amd import _lib
    n, cin, cout, h, w = shape
    d = _on_dev(shape, dev)
    y = torch.full((n, cout, h, w), 7.0, device=dev)
    ws = torch.empty(16 * cin * cout, device=dev)
    p = _lib.ptr
    st = support.tools().frh_conv3x3_nchw_bn_act_form(form, p(d['x']), p(d['w']), None, None, None, None, 0.0, p(y),
                                                      p(ws), n, cin, cout, h, w, 0, _lib.stream_of(y))
    torch.cuda.synchronize()
    assert st != 0
    assert bool((y == 7.0).all())


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', SHAPES)
def test_exact_borders(dev, shape, form):
    """x = 1, w = 1, no BN: every partial sum of every wave is a multiple of 1/4 below 2^24, so
    the split order cannot matter and the result is exactly cin x (valid taps): 4, 6 or 9 x cin."""
    if not _fits(shape, form):
        return _refused(shape, form, dev)
    n, cin, cout, h, w = shape
    x = torch.ones(n, cin, h, w, device=dev)
    wt = torch.ones(cout, cin, 3, 3, device=dev)
    taps = F.conv2d(torch.ones(1, 1, h, w), torch.ones(1, 1, 3, 3), padding=1)
    assert set(taps.unique().tolist()) <= {4.0, 6.0, 9.0}
    assert torch.equal(_fused(x, wt, form=form).cpu(), (taps * cin).expand(n, cout, h, w))


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', SHAPES)
def test_accuracy_against_float64(dev, shape, form):
    """|y - y64| <= 2 (cin + 16) 2^-24 magW per element and max|y - y64| <= 8 max|y32 - y64|."""
    if not _fits(shape, form):
        return _refused(shape, form, dev)
    c, d = _case(shape), _on_dev(shape, dev)
    y = _fused(d['x'], d['w'], form=form).cpu().double()
    bound = 2.0 * (shape[1] + 16) * 2.0 ** -24 * c['mag']
    err = (y - c['y64']).abs()
    err32 = (c['y32'].double() - c['y64']).abs()
    print('shape', shape, 'form', form, 'max err / bound', float((err / bound).max()),
          'max err / max direct-f32 err', float(err.max() / err32.max()))
    assert torch.isfinite(y).all()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float(err.max()) <= 8.0 * float(err32.max())


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', SHAPES)
def test_epilogue_bits_equal_bn_act(dev, shape, form):
    """fused(BN with signed gammas, relu or not) == frh_bn_act(fused raw output of the same form)."""
    if not _fits(shape, form):
        return _refused(shape, form, dev)
    from frcnn_amd import _lib
    d = _on_dev(shape, dev)
    raw = _fused(d['x'], d['w'], form=form)
    n, cout, h, w = raw.shape
    # frh_bn_act takes planes of a multiple of 4 elements: it is elementwise per channel, so a
    # plane that is not (5 x 34) goes through it padded and comes back cut
    hw = (h * w + 3) // 4 * 4
    src = torch.zeros(n, cout, hw, device=dev)
    src[:, :, :h * w] = raw.view(n, cout, h * w)
    p = _lib.ptr
    for relu in (False, True):
        ref = torch.empty_like(src)
        _lib.call('frh_bn_act', p(src), None, p(ref), *[p(t) for t in d['bn']], EPS, n, cout, hw, int(relu),
                  _lib.stream_of(raw))
        assert torch.equal(_fused(d['x'], d['w'], d['bn'], relu, form), ref[:, :, :h * w].view(n, cout, h, w))
    assert torch.equal(_fused(d['x'], d['w'], None, True, form), raw.clamp_min(0.0))


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', SHAPES)
def test_repeatability(dev, shape, form):
    """Two launches give equal bits; image i of the whole batch equals the n = 1 call on it."""
    if not _fits(shape, form):
        return _refused(shape, form, dev)
    d = _on_dev(shape, dev)
    y = _fused(d['x'], d['w'], d['bn'], True, form)
    assert torch.equal(y, _fused(d['x'], d['w'], d['bn'], True, form))
    for i in range(shape[0]):
        assert torch.equal(y[i:i + 1], _fused(d['x'][i:i + 1].contiguous(), d['w'], d['bn'], True, form))
