"""CPU side of the deformable convolution's HIP backward (tests/test_gpu_deform_conv_bwd.py):
hip_grad=True on CPU tensors is the restatement bit for bit and makes no library call; the
restatement's offset gradient -- the definition frh_deform_conv3x3_bwd has to meet -- at four
hand-derived points; and the sum-of-|terms| helper of the GPU bars against scalar loops."""
import math

import numpy as np
import torch

import deform_bwd_ref as ref
import ga_inputs


def _case(n, cin, cout, dg, h, w, seed, kind='eighths'):
    return [torch.from_numpy(a) for a in ga_inputs.deform_case(n, cin, cout, dg, h, w, kind, seed)]


def _grads(fn, ts):
    ts = [t.clone().requires_grad_(True) for t in ts]
    y = fn(*ts)
    ys = y if isinstance(y, (list, tuple)) else [y]
    g = torch.Generator().manual_seed(5)
    sum((v * torch.randn(v.shape, generator=g)).sum() for v in ys).backward()
    return [v.detach() for v in ys], [t.grad for t in ts]


def test_hip_grad_on_cpu_tensors_is_the_restatement(monkeypatch):
    from frcnn_amd import ops
    from frcnn_amd.dcn import DeformConv
    calls = []
    monkeypatch.setattr(ops, '_call', lambda name, *a: calls.append(name))
    x, off, wt = _case(2, 32, 64, 4, 5, 7, seed=1)
    want = _grads(lambda a, b, c: ops.deform_conv3x3_torch(a, b, c, 4, True), [x, off, wt])
    got = _grads(lambda a, b, c: ops.deform_conv3x3(a, b, c, 4, relu=True, hip_grad=True), [x, off, wt])
    lv = _grads(lambda a, b, c: ops.deform_conv3x3_levels([a], [b], c, 4, relu=True, hip_grad=True), [x, off, wt])
    for a, b, c in zip(want[0] + want[1], got[0] + got[1], lv[0] + lv[1]):
        assert torch.equal(a, b) and torch.equal(a, c)
    # guided mode: the offsets are the 1x1 convolution, differentiated by autograd
    g = torch.Generator().manual_seed(2)
    ow, s = torch.randn(72, 2, generator=g) * 0.3, torch.randn(2, 2, 5, 7, generator=g)
    want = _grads(lambda a, b, c, d: ops.deform_conv3x3_torch(
        a, torch.nn.functional.conv2d(b, d.view(72, 2, 1, 1)), c, 4), [x, s, wt, ow])
    got = _grads(lambda a, b, c, d: ops.deform_conv3x3(a, b, c, 4, offset_weight=d, hip_grad=True), [x, s, wt, ow])
    for a, b in zip(want[0] + want[1], got[0] + got[1]):
        assert torch.equal(a, b)
    m = DeformConv(32, 64, 3, padding=1, deformable_groups=4)
    assert DeformConv.hip_grad is False
    m.hip_grad = True
    assert torch.equal(m(x, off), ops.deform_conv3x3_torch(x, off, m.weight, 4))
    assert calls == [] and isinstance(ops._DEFORM_BWD_EXCLUDED, set)


def _goff_at(dy, dx, pos, gyv=2.0):
    """goff (dy, dx channels of the centre tap) at `pos` of a 1-channel 3 x 3 map x[i, j] = 3 i + j
    + 1 whose weight is 1 on the centre tap alone, for the centre tap's offset (dy, dx) there and
    an upstream gradient gyv at that position only."""
    from frcnn_amd.ops import deform_conv3x3_torch
    x = (torch.arange(9.0).reshape(1, 1, 3, 3) + 1).double()
    wt = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    wt[0, 0, 1, 1] = 1.0
    off = torch.zeros(1, 18, 3, 3, dtype=torch.float64)
    off[0, 8, pos[0], pos[1]], off[0, 9, pos[0], pos[1]] = dy, dx
    off.requires_grad_(True)
    gy = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    gy[0, 0, pos[0], pos[1]] = gyv
    deform_conv3x3_torch(x, off, wt, 1).backward(gy)
    g = off.grad
    assert int((g != 0).sum()) <= 2  # nothing outside the two channels at pos
    return float(g[0, 8, pos[0], pos[1]]), float(g[0, 9, pos[0], pos[1]])


def test_offset_gradient_witnesses():
    """x11 = 5, x12 = 6, x21 = 8, x22 = 9, x01 = 2, x02 = 3.
    fractional: (1.25, 1.5): dS/dpy = .5 (8 - 5) + .5 (9 - 6) = 3, dS/dpx = .75 (6 - 5) + .25 (9 - 8) = 1;
    integer: (2, 1): ly = lx = 0, the lower corners are outside the map: dS/dpy = 0 - x21 = -8 and
    dS/dpx = x22 - x21 = 1, the one-sided values (floor has derivative 0);
    -1 < py < 0: (-0.5, 1) from position (0, 1): the upper corners are outside: dS/dpy = x01 = 2,
    dS/dpx = .5 (x02 - x01) = .5;
    out of range: (6, 1): exactly 0."""
    assert _goff_at(0.25, 0.5, (1, 1)) == (6.0, 2.0)
    assert _goff_at(1.0, 0.0, (1, 1)) == (-16.0, 2.0)
    assert _goff_at(-0.5, 0.0, (0, 1)) == (4.0, 1.0)
    assert _goff_at(5.0, 0.0, (1, 1)) == (0.0, 0.0)
    assert _goff_at(float('nan'), 0.0, (1, 1)) == (0.0, 0.0)


def test_abs_terms_helper_against_scalar_loops():
    """1 image, 3 x 3, cin 8, dg 2, cout 2: the helper's sums of |terms| and its touch count
    against loops over the definition."""
    x, off, wt = _case(1, 8, 2, 2, 3, 3, seed=3)
    gy = torch.randn(1, 2, 3, 3, generator=torch.Generator().manual_seed(4))
    gxa, goffa, gwa, touch = ref.abs_terms(x, off, wt, 2, gy)
    H = W = 3
    ex = np.zeros((8, H, W))
    eo = np.zeros((36, H, W))
    ew = np.zeros((2, 8, 9))
    cnt = np.zeros((2, H, W), int)
    xa, wa, ga, o = x[0].double().abs().numpy(), wt.double().abs().numpy().reshape(2, 8, 9), \
        gy[0].double().abs().numpy(), off[0].double().numpy()
    for yy in range(H):
        for xx in range(W):
            for g in range(2):
                for k in range(9):
                    py, px = yy + k // 3 - 1 + o[g * 18 + 2 * k, yy, xx], xx + k % 3 - 1 + o[g * 18 + 2 * k + 1, yy, xx]
                    if not (-1 < py < H and -1 < px < W):
                        continue
                    y0, x0 = math.floor(py), math.floor(px)
                    ly, lx = py - y0, px - x0
                    hy, hx = 1 - ly, 1 - lx
                    cs = [(y0, x0, hy * hx, hx, hy), (y0, x0 + 1, hy * lx, lx, hy), (y0 + 1, x0, ly * hx, hx, ly),
                          (y0 + 1, x0 + 1, ly * lx, lx, ly)]
                    for cy, cx, _, _, _ in cs:
                        if 0 <= cy < H and 0 <= cx < W:
                            cnt[g, cy, cx] += 1
                    for c in range(4 * g, 4 * g + 4):
                        G = sum(wa[co, c, k] * ga[co, yy, xx] for co in range(2))
                        for cy, cx, wgt, wy, wx in cs:
                            if 0 <= cy < H and 0 <= cx < W:
                                ex[c, cy, cx] += G * wgt
                                eo[g * 18 + 2 * k, yy, xx] += G * wy * xa[c, cy, cx]
                                eo[g * 18 + 2 * k + 1, yy, xx] += G * wx * xa[c, cy, cx]
                                for co in range(2):
                                    ew[co, c, k] += ga[co, yy, xx] * wgt * xa[c, cy, cx]
    np.testing.assert_allclose(gxa[0].numpy(), ex, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(goffa[0].numpy(), eo, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(gwa.numpy().reshape(2, 8, 9), ew, rtol=1e-12, atol=1e-14)
    assert touch == cnt.max() and touch > 1
