"""Shared by tests/test_gpu_deform_conv_bwd.py and tests/test_deform_bwd_cpu.py: the f64 reference
gradients of the deformable 3x3 convolution (autograd on ops.deform_conv3x3_torch) and, from the
definition in include/frcnn_amd.h written out a second time here, the per-element sums of the
absolute values of the terms each gradient adds up -- the right-hand side of the error bars.

With S[n, c, k, p] the blended sample, G[n, c, k, p] = sum_co w[co, c, k] gy[n, co, p]:
  gx   adds G (hy hx, hy lx, ly hx, ly lx) to the sample's four corners,
  goff[n, g 18 + 2 k (+ 1), p] = sum_{c in g} G dS/dpy (dS/dpx),
       dS/dpy = hx (v10 - v00) + lx (v11 - v01), dS/dpx = hy (v01 - v00) + ly (v11 - v10),
  gw[co, c, k] = sum_{n, p} gy[n, co, p] S[n, c, k, p].
Every term is a product w gy (blend weight) (x or 1); the blend weights are >= 0, so for gx and gw
the sum of the absolute values of the terms is the restatement's own autograd on |x|, |w|, |gy|,
and for goff it is sum_{c in g} (sum_co |w| |gy|) (hx |v00| + lx |v01| + hx |v10| + lx |v11|) and
the x analogue -- `G` of that formula being the sum of ABSOLUTE products, as a sum of absolute
terms must be (|sum_co w gy| would be smaller than the error of an f32 sum that cancels)."""
import torch

U = 2.0 ** -24


def reference(x, off, wt, dg, gy):
    """(y, gx, goff, gw) in f64 by autograd on the restatement, without ReLU (the caller masks gy)."""
    from frcnn_amd.ops import deform_conv3x3_torch
    x, off, wt = [t.detach().double().clone().requires_grad_(True) for t in (x, off, wt)]
    y = deform_conv3x3_torch(x, off, wt, dg)
    y.backward(gy.double())
    return y.detach(), x.grad, off.grad, wt.grad


def sample_parts(off, dg, H, W):
    """From the definition: ok [n, dg, 9, H, W], (ly, lx, hy, hx), and the four corners
    (00, 01, 10, 11) as (flat cell index, in-map and ok) pairs."""
    n = off.shape[0]
    o = off.double().reshape(n, dg, 9, 2, H, W)
    k = torch.arange(9)
    ky = (k // 3 - 1).double().view(1, 1, 9, 1, 1)
    kx = (k % 3 - 1).double().view(1, 1, 9, 1, 1)
    py = torch.arange(H).double().view(1, 1, 1, H, 1) + ky + o[:, :, :, 0]
    px = torch.arange(W).double().view(1, 1, 1, 1, W) + kx + o[:, :, :, 1]
    ok = (py > -1) & (py < H) & (px > -1) & (px < W)
    py, px = torch.where(ok, py, torch.zeros_like(py)), torch.where(ok, px, torch.zeros_like(px))
    y0, x0 = py.floor().long(), px.floor().long()
    ly, lx = py - py.floor(), px - px.floor()
    corners = []
    for yy, xx in ((y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)):
        valid = ok & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        corners.append((yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1), valid))
    return ok, (ly, lx, 1 - ly, 1 - lx), corners


def abs_terms(x, off, wt, dg, gy):
    """Sum of |terms| of every element of (gx, goff, gw), f64, and the largest number of samples
    that touch one input element (a bincount of the in-map corner indices per image and group)."""
    from frcnn_amd.ops import deform_conv3x3_torch
    n, cin, H, W = x.shape
    cout, cpg = wt.shape[0], cin // dg
    xa, wa = x.detach().double().abs().requires_grad_(True), wt.detach().double().abs().requires_grad_(True)
    ga = gy.double().abs()
    deform_conv3x3_torch(xa, off.detach().double(), wa, dg).backward(ga)
    ok, (ly, lx, hy, hx), corners = sample_parts(off, dg, H, W)
    G = torch.einsum('ock,nop->nckp', wa.detach().reshape(cout, cin, 9), ga.reshape(n, cout, H * W))
    G = G.reshape(n, dg, cpg, 9, H, W)
    xg = xa.detach().reshape(n, dg, cpg, H * W)
    v = []
    hits = torch.zeros(n, dg, H * W, dtype=torch.long)
    for idx, valid in corners:
        flat = idx.reshape(n, dg, 1, 9 * H * W).expand(-1, -1, cpg, -1)
        v.append(xg.gather(3, flat).view(n, dg, cpg, 9, H, W) * valid.unsqueeze(2).double())
        for i in range(n):
            for g in range(dg):
                hits[i, g] += torch.bincount(idx[i, g][valid[i, g]], minlength=H * W)
    touch = int(hits.max())
    hx_, lx_, hy_, ly_ = [t.unsqueeze(2) for t in (hx, lx, hy, ly)]
    ty = (G * (hx_ * v[0] + lx_ * v[1] + hx_ * v[2] + lx_ * v[3])).sum(2) * ok.double()
    tx = (G * (hy_ * v[0] + hy_ * v[1] + ly_ * v[2] + ly_ * v[3])).sum(2) * ok.double()
    goff_abs = torch.stack([ty, tx], 3).reshape(n, 18 * dg, H, W)
    return xa.grad, goff_abs, wa.grad, touch


def check(name, got, want, terms, n_terms):
    """|got - want| <= (n_terms + 8) 2^-24 terms, element by element; prints max err / bound."""
    err = (got.detach().double().cpu() - want).abs()
    bound = (n_terms + 8) * U * terms
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print('{}: max err / bound = {:.4f} (n_terms {})'.format(name, ratio, n_terms))
    assert got.shape == want.shape and bool((err <= bound).all()), (name, ratio)
