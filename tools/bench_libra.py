"""Timing of the Libra R-CNN kernels against what they replace.

    python tools/bench_libra.py [--iters 200] [--out profiles/libra/bench_libra.json]

BFP neck (csrc/bfp.hip through necks.BFP) at the cfg2 level shapes -- B = 2, C = 256,
152x256 .. 10x16, channels-last, the last level the FPN's stride-2 view -- forward and
forward + backward, against the same function written with the reference's torch ops
(lib/necks.py:116-141: adaptive_max_pool2d / interpolate / sum / add) on the same GPU
tensors.  The IoU-balanced sampler (frh_sample_iou_balanced) against frh_sample_random on
one RCNN-sized input (2 images x 2 000 proposal rows + 8 gts, 512 / 128), both in their
list form.

Every figure is the mean of `iters` back-to-back calls between one HIP event pair after a
warm-up, repeated 5 times with the two sides alternating (the spread is reported).  GB/s are
the op's algorithmic bytes -- every input level read once and every output level written
once forward (the refine map and the argmax maps are extra traffic the op itself adds, not
counted); upstream gradients read once and input gradients written once backward -- over
that time."""
import argparse
import json
import os

import torch
import torch.nn.functional as F

from benchlib import REPO, compare, require_gpu, write_json

SIZES = [(152, 256), (76, 128), (38, 64), (19, 32), (10, 16)]
B, C, REFINE = 2, 256, 2


def torch_bfp(feats, r=REFINE):
    """The reference's BFP.forward, op for op."""
    size = feats[r].shape[-2:]
    uni = []
    for i, f in enumerate(feats):
        if i < r:
            uni.append(F.adaptive_max_pool2d(f, output_size=size))
        elif i > r:
            uni.append(F.interpolate(f, size=size, mode='nearest'))
    refine = sum(uni) / len(uni)
    outs = []
    for i, f in enumerate(feats):
        if i < r:
            res = F.interpolate(refine, size=f.shape[-2:], mode='nearest')
        elif i > r:
            res = F.adaptive_max_pool2d(refine, output_size=f.shape[-2:])
        else:
            res = refine
        outs.append(f + res)
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'libra', 'bench_libra.json'))
    args = ap.parse_args()
    require_gpu('bench_libra')
    from frcnn_amd import ops
    from frcnn_amd.necks import BFP
    from frcnn_amd.region import IoUBalancedNegSampler
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    levels = [torch.randn(B, C, h, w, device=dev).contiguous(memory_format=torch.channels_last) for h, w in SIZES[:4]]
    # the FPN's extra level: outs[-1][:, :, ::2, ::2] of the level before it
    feats = levels + [levels[3][:, :, ::2, ::2]]
    assert tuple(feats[4].shape[2:]) == SIZES[4]
    bfp = BFP(C, 5, REFINE)
    with torch.no_grad():
        same = all(torch.equal(a, b) for a, b in zip(bfp(feats), torch_bfp(feats)))
    level_bytes = sum(4 * B * C * h * w for h, w in SIZES)
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters,
           'shapes': {'batch': B, 'channels': C, 'levels': SIZES, 'refine_level': REFINE, 'layout': 'NHWC, last level strided'},
           'bfp_equals_torch_gpu_composition_bitwise': bool(same)}

    def fwd_hip():
        with torch.no_grad():
            bfp(feats)

    def fwd_torch():
        with torch.no_grad():
            torch_bfp(feats)
    th, tt, ah, at = compare(fwd_hip, fwd_torch, args.iters, args.iters, warmup=5)
    fb = 2 * level_bytes
    res['bfp_forward'] = {'hip_us': round(th, 2), 'torch_us': round(tt, 2), 'hip_runs_us': ah, 'torch_runs_us': at,
                          'algorithmic_bytes': fb, 'hip_GBps': round(fb / th / 1e3, 1),
                          'torch_GBps': round(fb / tt / 1e3, 1), 'speedup': round(tt / th, 2)}

    gin = [f.detach().clone().requires_grad_(True) for f in levels]
    gouts = [torch.randn(B, C, h, w, device=dev).contiguous(memory_format=torch.channels_last) for h, w in SIZES]

    def with_view(fn):
        def run():
            for t in gin:
                t.grad = None
            outs = fn(gin + [gin[3][:, :, ::2, ::2]])
            torch.autograd.backward(outs, gouts)
        return run
    half = max(args.iters // 2, 10)
    th, tt, ah, at = compare(with_view(bfp), with_view(torch_bfp), half, half, warmup=5)
    fbb = 4 * level_bytes
    res['bfp_forward_backward'] = {'hip_us': round(th, 2), 'torch_us': round(tt, 2), 'hip_runs_us': ah,
                                   'torch_runs_us': at, 'algorithmic_bytes': fbb,
                                   'hip_GBps': round(fbb / th / 1e3, 1), 'torch_GBps': round(fbb / tt / 1e3, 1),
                                   'speedup': round(tt / th, 2),
                                   'note': 'includes the stride-2 view\'s autograd and the grad reset on both sides'}

    # sampler: one RCNN-sized input
    S, n, max_num, pos_num = 2, 2008, 512, 128
    gen = torch.Generator().manual_seed(1)
    lab = torch.zeros(S, n, dtype=torch.int64)
    lab[torch.rand(S, n, generator=gen) < 0.05] = 3
    lab[torch.rand(S, n, generator=gen) < 0.02] = -1
    iou = (torch.rand(S, n, generator=gen) * 0.6).float()
    lab, iou = lab.to(dev), iou.to(dev)
    num = torch.full((S,), n, dtype=torch.int32, device=dev)
    smp = IoUBalancedNegSampler(max_num, pos_num, num_bins=3)
    ops.set_sampler_mode('device', seed=3)

    def iou_sampler():
        smp.sample(lab, iou, num, n, lists=True)

    def random_sampler():
        ops.sample_labels(lab, num, n, max_num, pos_num, lists=True)
    ti, tr, ai, ar = compare(iou_sampler, random_sampler, args.iters * 2, args.iters * 2, warmup=5)
    ops.set_sampler_mode('numpy')
    res['sampler'] = {'rows_per_image': n, 'images': S, 'max_num': max_num, 'pos_num': pos_num, 'num_bins': 3,
                      'iou_balanced_us': round(ti, 2), 'random_us': round(tr, 2), 'iou_balanced_runs_us': ai,
                      'random_runs_us': ar, 'note': 'host call to host call, output allocations included'}
    write_json(args.out, res)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
