"""Timing of the plain-FCOS kernels (csrc/fcos.hip) against the torch paths they replace.

    python tools/bench_fcos.py [--iters 200] [--out profiles/fcos/bench_fcos.json]

Shape: the config's (configs/fcos_r50_fpn.py) -- two images of 800x1333 padded to 800x1344, five
levels with strides 8..128 (22 400 cells per image, M = 44 800), C = 20; 8 and 40 random ground-
truth boxes per image; N(0, 1) class and centerness logits, ltrb predictions exp(N(0, 0.5)) times
the target scale.

(a) the target assignment (ops.fcos_assign, one launch for the batch) against the head's torch
    loop (FCOSHead.single_image_targets_torch per image: what forward_train ran before the kernel
    existed), on the same device tensors;
(b) the fused loss (ops.fcos_losses), forward + backward, against the module-by-module arm of
    FCOSHead.calc_loss_flat (FCOSHead.calc_loss_modules: the host read of the positive count, the
    boolean gathers and the three loss modules) on the targets of (a);
(c) the kernel launches (torch.profiler's device activity) and the device-to-host
    synchronisations (torch.cuda.set_sync_debug_mode('warn')) of one call of each path.

Every time is the mean of back-to-back calls between one HIP event pair after a warm-up, repeated
5 times with the two sides alternating (median reported, all runs kept); the torch target loop
runs a twentieth of the iterations (it takes milliseconds).  GB/s are the op's algorithmic bytes
over that time: the assignment writes 28 B per cell; the loss forward reads the class logits and
labels once plus the positives' predictions and targets, forward + backward the same twice plus
the three gradient tensors written once."""
import argparse
import json
import os

import numpy as np
import torch

from benchlib import PEAK_BYTES, REPO, compare, count_launches, count_syncs, on_path, require_gpu, write_json

on_path('tests', 'golden')

IMG_SHAPE, PAD = (800, 1333), (800, 1344)
STRIDES = [8, 16, 32, 64, 128]
GRIDS = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
B, C, REG_STD, REG_MEAN = 2, 20, 1200.0, 0.0
GT_COUNTS = (8, 40)


def row(th, tt, ah, at, nbytes):
    return {'hip_us': round(th, 2), 'torch_us': round(tt, 2), 'hip_runs_us': ah, 'torch_runs_us': at,
            'speedup': round(tt / th, 2), 'algorithmic_bytes': int(nbytes), 'hip_GBps': round(nbytes / th / 1e3, 1),
            'hip_fraction_of_8TBps': round(nbytes / th / 1e3 / (PEAK_BYTES / 1e9), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'fcos', 'bench_fcos.json'))
    args = ap.parse_args()
    require_gpu('bench_fcos')
    import inputs
    from frcnn_amd import ops
    from frcnn_amd.heads import fcos_head as head_mod
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    head = head_mod.FCOSHead(num_classes=C + 1, in_channels=8, stacked_convs=1, feat_channels=8, strides=STRIDES,
                             reg_std=REG_STD, reg_mean=REG_MEAN,
                             loss_cls=dict(type='FocalLoss', use_sigmoid=True, loss_weight=1.0),
                             loss_bbox=dict(type='GIoULoss', loss_weight=2.0),
                             loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0))
    metas = [{'img_shape': IMG_SHAPE + (3,), 'pad_shape': PAD + (3,), 'scale_factor': 1.0}] * B
    N = sum(h * w for h, w in GRIDS)
    M = B * N
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters,
           'shapes': {'images': B, 'image': list(IMG_SHAPE), 'padded': list(PAD), 'grids': GRIDS, 'M': M, 'classes': C}}
    for G in GT_COUNTS:
        gb = [torch.from_numpy(np.ascontiguousarray(inputs.random_boxes(900 + G + i, G, img=IMG_SHAPE, min_wh=16.0,
                                                                        max_wh=600.0))).to(dev) for i in range(B)]
        gl = [torch.from_numpy(np.random.default_rng(950 + G + i).integers(1, C + 1, G)).to(dev) for i in range(B)]

        def assign_hip():
            return head.targets_batched(GRIDS, gb, gl, metas)

        def assign_torch():
            return [head.single_image_targets_torch(GRIDS, gb[i], gl[i], metas[i]) for i in range(B)]
        cls_t, reg_t, ctr_t = assign_hip()
        per = assign_torch()
        same = all(torch.equal(torch.cat([x.reshape(-1) for x in per[i][0]]), cls_t[i]) and
                   torch.equal(torch.cat([x.reshape(-1, 4) for x in per[i][1]]), reg_t[i]) for i in range(B))
        ctr_diff = max(float((torch.cat([x.reshape(-1) for x in per[i][2]]) - ctr_t[i]).abs().max()) for i in range(B))
        labels, ltrb, ctrs = cls_t.view(-1), reg_t.view(-1, 4), ctr_t.view(-1)
        npos = int((labels > 0).sum())
        out = {'gts_per_image': G, 'positives': npos, 'ignored': int((labels < 0).sum()),
               'assign_labels_and_ltrb_equal_torch': bool(same), 'assign_largest_centerness_difference': ctr_diff}
        out['assign'] = row(*compare(assign_hip, assign_torch, args.iters, max(args.iters // 20, 3), warmup=3), 28 * M)
        out['assign']['note'] = 'torch: the per-image loop over gts and levels, two images'

        cls = torch.randn(C, M, device=dev, requires_grad=True)
        reg = ((ltrb.clamp(min=1.0) / REG_STD).t() * torch.exp(0.5 * torch.randn(4, M, device=dev))).contiguous()
        reg.requires_grad_(True)
        ctr = torch.randn(1, M, device=dev, requires_grad=True)

        def fwd_bwd(fn):
            def run():
                cls.grad = reg.grad = ctr.grad = None
                o = fn(cls, reg, ctr, labels, ltrb, ctrs)
                sum(o.values()).backward()
            return run
        with torch.no_grad():
            a = head.calc_loss_flat(cls, reg, ctr, labels, ltrb, ctrs)
            b = head.calc_loss_modules(cls, reg, ctr, labels, ltrb, ctrs)
        out['losses'] = {'hip': {k: float(v) for k, v in a.items()}, 'torch': {k: float(v) for k, v in b.items()}}
        fbytes = 4 * C * M + 8 * M + npos * (16 + 16 + 4 + 4)
        bbytes = 2 * fbytes + 4 * C * M + 16 * M + 4 * M
        hip, tor = fwd_bwd(head.calc_loss_flat), fwd_bwd(head.calc_loss_modules)
        out['loss_forward_backward'] = row(*compare(hip, tor, args.iters, max(args.iters // 4, 3), warmup=3), bbytes)
        out['loss_forward_backward']['note'] = ('includes the grad reset, the sum of the three losses and autograd on '
                                                'both sides')
        out['launches_and_syncs'] = {
            'assign': {'hip': [count_launches(assign_hip), count_syncs(assign_hip)],
                       'torch': [count_launches(assign_torch), count_syncs(assign_torch)]},
            'loss_forward_backward': {'hip': [count_launches(hip), count_syncs(hip)],
                                      'torch': [count_launches(tor), count_syncs(tor)]},
            'columns': ['device kernels per call (null: no device activity from the profiler)', 'host syncs per call']}
        res['gts_{}'.format(G)] = out
        print('gts', G, json.dumps(out), flush=True)
    write_json(args.out, res)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
