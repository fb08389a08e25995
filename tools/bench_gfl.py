"""Timing of the GFL kernels (csrc/gfl.hip) against the torch path they replace.

    python tools/bench_gfl.py [--iters 200] [--out profiles/gfl/bench_gfl.json]

Shape: the config's (configs/fcos_r50_fpn_atss_gfl.py) -- two images of 800x1333 padded to
800x1344, five levels with strides 8..128 (22 400 positions per image, M = 44 800), C = 20,
16 bins; ATSS targets of two VOC ground-truth sets (tests/golden/voc_gts.npz) scaled into the
image; N(0, 1) logits.

(a) the fused loss (ops.gfl_losses), forward and forward + backward, against
    losses.gfl_head_losses_torch on the same device tensors -- the computation FCOSHead made
    before the kernel existed;
(b) the DFL decode (ops.dfl_decode) of both images' five channels-last levels, called per image
    and level as FCOSHead.image_candidates calls it, against the torch decode of that method;
(c) the kernel launches (torch.profiler's device activity) and the device-to-host
    synchronisations (torch.cuda.set_sync_debug_mode('warn')) of one call of each path.

Every time is the mean of `iters` back-to-back calls between one HIP event pair after a warm-up,
repeated 5 times with the two sides alternating (median reported, all runs kept).  GB/s are the
op's algorithmic bytes over that time: forward the class logits and labels once plus the
positives' regression logits and targets; backward the same again plus both gradient tensors
written once; decode the regression logits read and the boxes written once."""
import argparse
import json
import os

import numpy as np
import torch

from benchlib import PEAK_BYTES, REPO, compare, count_launches, count_syncs, on_path, require_gpu, write_json

on_path('tests', 'golden')

IMG = (800, 1344)
STRIDES = [8, 16, 32, 64, 128]
GRIDS = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
B, C, BINS, DFL_STRIDE, REG_STD, REG_MEAN = 2, 20, 16, 0.08, 1200.0, 0.0
KW = dict(bins=BINS, stride=DFL_STRIDE, reg_mean=REG_MEAN, reg_std=REG_STD, norm_prob=False, beta=2.0,
          cls_weight=1.0, dfl_weight=0.25, bbox_weight=2.0, dfl_avg_factor=4.0)


def row(th, tt, ah, at, nbytes):
    return {'hip_us': round(th, 2), 'torch_us': round(tt, 2), 'hip_runs_us': ah, 'torch_runs_us': at,
            'speedup': round(tt / th, 2), 'algorithmic_bytes': int(nbytes), 'hip_GBps': round(nbytes / th / 1e3, 1),
            'hip_fraction_of_8TBps': round(nbytes / th / 1e3 / (PEAK_BYTES / 1e9), 4)}


def torch_decode(head_mod, utils, r, cell, img_size):
    """FCOSHead.image_candidates' torch decode of one image's level r [4*bins, H, W]."""
    gs = r.shape[-2:]
    p = r.reshape(BINS, -1).t().softmax(-1)
    ltrb = head_mod.class2length(p, DFL_STRIDE) * REG_STD + REG_MEAN
    return utils.clamp_bbox(head_mod.ltrb2bbox(ltrb.view(4, *gs), cell).reshape(4, -1), img_size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'gfl', 'bench_gfl.json'))
    args = ap.parse_args()
    require_gpu('bench_gfl')
    import inputs
    from frcnn_amd import ops, utils
    from frcnn_amd.heads import fcos_head as head_mod
    from frcnn_amd.losses import gfl_head_losses_torch
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    head = head_mod.FCOSHead(num_classes=C + 1, in_channels=8, stacked_convs=1, feat_channels=8, strides=STRIDES,
                             reg_std=REG_STD, reg_mean=REG_MEAN, atss_cfg=dict(topk=9, scale=8),
                             loss_cls=dict(type='QualityFocalLoss', use_sigmoid=True, loss_weight=1.0),
                             loss_bbox=dict(type='GIoULoss', loss_weight=2.0),
                             loss_dfl=dict(type='DistributionFocalLoss', cls_channels=BINS, stride=DFL_STRIDE,
                                           norm_prob=False, loss_weight=0.25))
    gts = inputs.voc_gts()[:2]
    f = IMG[0] / float(inputs.IMG_SHAPE[0])
    gb = [torch.from_numpy(g[0] * np.float32(f)).to(dev) for g in gts]
    gl = [torch.from_numpy(g[1]).to(dev) for g in gts]
    metas = [{'img_shape': IMG + (3,), 'pad_shape': IMG + (3,), 'scale_factor': f}] * B
    cls_t, reg_t, _ = head.targets_atss_batched(GRIDS, gb, gl, metas, dev)
    labels, ltrb = cls_t.view(-1), reg_t.view(-1, 4).contiguous()
    M = labels.numel()
    npos = int((labels > 0).sum())
    cls = torch.randn(C, M, device=dev, requires_grad=True)
    reg = torch.randn(4 * BINS, M, device=dev, requires_grad=True)
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters,
           'shapes': {'images': B, 'image': list(IMG), 'grids': GRIDS, 'M': M, 'classes': C, 'bins': BINS,
                      'positives': npos, 'ignored': int((labels < 0).sum())}}

    with torch.no_grad():
        a = ops.gfl_losses(cls, reg, labels, ltrb, **KW)
        b = gfl_head_losses_torch(cls, reg, labels, ltrb, **KW)
    res['losses'] = {'hip': [float(v) for v in a[:3]], 'torch': [float(v) for v in b[:3]]}

    def fwd(fn):
        def run():
            with torch.no_grad():
                fn(cls, reg, labels, ltrb, **KW)
        return run

    def fwd_bwd(fn):
        def run():
            cls.grad = reg.grad = None
            out = fn(cls, reg, labels, ltrb, **KW)
            (out[0] + out[1] + out[2]).backward()
        return run
    fbytes = 4 * C * M + 8 * M + npos * (4 * 4 * BINS + 16 + 4 * C)
    bbytes = 2 * fbytes + 4 * C * M + 4 * 4 * BINS * M
    res['loss_forward'] = row(*compare(fwd(ops.gfl_losses), fwd(gfl_head_losses_torch), args.iters, args.iters, warmup=5), fbytes)
    half = max(args.iters // 2, 10)
    res['loss_forward_backward'] = row(*compare(fwd_bwd(ops.gfl_losses), fwd_bwd(gfl_head_losses_torch), half, half,
                                                warmup=5), bbytes)
    res['loss_forward_backward']['note'] = 'includes the grad reset, the sum of the three losses and autograd on both sides'

    levels = [torch.randn(B, 4 * BINS, h, w, device=dev).contiguous(memory_format=torch.channels_last)
              for h, w in GRIDS]

    def dec_hip():
        for i in range(B):
            for lv, s in zip(levels, STRIDES):
                ops.dfl_decode(lv[i].unsqueeze(0), BINS, DFL_STRIDE, REG_STD, REG_MEAN, s, IMG)

    def dec_torch():
        for i in range(B):
            for lv, s in zip(levels, STRIDES):
                torch_decode(head_mod, utils, lv[i], s, IMG)
    dbytes = (4 * 4 * BINS + 16) * M
    res['decode'] = row(*compare(dec_hip, dec_torch, args.iters, args.iters, warmup=5), dbytes)
    res['decode']['note'] = 'ten calls: two images x five levels, as FCOSHead.image_candidates decodes'
    err = max(float((ops.dfl_decode(lv[:1], BINS, DFL_STRIDE, REG_STD, REG_MEAN, s, IMG)[0]
                     - torch_decode(head_mod, utils, lv[0], s, IMG)).abs().max()) for lv, s in zip(levels, STRIDES))
    res['decode']['largest_difference_px'] = err

    res['launches_and_syncs'] = {
        'loss_forward': {'hip': [count_launches(fwd(ops.gfl_losses)), count_syncs(fwd(ops.gfl_losses))],
                         'torch': [count_launches(fwd(gfl_head_losses_torch)),
                                   count_syncs(fwd(gfl_head_losses_torch))]},
        'loss_forward_backward': {'hip': [count_launches(fwd_bwd(ops.gfl_losses)), count_syncs(fwd_bwd(ops.gfl_losses))],
                                  'torch': [count_launches(fwd_bwd(gfl_head_losses_torch)),
                                            count_syncs(fwd_bwd(gfl_head_losses_torch))]},
        'decode': {'hip': [count_launches(dec_hip), count_syncs(dec_hip)],
                   'torch': [count_launches(dec_torch), count_syncs(dec_torch)]},
        'columns': ['device kernels per call (null: no device activity from the profiler)', 'host syncs per call']}
    write_json(args.out, res)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
