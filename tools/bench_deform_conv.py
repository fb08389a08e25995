"""Timing of the fused deformable 3x3 convolution (frh_deform_conv3x3_act / _levels, guided mode)
against the torch restatement it replaces at inference and against a plain convolution.

    python tools/bench_deform_conv.py [--iters 60] [--reps 5] [--out profiles/ga_rpn/bench_deform_conv.json]

Workload: the GA-RPN adaption layer of configs/ga_faster_rcnn_r50_fpn.py on the benchmark's
pyramid, 256 -> 256 channels, deformable_groups 4, batch 2, the five level shapes (152, 256) ...
(10, 16): 103 680 positions, 122.3 GFLOP a call (2 x positions x 2304 x 256; a sample outside
the map is counted as the dense layer counts a padded tap).  Per level shape and for the whole
pyramid it times, under no_grad,
  hip:    ops.deform_conv3x3 / ops.deform_conv3x3_levels in guided mode (the offsets formed in
          the kernel from the 2-channel shape map; weight repack + convolution, + ReLU),
  torch:  what the dispatch takes otherwise: the offset layer's 1x1 conv, then
          ops.deform_conv3x3_torch (gather + matmul) with ReLU, on the GPU,
  conv:   relu(F.conv2d(x, w, padding=1)) on channels-last tensors (MIOpen, cudnn.benchmark
          warmed): a plain convolution of the same shape, the yardstick that exists without this
          kernel and the lower bound a gather-fed convolution can approach.
`iters` calls back to back behind a torch.cuda._sleep between one event pair, `reps` repetitions
with the sides alternating.  warm: the same tensors every call; cold: rotating over three sets of
tensors, so a call does not find its inputs or its own output in the caches.  Reported per side:
the median and the spread (min, max) over the repetitions.  `hip_wins` is true only when the HIP
side's slowest cold repetition beats the torch side's fastest.  Also the HIP call's achieved
TFLOP/s and its share of the 157.3 TFLOP/s f32-matrix peak (a whole-call rate: both launches)."""
import argparse
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from benchlib import PEAK_FLOPS, REPO, max_rel_diff, measure, put_times, require_gpu, wins, write_json

CIN = COUT = 256
DG = 4
BATCH = 2
LEVELS = [(152, 256), (76, 128), (38, 64), (19, 32), (10, 16)]
SETS = 3


def warm_and_cold(sides, iters, reps):
    """{'<side>_warm' / '<side>_cold': Stat}; sides: {name: ([fn per set], iters scale)}.  Per
    repetition and side a warm window (set 0 only) and then a cold one (the sets in rotation)."""
    windows, n = {}, {}
    for k, (fns, scale) in sides.items():
        base = max(1, iters // scale)
        windows[k + '_warm'], n[k + '_warm'] = fns[:1], base
        windows[k + '_cold'], n[k + '_cold'] = fns, max(base, len(fns))
    return measure(windows, n, reps, warmup=0)


def step_times(dev, reps):
    """ms per forward_test of configs/faster_rcnn_r50_fpn.py and of configs/ga_faster_rcnn_r50_fpn.py
    (bench.py's --config list is fixed and does not take the new one): random weights, eval, two
    N(0, 1) images padded to 608 x 1024, wall time around a synchronised call, median of reps
    after two warm-up calls.  The GA proposal path synchronises per level (mask indexing)."""
    import time
    from frcnn_amd.builder import build_module
    from frcnn_amd.config import Config
    out = {}
    img = torch.randn(BATCH, 3, 608, 1024, device=dev)
    metas = [{'img_shape': (600, 1000, 3), 'pad_shape': (608, 1024, 3), 'scale_factor': 1.0}] * BATCH
    for name in ('faster_rcnn_r50_fpn', 'ga_faster_rcnn_r50_fpn'):
        cfg = Config.fromfile(os.path.join(REPO, 'pytorch-faster-rcnn_amd', 'configs', name + '.py'))
        torch.manual_seed(1)
        model = build_module(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
        model.init_weights()
        model = model.to(dev).eval()
        ts = []
        with torch.no_grad():
            for i in range(reps + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.forward_test(img, metas)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = {'ms_median': round(float(np.median(ts[2:])), 2), 'ms_min_max': [round(min(ts[2:]), 2),
                                                                                     round(max(ts[2:]), 2)]}
        print(name, out[name], flush=True)
        del model
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--no-step', action='store_true', help='skip the forward_test step times')
    ap.add_argument('--iters', type=int, default=60,
                    help='calls per timed window (a third of it for the torch side): tens of ms a window')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'ga_rpn', 'bench_deform_conv.json'))
    args = ap.parse_args()
    require_gpu('bench_deform_conv')
    from frcnn_amd import ops
    torch.backends.cudnn.benchmark = True
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    cl = torch.channels_last
    rows = []
    with torch.no_grad():
        w = (torch.randn(COUT, CIN, 3, 3, device=dev) * 0.02)
        w_cl = w.contiguous(memory_format=cl)
        ow = torch.randn(18 * DG, 2, device=dev) * 0.1  # the head's init: offsets of a pixel or so
        xs = [[torch.randn(BATCH, CIN, h, wd, device=dev).contiguous(memory_format=cl) for h, wd in LEVELS]
              for _ in range(SETS)]
        ss = [[torch.randn(BATCH, 2, h, wd, device=dev).contiguous(memory_format=cl) for h, wd in LEVELS]
              for _ in range(SETS)]

        def hip(i, l):
            return lambda: ops.deform_conv3x3(xs[i][l], ss[i][l], w, DG, relu=True, offset_weight=ow)

        def torch_path(i, l):
            return lambda: ops.deform_conv3x3_torch(xs[i][l], F.conv2d(ss[i][l], ow.view(18 * DG, 2, 1, 1)), w, DG,
                                                    relu=True)

        def conv(i, l):
            return lambda: torch.relu(F.conv2d(xs[i][l], w_cl, padding=1))

        def report(tag, positions, stat, extra):
            flops = 2.0 * positions * 9 * CIN * COUT
            row = dict(extra, shape=tag, positions=positions, gflop=round(flops / 1e9, 2))
            put_times(row, stat, 1)['hip_wins'] = wins(stat, 'hip_cold', 'torch_cold')
            row['hip_over_conv_cold'] = round(stat['hip_cold'][0] / stat['conv_cold'][0], 2)
            row['hip_TFLOPs_cold'] = round(flops / stat['hip_cold'][0] / 1e6, 1)
            row['hip_share_of_f32_matrix_peak'] = round(flops / stat['hip_cold'][0] / 1e6 / (PEAK_FLOPS / 1e12), 3)
            rows.append(row)
            print(tag, {k: row[k] for k in ('hip_cold_us', 'hip_warm_us', 'torch_cold_us', 'conv_cold_us', 'hip_wins',
                                            'hip_over_conv_cold', 'hip_share_of_f32_matrix_peak')}, flush=True)

        for l, (h, wd) in enumerate(LEVELS):
            sides = {'hip': ([hip(i, l) for i in range(SETS)], 1), 'torch': ([torch_path(i, l) for i in range(SETS)], 3),
                     'conv': ([conv(i, l) for i in range(SETS)], 1)}
            for fns, _ in sides.values():
                for f in fns:
                    f()
            torch.cuda.synchronize()
            a, b = sides['hip'][0][0](), sides['torch'][0][0]()
            diff = max_rel_diff(b, a)
            fused = bool(ops.deform_conv3x3_fused_ok(xs[0][l], ss[0][l], w, DG, ow))
            del a, b
            report('{}x{}'.format(h, wd), BATCH * h * wd, warm_and_cold(sides, args.iters, args.reps),
                   {'fused_in_ops': fused, 'max_rel_diff_vs_torch': diff})

        sides = {
            'hip': ([(lambda i=i: ops.deform_conv3x3_levels(xs[i], ss[i], w, DG, relu=True, offset_weight=ow))
                     for i in range(SETS)], 1),
            'torch': ([(lambda i=i: [torch_path(i, l)() for l in range(len(LEVELS))]) for i in range(SETS)], 3),
            'conv': ([(lambda i=i: [conv(i, l)() for l in range(len(LEVELS))]) for i in range(SETS)], 1)}
        for fns, _ in sides.values():
            fns[0]()
        torch.cuda.synchronize()
        report('pyramid', BATCH * sum(h * wd for h, wd in LEVELS), warm_and_cold(sides, args.iters, args.reps),
               {'launches': 'one repack + one convolution for the five levels'})
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'reps': args.reps, 'cin': CIN, 'cout': COUT,
           'deformable_groups': DG, 'batch': BATCH, 'shapes': rows}
    if not args.no_step:
        res['forward_test_step'] = step_times(dev, args.reps)
    write_json(args.out, res)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
