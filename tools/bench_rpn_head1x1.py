"""Timing of frh_rpn_head1x1_levels against the path it replaces.

    python tools/bench_rpn_head1x1.py [--iters 20] [--reps 7] [--out profiles/small_passes/bench_rpn_head1x1.json]

The RPN head's classifier (256 -> 3) and regressor (256 -> 12) over the five cfg2 levels of two
608 x 1024 images (152 x 256 down to 10 x 16, channels-last).  It times
  parent: the ten module calls (nn.Conv2d with bias; cudnn.benchmark warmed: MIOpen / CK),
  fused:  ops.rpn_head1x1_levels' entry (one launch),
both under no_grad, `iters` calls back to back behind a torch.cuda._sleep between one event
pair, `reps` repetitions with the sides alternating, rotating over three sets of tensors so a
call does not find its own input in the caches.  Reported per side: the median and the spread
(min and max over the repetitions); `fused_wins` is true only when the fused side's slowest
repetition beats the parent's fastest.  Also the fused entry's bytes (every level read once,
both outputs written once, the weights once) and its share of 8 TB/s."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'pytorch-faster-rcnn_amd'))

N, CIN, C_CLS, C_REG = 2, 256, 3, 12
LEVELS = ((152, 256), (76, 128), (38, 64), (19, 32), (10, 16))
PEAK_BYTES = 8.0e12
SETS = 3


def time_calls(fns, iters):
    """us per call of fns[i % len(fns)], queued behind a sleep so the host runs ahead."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(100000000)
    e0.record()
    for i in range(iters):
        fns[i % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'small_passes', 'bench_rpn_head1x1.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_rpn_head1x1 needs a HIP device')
    from frcnn_amd import ops
    torch.backends.cudnn.benchmark = True
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    with torch.no_grad():
        classifier = torch.nn.Conv2d(CIN, C_CLS, 1).to(dev).to(memory_format=torch.channels_last)
        regressor = torch.nn.Conv2d(CIN, C_REG, 1).to(dev).to(memory_format=torch.channels_last)
        xs = [[torch.randn(N, CIN, h, w, device=dev).contiguous(memory_format=torch.channels_last) for h, w in LEVELS]
              for _ in range(SETS)]
        assert ops.rpn_head1x1_fused_ok(classifier, regressor, xs[0])

        def parent(i):
            return lambda: ([classifier(h) for h in xs[i]], [regressor(h) for h in xs[i]])

        def fused(i):
            return lambda: ops.rpn_head1x1_levels(classifier, regressor, xs[i])
        sides = {'parent': [parent(i) for i in range(SETS)], 'fused': [fused(i) for i in range(SETS)]}
        for fns in sides.values():
            for f in fns:
                f()
                f()
        torch.cuda.synchronize()
        ref, got = sides['parent'][0](), sides['fused'][0]()
        maxdiff = max(float((a - b).abs().max() / a.abs().max()) for r, g in zip(ref, got) for a, b in zip(r, g))
        t = {k: [] for k in sides}
        for _ in range(args.reps):
            for k, fns in sides.items():
                t[k].append(time_calls(fns, args.iters))
    stat = {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in t.items()}
    pixels = N * sum(h * w for h, w in LEVELS)
    nbytes = 4.0 * (pixels * (CIN + C_CLS + C_REG) + CIN * (C_CLS + C_REG))
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'reps': args.reps, 'batch': N, 'cin': CIN,
           'c_cls': C_CLS, 'c_reg': C_REG, 'levels': LEVELS, 'max_rel_diff_vs_parent': maxdiff,
           'algorithmic_MB': round(nbytes / 1e6, 1), 'gflop': round(2.0 * pixels * CIN * (C_CLS + C_REG) / 1e9, 2)}
    for k, (med, lo, hi) in stat.items():
        res[k + '_us'] = round(med, 1)
        res[k + '_us_min_max'] = [round(lo, 1), round(hi, 1)]
    res['fused_wins'] = stat['fused'][2] < stat['parent'][1]
    res['fused_TBps'] = round(nbytes / stat['fused'][0] / 1e6, 2)
    res['fused_share_of_8TBps'] = round(nbytes / PEAK_BYTES * 1e6 / stat['fused'][0], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
