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

import torch

from benchlib import PEAK_BYTES, REPO, max_rel_diff, measure, put_times, require_gpu, wins, write_json

N, CIN, C_CLS, C_REG = 2, 256, 3, 12
LEVELS = ((152, 256), (76, 128), (38, 64), (19, 32), (10, 16))
SETS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'small_passes', 'bench_rpn_head1x1.json'))
    args = ap.parse_args()
    require_gpu('bench_rpn_head1x1')
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
        maxdiff = max_rel_diff(sides['parent'][0](), sides['fused'][0]())
        stat = measure(sides, args.iters, args.reps, warmup=2)
    pixels = N * sum(h * w for h, w in LEVELS)
    nbytes = 4.0 * (pixels * (CIN + C_CLS + C_REG) + CIN * (C_CLS + C_REG))
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'reps': args.reps, 'batch': N, 'cin': CIN,
           'c_cls': C_CLS, 'c_reg': C_REG, 'levels': LEVELS, 'max_rel_diff_vs_parent': maxdiff,
           'algorithmic_MB': round(nbytes / 1e6, 1), 'gflop': round(2.0 * pixels * CIN * (C_CLS + C_REG) / 1e9, 2)}
    put_times(res, stat, 1)
    res['fused_wins'] = wins(stat, 'fused', 'parent')
    res['fused_TBps'] = round(nbytes / stat['fused'][0] / 1e6, 2)
    res['fused_share_of_8TBps'] = round(nbytes / PEAK_BYTES * 1e6 / stat['fused'][0], 3)
    write_json(args.out, res)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
