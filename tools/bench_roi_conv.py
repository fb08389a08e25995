"""Timing of frh_roi_conv3x3_bn_act against the path it replaces.

    python tools/bench_roi_conv.py [--iters 20] [--reps 7] [--out profiles/roi_conv/bench_roi_conv.json]

The Double-Head regression branch's layer, Conv2d(256, 256, 3, padding=1, bias=False) +
BatchNorm2d + ReLU over r RoI tiles [r, 256, 7, 7], for r = 512, 1000 (one image's proposals)
and 2000 (the benchmark's two).  Per r it times
  parent: relu(bn(conv(x))) on PyTorch-ROCm (cudnn.benchmark warmed: MIOpen), eval mode,
  fused:  ops.roi_conv3x3_bn_act's entry (frh_roi_conv3x3_bn_act: weight repack + convolution),
both under no_grad, `iters` calls back to back behind a torch.cuda._sleep between one event
pair, `reps` repetitions with the sides alternating, rotating over three sets of tensors so a
call does not find its own output in the caches.  Reported per side: the median, and the
spread (min and max over the repetitions).  `fused_wins` is true only when the fused side's
slowest repetition beats the parent's fastest.

Also per r: FLOPs (2 x r x 49 x 2304 x 256, the zero-padded border taps counted as the dense
layer counts them), the fused entry's achieved TFLOP/s and its share of the 157.3 TFLOP/s
f32-matrix peak (a whole-call rate: both launches)."""
import argparse
import json
import os

import torch

from benchlib import PEAK_FLOPS, REPO, max_rel_diff, measure, put_times, require_gpu, wins, write_json

CIN = COUT = 256
ROIS = (512, 1000, 2000)
SETS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'roi_conv', 'bench_roi_conv.json'))
    args = ap.parse_args()
    require_gpu('bench_roi_conv')
    from frcnn_amd import _lib, ops
    torch.backends.cudnn.benchmark = True
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    p = _lib.ptr
    rows = []
    with torch.no_grad():
        conv = torch.nn.Conv2d(CIN, COUT, 3, padding=1, bias=False).to(dev)
        bn = torch.nn.BatchNorm2d(COUT).to(dev).eval()
        bn.running_var.uniform_(0.5, 2.0)
        bn.running_mean.uniform_(-1, 1)
        ws = torch.empty(_lib.query('frh_roi_conv3x3_workspace', CIN, COUT) // 4, dtype=torch.float32, device=dev)
        for r in ROIS:
            xs = [torch.randn(r, CIN, 7, 7, device=dev) for _ in range(SETS)]
            ys = [torch.empty(r, COUT, 7, 7, device=dev) for _ in range(SETS)]

            def parent(i):
                return lambda: torch.relu(bn(conv(xs[i])))

            def entry(i):
                a = (p(xs[i]), p(conv.weight), p(ys[i]), p(bn.weight), p(bn.bias), p(bn.running_mean),
                     p(bn.running_var), float(bn.eps), r, CIN, COUT, 1, p(ws), _lib.stream_of(xs[i]))
                return lambda: _lib.call('frh_roi_conv3x3_bn_act', *a)
            sides = {'parent': [parent(i) for i in range(SETS)], 'fused': [entry(i) for i in range(SETS)]}
            stat = measure(sides, args.iters, args.reps, warmup=2)
            ref = sides['parent'][0]()
            sides['fused'][0]()
            maxdiff = max_rel_diff(ref, ys[0])
            flops = 2.0 * r * 49 * 9 * CIN * COUT
            row = {'r': r, 'cin': CIN, 'cout': COUT, 'gflop': round(flops / 1e9, 2),
                   'fused_in_ops': bool(ops.roi_conv3x3_fused_ok(conv, bn, xs[0])),
                   'max_rel_diff_vs_parent': maxdiff}
            put_times(row, stat, 1)['fused_wins'] = wins(stat, 'fused', 'parent')
            row['fused_TFLOPs'] = round(flops / stat['fused'][0] / 1e6, 1)
            row['fused_share_of_f32_matrix_peak'] = round(flops / stat['fused'][0] / 1e6 / (PEAK_FLOPS / 1e12), 3)
            rows.append(row)
            print('r {:5d}  parent {:8.1f} us [{:.1f}, {:.1f}]  fused {:8.1f} us [{:.1f}, {:.1f}]  {:.1f} TFLOP/s '
                  '({:.0%} of peak)  wins {}'.format(r, *stat['parent'][:3], *stat['fused'][:3], row['fused_TFLOPs'],
                                                     row['fused_share_of_f32_matrix_peak'], row['fused_wins']),
                  flush=True)
            del xs, ys
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'reps': args.reps, 'shapes': rows}
    write_json(args.out, res)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
