"""Per-shape timing of frh_conv1x1_bn_act against the path it replaces.

    python tools/bench_conv1x1.py [--iters 40] [--out profiles/conv1x1/bench_conv1x1.json]

For every 1x1 / stride-1 convolution of the cfg2 trunk (ResNet-50, 2 images of 608 x 1024;
cin -> cout @ hw, with its count per step and its epilogue form) it times
  parent: F.conv2d (cudnn.benchmark warmed: MIOpen / Tensile) followed by ops.bn_act,
  fused:  ops.conv1x1_bn_act's entry (frh_conv1x1_bn_act, the product's step choice),
  steps:  both cin steps per barrier (16, 32), through the tools library (tools/build_tools.py),
all under no_grad, `iters` calls back to back behind a torch.cuda._sleep between one event
pair, 3 repetitions with the sides alternating (median reported), rotating over three sets of
tensors so a call does not find its own output in the caches.

Per shape it prints us for both paths, FLOPs, algorithmic bytes of the fused op (x, w, skip
read once, y written once) and the share of the binding limit the fused kernel reaches,
the limit being the larger of FLOPs / 157.3 TFLOP/s and bytes / 8 TB/s.  The weighted sums
are the per-step totals of the 33 launches.

    python tools/bench_conv1x1.py --mode pre [--out profiles/small_passes/bench_conv1x1_pre.json]
    python tools/bench_conv1x1.py --mode s2  [--out profiles/small_passes/bench_conv1x1_s2.json]

time the input-side forms of the same kernel against what they replace, 20 calls between the
event pair, 7 repetitions with the sides alternating, median with [min, max]; a side wins only
when its slowest repetition beats the other side's fastest:
  pre: the four conv3 classes; parent = frh_bn_act (bn2 + ReLU on conv2's raw output) then
       frh_conv1x1_bn_act; new = frh_conv1x1_bn_act_pre on the raw output.
  s2:  the three stride-2 projections; parent = F.conv2d stride 2 (MIOpen's search warmed) then
       frh_bn_act; new = frh_conv1x1_s2_bn_act."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

from benchlib import REPO, limit, max_rel_diff, measure, put_times, require_gpu, wins, write_json

N = 2
# (cin, cout, hw, launches per step, skip, relu, where)
SHAPES = [
    (64, 64, 38912, 1, False, True, 'stage 1 block 0 conv1'),
    (256, 64, 38912, 2, False, True, 'stage 1 conv1'),
    (64, 256, 38912, 1, False, False, 'stage 1 projection'),
    (64, 256, 38912, 3, True, True, 'stage 1 conv3'),
    (256, 128, 38912, 1, False, True, 'stage 2 block 0 conv1'),
    (512, 128, 9728, 3, False, True, 'stage 2 conv1'),
    (128, 512, 9728, 4, True, True, 'stage 2 conv3'),
    (512, 256, 9728, 1, False, True, 'stage 3 block 0 conv1'),
    (1024, 256, 2432, 5, False, True, 'stage 3 conv1'),
    (256, 1024, 2432, 6, True, True, 'stage 3 conv3'),
    (1024, 512, 2432, 1, False, True, 'stage 4 block 0 conv1'),
    (2048, 512, 608, 2, False, True, 'stage 4 conv1'),
    (512, 2048, 608, 3, True, True, 'stage 4 conv3'),
]
# conv3 (cin, cout, hw, launches per step): every one has the skip and the ReLU
PRE_SHAPES = [(64, 256, 38912, 3), (128, 512, 9728, 4), (256, 1024, 2432, 6), (512, 2048, 608, 3)]
# the stride-2 projections (cin, cout, input h, input w), one per step each
S2_SHAPES = [(256, 512, 152, 256), (512, 1024, 76, 128), (1024, 2048, 38, 64)]
SETS = 3


def _bn(c, dev):
    bn = torch.nn.BatchNorm2d(c).to(dev).eval()
    bn.running_var.uniform_(0.5, 2.0)
    bn.running_mean.uniform_(-1, 1)
    return bn


def _bn_ptrs(bn):
    from frcnn_amd import _lib
    return (_lib.ptr(bn.weight), _lib.ptr(bn.bias), _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var), float(bn.eps))


def input_forms(mode, out, iters=20, reps=7):
    """--mode pre / s2: the input-side forms against the launches they replace."""
    from frcnn_amd import _lib, ops
    torch.backends.cudnn.benchmark = True
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    p = _lib.ptr
    rows = []
    with torch.no_grad():
        for shape in (PRE_SHAPES if mode == 'pre' else S2_SHAPES):
            if mode == 'pre':
                cin, cout, hw, count = shape
                h, w, oh, ow = hw // 32, 32, hw // 32, 32
                stride = 1
            else:
                cin, cout, h, w = shape
                count, oh, ow, stride = 1, (h + 1) // 2, w // 2, 2
            conv = torch.nn.Conv2d(cin, cout, 1, stride=stride, bias=False).to(dev)
            bn, pre = _bn(cout, dev), _bn(cin, dev)
            xs = [torch.randn(N, cin, h, w, device=dev) for _ in range(SETS)]
            mids = [torch.empty(N, cin, h, w, device=dev) for _ in range(SETS)]
            sk = [torch.randn(N, cout, oh, ow, device=dev) if mode == 'pre' else None for _ in range(SETS)]
            ys = [torch.empty(N, cout, oh, ow, device=dev) for _ in range(SETS)]
            yp = [torch.empty(N, cout, oh, ow, device=dev) for _ in range(SETS)]
            st = _lib.stream_of(xs[0])

            def parent(i):
                if mode == 'pre':
                    def run():
                        _lib.call('frh_bn_act', p(xs[i]), None, p(mids[i]), *_bn_ptrs(pre), N, cin, h * w, 1, st)
                        _lib.call('frh_conv1x1_bn_act', p(mids[i]), p(conv.weight), p(sk[i]), p(yp[i]), *_bn_ptrs(bn), N,
                                  cin, cout, h * w, 1, st)
                    return run

                def run():
                    raw = F.conv2d(xs[i], conv.weight, stride=2)
                    _lib.call('frh_bn_act', p(raw), None, p(yp[i]), *_bn_ptrs(bn), N, cout, oh * ow, 0, st)
                return run

            def new(i):
                if mode == 'pre':
                    return lambda: _lib.call('frh_conv1x1_bn_act_pre', p(xs[i]), p(conv.weight), p(sk[i]), p(ys[i]),
                                             *_bn_ptrs(bn), *_bn_ptrs(pre), 1, N, cin, cout, h * w, 1, st)
                return lambda: _lib.call('frh_conv1x1_s2_bn_act', p(xs[i]), p(conv.weight), None, p(ys[i]),
                                         *_bn_ptrs(bn), N, cin, cout, h, w, 0, st)
            sides = {'parent': [parent(i) for i in range(SETS)], 'new': [new(i) for i in range(SETS)]}
            stat = measure(sides, iters, reps, warmup=2)
            maxdiff = max_rel_diff(yp[0], ys[0])
            row = {'cin': cin, 'cout': cout, 'input_hw': [h, w], 'launches_per_step': count,
                   'max_rel_diff_vs_parent': maxdiff, 'new_wins': wins(stat, 'new', 'parent'),
                   'parent_wins': wins(stat, 'parent', 'new')}
            rows.append(put_times(row, stat, 1))
            print('{} {:5d}->{:4d} @ {}x{} x{}  parent {:7.1f} us [{:.1f}, {:.1f}]  new {:7.1f} us [{:.1f}, {:.1f}]  '
                  'new wins {}  diff {:.1e}'.format(mode, cin, cout, h, w, count, *stat['parent'][:3], *stat['new'][:3],
                                                   row['new_wins'], maxdiff), flush=True)
            del xs, mids, sk, ys, yp
    res = {'device': torch.cuda.get_device_name(0), 'mode': mode, 'iters': iters, 'reps': reps, 'batch': N,
           'shapes': rows,
           'per_step_parent_us': round(sum(r['parent_us'] * r['launches_per_step'] for r in rows), 1),
           'per_step_new_us': round(sum(r['new_us'] * r['launches_per_step'] for r in rows), 1)}
    write_json(out, res)
    print(json.dumps({k: v for k, v in res.items() if k != 'shapes'}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--mode', default='stride1', choices=['stride1', 'pre', 's2'])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    require_gpu('bench_conv1x1')
    if args.mode != 'stride1':
        return input_forms(args.mode, args.out or os.path.join(REPO, 'profiles', 'small_passes',
                                                               'bench_conv1x1_{}.json'.format(args.mode)))
    args.out = args.out or os.path.join(REPO, 'profiles', 'conv1x1', 'bench_conv1x1.json')
    from frcnn_amd import _lib, ops
    try:
        import toolslib
        tools = toolslib.load()
    except (RuntimeError, OSError, AttributeError) as e:
        print('tools library unavailable ({}): cin steps not timed'.format(e), file=sys.stderr)
        tools = None
    torch.backends.cudnn.benchmark = True
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    p = _lib.ptr
    rows = []
    with torch.no_grad():
        for cin, cout, hw, count, skip, relu, where in SHAPES:
            h, w = hw // 32, 32
            assert h * w == hw, 'plane {} is not a multiple of 32'.format(hw)
            conv = torch.nn.Conv2d(cin, cout, 1, bias=False).to(dev)
            bn = torch.nn.BatchNorm2d(cout).to(dev).eval()
            bn.running_var.uniform_(0.5, 2.0)
            bn.running_mean.uniform_(-1, 1)
            xs = [torch.randn(N, cin, h, w, device=dev) for _ in range(SETS)]
            sk = [torch.randn(N, cout, h, w, device=dev) if skip else None for _ in range(SETS)]
            ys = [torch.empty(N, cout, h, w, device=dev) for _ in range(SETS)]

            def parent(i):
                return lambda: ops.bn_act(F.conv2d(xs[i], conv.weight), bn, skip=sk[i], relu=relu)

            def entry(i, tile=None):  # tile: the cin step, None = the product's choice
                a = (p(xs[i]), p(conv.weight), p(sk[i]), p(ys[i]), p(bn.weight), p(bn.bias), p(bn.running_mean),
                     p(bn.running_var), float(bn.eps), N, cin, cout, hw, int(relu), _lib.stream_of(xs[i]))
                if tile is None:
                    return lambda: _lib.call('frh_conv1x1_bn_act', *a)

                def run():
                    if tools.frh_conv1x1_bn_act_step(tile, *a) != 0:
                        raise RuntimeError('frh_conv1x1_bn_act_step({}) failed'.format(tile))
                return run
            sides = {'parent': [parent(i) for i in range(SETS)], 'fused': [entry(i) for i in range(SETS)]}
            if tools is not None:
                for t in (16, 32):
                    sides['step{}'.format(t)] = [entry(i, t) for i in range(SETS)]
            med = {k: s.median for k, s in measure(sides, args.iters, 3, warmup=2).items()}
            ref = sides['parent'][0]()
            sides['fused'][0]()
            maxdiff = max_rel_diff(ref, ys[0])
            flops = 2.0 * N * cin * cout * hw
            nbytes = 4.0 * (N * hw * (cin + cout * (2 if skip else 1)) + cin * cout)
            limit_us, bound = limit(flops, nbytes)
            row = {'where': where, 'cin': cin, 'cout': cout, 'hw': hw, 'launches_per_step': count, 'skip': skip,
                   'relu': relu, 'excluded_in_ops': (cin, cout) in ops._CONV1X1_EXCLUDED, 'parent_us': round(med['parent'], 2), 'fused_us': round(med['fused'], 2),
                   'steps_us': {k: round(v, 2) for k, v in med.items() if k.startswith('step')},
                   'gflop': round(flops / 1e9, 3), 'algorithmic_MB': round(nbytes / 1e6, 2),
                   'limit': bound, 'limit_us': round(limit_us, 2), 'fused_share_of_limit': round(limit_us / med['fused'], 3),
                   'fused_TFLOPs': round(flops / med['fused'] / 1e6, 1), 'fused_TBps': round(nbytes / med['fused'] / 1e6, 2),
                   'max_rel_diff_vs_parent': maxdiff}
            rows.append(row)
            print('{:24s} {:5d}->{:4d} @{:6d} x{}  parent {:8.2f} us  fused {:8.2f} us  {}  limit {:7.2f} us ({}, {:.0%})'
                  .format(where, cin, cout, hw, count, med['parent'], med['fused'], row['steps_us'], limit_us,
                          row['limit'], row['fused_share_of_limit']), flush=True)
            del xs, sk, ys
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'batch': N, 'shapes': rows,
           'per_step_parent_us': round(sum(r['parent_us'] * r['launches_per_step'] for r in rows), 1),
           'per_step_fused_us': round(sum(r['fused_us'] * r['launches_per_step'] for r in rows), 1)}
    write_json(args.out, res)
    print(json.dumps({k: v for k, v in res.items() if k != 'shapes'}))


if __name__ == '__main__':
    main()
