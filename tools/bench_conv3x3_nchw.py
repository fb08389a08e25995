"""Per-class timing of frh_conv3x3_nchw_bn_act against the path it replaces.

    python tools/bench_conv3x3_nchw.py [--out profiles/bottleneck_conv3x3/bench_conv3x3_nchw.json]
                                       [--parent-lib PATH/libfrcnn_amd.so] [--iters N --reps R --sides form1,form3]

For every stride-1 3x3 convolution class of the cfg2 trunk (ResNet-50 conv2, 2 images of
608 x 1024; cin -> cout @ h x w with its count per step) it times
  parent: F.conv2d (cudnn.benchmark warmed: MIOpen's search), followed by frh_bn_act (bn2 + ReLU)
          where the entry's epilogue replaces that pass (stage 4, whose conv3 does not take bn2
          on its input side);
  fused:  frh_conv3x3_nchw_bn_act with the product's form choice, weight transform included;
  parent_lib: frh_conv3x3_nchw_bn_act of another build loaded beside this one (--parent-lib: the
          parent commit's library, built from a clean export);
  formK:  every kernel form (FORMS) through the tools library (tools/build_tools.py),
under no_grad, 20 calls back to back behind a torch.cuda._sleep between one event pair, three
tensor sets in rotation, 7 repetitions with the sides alternating; median with [min, max].  A
class is dispatched only when the fused side's slowest repetition beats the parent's fastest.
The limit is the larger of Winograd FLOPs (16 multiply-adds per 2 x 2 outputs and channel pair)
/ 157.3 TFLOP/s and algorithmic bytes (x, w read once, y written once) / 8 TB/s."""
import argparse
import ctypes
import json
import os
import sys

import torch
import torch.nn.functional as F

from benchlib import REPO, limit, max_rel_diff, measure, put_times, require_gpu, wins, write_json

N = 2
# (cin = cout, h, w, launches per step, bn2 + ReLU in the epilogue, where)
CLASSES = [
    (64, 152, 256, 3, False, 'stage 1 conv2'),
    (128, 76, 128, 3, False, 'stage 2 conv2'),
    (256, 38, 64, 5, False, 'stage 3 conv2'),
    (512, 19, 32, 2, True, 'stage 4 conv2'),
]
SETS, ITERS, REPS = 3, 20, 7
# 0 .. 2: (NT, NC), one wave per work item; 3, 4: cin split S over a workgroup of S x TR waves (the
# product's forms); 5 ..: the laboratory forms with U through LDS (tools/csrc/conv3x3_nchw_lab.hip)
FORMS = ['(2, 1)', '(1, 2)', '(1, 1)', 'NC1 S4 TR1', 'NC1 S2 TR2', 'NC2 S1 TR4 lds', 'NC1 S2 TR2 lds', 'NC1 S1 TR4 lds']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'bottleneck_conv3x3', 'bench_conv3x3_nchw.json'))
    ap.add_argument('--parent-lib', default=None, help="another build's libfrcnn_amd.so (the parent commit's, built "
                    "from a clean export): its frh_conv3x3_nchw_bn_act is timed as the side parent_lib")
    ap.add_argument('--iters', type=int, default=ITERS, help='calls per repetition')
    ap.add_argument('--reps', type=int, default=REPS)
    ap.add_argument('--sides', default='', help='comma-separated subset of parent,fused,form0.. (a counter pass '
                    'times few launches of few sides; the parent and fused sides are needed for the comparison fields)')
    args = ap.parse_args()
    require_gpu('bench_conv3x3_nchw')
    from frcnn_amd import _lib, ops
    try:
        import toolslib
        tools = toolslib.load()
    except (RuntimeError, OSError, AttributeError) as e:
        print('tools library unavailable ({}): forms not timed'.format(e), file=sys.stderr)
        tools = None
    plib = None
    if args.parent_lib:
        plib = ctypes.CDLL(os.path.abspath(args.parent_lib))
        plib.frh_conv3x3_nchw_bn_act.restype, plib.frh_conv3x3_nchw_bn_act.argtypes = \
            _lib.SIGNATURES['frh_conv3x3_nchw_bn_act']
    torch.backends.cudnn.benchmark = True
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    p = _lib.ptr
    rows = []
    with torch.no_grad():
        for c, h, w, count, epi, where in CLASSES:
            conv = torch.nn.Conv2d(c, c, 3, padding=1, bias=False).to(dev)
            bn = torch.nn.BatchNorm2d(c).to(dev).eval()
            bn.running_var.uniform_(0.5, 2.0)
            bn.running_mean.uniform_(-1, 1)
            bnp = (p(bn.weight), p(bn.bias), p(bn.running_mean), p(bn.running_var), float(bn.eps))
            nobn = (None, None, None, None, 0.0)
            xs = [torch.randn(N, c, h, w, device=dev) for _ in range(SETS)]
            ys = [torch.empty(N, c, h, w, device=dev) for _ in range(SETS)]
            yp = [torch.empty(N, c, h, w, device=dev) for _ in range(SETS)]
            ws = torch.empty(16 * c * c, device=dev)
            st = _lib.stream_of(xs[0])

            def parent(i):
                def run():
                    raw = F.conv2d(xs[i], conv.weight, padding=1)
                    if epi:
                        _lib.call('frh_bn_act', p(raw), None, p(yp[i]), *bnp, N, c, h * w, 1, st)
                    else:
                        yp[i] = raw
                return run

            def entry(i, form=None):
                a = (p(xs[i]), p(conv.weight), *(bnp if epi else nobn), p(ys[i]), p(ws), N, c, c, h, w, int(epi), st)
                if form is None:
                    return lambda: _lib.call('frh_conv3x3_nchw_bn_act', *a)
                if form == 'parent_lib':
                    def run_parent():
                        if plib.frh_conv3x3_nchw_bn_act(*a) != 0:
                            raise RuntimeError('the parent library\'s frh_conv3x3_nchw_bn_act failed')
                    return run_parent

                def run():
                    if tools.frh_conv3x3_nchw_bn_act_form(form, *a) != 0:
                        raise RuntimeError('frh_conv3x3_nchw_bn_act_form({}) failed'.format(form))
                return run
            sides = {'parent': [parent(i) for i in range(SETS)], 'fused': [entry(i) for i in range(SETS)]}
            if plib is not None:
                sides['parent_lib'] = [entry(i, 'parent_lib') for i in range(SETS)]
            if tools is not None:
                for f in range(len(FORMS)):
                    sides['form{}'.format(f)] = [entry(i, f) for i in range(SETS)]
            if args.sides:
                sides = {k: v for k, v in sides.items() if k in ('parent', 'fused', 'parent_lib') or k in args.sides.split(',')}
            stat = measure(sides, args.iters, args.reps, warmup=2)
            sides['parent'][0]()
            sides['fused'][0]()
            maxdiff = max_rel_diff(yp[0], ys[0])
            flops = 2.0 * 16 * N * c * c * ((h + 1) // 2) * ((w + 1) // 2)
            nbytes = 4.0 * (2 * N * c * h * w + 9 * c * c)
            limit_us, bound = limit(flops, nbytes)
            row = {'where': where, 'cin': c, 'cout': c, 'hw': [h, w], 'launches_per_step': count,
                   'bn_relu_epilogue': epi, 'excluded_in_ops': (c, c) in ops._CONV3X3_NCHW_EXCLUDED,
                   'fused_wins': wins(stat, 'fused', 'parent'),
                   'fused_beats_parent_lib': wins(stat, 'fused', 'parent_lib') if plib is not None else None,
                   'winograd_gflop': round(flops / 1e9, 3), 'algorithmic_MB': round(nbytes / 1e6, 2),
                   'limit': bound,
                   'limit_us': round(limit_us, 2), 'fused_share_of_limit': round(limit_us / stat['fused'][0], 3),
                   'parent_share_of_limit': round(limit_us / stat['parent'][0], 3),
                   'max_rel_diff_vs_parent': maxdiff}
            rows.append(put_times(row, stat, 1))
            print('{:14s} {:4d}->{:4d} @ {}x{} x{}  parent {:7.1f} [{:.1f}, {:.1f}]  fused {:7.1f} [{:.1f}, {:.1f}]  {}  '
                  'limit {:.1f} us  wins {}  diff {:.1e}'.format(
                      where, c, c, h, w, count, *stat['parent'][:3], *stat['fused'][:3],
                      {k: round(v[0], 1) for k, v in stat.items() if k.startswith('form')}, limit_us,
                      row['fused_wins'], maxdiff), flush=True)
            del xs, ys, yp
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'reps': args.reps, 'batch': N, 'forms': FORMS,
           'classes': rows,
           'per_step_parent_us': round(sum(r['parent_us'] * r['launches_per_step'] for r in rows), 1),
           'per_step_fused_us': round(sum(r['fused_us'] * r['launches_per_step'] for r in rows), 1)}
    write_json(args.out, res)
    print(json.dumps({k: v for k, v in res.items() if k != 'classes'}))


if __name__ == '__main__':
    main()
