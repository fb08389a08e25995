"""Per-level timing of frh_conv3x3_bias_act against the path it replaces.

    python tools/bench_conv3x3.py [--iters 20] [--out profiles/conv3x3/bench_conv3x3.json] [--fused-only]

For the nine 3x3 / stride-1 / 256 -> 256 convolutions of the cfg2 neck and RPN head (2 images
of 608 x 1024: P2 152x256, P3 76x128, P4 38x64, P5 19x32, P6 10x16; FPN form = bias, no ReLU,
on P2..P5; RPN form = bias + ReLU, shared weights, on P2..P6, P6 the ::2 view of P5) it times
  parent: what ran before -- the conv module (FPN form) or ops.conv_bias_relu (RPN form) with
          cudnn.benchmark warmed (MIOpen's search); the strided P6 view as the module gets it,
  fused:  the new entry (frh_conv3x3_bias_act: weight transform + Winograd kernel),
and, for the RPN form, all five levels in one frh_conv3x3_bias_act_levels call against the five
parent calls and against five fused calls (the weight transform's own time is in the kernel
statistics of tools/step_breakdown.py).  All under no_grad, `iters` calls back to back
behind a torch.cuda._sleep between one event pair, 3 repetitions with the sides alternating
(median reported), rotating over three sets of tensors so a call does not find its own output
in the caches.

Per level it prints us for both paths, the Winograd FLOPs (16 multiply-adds per 2 x 2 outputs
and channel pair), the algorithmic bytes (x, w read once, y written once) and the share of the
binding limit the fused call reaches, the limit being the larger of FLOPs / 157.3 TFLOP/s and
bytes / 8 TB/s."""
import argparse
import json
import os

import torch

from benchlib import REPO, limit, max_rel_diff, measure, require_gpu, write_json

N, C = 2, 256
LEVELS = [('P2', 152, 256), ('P3', 76, 128), ('P4', 38, 64), ('P5', 19, 32), ('P6', 10, 16)]
SETS = 3


def medians(sides, iters):
    return {k: s.median for k, s in measure(sides, iters, 3, warmup=2).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'conv3x3', 'bench_conv3x3.json'))
    ap.add_argument('--fused-only', action='store_true',
                    help='time only the fused entries (no MIOpen side, no search): for counter passes')
    args = ap.parse_args()
    require_gpu('bench_conv3x3')
    from frcnn_amd import _lib, ops
    from frcnn_amd.utils import conv_layout
    torch.backends.cudnn.benchmark = True
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    cl = torch.channels_last
    rows = []
    with torch.no_grad():
        conv = torch.nn.Conv2d(C, C, 3, padding=1).to(dev)
        conv_layout(conv)
        conv.bias.uniform_(-0.5, 0.5)
        ws = torch.empty(16 * C * C, device=dev)
        p = _lib.ptr

        def level_inputs(name, h, w):
            if name == 'P6':  # the ::2 view of a P5-sized level, as FPN.forward makes it
                return [torch.randn(N, C, 19, 32, device=dev).contiguous(memory_format=cl)[:, :, ::2, ::2]
                        for _ in range(SETS)]
            return [torch.randn(N, C, h, w, device=dev).contiguous(memory_format=cl) for _ in range(SETS)]

        def entry(x, y, relu):
            a = (p(x), p(conv.weight), p(conv.bias), p(y), p(ws), N, C, C, x.shape[2], x.shape[3], x.stride(0),
                 x.stride(2), x.stride(3), int(relu), _lib.stream_of(x))
            return lambda: _lib.call('frh_conv3x3_bias_act', *a)

        all_x = {}
        for name, h, w in LEVELS:
            xs = all_x[name] = level_inputs(name, h, w)
            ys = [torch.empty(N, C, h, w, device=dev).contiguous(memory_format=cl) for _ in range(SETS)]
            for form, relu in (('fpn', False), ('rpn', True)):
                if form == 'fpn' and name == 'P6':
                    continue
                if relu:
                    parent = [(lambda x=x: ops.conv_bias_relu(conv, x)) for x in xs]
                else:
                    parent = [(lambda x=x: conv(x)) for x in xs]
                sides = {'parent': parent, 'fused': [entry(x, y, relu) for x, y in zip(xs, ys)]}
                if args.fused_only:
                    del sides['parent']
                med = medians(sides, args.iters)
                med.setdefault('parent', float('nan'))
                maxdiff = float('nan')
                if not args.fused_only:
                    ref = parent[0]()
                    sides['fused'][0]()
                    maxdiff = max_rel_diff(ref, ys[0])
                flops = 2.0 * 16 * N * ((h + 1) // 2) * ((w + 1) // 2) * C * C
                nbytes = 4.0 * (2 * N * h * w * C + 9 * C * C)
                limit_us, bound = limit(flops, nbytes)
                row = {'level': name, 'h': h, 'w': w, 'form': form, 'excluded_in_ops': (h, w) in ops._CONV3X3_EXCLUDED,
                       'parent_us': round(med['parent'], 2), 'fused_us': round(med['fused'], 2),
                       'winograd_gflop': round(flops / 1e9, 3), 'direct_gflop': round(flops * 2.25 / 1e9, 3),
                       'algorithmic_MB': round(nbytes / 1e6, 2), 'limit': bound,
                       'limit_us': round(limit_us, 2), 'fused_share_of_limit': round(limit_us / med['fused'], 3),
                       'fused_winograd_TFLOPs': round(flops / med['fused'] / 1e6, 1),
                       'max_rel_diff_vs_parent': maxdiff}
                rows.append(row)
                print('{} {:3d}x{:3d} {}  parent {:8.2f} us  fused {:8.2f} us  limit {:7.2f} us ({}, {:.0%})  diff {:.1e}'
                      .format(name, h, w, form, med['parent'], med['fused'], limit_us, row['limit'],
                              row['fused_share_of_limit'], maxdiff), flush=True)

        # the RPN head: five parent calls against one multi-level call
        names = [l[0] for l in LEVELS]
        outs = [[torch.empty(N, C, h, w, device=dev).contiguous(memory_format=cl) for _, h, w in LEVELS]
                for _ in range(SETS)]

        def parent_all(i):
            return lambda: [ops.conv_bias_relu(conv, all_x[k][i]) for k in names]

        def levels_all(i):
            xs = [all_x[k][i] for k in names]
            a = (len(xs), _lib.ptr_array(xs), _lib.ptr_array([conv.weight] * 5), _lib.ptr_array([conv.bias] * 5),
                 _lib.ptr_array(outs[i]), p(ws), ws.numel() * 4, N, C, C,
                 _lib.i32_array([v for x in xs for v in x.shape[2:]]),
                 _lib.i64_array([v for x in xs for v in (x.stride(0), x.stride(2), x.stride(3))]), 1,
                 _lib.stream_of(xs[0]))
            return lambda: _lib.call('frh_conv3x3_bias_act_levels', *a)

        def per_level_all(i):
            fs = [entry(all_x[k][i], y, True) for k, y in zip(names, outs[i])]
            return lambda: [f() for f in fs]

        sides = {'parent': [parent_all(i) for i in range(SETS)], 'levels': [levels_all(i) for i in range(SETS)],
                 'per_level': [per_level_all(i) for i in range(SETS)]}
        if args.fused_only:
            del sides['parent']
        med = medians(sides, args.iters)
        med.setdefault('parent', float('nan'))
        head = {k + '_us': round(v, 2) for k, v in med.items()}
        print('RPN head, five levels: parent {parent_us} us, one launch {levels_us} us, five launches {per_level_us} us'
              .format(**head), flush=True)
        # the FPN's four output convs (one weight each): four parent calls against one launch
        convs = [torch.nn.Conv2d(C, C, 3, padding=1).to(dev) for _ in range(4)]
        for c in convs:
            conv_layout(c)
        ws4 = torch.empty(4 * 16 * C * C, device=dev)

        def fpn_parent(i):
            return lambda: [c(all_x[k][i]) for c, k in zip(convs, names)]

        def fpn_levels(i):
            xs = [all_x[k][i] for k in names[:4]]
            a = (4, _lib.ptr_array(xs), _lib.ptr_array([c.weight for c in convs]),
                 _lib.ptr_array([c.bias for c in convs]), _lib.ptr_array(outs[i][:4]), p(ws4), ws4.numel() * 4, N, C, C,
                 _lib.i32_array([v for x in xs for v in x.shape[2:]]),
                 _lib.i64_array([v for x in xs for v in (x.stride(0), x.stride(2), x.stride(3))]), 0,
                 _lib.stream_of(xs[0]))
            return lambda: _lib.call('frh_conv3x3_bias_act_levels', *a)

        sides = {'parent': [fpn_parent(i) for i in range(SETS)], 'levels': [fpn_levels(i) for i in range(SETS)]}
        if args.fused_only:
            del sides['parent']
        med = medians(sides, args.iters)
        med.setdefault('parent', float('nan'))
        neck = {k + '_us': round(v, 2) for k, v in med.items()}
        print('FPN output convs, four levels: parent {parent_us} us, one launch {levels_us} us'.format(**neck),
              flush=True)
    fpn = [r for r in rows if r['form'] == 'fpn']
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'batch': N, 'channels': C, 'levels': rows,
           'rpn_head_five_levels': head, 'fpn_outputs_four_levels': neck,
           'fpn_outputs_parent_us': round(sum(r['parent_us'] for r in fpn), 1),
           'fpn_outputs_fused_us': round(sum(r['fused_us'] for r in fpn), 1)}
    write_json(args.out, res)
    print(json.dumps({k: v for k, v in res.items() if k != 'levels'}))


if __name__ == '__main__':
    main()
