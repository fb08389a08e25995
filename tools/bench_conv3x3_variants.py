"""A/B of the Winograd 3x3 kernel's laboratory forms, the product kernel and a parent build.

    python tools/bench_conv3x3_variants.py --variants 16,116,14,114 [--parent-lib PATH/libfrcnn_amd.so]
                                           [--reps 7] [--iters 20] [--out FILE.json]

Sides: `product` (this tree's frh_conv3x3_bias_act_levels), `parent` (the same entry of another
build of the product library, loaded beside this one), and `v<variant>` (tools/csrc/
conv3x3_wino_lab.hip through the tools library; variant = 100 * DMA form + positions before the
barrier).  Launch shapes of the cfg2 step, 2 images of 608 x 1024, 256 -> 256 channels:
  p2    P2 152 x 256 alone (bias + ReLU),
  rpn5  the RPN head's shared conv on P2..P6 (P6 the ::2 view of a P5-sized level), one launch,
  fpn4  the FPN output convs on P2..P5, a weight per level, no ReLU, one launch.
Every side's output must equal the product's bit for bit before anything is timed.  Timing as
tools/bench_conv3x3.py (`iters` calls back to back behind a GPU hold between one event pair, three
tensor sets in rotation, the weight transform included); `reps` repetitions, the order of the
sides reversed on every other one; median [min, max] per side and shape."""
import argparse
import ctypes
import os

import torch

from benchlib import REPO, measure, require_gpu, write_json

N, C = 2, 256
LEVELS = [('P2', 152, 256), ('P3', 76, 128), ('P4', 38, 64), ('P5', 19, 32), ('P6', 10, 16)]
SETS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variants', default='16,116')
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'conv3x3_issue', 'bench_conv3x3_variants.json'))
    args = ap.parse_args()
    require_gpu('bench_conv3x3_variants')
    from frcnn_amd import _lib
    from frcnn_amd.utils import conv_layout
    import toolslib
    variants = [int(v) for v in args.variants.split(',') if v]
    tools = toolslib.load() if variants else None
    sig = _lib.SIGNATURES['frh_conv3x3_bias_act_levels']
    libs = {'product': _lib.load().frh_conv3x3_bias_act_levels}
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.frh_conv3x3_bias_act_levels.restype, parent.frh_conv3x3_bias_act_levels.argtypes = sig
        libs['parent'] = parent.frh_conv3x3_bias_act_levels
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    cl = torch.channels_last
    with torch.no_grad():
        convs = [torch.nn.Conv2d(C, C, 3, padding=1).to(dev) for _ in range(4)]
        for c in convs:
            conv_layout(c)
            c.bias.uniform_(-0.5, 0.5)
        ws = torch.empty(4 * 16 * C * C, device=dev)

        def level_x(name, h, w):
            if name == 'P6':
                return torch.randn(N, C, 19, 32, device=dev).contiguous(memory_format=cl)[:, :, ::2, ::2]
            return torch.randn(N, C, h, w, device=dev).contiguous(memory_format=cl)

        xs = [[level_x(*l) for l in LEVELS] for _ in range(SETS)]
        shapes = {'p2': (1, True, True), 'rpn5': (5, True, True), 'fpn4': (4, False, False)}

        def make(side, shape, i, outs):
            nlev, shared, relu = shapes[shape]
            x = xs[i][:nlev]
            wts = [convs[0].weight] * nlev if shared else [c.weight for c in convs[:nlev]]
            bs = [convs[0].bias] * nlev if shared else [c.bias for c in convs[:nlev]]
            a = (nlev, _lib.ptr_array(x), _lib.ptr_array(wts), _lib.ptr_array(bs), _lib.ptr_array(outs), _lib.ptr(ws),
                 ws.numel() * 4, N, C, C, _lib.i32_array([v for t in x for v in t.shape[2:]]),
                 _lib.i64_array([v for t in x for v in (t.stride(0), t.stride(2), t.stride(3))]), int(relu),
                 _lib.stream_of(ws))
            if side in libs:
                fn, full = libs[side], a
            else:
                fn, full = tools.frh_conv3x3_bias_act_levels_variant, (int(side[1:]), None) + a

            def run():
                if fn(*full) != 0:
                    raise RuntimeError('{} failed: {}'.format(side, _lib.load().frh_last_error().decode()))
            return run

        sides = list(libs) + ['v%d' % v for v in variants]
        res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'reps': args.reps, 'shapes': {}}
        for shape, (nlev, _, _) in shapes.items():
            outs = {s: [[torch.empty(N, C, h, w, device=dev).contiguous(memory_format=cl) for _, h, w in LEVELS[:nlev]]
                        for _ in range(SETS)] for s in sides}
            fns = {s: [make(s, shape, i, outs[s][i]) for i in range(SETS)] for s in sides}
            for s in sides:  # equal bits first
                for i in range(SETS):
                    for o in outs[s][i]:
                        o.fill_(float('nan'))
                    fns[s][i]()
            torch.cuda.synchronize()
            for s in sides:
                for i in range(SETS):
                    for o, want in zip(outs[s][i], outs['product'][i]):
                        if not torch.equal(o, want):
                            raise SystemExit('{} {}: output differs from the product kernel'.format(s, shape))
            row = {s: {'median_us': round(v.median, 2), 'min_us': round(v.min, 2), 'max_us': round(v.max, 2),
                       'all_us': [round(x, 2) for x in v.runs]}
                   for s, v in measure(fns, args.iters, args.reps, warmup=0, reverse=True).items()}
            res['shapes'][shape] = row
            print(shape, '  '.join('{} {:.1f} [{:.1f}, {:.1f}]'.format(s, r['median_us'], r['min_us'], r['max_us'])
                                   for s, r in row.items()), flush=True)
    write_json(args.out, res)


if __name__ == '__main__':
    main()
