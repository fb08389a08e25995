"""VGG16's convolutions on the fused Winograd entries against the modules they replace.

    python tools/bench_vgg.py [--iters 5] [--reps 5] [--out profiles/vgg16/bench_vgg.json]

For a batch of 2 images of 608 x 1024, under no_grad:
  classes: per dispatch class (cin, cout, pool) of frcnn_amd.ops._VGG_CONV_EXCLUDED -- the stem as
          (3, 64, False) -- every layer of the class at its grid, as one forward runs them
          (conv5's three layers and conv4_2 share (512, 512, False)):
            fused:   ops.vgg_conv / ops.vgg_stem with every class dispatched,
            modules: what they run otherwise on the same channels-last input: the MIOpen NHWC
                     conv, frh_bias_act_nhwc (ops.conv_bias_relu), F.max_pool2d; the stem's module
                     and a ReLU on the NCHW image;
          benchlib.wins(stat, 'fused', 'modules') decides the class, benchlib.limit gives its floor
          (Winograd FLOPs: 16 multiply-adds per 2 x 2 outputs and channel pair, the stem at its
          padded cin of 8; bytes: x and w read once, y -- pooled where it is -- written once);
  trunk:  VGG16.forward, fused against modules (ops.vgg_conv_fused_ok forced false);
  detector: forward_test of configs/faster_rcnn_vgg16.py (bench.make_model), both ways, img/s.
cudnn.benchmark is on and every side is warmed, so MIOpen's search (at most --conv-search-iterations
configurations per solver, bench.py's default) is done before the clock runs.  Windows of `iters`
calls behind a torch.cuda._sleep between one event pair, `reps` repetitions, the sides' order
reversed on the odd ones, inputs rotating over two sets."""
import argparse
import json
import os

import torch
import torch.nn.functional as F

from benchlib import REPO, limit, measure, on_path, put_times, require_gpu, wins, write_json

N, H, W = 2, 608, 1024
SETS = 2
# (cin, cout, pool) -> [(h, w) of every layer of the class in one forward]
CLASSES = [
    ((3, 64, False), [(608, 1024)]),
    ((64, 64, True), [(608, 1024)]),
    ((64, 128, False), [(304, 512)]),
    ((128, 128, True), [(304, 512)]),
    ((128, 256, False), [(152, 256)]),
    ((256, 256, False), [(152, 256)]),
    ((256, 256, True), [(152, 256)]),
    ((256, 512, False), [(76, 128)]),
    ((512, 512, False), [(76, 128), (38, 64), (38, 64), (38, 64)]),
    ((512, 512, True), [(76, 128)]),
]


def class_limit(cin, cout, pool, grids):
    kin = max(cin, 8)
    flops = sum(2.0 * 16 * N * ((h + 1) // 2) * ((w + 1) // 2) * kin * cout for h, w in grids)
    nbytes = sum(4.0 * (N * h * w * cin + N * (h // 2 if pool else h) * (w // 2 if pool else w) * cout
                        + 9 * cin * cout) for h, w in grids)
    return flops, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--conv-search-iterations', type=int, default=32)
    ap.add_argument('--skip-detector', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'vgg16', 'bench_vgg.json'))
    args = ap.parse_args()
    require_gpu('bench_vgg')
    if args.conv_search_iterations > 0:
        os.environ.setdefault('MIOPEN_DEBUG_TUNING_ITERATIONS_MAX', str(args.conv_search_iterations))
    from frcnn_amd import ops
    from frcnn_amd.backbones import VGG16
    from frcnn_amd.utils import conv_layout
    torch.backends.cudnn.benchmark = True
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    cl = torch.channels_last
    shipped = ops._VGG_CONV_EXCLUDED
    fused_ok = ops.vgg_conv_fused_ok
    ops._VGG_CONV_EXCLUDED = frozenset()  # the fused side: every class dispatched

    def no_fused(fn):
        def run():
            ops.vgg_conv_fused_ok = lambda conv, x, pool: False
            try:
                return fn()
            finally:
                ops.vgg_conv_fused_ok = fused_ok
        return run

    rows = []
    with torch.no_grad():
        for (cin, cout, pool), grids in CLASSES:
            conv = torch.nn.Conv2d(cin, cout, 3, padding=1).to(dev)
            conv_layout(conv)
            conv.bias.uniform_(-0.5, 0.5)
            if cin == 3:
                sets = [[torch.randn(N, 3, h, w, device=dev) for h, w in grids] for _ in range(SETS)]
                fused = [(lambda xs=xs: [ops.vgg_stem(conv, x) for x in xs]) for xs in sets]
                modules = [(lambda xs=xs: [torch.relu(conv(x)) for x in xs]) for xs in sets]
            else:
                sets = [[torch.randn(N, cin, h, w, device=dev).contiguous(memory_format=cl) for h, w in grids]
                        for _ in range(SETS)]
                fused = [(lambda xs=xs: [ops.vgg_conv(conv, x, pool) for x in xs]) for xs in sets]

                def module_side(xs):
                    ys = [ops.conv_bias_relu(conv, x) for x in xs]
                    return [F.max_pool2d(y, 2) for y in ys] if pool else ys
                modules = [(lambda xs=xs: module_side(xs)) for xs in sets]
            got, ref = fused[0](), modules[0]()
            diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, ref))
            del got, ref
            stat = measure({'fused': fused, 'modules': modules}, args.iters, args.reps, warmup=2, reverse=True)
            flops, nbytes = class_limit(cin, cout, pool, grids)
            limit_us, bound = limit(flops, nbytes)
            row = put_times({'class': [cin, cout, pool], 'grids': grids, 'fused_wins': wins(stat, 'fused', 'modules'),
                             'excluded_in_ops': (cin, cout, pool) in shipped, 'limit': bound,
                             'limit_us': round(limit_us, 1), 'winograd_gflop': round(flops / 1e9, 2),
                             'algorithmic_MB': round(nbytes / 1e6, 1),
                             'fused_share_of_limit': round(limit_us / stat['fused'].median, 3),
                             'max_rel_diff_vs_modules': diff}, stat, 1)
            rows.append(row)
            print('{!s:18} fused {:8.1f} us [{:.1f}, {:.1f}]  modules {:8.1f} us [{:.1f}, {:.1f}]  limit {:7.1f} us '
                  '({})  wins {}  diff {:.1e}'.format((cin, cout, pool), *stat['fused'][:3], *stat['modules'][:3],
                                                      limit_us, bound, row['fused_wins'], diff), flush=True)
            del sets, fused, modules
            torch.cuda.empty_cache()

        # the whole trunk
        model = VGG16(pretrained=False)
        model.init_weights()
        model = model.to(dev).eval()
        imgs = [torch.randn(N, 3, H, W, device=dev) for _ in range(SETS)]
        fused = [(lambda x=x: model(x)) for x in imgs]
        modules = [no_fused(lambda x=x: model(x)) for x in imgs]
        stat = measure({'fused': fused, 'modules': modules}, args.iters, args.reps, warmup=2, reverse=True)
        trunk = put_times({'fused_wins': wins(stat, 'fused', 'modules'),
                           'limit_us': round(sum(r['limit_us'] for r in rows), 1)}, stat, 1)
        print('trunk: fused {fused_us} us {fused_us_min_max}, modules {modules_us} us {modules_us_min_max}'
              .format(**trunk), flush=True)
        del model, fused, modules
        torch.cuda.empty_cache()

        detector = None
        if not args.skip_detector:
            on_path()
            import bench
            from frcnn_amd import set_sampler_mode
            set_sampler_mode('device', seed=3)
            det, _ = bench.make_model(dev, seed=0, config=os.path.join(REPO, 'pytorch-faster-rcnn_amd', 'configs',
                                                                       'faster_rcnn_vgg16.py'))
            det.eval()
            batches = [bench.make_batch(dev, N, seed=s) for s in range(SETS)]
            fused = [(lambda b=b: det.forward_test(b[0], b[3])) for b in batches]
            modules = [no_fused(lambda b=b: det.forward_test(b[0], b[3])) for b in batches]
            stat = measure({'fused': fused, 'modules': modules}, args.iters, args.reps, warmup=2, reverse=True,
                           sleep=False)
            detector = put_times({'fused_wins': wins(stat, 'fused', 'modules'),
                                  'fused_img_per_s': round(N * 1e6 / stat['fused'].median, 1),
                                  'modules_img_per_s': round(N * 1e6 / stat['modules'].median, 1)}, stat, 1)
            print('forward_test: fused {fused_img_per_s} img/s, modules {modules_img_per_s} img/s'.format(**detector),
                  flush=True)
    ops._VGG_CONV_EXCLUDED = shipped
    res = {'device': torch.cuda.get_device_name(0), 'batch': N, 'image': [H, W], 'iters': args.iters,
           'reps': args.reps, 'classes': rows, 'lost': [r['class'] for r in rows if not r['fused_wins']],
           'trunk': trunk, 'forward_test': detector}
    write_json(args.out, res)
    print(json.dumps({k: v for k, v in res.items() if k != 'classes'}))


if __name__ == '__main__':
    main()
