"""Timing of the deformable 3x3 convolution's training path: forward + backward on the HIP entries
(hip_grad=True: frh_deform_conv3x3_act / _levels, then frh_deform_conv3x3_bwd per level) against
forward + backward of the torch restatement, the path taken without the flag.

    python tools/bench_deform_conv_bwd.py [--iters 12] [--reps 5] [--out profiles/ga_rpn_bwd/bench_deform_conv_bwd.json]

Workload and protocol as tools/bench_deform_conv.py: the GA-RPN adaption layer on the benchmark's
pyramid, 256 -> 256 channels, deformable_groups 4, batch 2, guided mode, the five level shapes and
the whole pyramid.  x, the weight and the offset layer's weight need gradients (the shape map is
detached in the head); upstream gradients are N(0, 1).  A call is the forward plus
torch.autograd.grad of its outputs.  `iters` calls (a quarter of it for the restatement) back to
back behind a torch.cuda._sleep between one event pair, rotating over two sets of tensors, `reps`
repetitions with the sides alternating; per side the median and the spread.  `hip_wins` is true
only when the HIP side's slowest repetition beats the restatement's fastest (benchlib.wins).  Per
side also torch.cuda.max_memory_allocated over one call, above what the inputs hold.

For the pyramid the HIP side is split further, each timed alone in the same way: the forward
(no_grad), the backward with only the weight wanting a gradient (weight launch + slab reduce) and
with only x and the offset weight wanting one (repack + data launch); the data launch is set
against its atomic floor (gx bytes added / 1.3 TB/s) and the weight launch against the forward,
which runs the same gather and FLOPs.

--step: also time the GA detector's forward_train + backward with GuidedAnchor.hip_grad off and
on (random weights, bench.py's batch), median of 5 synchronised calls after two warm-up calls,
into ga_train_step.json next to --out."""
import argparse
import json
import os
import time

import numpy as np
import torch

from benchlib import REPO, max_rel_diff, measure, on_path, put_times, require_gpu, wins, write_json

CIN = COUT = 256
DG = 4
BATCH = 2
LEVELS = [(152, 256), (76, 128), (38, 64), (19, 32), (10, 16)]
SETS = 2
ATOMIC_BYTES_PER_S = 1.3e12  # chip-wide float-atomic rate of added bytes


def peak_memory(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def train_step_times(dev, out_path):
    on_path()
    import bench
    from frcnn_amd.heads.guided_head import GuidedAnchor
    config = os.path.join(REPO, 'pytorch-faster-rcnn_amd', 'configs', 'ga_faster_rcnn_r50_fpn.py')
    model, _ = bench.make_model(dev, 0, config=config)
    batch = bench.make_batch(dev, BATCH, 0)
    res = {}
    for flag in (False, True):
        GuidedAnchor.hip_grad = flag
        ts = []
        for i in range(7):
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sum(model.forward_train(*batch).values()).backward()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        key = 'hip_grad_on' if flag else 'hip_grad_off'
        res[key] = {'ms_median': round(float(np.median(ts[2:])), 2),
                    'ms_min_max': [round(min(ts[2:]), 2), round(max(ts[2:]), 2)]}
        print(key, res[key], flush=True)
    GuidedAnchor.hip_grad = False
    res.update(device=torch.cuda.get_device_name(0), config='configs/ga_faster_rcnn_r50_fpn.py',
               step='forward_train + backward, batch 2, 608 x 1024, median of 5 synchronised calls after 2 warm-up calls')
    write_json(out_path, res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=12, help='calls per timed window (a quarter of it for the restatement)')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--step', action='store_true', help='also time the GA train step with the flag off and on')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'ga_rpn_bwd', 'bench_deform_conv_bwd.json'))
    args = ap.parse_args()
    require_gpu('bench_deform_conv_bwd')
    from frcnn_amd import ops
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    cl = torch.channels_last
    w = (torch.randn(COUT, CIN, 3, 3, device=dev) * 0.02).requires_grad_(True)
    ow = (torch.randn(18 * DG, 2, device=dev) * 0.1).requires_grad_(True)
    xs = [[torch.randn(BATCH, CIN, h, wd, device=dev).contiguous(memory_format=cl).requires_grad_(True)
           for h, wd in LEVELS] for _ in range(SETS)]
    ss = [[torch.randn(BATCH, 2, h, wd, device=dev).contiguous(memory_format=cl) for h, wd in LEVELS]
          for _ in range(SETS)]
    gys = [[torch.randn(BATCH, COUT, h, wd, device=dev).contiguous(memory_format=cl) for h, wd in LEVELS]
           for _ in range(SETS)]

    excluded = set(ops._DEFORM_BWD_EXCLUDED)
    ops._DEFORM_BWD_EXCLUDED.clear()  # every shape is timed on the HIP entries; the row says what ops does with it

    def step(i, ls, hip, relu=True):
        """forward + backward of levels ls of set i."""
        def run():
            x = [xs[i][l] for l in ls]
            ys = ops.deform_conv3x3_levels(x, [ss[i][l] for l in ls], w, DG, relu=relu, offset_weight=ow, hip_grad=hip)
            return torch.autograd.grad(ys, [w, ow] + x, [gys[i][l] for l in ls])
        return run

    def backward_only(i, ls, weight_side):
        """The backward alone, of a forward in which only the weight (weight_side), or only x and the
        offset weight, need a gradient: the entry then runs only that side's launches."""
        x = [xs[i][l].detach() if weight_side else xs[i][l] for l in ls]
        w_, ow_ = (w, ow.detach()) if weight_side else (w.detach(), ow)
        ys = ops.deform_conv3x3_levels(x, [ss[i][l] for l in ls], w_, DG, relu=True, offset_weight=ow_, hip_grad=True)
        return lambda: torch.autograd.grad(ys, [w] if weight_side else [ow] + x, [gys[i][l] for l in ls],
                                           retain_graph=True)

    rows = []
    n_torch = max(1, args.iters // 4)
    for tag, ls in [('{}x{}'.format(h, wd), [l]) for l, (h, wd) in enumerate(LEVELS)] + [('pyramid', list(range(5)))]:
        sides = {'hip': [step(i, ls, True) for i in range(SETS)], 'torch': [step(i, ls, False) for i in range(SETS)]}
        # the gradients of the two paths without ReLU: with it, an output within rounding of 0 has
        # its mask flipped between the two forwards, which is no property of the backward
        a, b = step(0, ls, True, relu=False)(), step(0, ls, False, relu=False)()
        row = {'shape': tag, 'positions': BATCH * sum(LEVELS[l][0] * LEVELS[l][1] for l in ls),
               'max_rel_diff_vs_torch_no_relu': max_rel_diff(list(b), list(a)),
               'excluded_in_ops': len(ls) == 1 and (CIN, COUT, BATCH) + LEVELS[ls[0]] in excluded}
        del a, b
        row['hip_peak_MiB'] = peak_memory(sides['hip'][0])
        row['torch_peak_MiB'] = peak_memory(sides['torch'][0])
        stat = measure(sides, {'hip': args.iters, 'torch': n_torch}, args.reps, warmup=1, reverse=True)
        put_times(row, stat, 1)['hip_wins'] = wins(stat, 'hip', 'torch')
        rows.append(row)
        print(row, flush=True)

    ls = list(range(5))
    def forward(i):
        def run():
            with torch.no_grad():
                return ops.deform_conv3x3_levels(xs[i], ss[i], w, DG, relu=True, offset_weight=ow)
        return run

    parts = {'forward': [forward(i) for i in range(SETS)],
             'backward_weight': [backward_only(i, ls, True) for i in range(SETS)],
             'backward_data': [backward_only(i, ls, False) for i in range(SETS)]}
    stat = measure(parts, args.iters, args.reps, warmup=1)
    positions = BATCH * sum(h * wd for h, wd in LEVELS)
    floor_us = positions * CIN * 36 * 4 / ATOMIC_BYTES_PER_S * 1e6
    split = put_times({'gx_atomic_bytes': positions * CIN * 36 * 4, 'atomic_floor_us': round(floor_us, 1)}, stat, 1)
    split['backward_data_over_atomic_floor'] = round(stat['backward_data'][0] / floor_us, 2)
    split['backward_weight_over_forward'] = round(stat['backward_weight'][0] / stat['forward'][0], 2)
    print(split, flush=True)
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'torch_iters': n_torch, 'reps': args.reps,
           'cin': CIN, 'cout': COUT, 'deformable_groups': DG, 'batch': BATCH, 'shapes': rows, 'pyramid_split': split}
    write_json(args.out, res)
    print(json.dumps(res))
    if args.step:
        train_step_times(dev, os.path.join(os.path.dirname(os.path.abspath(args.out)), 'ga_train_step.json'))


if __name__ == '__main__':
    main()
