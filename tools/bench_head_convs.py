"""Timing of the one-stage heads' convolutions on the fused HIP entries against the modules.

    python tools/bench_head_convs.py [--iters 20] [--reps 9] [--out profiles/head_convs/bench_head_convs.json]

Two 608 x 1024 images over P3..P7 (76 x 128 down to 5 x 8, 256 channels, channels-last), VOC's 20
classes.  It times, under no_grad,
  tower:   one tower layer (256 -> 256, + ReLU) over the five levels: ops.conv3x3_bias_act_levels
           (frh_conv3x3_bias_act_levels, weight transform included) against the five module calls
           with their ReLU;
  outputs: each output group -- Retina's classifier (180) and regressor (36), FCOS's classifier
           (20) and regressor + centerness (4, 1; exp(conv * coef)), GFL's (64, 1; conv * coef) --
           as one frh_conv3x3_out_levels launch against the module expressions with their bias
           passes and the exp / multiply;
  forward: the whole forward of the four heads, as dispatched (ops._HEAD_CONVS_EXCLUDED as
           committed), with every part fused (the table emptied), and with the modules only.
cudnn.benchmark is on and every side is warmed, so MIOpen's search is done before the clock runs.
`iters` calls run back to back behind a torch.cuda._sleep between one event pair; `reps`
repetitions, the order of the sides reversed every other one; the calls rotate over SETS sets of
levels (more than the 256 MB of MALL), so no call finds its input in a cache.  Reported per side:
the median and [min, max] over the repetitions; `fused_wins` is true only when the fused side's
slowest repetition beat the modules' fastest, which is the rule the exclusion table follows.
Also each part's algorithmic bytes and direct-convolution FLOPs and the share of 8 TB/s and of
the 157.3 TFLOP/s f32 MFMA peak the fused side reaches."""
import argparse
import json
import os

import torch
from torch import nn

from benchlib import PEAK_BYTES, PEAK_FLOPS, REPO, max_rel_diff, measure, put_times, require_gpu, wins, write_json

N, CIN, CLASSES, BINS = 2, 256, 20, 16
LEVELS = ((76, 128), (38, 64), (19, 32), (10, 16), (5, 8))
SETS = 12
OUT_GROUPS = (('retina_cls', (9 * CLASSES,), None), ('retina_reg', (36,), None), ('fcos_cls', (CLASSES,), None),
              ('fcos_reg_ctr', (4, 1), 'exp'), ('gfl_reg_ctr', (4 * BINS, 1), 'mul'))


def timed_row(sides, iters, reps):
    """(stat, its row with fused_wins).  Every callable is warmed once and each side's first once
    more; the order of the sides is reversed every other repetition."""
    for fns in sides.values():
        for f in fns:
            f()
        fns[0]()
    torch.cuda.synchronize()
    stat = measure(sides, iters, reps, warmup=0, reverse=True)
    return stat, dict(put_times({}, stat, 1), fused_wins=wins(stat, 'fused', 'modules'))


def shares(res, nbytes, flops, us):
    res.update(algorithmic_MB=round(nbytes / 1e6, 1), gflop=round(flops / 1e9, 2),
               fused_share_of_8TBps=round(nbytes / PEAK_BYTES * 1e6 / us, 3),
               fused_share_of_f32_mfma_peak=round(flops / PEAK_FLOPS * 1e6 / us, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'head_convs', 'bench_head_convs.json'))
    args = ap.parse_args()
    require_gpu('bench_head_convs')
    from frcnn_amd import ops
    from frcnn_amd.heads.fcos_head import FCOSHead
    from frcnn_amd.heads.retina_head import RetinaHead
    torch.backends.cudnn.benchmark = True
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    shipped = ops._HEAD_CONVS_EXCLUDED
    pixels = N * sum(h * w for h, w in LEVELS)
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'reps': args.reps, 'batch': N, 'cin': CIN,
           'levels': LEVELS, 'sets': SETS, 'excluded_as_committed': sorted(map(list, shipped)), 'outputs': {}, 'forward': {}}
    conv_of = lambda c: nn.Conv2d(CIN, c, 3, padding=1).to(dev).to(memory_format=torch.channels_last)
    with torch.no_grad():
        xs = [[torch.randn(N, CIN, h, w, device=dev).contiguous(memory_format=torch.channels_last) for h, w in LEVELS]
              for _ in range(SETS)]

        # ---- one tower layer
        ops._HEAD_CONVS_EXCLUDED = frozenset()
        tower = conv_of(CIN)
        sides = {'modules': [lambda i=i: [torch.relu_(tower(x)) for x in xs[i]] for i in range(SETS)],
                 'fused': [lambda i=i: ops.conv3x3_bias_act_levels(tower, xs[i], relu=True) for i in range(SETS)]}
        stat, r = timed_row(sides, args.iters, args.reps)
        r['max_rel_diff_vs_modules'] = max_rel_diff(sides['modules'][0](), sides['fused'][0]())
        shares(r, 4.0 * (2 * pixels * CIN + 9 * CIN * CIN), 2.0 * pixels * 9 * CIN * CIN, stat['fused'][0])
        res['tower'] = r
        print('tower', json.dumps(r), flush=True)

        # ---- the output groups
        coef = torch.rand(len(LEVELS), device=dev) + 0.5
        for name, widths, epi in OUT_GROUPS:
            convs = [conv_of(c) for c in widths]
            if epi == 'exp':
                scale = coef.view(-1, 1).expand(-1, 4).contiguous()
            elif epi == 'mul':
                scale = (coef.view(-1, 1) * torch.ones(BINS, device=dev)).unsqueeze(2).expand(-1, -1, 4).reshape(len(LEVELS), -1)
            kw = dict(scales=[[scale[l] for l in range(len(LEVELS))]] + [None] * (len(convs) - 1),
                      exp=[epi == 'exp'] + [False] * (len(convs) - 1)) if epi else {}

            def modules(i, convs=convs, epi=epi, kw=kw):
                out = []
                for k, conv in enumerate(convs):
                    ys = [conv(x) for x in xs[i]]
                    if epi and k == 0:
                        ys = [y * s.view(-1, 1, 1) for y, s in zip(ys, kw['scales'][0])]
                        if epi == 'exp':
                            ys = [torch.exp(y) for y in ys]
                    out.append(ys)
                return out
            assert ops.conv3x3_out_fused_ok(convs, xs[0], kw.get('scales'))
            sides = {'modules': [lambda i=i: modules(i) for i in range(SETS)],
                     'fused': [lambda i=i, convs=convs, kw=kw: ops.conv3x3_out_levels(convs, xs[i], **kw)
                               for i in range(SETS)]}
            stat, r = timed_row(sides, args.iters, args.reps)
            ref, got = sides['modules'][0](), sides['fused'][0]()
            r['max_rel_diff_vs_modules'] = max_rel_diff(ref, got)
            c = sum(widths)
            shares(r, 4.0 * (pixels * (CIN + c) + 9 * CIN * c), 2.0 * pixels * 9 * CIN * c, stat['fused'][0])
            r['class'] = ['out', CIN, widths[0], widths[1] if len(widths) > 1 else 0]
            res['outputs'][name] = r
            print(name, json.dumps(r), flush=True)

        # ---- the whole forward of the four heads
        focal = dict(type='FocalLoss', use_sigmoid=True, loss_weight=1.0)
        giou = dict(type='GIoULoss', loss_weight=2.0)
        ctr = dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)
        atss = dict(topk=9, scale=8)
        fcos = dict(num_classes=CLASSES + 1, in_channels=CIN, stacked_convs=4, feat_channels=CIN, strides=[8, 16, 32, 64, 128],
                    loss_bbox=giou)
        heads = {
            'retinanet_r50_fpn': lambda: RetinaHead(CLASSES + 1, CIN, 4, CIN, loss_cls=focal,
                                                    loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0)),
            'fcos_r50_fpn': lambda: FCOSHead(loss_cls=focal, loss_centerness=ctr, **fcos),
            'fcos_r50_fpn_atss': lambda: FCOSHead(loss_cls=focal, loss_centerness=ctr, atss_cfg=atss, **fcos),
            'fcos_r50_fpn_atss_gfl': lambda: FCOSHead(
                loss_cls=dict(type='QualityFocalLoss', use_sigmoid=True, loss_weight=1.0), atss_cfg=atss,
                loss_dfl=dict(type='DistributionFocalLoss', cls_channels=BINS, stride=0.08, norm_prob=False,
                              loss_weight=0.25), **fcos)}
        real_ok = ops.head_convs_fused_ok

        def forward(head, i, table, fused_path=True):
            ops._HEAD_CONVS_EXCLUDED = table
            ops.head_convs_fused_ok = real_ok if fused_path else (lambda *a, **k: False)
            try:
                return head(xs[i])
            finally:
                ops._HEAD_CONVS_EXCLUDED, ops.head_convs_fused_ok = shipped, real_ok
        for name, make in heads.items():
            head = make().to(dev)
            sides = {'modules': [lambda i=i: forward(head, i, shipped, False) for i in range(SETS)],
                     'fused': [lambda i=i: forward(head, i, shipped) for i in range(SETS)],
                     'fused_every_part': [lambda i=i: forward(head, i, frozenset()) for i in range(SETS)]}
            stat, r = timed_row(sides, args.iters, args.reps)
            ref, got = sides['modules'][0](), sides['fused'][0]()
            r['max_rel_diff_vs_modules'] = max_rel_diff(ref, got)
            res['forward'][name] = r
            print(name, json.dumps(r), flush=True)
            del head
    ops._HEAD_CONVS_EXCLUDED = shipped
    write_json(args.out, res)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
