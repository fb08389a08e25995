"""Timing of the dense-head candidate selection (csrc/dense_candidates.hip) against the torch loop
it replaces.

    python tools/bench_dense_candidates.py [--iters 200] [--out profiles/dense_candidates/bench_dense_candidates.json]

Shapes: each config's own -- two images of 800x1333 padded to 800x1344, five levels with strides
8..128 (grids 100x168 .. 7x11), C = 20, pre_nms 1000:
  fcos    plain FCOS with centerness (LTRB decode), 22 400 columns per image;
  gfl     the same cells with 16 DFL bins (64 regression channels), no centerness;
  retina  A = 9 anchors per cell (DELTA decode), 201 600 columns per image.
For every config, with NCHW and with channels-last head outputs:
(a) ops.dense_candidates (one call for the batch) against the per-image image_candidates loop of
    the same head (what predict_bboxes ran before the kernels existed: FCOSHead.image_candidates
    / AnchorHead.image_candidates, the GFL one with its per-level ops.dfl_decode) on the same
    device tensors;
(b) the kernel launches (torch.profiler's device activity) and the device-to-host
    synchronisations (torch.cuda.set_sync_debug_mode('warn')) of one call of each side;
(c) the algorithmic bytes of the fused call: every class logit (and centerness logit) read once,
    the regression channels of every column the filter needs (LTRB, DFL) or of the selected rows
    (DELTA), the selected rows written (boxes, C scores, factor, valid, index).
Every time is the mean of back-to-back calls between one HIP event pair after a warm-up, repeated
5 times with the two sides alternating (median reported, all runs kept); the torch loop runs a
tenth of the iterations.  The selected column sets of the two sides are compared first."""
import argparse
import json
import os

import torch

from benchlib import PEAK_BYTES, REPO, compare, count_launches, count_syncs, on_path, require_gpu, write_json

on_path('tests', 'golden')

IMG_SHAPE, PAD = (800, 1333), (800, 1344)
STRIDES = [8, 16, 32, 64, 128]
GRIDS = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
B, C, PRE_NMS = 2, 20, 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'dense_candidates', 'bench_dense_candidates.json'))
    args = ap.parse_args()
    require_gpu('bench_dense_candidates')
    import dense_inputs as di
    from frcnn_amd import ops
    from frcnn_amd.config import ConfigDict
    from frcnn_amd.heads.fcos_head import FCOSHead
    from frcnn_amd.heads.retina_head import RetinaHead
    dev = torch.device('cuda', 0)
    metas = [{'img_shape': IMG_SHAPE + (3,), 'pad_shape': PAD + (3,), 'scale_factor': 1.0}] * B
    cfg = ConfigDict(dict(pre_nms=PRE_NMS, min_bbox_size=0, min_score=0.05, nms_iou=0.5, max_per_img=100))
    img_hw, mins = [IMG_SHAPE] * B, [0.0] * B
    cells = sum(h * w for h, w in GRIDS)
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters,
           'shapes': {'images': B, 'image': list(IMG_SHAPE), 'padded': list(PAD), 'grids': GRIDS, 'classes': C,
                      'pre_nms': PRE_NMS, 'cells_per_image': cells}}
    fkw = dict(num_classes=C + 1, in_channels=8, stacked_convs=1, feat_channels=8, strides=STRIDES, reg_mean=0.0)
    heads = {
        'fcos': FCOSHead(reg_std=1200.0, loss_cls=di._FOCAL, loss_bbox=di._GIOU, loss_centerness=di._CTR, **fkw),
        'gfl': FCOSHead(reg_std=100.0, loss_cls=di._QFL, loss_bbox=di._GIOU, loss_dfl=di._DFL,
                        atss_cfg=dict(topk=9, scale=8), **fkw),
        'retina': RetinaHead(C + 1, 8, 1, 8, loss_cls=di._FOCAL,
                             loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0)),
    }
    for name, head in heads.items():
        head = head.to(dev)
        A = 9 if name == 'retina' else 1
        if name == 'retina':
            cls, reg = di.retina_outputs(70, GRIDS, A, C, B)
            ctr = None
        else:
            cls, reg, ctr = di.fcos_outputs(71, GRIDS, C, B, kind=name, reg_std=head.reg_std, ctr=name == 'fcos')
        rows = sum(ops.dense_candidates_rows(GRIDS, A, PRE_NMS))
        reg_ch = reg[0].shape[1]
        cols = A * cells
        # bytes: class (+ centerness) logits once; regression of every column (the filter runs before
        # the top-k) for LTRB / DFL, of the selected rows for DELTA; the rows written
        read = 4 * B * cols * C + (4 * B * cols if name == 'fcos' else 0)
        read += 4 * B * (rows * 4 if name == 'retina' else cols * reg_ch)
        written = B * rows * (16 + 4 * C + (4 if name == 'fcos' else 0) + 1 + 4)
        out = {'columns_per_image': cols, 'rows_per_image': rows, 'algorithmic_bytes': int(read + written)}
        for layout in ('nchw', 'channels_last'):
            def put(arrs):
                ts = [torch.from_numpy(a).to(dev) for a in arrs]
                return [t.contiguous(memory_format=torch.channels_last) for t in ts] if layout != 'nchw' else ts
            dc, dr = put(cls), put(reg)
            dt = put(ctr) if name == 'fcos' else None
            if name == 'retina':
                anchors = head._flat_anchors(GRIDS, dev)
                level_anchors = head.create_anchors(GRIDS)

                def fused():
                    return ops.dense_candidates(dc, dr, None, 'DELTA', img_hw, mins, PRE_NMS, num_anchors=A,
                                                anchors=anchors, means=head.target_means, stds=head.target_stds)

                def loop():
                    return [head.image_candidates([x[b] for x in dc], [x[b] for x in dr], level_anchors, metas[b], cfg)
                            for b in range(B)]
            else:
                dfl = dict(bins=16, dfl_stride=head.loss_dfl.stride) if name == 'gfl' else {}

                def fused():
                    return ops.dense_candidates(dc, dr, dt, 'DFL' if name == 'gfl' else 'LTRB', img_hw, mins, PRE_NMS,
                                                strides=STRIDES, reg_std=head.reg_std, reg_mean=0.0, **dfl)

                def loop():
                    return [head.image_candidates([x[b] for x in dc], [x[b] for x in dr],
                                                  [x[b] for x in dt] if dt is not None else None, metas[b], cfg)
                            for b in range(B)]
            # the two sides select the same rows: compare the best-class scores, sorted per image
            fo, lo = fused(), loop()
            diff = 0.0
            for b in range(B):
                sc = lo[b][0] if name == 'retina' else lo[b][1]
                a_ = torch.sort(fo[1][b][fo[3][b]].max(1)[0])[0]
                b_ = torch.sort(sc.max(0)[0])[0]
                diff = max(diff, float((a_ - b_).abs().max()) if a_.shape == b_.shape else float('inf'))
            th, tt, ah, at = compare(fused, loop, args.iters, max(args.iters // 10, 3), warmup=3)
            r = {'hip_us': round(th, 2), 'torch_us': round(tt, 2), 'hip_runs_us': ah, 'torch_runs_us': at,
                 'speedup': round(tt / th, 2), 'hip_GBps': round((read + written) / th / 1e3, 1),
                 'hip_fraction_of_8TBps': round((read + written) / th / 1e3 / (PEAK_BYTES / 1e9), 4),
                 'largest_best_score_difference_of_the_selected_rows': diff,
                 'launches_and_syncs': {'hip': [count_launches(fused), count_syncs(fused)],
                                        'torch': [count_launches(loop), count_syncs(loop)],
                                        'columns': ['device kernels per call (null: no device activity from the '
                                                    'profiler)', 'host syncs per call']}}
            r['fused_is_faster'] = bool(th < tt)
            out[layout] = r
            print(name, layout, json.dumps(r), flush=True)
        res[name] = out
    write_json(args.out, res)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
