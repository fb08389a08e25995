"""Generate the plain-FCOS golden vectors by running the REFERENCE's own code (this container
only), in the style of gen_gfl_golden.py and with gen_golden.py's shims:

    python -B tests/golden/gen_fcos_golden.py

Writes, next to this file,
  fcos_targets.npz  per case of fcos_inputs.REFERENCE_TARGET_CASES and image: the reference's
                    FCOSHead.single_image_targets (lib/heads/fcos_head.py:371-416), its per-level
                    maps flattened and concatenated: `<tag>_cls_<b>` [N] i64, `<tag>_reg_<b>` [N, 4]
                    f32, `<tag>_ctr_<b>` [N] f32;
  fcos_loss.npz     per case of fcos_inputs.REFERENCE_LOSS_CASES: the three losses of the
                    reference's FCOSHead.calc_loss (:419-515, its arm without GFL) in the order
                    (cls, bbox, ctr), in f32 (`<tag>_f32`) and from .double() inputs (`<tag>_f64`),
                    the positive count, and the f64 gradients of each loss with respect to the
                    head output it depends on (`<tag>_gcls`, `<tag>_greg`, `<tag>_gctr`; the other
                    six pairs are identically zero, which the generator asserts);
  whole_fcos.json / whole_fcos.npz
                    forward_train's loss dict and forward_test's detections of the reference's
                    configs/fcos_r50_fpn.py model on inputs.ftrain_case((384, 640)) with
                    inputs.seeded_state weights, as gen_gfl_golden.gen_whole writes them for GFL;
                    plus the model's state_dict keys and shapes.
Exits cleanly (code 0, message) when the reference is not present; no test reads the reference
or this file."""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fcos_inputs  # noqa: E402
import gen_golden as gg  # noqa: E402
import inputs  # noqa: E402


def _head(fcos_head_mod, num_classes, reg_std=fcos_inputs.REG_STD, reg_mean=fcos_inputs.REG_MEAN):
    w = fcos_inputs.WEIGHTS
    return fcos_head_mod.FCOSHead(
        num_classes=num_classes, in_channels=8, stacked_convs=1, feat_channels=8, strides=list(fcos_inputs.STRIDES),
        reg_std=reg_std, reg_mean=reg_mean,
        loss_cls=gg.cd(dict(type='FocalLoss', use_sigmoid=True, loss_weight=w['cls_weight'])),
        loss_bbox=gg.cd(dict(type='GIoULoss', loss_weight=w['bbox_weight'])),
        loss_centerness=gg.cd(dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=w['ctr_weight'])))


def gen_targets(fcos_head_mod):
    res = {}
    outs = [torch.from_numpy(x) for x in fcos_inputs.level_outputs()]
    for tag in fcos_inputs.REFERENCE_TARGET_CASES:
        boxes, labels, thr = fcos_inputs.TARGET_CASES[tag]
        head = _head(fcos_head_mod, 21)
        head.level_scale_thr = list(thr)
        for b, meta in enumerate(fcos_inputs.img_metas()):
            cls, reg, ctr = head.single_image_targets(outs, outs, outs, torch.from_numpy(boxes[b]),
                                                      torch.from_numpy(labels[b]), meta, None)
            res['{}_cls_{}'.format(tag, b)] = torch.cat([x.reshape(-1) for x in cls]).numpy()
            res['{}_reg_{}'.format(tag, b)] = torch.cat([x.reshape(-1, 4) for x in reg]).numpy()
            res['{}_ctr_{}'.format(tag, b)] = torch.cat([x.reshape(-1) for x in ctr]).numpy()
            c = res['{}_cls_{}'.format(tag, b)]
            # the fixture must not depend on this CPU's square root: every centerness is the
            # correctly rounded one of its own ltrb
            v = res['{}_reg_{}'.format(tag, b)][c > 0] + np.float32(1e-6)
            want = np.sqrt((np.minimum(v[:, 0], v[:, 2]) / np.maximum(v[:, 0], v[:, 2])) *
                           (np.minimum(v[:, 1], v[:, 3]) / np.maximum(v[:, 1], v[:, 3])))
            assert np.array_equal(res['{}_ctr_{}'.format(tag, b)][c > 0], want), (tag, b)
            print(tag, b, 'positives', int((c > 0).sum()), 'labels', sorted(set(c.tolist())), flush=True)
    gg.save('fcos_targets.npz', **res)


def _calc_loss(head, c, cls, reg, ctr, dtype):
    """The reference's calc_loss on the flat tensors, split into its per-image lists of per-level maps."""
    labels = torch.from_numpy(c['labels'])
    ltrb = torch.from_numpy(c['ltrb']).to(dtype)
    ctr_t = torch.from_numpy(c['ctr_t']).to(dtype)
    per = [[[] for _ in range(6)] for _ in range(c['batch'])]
    for b, _, (h, w), sl in fcos_inputs.level_slices(c):
        per[b][0].append(cls[:, sl].reshape(-1, h, w))
        per[b][1].append(reg[:, sl].reshape(-1, h, w))
        per[b][2].append(ctr[sl].reshape(1, h, w))
        per[b][3].append(labels[sl].view(h, w, 1))
        per[b][4].append(ltrb[sl].view(h, w, 4))
        per[b][5].append(ctr_t[sl].view(h, w, 1))
    return head.calc_loss(*[[per[b][k] for b in range(c['batch'])] for k in range(6)])


ORDER = ('cls_loss', 'bbox_loss', 'ctr_loss')


def gen_loss(fcos_head_mod):
    res = {}
    for tag in fcos_inputs.REFERENCE_LOSS_CASES:
        c = fcos_inputs.loss_case(tag)
        pos = c['labels'] > 0
        head = _head(fcos_head_mod, c['C'] + 1, c['reg_std'], c['reg_mean'])
        t32 = [torch.from_numpy(c[k]) for k in ('cls', 'reg', 'ctr')]
        with torch.no_grad():
            l32 = _calc_loss(head, c, *t32, torch.float32)
        assert sorted(l32) == sorted(ORDER), list(l32)
        t64 = [t.double().requires_grad_(True) for t in t32]
        l64 = _calc_loss(head.double(), c, *t64, torch.float64)
        res[tag + '_f32'] = np.array([float(l32[k]) for k in ORDER], np.float32)
        res[tag + '_f64'] = np.array([float(l64[k]) for k in ORDER], np.float64)
        res[tag + '_num_pos'] = np.int64(pos.sum())
        for i, (name, key) in enumerate(zip(ORDER, ('gcls', 'greg', 'gctr'))):
            g = torch.autograd.grad(l64[name], t64, retain_graph=True, allow_unused=True)
            for j, other in enumerate(g):
                assert j == i or other is None or not other.any(), (tag, name, j)
            res['{}_{}'.format(tag, key)] = g[i].numpy()
        print(tag, int(pos.sum()), res[tag + '_f32'], res[tag + '_f64'], flush=True)
    gg.save('fcos_loss.npz', **res)


def gen_whole():
    sys.path.insert(0, os.path.join(gg.REPO, 'pytorch-faster-rcnn_amd'))
    from frcnn_amd.config import Config
    import lib.builder as rb
    tag, fname, over, shape = fcos_inputs.WHOLE_FCOS
    img, boxes, labels, metas = inputs.ftrain_case(shape)
    cfg = Config.fromfile(os.path.join(gg.REF, 'configs', fname))
    cfg.model.backbone.pretrained = False
    cfg.test_cfg.update(over)
    model = rb.build_module(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    shapes = {k: list(v.shape) for k, v in model.state_dict().items()}
    sd = inputs.seeded_state(shapes)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.train()
    np.random.seed(inputs.FTRAIN_NP_SEED)
    with torch.no_grad():
        losses = model.forward_train(torch.from_numpy(img), [torch.from_numpy(b) for b in boxes],
                                     [torch.from_numpy(l) for l in labels], metas)
    out = {k: float(v) for k, v in losses.items()}
    model.eval()
    with torch.no_grad():
        dets = model.forward_test(torch.from_numpy(img), metas)
    with open(os.path.join(HERE, 'whole_{}.json'.format(tag)), 'w') as f:
        json.dump({'losses': out, 'np_seed': inputs.FTRAIN_NP_SEED, 'config': 'configs/' + fname,
                   'test_cfg_overrides': over, 'image_shape': list(shape), 'state_dict_shapes': shapes}, f, indent=1)
    dets = list(zip(*dets[:3]))
    res = {'n': np.int64(len(dets))}
    for i, (b, sc, lb) in enumerate(dets):
        b = b.detach().numpy().astype(np.float32)
        res['boxes_{}'.format(i)] = (b.T if b.shape[0] == 4 and b.ndim == 2 and b.shape[1] != 4 else b).reshape(-1, 4)
        res['scores_{}'.format(i)] = sc.detach().numpy().astype(np.float32).reshape(-1)
        res['labels_{}'.format(i)] = lb.detach().numpy().astype(np.int64).reshape(-1)
    gg.save('whole_{}.npz'.format(tag), **res)
    print(tag, out, [len(d[1]) for d in dets], flush=True)


def main():
    if not os.path.isdir(os.path.join(gg.REF, 'lib')):
        print('reference not found at {}: nothing to generate (fixtures are committed)'.format(gg.REF))
        return 0
    gg.install_shims()
    sys.path.insert(0, gg.REF)
    import lib.heads.fcos_head as fcos_head_mod
    torch.set_num_threads(8)
    gen_targets(fcos_head_mod)
    gen_loss(fcos_head_mod)
    if '--no-whole' not in sys.argv:
        gen_whole()
    return 0


if __name__ == '__main__':
    sys.exit(main())
