"""Generate the GFL golden vectors by running the REFERENCE's own code (this container only), in
the style of gen_golden.py / gen_libra_golden.py and with their shims:

    python -B tests/golden/gen_gfl_golden.py

Writes, next to this file,
  gfl_loss.npz    per case of gfl_inputs.LOSS_CASES: the three losses of the reference's
                  FCOSHead.calc_loss (lib/heads/fcos_head.py:419-515) in f32 (`<tag>_f32`), the
                  same from .double() inputs (`<tag>_f64`), the positive count, and the f64
                  gradients of each loss with respect to the logits (`<tag>_gcls_cls`,
                  `<tag>_greg_dfl`, `<tag>_greg_bbox`; the other three pairs are identically zero,
                  which the generator asserts);
  gfl_decode.npz  the reference's decoded and clamped boxes per level (fcos_head.py:579-600:
                  its class2length, ltrb2bbox and utils.clamp_bbox) on gfl_inputs.decode_case(),
                  in f32 and from .double() logits;
  whole_gfl.json / whole_gfl.npz
                  forward_train's loss dict and forward_test's detections of the reference's
                  configs/fcos_r50_fpn_atss_gfl.py model on inputs.ftrain_case((384, 640)) with
                  inputs.seeded_state weights, as gen_golden.gen_whole_detectors writes them for
                  cfg5; plus the model's state_dict keys and shapes, and box_f32_err: the largest
                  |f32 - f64| over the reference's decode (before the clamp) of that image's own
                  (f32) regression outputs, evaluated in f32 and in f64.
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

import gen_golden as gg  # noqa: E402
import gfl_inputs  # noqa: E402
import inputs  # noqa: E402


def _head(fcos_head_mod, c):
    w = gfl_inputs.WEIGHTS
    return fcos_head_mod.FCOSHead(
        num_classes=c['C'] + 1, in_channels=8, stacked_convs=1, feat_channels=8, strides=[8, 16, 32, 64, 128],
        reg_std=c['reg_std'], reg_mean=c['reg_mean'], atss_cfg=gg.cd(dict(topk=9, scale=8)),
        loss_cls=gg.cd(dict(type='QualityFocalLoss', use_sigmoid=True, loss_weight=w['cls_weight'])),
        loss_bbox=gg.cd(dict(type='GIoULoss', loss_weight=w['bbox_weight'])),
        loss_dfl=gg.cd(dict(type='DistributionFocalLoss', cls_channels=c['bins'], stride=c['stride'],
                            norm_prob=c['norm_prob'], loss_weight=w['dfl_weight'])))


def _calc_loss(head, c, cls, reg, dtype):
    """The reference's calc_loss on the flat tensors, split into its per-image lists of per-level maps."""
    labels = torch.from_numpy(c['labels'])
    ltrb = torch.from_numpy(c['ltrb']).to(dtype)
    per = [[[] for _ in range(6)] for _ in range(c['batch'])]
    for b, _, (h, w), sl in gfl_inputs.level_slices(c):
        n = h * w
        per[b][0].append(cls[:, sl].reshape(-1, h, w))
        per[b][1].append(reg[:, sl].reshape(-1, h, w))
        per[b][2].append(torch.zeros(1, h, w, dtype=dtype))
        per[b][3].append(labels[sl].view(h, w, 1))
        per[b][4].append(ltrb[sl].view(h, w, 4))
        per[b][5].append(torch.zeros(n, dtype=dtype).view(h, w, 1))
    return head.calc_loss(*[[per[b][k] for b in range(c['batch'])] for k in range(6)])


def gen_loss(fcos_head_mod):
    res = {}
    for tag in gfl_inputs.LOSS_CASES:
        c = gfl_inputs.loss_case(tag)
        pos = c['labels'] > 0
        # the reference itself must run: every positive target below the top bin
        assert (c['ltrb'][pos] / np.float32(c['reg_std']) < np.float32((c['bins'] - 1) * c['stride'])).all(), tag
        head = _head(fcos_head_mod, c)
        with torch.no_grad():
            l32 = _calc_loss(head, c, torch.from_numpy(c['cls']), torch.from_numpy(c['reg']), torch.float32)
        assert list(l32) == ['cls_loss', 'dfl_loss', 'bbox_loss'], list(l32)
        cls = torch.from_numpy(c['cls']).double().requires_grad_(True)
        reg = torch.from_numpy(c['reg']).double().requires_grad_(True)
        l64 = _calc_loss(head.double(), c, cls, reg, torch.float64)
        res[tag + '_f32'] = np.array([float(v) for v in l32.values()], np.float32)
        res[tag + '_f64'] = np.array([float(v) for v in l64.values()], np.float64)
        res[tag + '_num_pos'] = np.int64(pos.sum())
        for name, wrt in (('cls', 0), ('dfl', 1), ('bbox', 1)):
            g = torch.autograd.grad(l64[name + '_loss'], [cls, reg], retain_graph=True, allow_unused=True)
            other = g[1 - wrt]
            assert other is None or not other.any(), (tag, name)
            res['{}_g{}_{}'.format(tag, 'cls' if wrt == 0 else 'reg', name)] = g[wrt].numpy()
        print(tag, int(pos.sum()), res[tag + '_f32'], res[tag + '_f64'], flush=True)
    gg.save('gfl_loss.npz', **res)


def _decode(fcos_head_mod, utils, reg, cell, bins, stride, reg_std, reg_mean, img_size):
    """fcos_head.py:579-600 for one image's level: reg [4*bins, H, W] -> clamped boxes [4, H*W]
    (img_size None: the boxes before utils.clamp_bbox)."""
    gs = reg.shape[-2:]
    r = reg.reshape(bins, -1).t().softmax(-1)
    ltrb = fcos_head_mod.class2length(r, stride) * reg_std + reg_mean
    bbox = fcos_head_mod.ltrb2bbox(ltrb.view(4, *gs), cell).view(4, -1)
    return bbox if img_size is None else utils.clamp_bbox(bbox, img_size)


def gen_decode(fcos_head_mod, utils):
    res = {}
    for i, (cell, reg) in enumerate(gfl_inputs.decode_case()):
        for name, t in (('f32', torch.from_numpy(reg)), ('f64', torch.from_numpy(reg).double())):
            res['boxes_{}_{}'.format(name, i)] = np.stack([
                _decode(fcos_head_mod, utils, t[b], cell, gfl_inputs.DECODE_BINS, gfl_inputs.DECODE_STRIDE,
                        gfl_inputs.REG_STD, gfl_inputs.REG_MEAN, gfl_inputs.DECODE_IMG).numpy() for b in range(2)])
    err = max(float(np.abs(res['boxes_f32_{}'.format(i)] - res['boxes_f64_{}'.format(i)]).max())
              for i in range(len(gfl_inputs.DECODE_LEVELS)))
    print('decode: largest |reference f32 - reference f64| = {:.3e} px'.format(err), flush=True)
    gg.save('gfl_decode.npz', **res)


def gen_whole(fcos_head_mod, utils):
    sys.path.insert(0, os.path.join(gg.REPO, 'pytorch-faster-rcnn_amd'))
    from frcnn_amd.config import Config
    import lib.builder as rb
    tag, fname, over, shape = gfl_inputs.WHOLE_GFL
    img, boxes, labels, metas = inputs.ftrain_case(shape)
    cfg = Config.fromfile(os.path.join(gg.REF, 'configs', fname))
    cfg.model.backbone.pretrained = False
    for k, v in over.items():
        cfg.test_cfg[k].update(v)
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
        _, reg_outs, _ = model.bbox_head(model.extract_feat(torch.from_numpy(img)))
    head, err = model.bbox_head, 0.0
    for i, r in enumerate(reg_outs):  # the f32 decode's own error on this image's regression outputs
        # before the clamp: at this image size nearly every box is clamped to the image's border,
        # which hides the expectation's rounding in all but the few coordinates that matter
        args = (head.strides[i], head.loss_dfl.cls_channels, head.loss_dfl.stride, head.reg_std, head.reg_mean, None)
        b32 = _decode(fcos_head_mod, utils, r[0], *args)
        b64 = _decode(fcos_head_mod, utils, r[0].double(), *args)
        err = max(err, float((b32.double() - b64).abs().max()))
    with open(os.path.join(HERE, 'whole_{}.json'.format(tag)), 'w') as f:
        json.dump({'losses': out, 'np_seed': inputs.FTRAIN_NP_SEED, 'config': 'configs/' + fname,
                   'test_cfg_overrides': over, 'image_shape': list(shape), 'box_f32_err': err,
                   'state_dict_shapes': shapes}, f, indent=1)
    dets = list(zip(*dets[:3]))
    res = {'n': np.int64(len(dets))}
    for i, (b, sc, lb) in enumerate(dets):
        b = b.detach().numpy().astype(np.float32)
        res['boxes_{}'.format(i)] = (b.T if b.shape[0] == 4 and b.ndim == 2 and b.shape[1] != 4 else b).reshape(-1, 4)
        res['scores_{}'.format(i)] = sc.detach().numpy().astype(np.float32).reshape(-1)
        res['labels_{}'.format(i)] = lb.detach().numpy().astype(np.int64).reshape(-1)
    gg.save('whole_{}.npz'.format(tag), **res)
    print(tag, out, [len(d[1]) for d in dets], 'box_f32_err', err, flush=True)


def main():
    if not os.path.isdir(os.path.join(gg.REF, 'lib')):
        print('reference not found at {}: nothing to generate (fixtures are committed)'.format(gg.REF))
        return 0
    gg.install_shims()
    sys.path.insert(0, gg.REF)
    import lib.utils as utils
    import lib.heads.fcos_head as fcos_head_mod
    gg._topk_by_center_floor(fcos_head_mod)
    torch.set_num_threads(8)
    gen_loss(fcos_head_mod)
    gen_decode(fcos_head_mod, utils)
    if '--no-whole' not in sys.argv:
        gen_whole(fcos_head_mod, utils)
    return 0


if __name__ == '__main__':
    sys.exit(main())
