"""Generate the Libra R-CNN golden vectors by running the REFERENCE's own code (this
container only), in the style of gen_golden.py and with its shims:

    python -B tests/golden/gen_libra_golden.py

Writes, next to this file,
  libra_sampler.npz  the reference's IoUBalancedNegSampler (lib/region.py:128-172) on the
                     cases of libra_inputs.SAMPLER_FIXTURE_CASES after np.random.seed: the
                     sampled labels per image and the legacy RNG's state afterwards;
  libra_targets.npz  the reference's bbox_target (lib/bbox.py:6-82) with that sampler on
                     libra_inputs.target_case();
  whole_libra.json / whole_libra.npz
                     forward_train's loss dict and forward_test's detections of the
                     reference's configs/libra_faster_rcnn_r50_fpn.py model, as
                     gen_golden.gen_whole_detectors writes them for the BASELINE configs.
Exits cleanly (code 0, message) when the reference is not present; no GPU test reads the
reference or this file."""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gen_golden as gg  # noqa: E402
import inputs  # noqa: E402
import libra_inputs  # noqa: E402


def gen_sampler(region):
    res = {}
    for tag in libra_inputs.SAMPLER_FIXTURE_CASES:
        c = libra_inputs.sampler_case(tag)
        sampler = region.IoUBalancedNegSampler(c['max_num'], c['pos_num'], num_bins=c['num_bins'],
                                               max_iou=c['max_iou'], floor_thr=-1, floor_fraction=0)
        np.random.seed(c['np_seed'])
        for i, (lab, iou) in enumerate(zip(c['labels'], c['ious'])):
            out = sampler(torch.from_numpy(lab), torch.from_numpy(iou), None, None)
            res['{}_labels_{}'.format(tag, i)] = out.numpy()
        st = np.random.get_state()
        res['{}_rng_keys'.format(tag)] = np.asarray(st[1], np.uint32)
        res['{}_rng_pos'.format(tag)] = np.int64(st[2])
    gg.save('libra_sampler.npz', **res)


def gen_targets(region, bbox_mod):
    res = {}
    s = libra_inputs.TARGET_SAMPLER
    np.random.seed(libra_inputs.TARGET_NP_SEED)
    for i, (props, gb, gl) in enumerate(libra_inputs.target_case()):
        out = bbox_mod.bbox_target(torch.from_numpy(props), torch.from_numpy(gb), torch.from_numpy(gl),
                                   region.MaxIoUAssigner(*libra_inputs.TARGET_ASSIGNER),
                                   region.IoUBalancedNegSampler(s['max_num'], s['pos_num'], num_bins=s['num_bins'],
                                                                max_iou=s['max_iou']),
                                   (0.0,) * 4, libra_inputs.TARGET_STDS)
        for k, v in zip(('tar_props', 'tar_bbox', 'tar_label', 'tar_param', 'tar_is_gt'), out):
            res['{}_{}'.format(i, k)] = v.numpy()
    gg.save('libra_targets.npz', **res)


def gen_whole():
    sys.path.insert(0, os.path.join(gg.REPO, 'pytorch-faster-rcnn_amd'))
    from frcnn_amd.config import Config
    import lib.builder as rb
    tag, fname, over, shape = libra_inputs.WHOLE_LIBRA
    img, boxes, labels, metas = inputs.ftrain_case(shape)
    cfg = Config.fromfile(os.path.join(gg.REF, 'configs', fname))
    cfg.model.backbone.pretrained = False
    for k, v in over.items():
        cfg.test_cfg[k].update(v)
    model = rb.build_module(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    sd = inputs.seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.train()
    np.random.seed(inputs.FTRAIN_NP_SEED)
    with torch.no_grad():
        losses = model.forward_train(torch.from_numpy(img), [torch.from_numpy(b) for b in boxes],
                                     [torch.from_numpy(l) for l in labels], metas)
    out = {k: float(v) for k, v in losses.items()}
    with torch.no_grad():  # the neck's outputs (FPN -> BFP), pinned bit for bit by their hashes
        feat_sha = [gg.sha(f.numpy()) for f in model.extract_feat(torch.from_numpy(img))]
    with open(os.path.join(HERE, 'whole_{}.json'.format(tag)), 'w') as f:
        json.dump({'losses': out, 'np_seed': inputs.FTRAIN_NP_SEED, 'config': 'configs/' + fname,
                   'test_cfg_overrides': over, 'image_shape': list(shape), 'feat_sha256': feat_sha}, f, indent=1)
    model.eval()
    with torch.no_grad():
        dets = model.forward_test(torch.from_numpy(img), metas)
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
    import lib.region as region
    import lib.bbox as bbox_mod
    torch.set_num_threads(8)
    gen_sampler(region)
    gen_targets(region, bbox_mod)
    if '--no-whole' not in sys.argv:
        gen_whole()
    return 0


if __name__ == '__main__':
    sys.exit(main())
