"""Generate the Double-Head R-CNN golden vectors by running the REFERENCE's own code (where it is
present), in the style of gen_libra_golden.gen_whole and with gen_golden's shims:

    python -B tests/golden/gen_dh_golden.py

Writes, next to this file,
  whole_dh.json / whole_dh.npz
      forward_train's loss dict and forward_test's detections of the reference's
      configs/dh_rcnn_r50_fpn.py model on inputs.ftrain_case, with inputs.seeded_state weights.

Running statistics: the head's BatchNorm2d is live (the reference freezes only the backbone's
BN), so forward_train in train mode moves its running mean / variance even under no_grad.  The
seeded state dict is therefore loaded AGAIN before model.eval() / forward_test: the detections
belong to the seeded weights alone, not to statistics left by the training pass.  The test
reloads the state at the same point.

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
import dh_inputs  # noqa: E402


def gen_whole():
    sys.path.insert(0, os.path.join(gg.REPO, 'pytorch-faster-rcnn_amd'))
    from frcnn_amd.config import Config
    import lib.builder as rb
    tag, fname, over, shape = dh_inputs.WHOLE_DH
    img, boxes, labels, metas = inputs.ftrain_case(shape)
    cfg = Config.fromfile(os.path.join(gg.REF, 'configs', fname))
    cfg.model.backbone.pretrained = False
    for k, v in over.items():
        cfg.test_cfg[k].update(v)
    model = rb.build_module(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    sd = inputs.seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()})
    state = {k: torch.from_numpy(v) for k, v in sd.items()}
    model.load_state_dict(state)
    model.train()
    np.random.seed(inputs.FTRAIN_NP_SEED)
    with torch.no_grad():
        losses = model.forward_train(torch.from_numpy(img), [torch.from_numpy(b) for b in boxes],
                                     [torch.from_numpy(l) for l in labels], metas)
    out = {k: float(v) for k, v in losses.items()}
    with open(os.path.join(HERE, 'whole_{}.json'.format(tag)), 'w') as f:
        json.dump({'losses': out, 'np_seed': inputs.FTRAIN_NP_SEED, 'config': 'configs/' + fname,
                   'test_cfg_overrides': over, 'image_shape': list(shape)}, f, indent=1)
    model.load_state_dict(state)  # the head BN's running statistics moved in forward_train
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
    torch.set_num_threads(8)
    gen_whole()
    return 0


if __name__ == '__main__':
    sys.exit(main())
