"""Record the output bits of frh_conv3x3_bias_act for tests/test_gpu_conv3x3_pipeline.py.

    python tools/record_conv3x3_bits.py [--out tests/golden/conv3x3_bits.json]

For each shape (n, cin, cout, h, w) below: seeded CPU torch.randn x, w, bias (the generator
and the draw order of tests/test_gpu_conv3x3_pipeline.py::_randn_case), the fused call with
bias and ReLU on cuda:0, and the SHA-256 of the output's bytes (channels-last storage order)
and of the three inputs' bytes.  Run it on the build whose bits are to be kept: a later
kernel must reproduce them."""
import argparse
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'pytorch-faster-rcnn_amd'))

SHAPES = [(2, 64, 64, 19, 32), (2, 256, 128, 10, 16), (1, 32, 192, 17, 34)]


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def randn_case(shape):
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(9000 + cin + 7 * cout + h * w)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g)
    bias = torch.randn(cout, generator=g)
    return x, wt, bias


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden', 'conv3x3_bits.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('record_conv3x3_bits needs a HIP device')
    from frcnn_amd import _lib
    dev = torch.device('cuda', 0)
    cl = torch.channels_last
    cases = []
    for shape in SHAPES:
        n, cin, cout, h, w = shape
        x, wt, bias = randn_case(shape)
        xd, wd, bd = x.to(dev).contiguous(memory_format=cl), wt.to(dev).contiguous(memory_format=cl), bias.to(dev)
        y = torch.empty(n, cout, h, w, device=dev).contiguous(memory_format=cl)
        ws = torch.empty(16 * cin * cout, device=dev)
        p = _lib.ptr
        _lib.call('frh_conv3x3_bias_act', p(xd), p(wd), p(bd), p(y), p(ws), n, cin, cout, h, w, xd.stride(0),
                  xd.stride(2), xd.stride(3), 1, _lib.stream_of(xd))
        torch.cuda.synchronize()
        # bytes in NHWC order, the order of the kernel's stores
        cases.append({'shape': list(shape), 'x': sha(x), 'w': sha(wt), 'bias': sha(bias),
                      'y_nhwc': sha(y.permute(0, 2, 3, 1))})
        print(cases[-1], flush=True)
    res = {'entry': 'frh_conv3x3_bias_act, bias and ReLU', 'device': torch.cuda.get_device_name(0), 'cases': cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
