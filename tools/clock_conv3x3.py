"""The shader clock under the Winograd 3x3 kernel, and where a workgroup's lifetime goes.

    python tools/clock_conv3x3.py [--variant 16] [--seconds 1.5] [--out FILE.json]

Runs the stamped laboratory build (tools/csrc/conv3x3_wino_lab.hip, `variant` as in
tools/bench_conv3x3_variants.py) on P2 alone (2 x 256 x 152 x 256, random data, 1280
workgroups = five rounds on 256 CUs) back to back for `seconds`, then reads the last launch's
stamps: thread 0 of every workgroup stored s_memtime (shader cycles) and s_memrealtime
(100 MHz) at entry, before and after the main loop and after the epilogue.
  clock      = d s_memtime / d s_memrealtime x 100 MHz around the main loop, median over workgroups
  lifetime   = entry .. end, with its prologue / loop / epilogue parts, in cycles and us
  rounds     = the launch's span (first entry .. last end) against five median lifetimes: what
               is lost between workgroups."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, 'pytorch-faster-rcnn_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variant', type=int, default=16)
    ap.add_argument('--seconds', type=float, default=1.5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('clock_conv3x3 needs a HIP device')
    from frcnn_amd import _lib
    from frcnn_amd.utils import conv_layout
    import toolslib
    tools = toolslib.load()
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    n, c, h, w = 2, 256, 152, 256
    cl = torch.channels_last
    with torch.no_grad():
        conv = torch.nn.Conv2d(c, c, 3, padding=1).to(dev)
        conv_layout(conv)
        xs = [torch.randn(n, c, h, w, device=dev).contiguous(memory_format=cl) for _ in range(3)]
        y = torch.empty(n, c, h, w, device=dev).contiguous(memory_format=cl)
        ws = torch.empty(16 * c * c, device=dev)
        wgs = n * ((h + 15) // 16) * ((w + 15) // 16) * (c // 64)
        stamps = torch.zeros(wgs * 8, dtype=torch.int64, device=dev)

        def call(x):
            a = (args.variant, _lib.ptr(stamps), 1, _lib.ptr_array([x]), _lib.ptr_array([conv.weight]),
                 _lib.ptr_array([conv.bias]), _lib.ptr_array([y]), _lib.ptr(ws), ws.numel() * 4, n, c, c,
                 _lib.i32_array([h, w]), _lib.i64_array([x.stride(0), x.stride(2), x.stride(3)]), 1,
                 _lib.stream_of(ws))
            if tools.frh_conv3x3_bias_act_levels_variant(*a) != 0:
                raise RuntimeError(tools.frh_last_error().decode())

        t0, launches = time.time(), 0
        while time.time() - t0 < args.seconds:
            for _ in range(50):
                call(xs[launches % 3])
                launches += 1
            torch.cuda.synchronize()
        call(xs[launches % 3])
        torch.cuda.synchronize()
        s = stamps.cpu().numpy().reshape(wgs, 4, 2).astype(np.float64)
    cyc, rt = s[:, :, 0], s[:, :, 1]
    clock = (cyc[:, 2] - cyc[:, 1]) / (rt[:, 2] - rt[:, 1]) * 100e6
    med = lambda v: float(np.median(v))
    life_us = (rt[:, 3] - rt[:, 0]) / 100.0
    span_us = (rt[:, 3].max() - rt[:, 0].min()) / 100.0
    res = {
        'variant': args.variant, 'launches_before': launches, 'workgroups': wgs,
        'clock_GHz': {'median': round(med(clock) / 1e9, 4), 'p5': round(float(np.percentile(clock, 5)) / 1e9, 4),
                      'p95': round(float(np.percentile(clock, 95)) / 1e9, 4)},
        'cycles': {'prologue': round(med(cyc[:, 1] - cyc[:, 0])), 'loop': round(med(cyc[:, 2] - cyc[:, 1])),
                   'epilogue': round(med(cyc[:, 3] - cyc[:, 2])), 'lifetime': round(med(cyc[:, 3] - cyc[:, 0]))},
        'lifetime_us': {'median': round(med(life_us), 2), 'p5': round(float(np.percentile(life_us, 5)), 2),
                        'p95': round(float(np.percentile(life_us, 95)), 2)},
        'launch_span_us': round(span_us, 2),
        'rounds': wgs / 256.0,
        'span_minus_rounds_x_lifetime_us': round(span_us - wgs / 256.0 * med(life_us), 2),
    }
    res['epilogue_share_of_lifetime'] = round(res['cycles']['epilogue'] / res['cycles']['lifetime'], 4)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
