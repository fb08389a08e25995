"""What the timing tools under tools/ share: the paths, the event-pair timer, the repetition
loop, the rule by which a fused path is dispatched, the peaks and the two counters.  This file
is the definition of the measurement method DESIGN section 4 quotes; each tool keeps its own
shapes, sides, byte and FLOP formulas, flags and printed lines, and passes its protocol (calls
per window, repetitions, warm-up calls, hold or no hold, order of the sides) as arguments.

Importing it puts pytorch-faster-rcnn_amd on sys.path and does not touch the device."""
import collections
import json
import os
import sys
import warnings

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'pytorch-faster-rcnn_amd'))

PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12  # MI355X: f32 MFMA FLOP/s, HBM B/s

Stat = collections.namedtuple('Stat', 'median min max runs')  # us per call over the repetitions of one side


def on_path(*parts):
    """Put REPO/parts on sys.path: () for bench.py, ('tests', 'golden') for the fixtures' loaders."""
    sys.path.insert(0, os.path.join(REPO, *parts))


def require_gpu(tool_name):
    if not torch.cuda.is_available():
        raise SystemExit('{} needs a HIP device'.format(tool_name))


def write_json(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(res, f, indent=1)


def rotate(fns, n):
    """The n calls of one window in order: fns itself, or fns[i % len(fns)] of a list."""
    fns = fns if isinstance(fns, (list, tuple)) else [fns]
    return (fns[i % len(fns)] for i in range(n))


def time_calls(fns, iters, sleep, warmup=0):
    """us per call of `iters` back-to-back calls (see rotate) between one HIP event pair.
    sleep: the calls are queued behind a GPU hold, so the host runs ahead of the device.
    warmup: that many calls and a synchronise before the window."""
    for f in rotate(fns, warmup):
        f()
    if warmup:
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if sleep:
        torch.cuda._sleep(100000000)
    e0.record()
    for f in rotate(fns, iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def stat_of(runs):
    return Stat(float(np.median(runs)), float(min(runs)), float(max(runs)), list(runs))


def measure(sides, iters, reps, warmup, reverse=False, sleep=True, timer=time_calls):
    """{side: Stat} of `reps` windows per side.  sides: {name: callable or list of callables};
    iters: calls per window, or {name: calls}.  Every callable is first called `warmup` times,
    then one synchronise; each repetition times the sides in the given order, or, with reverse,
    in the reversed order on the odd ones.  timer stands in for time_calls in the tests."""
    for fns in sides.values():
        for f in (fns if isinstance(fns, (list, tuple)) else [fns]):
            for _ in range(warmup):
                f()
    if warmup:
        torch.cuda.synchronize()
    runs = {k: [] for k in sides}
    for rep in range(reps):
        for k in (list(sides)[::-1] if reverse and rep % 2 else list(sides)):
            runs[k].append(timer(sides[k], iters[k] if isinstance(iters, dict) else iters, sleep=sleep))
    return {k: stat_of(v) for k, v in runs.items()}


def compare(a, b, iters_a, iters_b, warmup, reps=5):
    """Two callables without the hold, alternating: (median a, median b, all a, all b) in us."""
    s = measure({'a': a, 'b': b}, {'a': iters_a, 'b': iters_b}, reps, warmup, sleep=False)
    return s['a'].median, s['b'].median, [round(v, 2) for v in s['a'].runs], [round(v, 2) for v in s['b'].runs]


def wins(stat, a, b):
    """True only when side a's slowest repetition is strictly below side b's fastest.  This is
    the rule the exclusion tables of frcnn_amd/ops.py follow (_CONV1X1_EXCLUDED,
    _CONV1X1_PRE_EXCLUDED, _CONV1X1_S2_EXCLUDED, _CONV3X3_EXCLUDED, _CONV3X3_NCHW_EXCLUDED,
    _HEAD_CONVS_EXCLUDED): a class is dispatched to the fused kernel only where wins(stat,
    fused, parent) held; a lower median with overlapping spreads is not a win."""
    return bool(stat[a][2] < stat[b][1])


def put_times(row, stat, digits):
    """row['<side>_us'] = median and row['<side>_us_min_max'] = [min, max] for every side."""
    for k, s in stat.items():
        row[k + '_us'] = round(s[0], digits)
        row[k + '_us_min_max'] = [round(s[1], digits), round(s[2], digits)]
    return row


def limit(flops, nbytes):
    """(us, which): the larger of flops / PEAK_FLOPS and nbytes / PEAK_BYTES, and its name."""
    compute, bandwidth = flops / PEAK_FLOPS, nbytes / PEAK_BYTES
    return max(compute, bandwidth) * 1e6, 'compute' if compute > bandwidth else 'bandwidth'


def max_rel_diff(ref, got):
    """max |ref - got| / max |ref| of two tensors; of (nested) lists of them, the largest."""
    if torch.is_tensor(ref):
        return float((ref - got).abs().max() / ref.abs().max())
    return max(max_rel_diff(a, b) for a, b in zip(ref, got))


def count_launches(fn):
    """Device kernels of one call (None when the profiler gives no device activity here)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')
                and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())
        return n or None
    except Exception as exc:  # the profiler is optional equipment of the tools
        print('profiler unavailable: {}'.format(exc), file=sys.stderr)
        return None


def count_syncs(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    return sum(1 for x in w if 'synchroniz' in str(x.message).lower())
