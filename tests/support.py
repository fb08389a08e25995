"""What the test files share, once: the whole-detector scaffolding (moving containers between
devices, the CPU layers run as the fixtures' generators ran them, building a config's model on the
seeded weights, the comparisons with whole_<name>.json / .npz), the spies on the library's entry
points, and the inputs and references of the fused-conv and RoI tests.

Imported as `import support`: tests/ has no __init__.py, so it is found on sys.path as `inputs`
is.  A helper that two files need lives here; a helper of one file stays in that file."""
import contextlib
import copy
import hashlib
import os
import socket
import sys

import numpy as np
import pytest
import torch

import inputs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_THREADS = 8


# ----------------------------------------------------------------- containers, CPU layers
def to(x, dev):
    """x on dev: a tensor, or a (nested) list / tuple of them; anything else is passed through."""
    if torch.is_tensor(x):
        return x.to(dev)
    if isinstance(x, (list, tuple)):
        return type(x)(to(v, dev) for v in x)
    return x


def nchw(x):
    """x NCHW-contiguous, containers as in `to`."""
    if torch.is_tensor(x):
        return x.contiguous()
    return type(x)(nchw(v) for v in x) if isinstance(x, (list, tuple)) else x


@contextlib.contextmanager
def fixture_threads():
    """PyTorch's CPU convolutions round differently with the thread count (their reduction is
    split by it), so the CPU layers of a parity test run with the thread count the fixture was
    generated with: the `main` of every tests/golden/gen_*_golden.py sets FIXTURE_THREADS (8)."""
    n = torch.get_num_threads()
    torch.set_num_threads(FIXTURE_THREADS)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def on_cpu(module, dev, pinned=True):
    """Run `module` (a PyTorch conv / FC stack) on a CPU copy of itself, outputs back on dev.
    pinned: as the fixture ran it, with NCHW-contiguous inputs (PyTorch's CPU convolution rounds
    differently on the channels-last levels the HIP path writes) under fixture_threads; without,
    the inputs as they come and the thread count as it is."""
    cpu = copy.deepcopy(module).cpu()

    def forward(*args):
        with torch.no_grad(), (fixture_threads() if pinned else contextlib.nullcontext()):
            args = [to(a, 'cpu') for a in args]
            return to(cpu(*(nchw(args) if pinned else args)), dev)
    module.forward = forward


# ----------------------------------------------------------------- spies
def count_calls(monkeypatch, names):
    """Wrap the named ops.<name> functions; the returned dict counts their calls."""
    from frcnn_amd import ops
    count = {n: 0 for n in names}
    for n in names:
        orig = getattr(ops, n)

        def wrapped(*a, _orig=orig, _n=n, **kw):
            count[_n] += 1
            return _orig(*a, **kw)
        monkeypatch.setattr(ops, n, wrapped)
    return count


class EntrySpy(object):
    """The library entries called since the spy was set or cleared: `names` in call order,
    `calls` the (name, args) pairs."""

    def __init__(self):
        self.names = []
        self.calls = []

    def clear(self):
        del self.names[:]
        del self.calls[:]

    def ran(self, fn):
        """(fn(), the names of the entries it called)."""
        self.clear()
        out = fn()
        return out, list(self.names)


def spy_entries(monkeypatch):
    """Record every C-ABI entry the package calls, then call it.  Wraps ops._call, the innermost
    hook: ops.call looks it up as a module global, so every entry that goes through ops is seen."""
    from frcnn_amd import ops
    spy = EntrySpy()
    real = ops._call

    def _call(name, *args):
        spy.names.append(name)
        spy.calls.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(ops, '_call', _call)
    return spy


def no_sync(fn):
    """fn() with PyTorch's sync debug mode raising on every device-to-host synchronisation."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        return fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')


# ----------------------------------------------------------------- whole detectors
def whole_config(config_name, test_cfg_over):
    """configs/<config_name> with test_cfg_over ({section: {key: value}}) applied to its test_cfg."""
    from frcnn_amd.config import Config
    cfg = Config.fromfile(os.path.join(REPO, 'pytorch-faster-rcnn_amd', 'configs', config_name))
    for k, v in test_cfg_over.items():
        cfg.test_cfg[k].update(v)
    return cfg


def build_whole(config_name, test_cfg_over):
    from frcnn_amd.builder import build_module
    cfg = whole_config(config_name, test_cfg_over)
    return build_module(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)


def load_seeded(model, state=inputs.seeded_state):
    """Load the deterministic weights the fixtures' reference models were given (`state`: shapes
    -> arrays, inputs.seeded_state unless the fixture drew its own)."""
    sd = state({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model


def gts_on(dev, boxes, labels):
    """The numpy gt boxes and labels of inputs.ftrain_case as lists of device tensors."""
    return [torch.from_numpy(b).to(dev) for b in boxes], [torch.from_numpy(l).to(dev) for l in labels]


def use_cpu_trunk(model, x):
    """Give the detector's trunk hook (graphed_trunk) the features and RPN outputs that
    model.extract_feat / model.rpn_head -- the CPU layers of the test -- compute for x."""
    feats = model.extract_feat(x)
    rpn = model.rpn_head(feats)

    class CpuTrunk(object):
        def matches(self, img_data):
            return True

        def __call__(self, img_data):
            return feats, rpn[0], rpn[1]
    model.graphed_trunk = CpuTrunk()


def assert_losses_match(losses, ref, rel, ordered=False):
    """The loss dict against the reference's {name: value}: the same keys (in the same order if
    `ordered`), every value within rel."""
    if ordered:
        assert list(losses) == list(ref)
    else:
        assert set(losses) == set(ref)
    for k, v in ref.items():
        print(k, float(losses[k]), float(v))
    for k, v in ref.items():
        assert float(losses[k]) == pytest.approx(float(v), rel=rel), (k, float(losses[k]), float(v))


def assert_detections_match(dets, z, score_rtol, box_rtol, box_atol):
    """forward_test's (boxes [4, K], scores [K], labels [K]) per image against whole_<name>.npz
    (n, boxes_i [K, 4], scores_i, labels_i): as many images, every image with detections, in the
    reference's order, labels exact."""
    boxes, scores, labels = dets[:3]
    assert len(boxes) == int(z['n'])
    for i in range(int(z['n'])):
        rb, rs, rl = z['boxes_{}'.format(i)], z['scores_{}'.format(i)], z['labels_{}'.format(i)]
        gb = boxes[i].t().cpu().numpy()
        gs, gl = scores[i].cpu().numpy(), labels[i].cpu().numpy()
        assert len(rs) > 0 and gs.shape == rs.shape, (gs.shape, rs.shape)
        np.testing.assert_array_equal(gl, rl)
        np.testing.assert_allclose(gs, rs, rtol=score_rtol, atol=0)
        print('largest box difference', float(np.abs(gb - rb).max()), 'atol', box_atol)
        np.testing.assert_allclose(gb, rb, rtol=box_rtol, atol=box_atol)


# ----------------------------------------------------------------- fused convs
BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


def wino_magnitude(x, w):
    """|A^T| (sum_c (|G||g||G^T|) * (|B^T||d||B|)) |A| in float64 for NCHW x [n, cin, h, w] and
    w [cout, cin, 3, 3]: the sum of the magnitudes of every term Winograd F(2x2, 3x3) adds up, per
    output element (the layout of x and w in memory does not enter)."""
    n, cin, h, wd = x.shape
    ht, wt = (h + 1) // 2, (wd + 1) // 2
    xp = torch.zeros(n, cin, 2 * ht + 2, 2 * wt + 2, dtype=torch.float64)
    xp[:, :, 1:h + 1, 1:wd + 1] = x.double().abs()
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)  # n, cin, ht, wt, 4, 4
    va = BT.abs() @ d @ BT.t().abs()
    ua = G.abs() @ w.double().abs() @ G.t().abs()  # cout, cin, 4, 4
    ma = torch.einsum('ocab,nchwab->nohwab', ua, va)
    ya = AT.abs() @ ma @ AT.t().abs()  # n, cout, ht, wt, 2, 2
    return ya.permute(0, 1, 2, 4, 3, 5).reshape(n, -1, 2 * ht, 2 * wt)[:, :, :h, :wd]


def bn_params(c, g):
    """(gamma of both signs, beta, mean, var) of a frozen BN over c channels, drawn from g."""
    gamma = (torch.rand(c, generator=g) + 0.5) * torch.where(torch.rand(c, generator=g) < 0.5, -1.0, 1.0)
    beta, mean = torch.rand(c, generator=g) - 0.5, torch.rand(c, generator=g) * 2 - 1
    return gamma, beta, mean, torch.rand(c, generator=g) * 1.5 + 0.5


def ints(g, lo, hi, *size):
    """Integers of [lo, hi] as f32, drawn from g."""
    return torch.randint(lo, hi + 1, size, generator=g).float()


def block(dev, args, randomise_bn):
    """(an eval Bottleneck(*args) on dev, every BN through the caller's randomise_bn; its input)."""
    from frcnn_amd.backbones import Bottleneck
    torch.manual_seed(11)
    blk = Bottleneck(*args).to(dev).eval()
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            randomise_bn(m)
    return blk, torch.randn(2, args[0], 8, 16, device=dev)


def bottleneck_unfused(blk, x):
    """The Bottleneck's forward as conv + frh_bn_act passes, no fused conv."""
    from frcnn_amd import ops
    y = ops.bn_act(blk.conv1(x), blk.bn1)
    y = ops.bn_act(blk.conv2(y), blk.bn2)
    skip = ops.bn_act(blk.downsample[0](x), blk.downsample[1], relu=False) if blk.do_downsample else x
    return ops.bn_act(blk.conv3(y), blk.bn3, skip=skip)


def tools():
    """The tools library (tools/toolslib.py): the A/B forms the equality tests compare with."""
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import toolslib
    return toolslib.load()


def loss_values(out):
    """The three loss sums of a fused head loss's output as a numpy array."""
    return np.array([float(o.detach()) for o in out[:3]])


# ----------------------------------------------------------------- arrays, RoIs
def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def canon_ties(boxes, scores):
    """Reorder columns so that runs of equal scores are sorted by coordinates."""
    order = np.lexsort((boxes[3], boxes[2], boxes[1], boxes[0], -scores.astype(np.float64)))
    return boxes[:, order]


def rois(seed, n, batch):
    """[n, 5] (image, x1, y1, x2, y2): inputs.random_boxes, the first eight replaced by border,
    outside, degenerate and sub-pixel ones."""
    b = inputs.random_boxes(seed, n, min_wh=1.0, max_wh=500.0)
    b[:, :8] = np.array([[-20, -20, 10, 10], [990, 590, 1200, 700], [0, 0, 0, 0], [5, 5, 5.5, 5.2],
                         [998.9, 598.9, 999, 599], [-300, -300, -200, -100], [0, 0, 999, 599],
                         [100.25, 200.75, 101.0, 260.5]], np.float32).T
    bi = np.random.default_rng(seed + 1).integers(0, batch, n).astype(np.float32)
    return np.concatenate([bi[None], b], 0).T.copy()


def pathological_rois(batch):
    """RoIs whose dense tap windows defeat row bands: far larger than a 10 x 30 level, so one bin
    row's two samples lie 3.6 rows apart with every row between them inside the window (the
    channel-group kernel stages such a bin row as its 4 tap-list rows), plus RoIs hanging off
    every edge, tiny and degenerate ones."""
    r = np.array([[0, 0, 0, 400, 200], [1, -50, -40, 380, 230], [0, 3, 2, 900, 60], [1, 100, 0, 119.5, 300],
                  [0, -500, -500, 600, 600], [1, 0, 30, 119, 36], [0, 60, 10, 61, 11], [1, 119, 39, 119, 39],
                  [0, -30, -30, -1, -1], [1, 10, -10, 110, 45], [0, 0, 0, 1000, 200]], np.float32)
    r[:, 0] %= batch
    return r


# ----------------------------------------------------------------- process groups
def free_port():
    """A TCP port that was free a moment ago, for a test's own process group."""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p
