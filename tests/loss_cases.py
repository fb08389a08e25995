"""Deterministic cases for the fused detection losses (csrc/losses.hip) and their float64
references; CPU only, no kernel call.  tests/test_loss_cases_cpu.py checks that every builder
hits the edge it is named for, tests/test_gpu_losses_f64.py runs the kernels on them.

A classification case is logits x [n, C] (f32), labels [n] (int64, -1 = ignored padding row) and
the focal parameters.  The reference is the restatement of lib/losses.py in frcnn_amd.losses
(sigmoid_focal_loss, binary_cross_entropy_with_logits, cross_entropy) under autograd on
.double() copies of the same f32 inputs, over the rows that are not ignored (an ignored row's
gradient is then zero, as the kernels' contract says).  Each case also carries the same
computation in f32 on the CPU; E32 = max |g32 - g64| over the case, the reference's own f32
error, is the yardstick of the gradient bound.

A regression case is x, y, labels and beta for SmoothL1Loss.masked / class_selected, whose CPU
path (torch.where masking around smooth_l1_loss_v2) is the reference in both precisions.

The focal gamma domain the kernels support is gamma == 0 or gamma >= 1: for 0 < gamma < 1 the
derivative gamma q^(gamma-1) is infinite at q == 0 in torch as well, so that range has no case."""
import functools

import torch
import torch.nn.functional as F

from frcnn_amd import losses, utils

KINDS = ('focal', 'bce', 'softmax')
KIND_ID = {'focal': 0, 'bce': 1, 'softmax': 2}           # ops.CLS_FOCAL / CLS_SIGMOID_BCE / CLS_SOFTMAX_CE
# |x| classes: around zero; ordinary; where 1 + e^-|x| rounds to 1 in f32 (p == 1, q = 1 - pt == 0);
# far in the tail; at and past expf overflow (ln FLT_MAX = 88.72); absurd
MAGNITUDES = {'unit': (0.0, 1e-4, 1.0), 'mid': (5.0, 10.0), 'round_to_one': (16.0, 17.0, 20.0),
              'tail': (30.0, 87.0), 'exp_overflow': (88.8, 100.0), 'huge': (1e4,)}
FOCAL_PARAMS = ((0.25, 2.0), (0.5, 0.0), (0.5, 1.0), (0.25, 1.5))
LAYOUTS = ('rows', 'channel_major', 'row_slice', 'col_stride')
SCALES = (0.37, 1e-8, 1e4)                                # upstream gradients (rounded to f32)
# element counts around one workgroup (256) and the capped grid (256 x 256 = 65 536)
SIGMOID_COUNTS = ((1, 1), (255, 1), (256, 1), (257, 1), (65535, 1), (65536, 1), (65537, 1), (131075, 1),
                  (16384, 4), (16385, 4), (21846, 3))
SOFTMAX_COUNTS = ((1, 3), (257, 3), (65536, 3), (65537, 3))
L1_BETAS = (1.0 / 9.0, 0.5, 1.0)
L1_VARIANTS = ('edges', 'large', 'no_pos', 'class_select')
L1_CLASSES = 21
PAD_COLS = 5                                              # strided-view buffers are [n, C + PAD_COLS]


def f32_scale(scale):
    """The upstream gradient as the kernel reads it: `scale` rounded to f32, as a Python float."""
    return float(torch.tensor(scale, dtype=torch.float32))


# ---------------------------------------------------------------- layouts
def buffer_shape(n, c, layout):
    wide = (n, c + PAD_COLS)
    return {'rows': (n, c), 'channel_major': (c, n), 'row_slice': wide, 'col_stride': wide}[layout]


def view_of(buf, c, layout):
    """The [n, C] view of a layout's buffer: contiguous; the .t() of a contiguous [C, n]; the
    first C columns of a wider [n, C + 5] buffer (sr > C); every other column of such a buffer
    (sc = 2; C <= 6 fits)."""
    if layout == 'rows':
        return buf
    if layout == 'channel_major':
        return buf.t()
    if layout == 'row_slice':
        return buf[:, :c]
    return buf[:, :2 * c:2]


def place(x, layout, fill=float('nan')):
    """A buffer in `layout` whose view_of() equals x; the elements outside the view are `fill`
    (NaN: a kernel that reads one of them poisons its sum)."""
    n, c = x.shape
    buf = torch.full(buffer_shape(n, c, layout), fill, dtype=x.dtype)
    view_of(buf, c, layout).copy_(x)
    return buf


# ---------------------------------------------------------------- classification references
def cls_loss_torch(kind, x, lab, alpha, gamma):
    """The summed loss of the rows with lab >= 0, in x's dtype (autograd reaches x)."""
    keep = lab >= 0
    xs, ls = x[keep], lab[keep]
    c = x.shape[1]
    if kind == 'focal':
        return losses.sigmoid_focal_loss(xs, ls, alpha, gamma)
    if kind == 'bce':
        tgt = ls.view(-1, 1).to(x.dtype) if c == 1 else utils.one_hot_embedding(ls, c + 1)[:, 1:].to(x.dtype)
        return F.binary_cross_entropy_with_logits(xs, tgt, reduction='sum')
    return F.cross_entropy(xs, ls, reduction='sum')


def _with_references(case, loss_fn):
    """Adds loss64 / loss32 (Python floats) and grads[scale] = (g64, g32, E32) to a case."""
    x = case['x']
    x64 = x.double().requires_grad_(True)
    l64 = loss_fn(x64)
    g64, = torch.autograd.grad(l64, x64)
    x32 = x.clone().requires_grad_(True)
    l32 = loss_fn(x32)
    case['loss64'], case['loss32'] = float(l64), float(l32)
    case['grads'] = {}
    for s in SCALES:
        g32, = torch.autograd.grad(l32, x32, torch.tensor(s, dtype=torch.float32), retain_graph=True)
        gs = g64 * f32_scale(s)
        case['grads'][s] = (gs, g32, float((g32.double() - gs).abs().max()))
    return case


def _cls_case(kind, x, lab, alpha=0.25, gamma=2.0):
    case = dict(kind=kind, x=x, lab=lab, alpha=alpha, gamma=gamma)
    return _with_references(case, lambda v: cls_loss_torch(kind, v, lab, alpha, gamma))


def _signed(mags):
    return [s * m for m in mags for s in (1.0, -1.0)]


@functools.lru_cache(maxsize=None)
def magnitude_case(kind, mag, alpha=0.25, gamma=2.0):
    """C = 3, one row per (first value, label): row j holds the class's signed values v[j], v[j+1],
    v[j+2] (cyclically), so both signs mix within a row, and the label runs over -1 and every
    class.  For the sigmoid kinds (labels -1..3, target of column k = label == k + 1) every value
    meets target 0 and target 1; for softmax (labels -1..2) every row is labelled at its maximum
    and at its minimum logit in turn."""
    v = _signed(MAGNITUDES[mag])
    labels = [-1, 0, 1, 2] + ([3] if kind != 'softmax' else [])
    rows, lab = [], []
    for j in range(len(v)):
        for l in labels:
            rows.append([v[(j + k) % len(v)] for k in range(3)])
            lab.append(l)
    return _cls_case(kind, torch.tensor(rows, dtype=torch.float32), torch.tensor(lab, dtype=torch.int64), alpha, gamma)


def _labels(n, hi, gen, last_ignored):
    """About 25 % positives (1..hi), about 20 % ignored (-1), the rest 0, scattered."""
    r = torch.rand(n, generator=gen)
    lab = torch.zeros(n, dtype=torch.int64)
    pos = torch.randint(1, hi + 1, (n,), generator=gen)
    lab[r < 0.25] = pos[r < 0.25]
    lab[r > 0.8] = -1
    if last_ignored:
        lab[-1] = -1
    if n == 1:
        lab[0] = 1
    return lab


@functools.lru_cache(maxsize=None)
def count_case(kind, n, c):
    """randn * 3 logits at an element count next to a launch-shape threshold; the default focal
    parameters.  n = 257 and n = 65 537 end on an ignored row (the last partial workgroup and the
    first element of the second grid-stride pass)."""
    gen = torch.Generator().manual_seed(1000 * KIND_ID[kind] + 7 * c + n)
    x = torch.randn(n, c, generator=gen) * 3
    hi = c - 1 if kind == 'softmax' else c
    return _cls_case(kind, x, _labels(n, hi, gen, n in (257, 65537)))


def written_case(kind, n, c):
    """Inputs only (no reference) for the every-element-written test; softmax with C == 1 has the
    labels 0 and -1 alone."""
    gen = torch.Generator().manual_seed(77 + 1000 * KIND_ID[kind] + 7 * c + n)
    x = torch.randn(n, c, generator=gen) * 3
    hi = c - 1 if kind == 'softmax' else c
    lab = _labels(n, hi, gen, True) if hi > 0 else -(torch.rand(n, generator=gen) > 0.8).long()
    lab[-1] = -1
    return dict(kind=kind, x=x, lab=lab, alpha=0.25, gamma=2.0)


# ---------------------------------------------------------------- smooth L1
def l1_loss_torch(case, x):
    """SmoothL1Loss's CPU path on x (x's dtype); a row labelled past the last class counts as masked."""
    mod = losses.SmoothL1Loss(case['beta'])
    y = case['y'].to(x.dtype)
    lab = case['lab']
    if case['classes']:
        lab = torch.where(lab >= case['classes'], torch.zeros_like(lab), lab)
        return mod.class_selected(x, case['classes'], y, lab)
    return mod.masked(x, y, lab, case['rows_dim'])


def _l1_element(case, i, j):
    """(x, y) index of logical element (row i, column j) of a regression case."""
    if case['classes']:
        return (i, j * case['classes'] + int(case['lab'][i])), (i, j)
    return ((i, j), (i, j)) if case['rows_dim'] == 0 else ((j, i), (j, i))


def l1_diff(case, i, j):
    xi, yi = _l1_element(case, i, j)
    return float(case['x'][xi] - case['y'][yi])  # f32 subtraction, as the kernel's


@functools.lru_cache(maxsize=None)
def l1_case(beta, rows_dim, variant, n=300):
    """n rows of 4 (1200 elements: five workgroups, the last one partial).  Rows 0..4 are positive
    and carry the edge elements: x - y == +beta32 at (0, 0), -beta32 at (1, 1), 0 at (2, 2) (beta32
    = beta rounded to f32; 2 beta32 - beta32 is exact), and in 'large' +-1e4 at (3, 3) and (4, 0),
    kept apart so that they do not drown the other rows' sum.  'no_pos': every label <= 0.
    'class_select': x [n, 4 * 21] viewed [n, 4, 21], labels up to 20, row 0 labelled 20."""
    gen = torch.Generator().manual_seed(int(beta * 1000) + 10 * rows_dim + L1_VARIANTS.index(variant))
    classes = L1_CLASSES if variant == 'class_select' else 0
    if classes and rows_dim != 0:
        raise AssertionError('class select has rows along dim 0')
    lab = _labels(n, classes - 1 if classes else 1, gen, True)
    lab[:5] = 1
    if classes:
        lab[0], lab[7] = classes - 1, classes - 1
    if variant == 'no_pos':
        lab.clamp_(max=0)
    x = torch.randn(n, 4 * max(classes, 1), generator=gen) * 0.5
    y = torch.randn(n, 4, generator=gen) * 0.5
    if rows_dim == 1:
        x, y = x.t().contiguous(), y.t().contiguous()
    case = dict(x=x, y=y, lab=lab, beta=beta, rows_dim=rows_dim, classes=classes, variant=variant, n=n)
    b32 = f32_scale(beta)
    edges = [((0, 0), 2 * b32, b32), ((1, 1), b32, 2 * b32), ((2, 2), 0.375, 0.375)]
    if variant == 'large':
        edges += [((3, 3), 1e4, 0.0), ((4, 0), 0.0, 1e4)]
    for (i, j), xv, yv in edges:
        xi, yi = _l1_element(case, i, j)
        x[xi], y[yi] = xv, yv
    return _with_references(case, lambda v: l1_loss_torch(case, v))


@functools.lru_cache(maxsize=None)
def l1_rows_case(n, beta=1.0 / 9.0):
    """n rows of 4 along dim 0 for the one-launch head loss's unequal halves: up to 3 rows all
    positive (one workgroup), otherwise labelled as everywhere else."""
    gen = torch.Generator().manual_seed(900 + n)
    lab = torch.ones(n, dtype=torch.int64) if n <= 3 else _labels(n, 1, gen, True)
    x = torch.randn(n, 4, generator=gen) * 0.5
    y = torch.randn(n, 4, generator=gen) * 0.5
    case = dict(x=x, y=y, lab=lab, beta=beta, rows_dim=0, classes=0, variant='rows', n=n)
    return _with_references(case, lambda v: l1_loss_torch(case, v))


@functools.lru_cache(maxsize=None)
def l1_bad_label_case(n=40):
    """Class select with row 3 labelled 21 == n_sel: the forward is NaN, the backward leaves that
    row alone; the gradient reference treats the row as masked."""
    gen = torch.Generator().manual_seed(4321)
    lab = _labels(n, L1_CLASSES - 1, gen, True)
    lab[:5] = torch.tensor([L1_CLASSES - 1, 1, 2, L1_CLASSES, 5])
    x = torch.randn(n, 4 * L1_CLASSES, generator=gen) * 0.5
    y = torch.randn(n, 4, generator=gen) * 0.5
    case = dict(x=x, y=y, lab=lab, beta=1.0, rows_dim=0, classes=L1_CLASSES, variant='bad_label', n=n)
    return _with_references(case, lambda v: l1_loss_torch(case, v))


def l1_selected_mask(case):
    """Bool mask over x of the elements the backward may write: the four (selected-class) elements
    of every row with 0 < label < n_sel."""
    mask = torch.zeros_like(case['x'], dtype=torch.bool)
    n_sel = case['classes'] or 1
    for i in (case['lab'] > 0).nonzero().view(-1).tolist():
        if case['classes'] and int(case['lab'][i]) >= n_sel:
            continue
        for j in range(4):
            mask[_l1_element(case, i, j)[0]] = True
    return mask
