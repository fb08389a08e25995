"""The dense entries under the guarded allocator (tests/guarded.py): every case runs one entry on
plain tensors as its own test file does, then twice with guarded copies of the inputs and guarded
outputs and workspaces, once 0x00-filled and once 0xFF-filled (guarded.sweep).  Asserted per case:
every guard band intact (no store outside an output or a workspace), every float output
poison-free and finite, the two guarded runs bit-identical (no output element left unwritten, no
workspace word read before it is written) and bit-identical to the plain call (an over-read of an
input picks up the guards' NaN).  The float64 bars of the entries' own files are not repeated:
equality with the call those files validate carries them.

Shapes and input builders are those of the entries' own test files (imported inside the cases:
this module must import without a device, tests/test_guarded_cpu.py reads its case table).  Where
that file's caller allocates with torch.empty it is called as it is (the allocator reroutes it);
where it NaN-fills its output (torch.full) the file's caller takes the output allocator as an
argument and the case passes torch.empty; where the file itself goes through the ops wrapper so
does the case, and checks that the entry really ran.  A strided input view is copied with its own strides and extent, so the guard
sits behind the view's last element; test_conv3x3_strided_view copies the parent instead, as
test_strided_view_equals_its_copy lays it out.

Every call is a valid one: sizes, strides and workspace sizes are what include/frcnn_amd.h
documents.  frh_deform_conv3x3_bwd and the float-atomic RoI backwards sum with float atomics, so
their runs are compared at their own files' tolerances (quoted at the cases) instead of bit for
bit.

Every entry of this file's families is in a case: NOT_GUARDED (name -> reason, for an entry that
cannot be guarded) is empty here.
"""
import pytest
import torch

import guarded

pytestmark = pytest.mark.gpu
CL = torch.channels_last
EPS = 1e-5

NOT_GUARDED = {}
CASES = []
# With the ReLU on (and a skip, a bias, a BN where the entry has one) as the trunk runs them, and with
# it off: v_max_f32 returns the other operand for a NaN, so a ReLU turns the NaN of an over-read or
# of a poisoned workspace word into 0, which only differs from the right value where that is positive.
RELUS = (True, False)


def case(name, *entries):
    def add(fn):
        CASES.append((name, entries, fn))
        return fn
    return add


def swept_entries():
    return {e for _, entries, _ in CASES for e in entries}


def _dev():
    return torch.device('cuda', 0)


def _lib():
    from frcnn_amd import _lib
    return _lib


def _empty(shape, dev):
    """The output allocator handed to the test files' callers: torch.empty, which the allocator reroutes."""
    return torch.empty(shape, device=dev)


def _empty_level(n, c, x):
    return torch.empty((n, c, x.shape[2], x.shape[3]), device=x.device, memory_format=CL)


# ----------------------------------------------------------------- 1x1 convs
def _conv1x1_cases():
    import test_gpu_conv1x1 as t
    return t


for _i in range(5):
    @case('conv1x1[{}]'.format(_i), 'frh_conv1x1_bn_act')
    def _conv1x1(mp, i=_i):
        t = _conv1x1_cases()
        shape = t.SHAPES[i]
        for relu in RELUS:
            guarded.sweep(mp, lambda d: t._fused(d, True, relu), lambda: dict(t._on_dev(shape, _dev())),
                          ['frh_conv1x1_bn_act'])

    @case('conv1x1_pre[{}]'.format(_i), 'frh_conv1x1_bn_act_pre')
    def _conv1x1_pre(mp, i=_i):
        import test_gpu_conv1x1_pre as t
        shape = t.SHAPES[i]
        for relu in RELUS:
            guarded.sweep(mp, lambda d: t._pre(d, d['x'], d['skip'], relu, alloc=_empty),
                          lambda: dict(t._case(*shape, _dev())), ['frh_conv1x1_bn_act_pre'])


@case('conv1x1_s2[odd_h]', 'frh_conv1x1_s2_bn_act')
def _conv1x1_s2(mp):
    """The (6, 8) output plane of S2_PLANES from an input with 11 rows, and the (2, 4) one."""
    import test_gpu_conv1x1_pre as t
    for cin, cout, h, w in ((64, 128, 11, 16), (256, 512, 4, 8)):
        for relu in RELUS:
            guarded.sweep(mp, lambda d: t._s2(d, d['x'], d['skip2'], relu, alloc=_empty),
                          lambda: dict(t._case(2, cin, cout, h, w, _dev())), ['frh_conv1x1_s2_bn_act'])


# ----------------------------------------------------------------- Winograd 3x3, channels-last
for _shape in ((1, 8, 64, 3, 5), (2, 64, 64, 19, 32), (1, 32, 192, 17, 34)):
    @case('conv3x3[{}]'.format('-'.join(map(str, _shape))), 'frh_conv3x3_bias_act')
    def _conv3x3(mp, shape=_shape):
        """The workspace is exactly 16 cin cout floats (the file's own _fused)."""
        import test_gpu_conv3x3 as t
        assert shape in t.SHAPES
        for relu in RELUS:
            guarded.sweep(mp, lambda d: t._fused(d['x'], d['w'], d['bias'], relu), lambda: dict(t._on_dev(shape, _dev())),
                          ['frh_conv3x3_bias_act'])


@case('conv3x3[strided_view]', 'frh_conv3x3_bias_act')
def _conv3x3_view(mp):
    """test_strided_view_equals_its_copy's input: the parent is copied, so the guard sits right
    behind the parent's last element, one column past the view's."""
    import test_gpu_conv3x3 as t
    g = torch.Generator().manual_seed(5)
    p5 = torch.randn(2, 64, 19, 32, generator=g).to(_dev()).contiguous(memory_format=CL)
    w = torch.randn(64, 64, 3, 3, generator=g).to(_dev()).contiguous(memory_format=CL)
    b = torch.randn(64, generator=g).to(_dev())
    for relu in RELUS:
        guarded.sweep(mp, lambda a: t._fused(a[0][:, :, ::2, ::2], a[1], a[2], relu), lambda: (p5, w, b),
                      ['frh_conv3x3_bias_act'])


def _levels_call(xs, ws, bs, relu):
    """frh_conv3x3_bias_act_levels as test_levels_launch_equals_per_level_launches calls it."""
    L = _lib()
    n, cin = xs[0].shape[:2]
    cout = ws[0].shape[0]
    distinct = len({w.data_ptr() for w in ws})
    ys = [torch.empty(n, cout, x.shape[2], x.shape[3], device=x.device, memory_format=CL) for x in xs]
    work = torch.empty(distinct * 16 * cin * cout, device=xs[0].device)
    nul = (L.c_vp * len(xs))(*[None if b is None else b.data_ptr() for b in bs])
    L.call('frh_conv3x3_bias_act_levels', len(xs), L.ptr_array(xs), L.ptr_array(ws), nul, L.ptr_array(ys), L.ptr(work),
           work.numel() * 4, n, cin, cout, L.i32_array([v for x in xs for v in x.shape[2:]]),
           L.i64_array([v for x in xs for v in (x.stride(0), x.stride(2), x.stride(3))]), int(relu),
           L.stream_of(work))
    return ys


for _shared in (True, False):
    @case('conv3x3_levels[{}]'.format('shared' if _shared else 'per_level'), 'frh_conv3x3_bias_act_levels')
    def _conv3x3_levels(mp, shared=_shared):
        """Five levels from 19 x 32 down to 2 x 2 in one launch, one weight or one per level."""
        g = torch.Generator().manual_seed(7)
        cin, cout, n = 32, 128, 2
        sizes = ((19, 32), (10, 16), (5, 8), (3, 4), (2, 2))
        xs = [torch.randn(n, cin, h, w, generator=g).to(_dev()).contiguous(memory_format=CL) for h, w in sizes]
        ws = [torch.randn(cout, cin, 3, 3, generator=g).to(_dev()).contiguous(memory_format=CL)
              for _ in range(1 if shared else 5)]
        bs = [torch.randn(cout, generator=g).to(_dev()) for _ in range(5)]

        def run(a, relu):
            xs, ws, bs = a
            return _levels_call(xs, ws * 5 if shared else ws, bs, relu)
        for relu in RELUS:
            guarded.sweep(mp, lambda a: run(a, relu), lambda: (xs, ws, bs), ['frh_conv3x3_bias_act_levels'])


for _shape in ((1, 8, 64, 4, 6), (1, 64, 64, 7, 9), (2, 64, 128, 6, 10)):
    @case('conv3x3_pool[{}]'.format('-'.join(map(str, _shape))), 'frh_conv3x3_bias_act_pool')
    def _conv3x3_pool(mp, shape=_shape):
        """Even and odd planes (the pool drops an odd last row and column)."""
        L = _lib()
        n, cin, cout, h, w = shape
        g = torch.Generator().manual_seed(9000 + cin + h * w)
        x = torch.randn(n, cin, h, w, generator=g).to(_dev()).contiguous(memory_format=CL)
        wt = torch.randn(cout, cin, 3, 3, generator=g).to(_dev()).contiguous(memory_format=CL)
        b = torch.randn(cout, generator=g).to(_dev())

        def run(a):
            x, wt, b = a
            y = torch.empty(n, cout, h // 2, w // 2, device=x.device, memory_format=CL)
            ws = torch.empty(16 * cin * cout, device=x.device)
            L.call('frh_conv3x3_bias_act_pool', L.ptr(x), L.ptr(wt), L.ptr(b), L.ptr(y), L.ptr(ws), n, cin, cout, h, w,
                   x.stride(0), x.stride(2), x.stride(3), 1, L.stream_of(x))
            return y
        guarded.sweep(mp, run, lambda: (x, wt, b), ['frh_conv3x3_bias_act_pool'])


@case('nchw_to_nhwc8', 'frh_nchw_to_nhwc8')
def _nhwc8(mp):
    L = _lib()
    for n, cin, h, w in ((1, 3, 5, 7), (2, 3, 19, 33), (1, 1, 1, 1)):
        img = torch.randn(n, cin, h, w, generator=torch.Generator().manual_seed(h)).to(_dev())

        def run(img):
            x8 = torch.empty((n, h, w, 8), device=img.device)
            L.call('frh_nchw_to_nhwc8', L.ptr(img), L.ptr(x8), n, cin, h, w, L.stream_of(img))
            return x8
        guarded.sweep(mp, run, lambda: img, ['frh_nchw_to_nhwc8'])


# ----------------------------------------------------------------- Winograd 3x3, NCHW + BN
def _nchw_shapes():
    import test_gpu_conv3x3_nchw as a
    import test_gpu_conv3x3_nchw_lds as b
    return a, list(a.SHAPES) + [s for s in b.SHAPES if s not in a.SHAPES]


for _i in range(8):
    @case('conv3x3_nchw[{}]'.format(_i), 'frh_conv3x3_nchw_bn_act')
    def _conv3x3_nchw(mp, i=_i):
        """The four shapes of test_gpu_conv3x3_nchw.py, then the four of _lds.py it does not have:
        (1, 4, 16, 3, 8), (1, 20, 32, 5, 34), (1, 32, 48, 17, 36), (2, 48, 192, 2, 2)."""
        t, shapes = _nchw_shapes()
        assert len(shapes) == 8
        for relu in RELUS:
            guarded.sweep(mp, lambda d: t._fused(d['x'], d['w'], d['bn'], relu), lambda: dict(t._on_dev(shapes[i], _dev())),
                          ['frh_conv3x3_nchw_bn_act'])


# ----------------------------------------------------------------- head output convs, RPN 1x1 heads, RoI tiles
for _i in range(6):
    @case('conv3x3_out[{}]'.format(_i), 'frh_conv3x3_out_levels')
    def _conv3x3_out(mp, i=_i):
        """The file's _entry (bias and scale epilogues on) with torch.empty outputs."""
        import test_gpu_conv3x3_out as t
        c = t.CASES[i]
        guarded.sweep(mp, lambda d: t._entry(d['xs'], d['ws'], d['bs'], d['scales'], mk=_empty_level),
                      lambda: dict(t._on_dev(c, 'randn', _dev())), ['frh_conv3x3_out_levels'])


for _i in range(3):
    @case('rpn_head1x1[{}]'.format(_i), 'frh_rpn_head1x1_levels')
    def _rpn_head1x1(mp, i=_i):
        """The file's _entry with torch.empty outputs."""
        import test_gpu_rpn_head1x1 as t
        guarded.sweep(mp, lambda d: t._entry(d['xs'], d['wc'], d['bc'], d['wr'], d['br'], mk=_empty_level),
                      lambda: dict(t._on_dev(t.CASES[i], 'randn', _dev())), ['frh_rpn_head1x1_levels'])


for _i in range(4):
    @case('roi_conv3x3[{}]'.format(_i), 'frh_roi_conv3x3_bn_act')
    def _roi_conv3x3(mp, i=_i):
        """The four SHAPES of the file through its _fused, workspace of the size query."""
        import test_gpu_roi_conv3x3 as t
        shape = t.SHAPES[i]
        for relu in RELUS:
            guarded.sweep(mp, lambda d: t._fused(d['x'], d['w'], d['bn'], relu),
                          lambda: dict(t._on_dev('randn', shape, _dev())), ['frh_roi_conv3x3_bn_act'])


# ----------------------------------------------------------------- deformable conv
def _deform(mp, n, cin, cout, dg, h, w, seed, view=False):
    import test_gpu_deform_conv as t
    from frcnn_amd import ops
    _, (x, off, wt) = t._inputs(_dev(), n, cin, cout, dg, 2 * h - 1 if view else h, 2 * w - 1 if view else w, seed=seed)
    if view:
        _, (_, off, _) = t._inputs(_dev(), n, cin, cout, dg, h, w, seed=seed + 1)
    for relu in RELUS:
        guarded.sweep(mp, lambda a: ops.deform_conv3x3(a[0][:, :, ::2, ::2] if view else a[0], a[1], a[2], dg, relu=relu),
                      lambda: (x, off, wt), ['frh_deform_conv3x3_act'])


def _one_pixel(x):
    """A [n, c, 1, 1] map with the strides (c, 1, c, c).  .contiguous(channels_last) leaves a
    one-pixel map at (c, 1, 1, 1), whose column stride 1 < cin ops takes for a reason to run the
    restatement (so does test_vs_restatement at 1 x 1); the header takes any sx >= cin."""
    n, c = x.shape[:2]
    v = torch.empty_strided((n, c, 1, 1), (c, 1, c, c), dtype=x.dtype, device=x.device)
    return v.copy_(x)


@case('deform[1x1]', 'frh_deform_conv3x3_act')
def _deform_1x1(mp):
    """(2, 32, 64, dg 4) at 1 x 1, explicit and guided: two positions in a 64-position tile, every
    neighbour tap outside the map.  No other test runs the entry at this size, so each result is
    also held to test_gpu_deform_conv.py's bar against the f64 restatement (its _check)."""
    import test_gpu_deform_conv as t
    from frcnn_amd import ops
    host, (x, off, wt) = t._inputs(_dev(), 2, 32, 64, 4, 1, 1, seed=65)
    x = _one_pixel(x)
    for relu in RELUS:
        for y in guarded.sweep(mp, lambda a: ops.deform_conv3x3(a[0], a[1], a[2], 4, relu=relu), lambda: (x, off, wt),
                               ['frh_deform_conv3x3_act']):
            t._check(y[0], host, 4, relu=relu)
    xs, ss, offs, ow, wt = t._guided(_dev(), [(1, 1)])
    xs = [_one_pixel(xs[0])]
    runs = guarded.sweep(mp, lambda a: [ops.deform_conv3x3(a[0], a[1], a[3], 4, relu=True, offset_weight=a[2]),
                                        ops.deform_conv3x3(a[0], a[4], a[3], 4, relu=True)],
                         lambda: (xs[0], ss[0], ow, wt, offs[0]), ['frh_deform_conv3x3_act'])
    assert guarded.same_bits(runs[0][0], runs[0][1])  # guided == explicit on the same offsets


@case('deform[5x7]', 'frh_deform_conv3x3_act')
def _deform_5x7(mp):
    _deform(mp, 2, 32, 64, 4, 5, 7, 69)


@case('deform[19x32]', 'frh_deform_conv3x3_act')
def _deform_19x32(mp):
    _deform(mp, 2, 32, 64, 4, 19, 32, 83)


@case('deform[256ch_6x6]', 'frh_deform_conv3x3_act')
def _deform_256(mp):
    _deform(mp, 2, 256, 256, 4, 6, 6, 21)


@case('deform[stride2_view]', 'frh_deform_conv3x3_act')
def _deform_view(mp):
    """x[:, :, ::2, ::2] of a 9 x 13 channels-last parent; the parent is what is copied."""
    _deform(mp, 2, 32, 64, 4, 5, 7, 23, view=True)


@case('deform[guided]', 'frh_deform_conv3x3_act')
def _deform_guided(mp):
    import test_gpu_deform_conv as t
    from frcnn_amd import ops
    xs, ss, _, ow, wt = t._guided(_dev(), [(5, 7), (19, 32)])
    guarded.sweep(mp, lambda a: [ops.deform_conv3x3(x, s, a[3], 4, relu=True, offset_weight=a[2])
                                 for x, s in zip(a[0], a[1])],
                  lambda: (xs, ss, ow, wt), ['frh_deform_conv3x3_act'])


for _guided in (True, False):
    @case('deform_levels[{}]'.format('guided' if _guided else 'explicit'), 'frh_deform_conv3x3_act_levels')
    def _deform_levels(mp, guided_=_guided):
        """test_levels_equal_the_per_level_calls: five levels, the last a stride-2 view of a 3 x 3 map."""
        import test_gpu_deform_conv as t
        from frcnn_amd import ops
        xs, ss, offs, ow, wt = t._guided(_dev(), [(19, 32), (10, 16), (5, 8), (3, 4), (2, 2)], seed=32)
        big = torch.randn(2, 32, 3, 3, generator=torch.Generator().manual_seed(33)).to(_dev()).contiguous(memory_format=CL)

        def run(a):
            big, xs, maps, ow, wt = a
            xs = list(xs[:4]) + [big[:, :, ::2, ::2]]
            return ops.deform_conv3x3_levels(xs, maps, wt, 4, relu=True, offset_weight=ow if guided_ else None)
        guarded.sweep(mp, run, lambda: (big, xs, ss if guided_ else offs, ow, wt), ['frh_deform_conv3x3_act_levels'])


def _deform_bwd(mp, shape, seed, relu=False, view=False):
    """Forward and backward through ops.deform_conv3x3(hip_grad=True).  gx and goff are summed with
    float atomics, so each run is held to test_gpu_deform_conv_bwd.py's own bar against the f64
    autograd of the restatement -- per gradient element |err| <= (n_terms + 8) 2^-24 sum |terms|,
    n_terms = cout + the most samples touching one input element (gx), cout + 4 cin / dg (goff),
    n h w (gw) -- by that file's _check_all; y and the guards are compared as everywhere."""
    import test_gpu_deform_conv_bwd as t
    from frcnn_amd import ops
    n, cin, cout, dg, h, w = shape
    host, gy = t._case(n, cin, cout, dg, h, w, seed=seed)
    if view:
        (xb, _, _), _ = t._case(n, cin, cout, dg, 2 * h - 1, 2 * w - 1, seed=seed - 1)
        host = [xb, host[1], host[2]]
    dev_in = [host[0].to(_dev()).contiguous(memory_format=CL), host[1].to(_dev()), host[2].to(_dev()), gy.to(_dev())]

    def run(a):
        x, off, wt, g = [v.detach().requires_grad_(i < 3) for i, v in enumerate(a)]
        y = ops.deform_conv3x3(x[:, :, ::2, ::2] if view else x, off, wt, dg, relu=relu, hip_grad=True)
        y.backward(g)
        return [y.detach(), x.grad, off.grad, wt.grad]
    plain, clean, poison = guarded.sweep(mp, run, lambda: dev_in, ['frh_deform_conv3x3_act', 'frh_deform_conv3x3_bwd'],
                                         bits=False)
    ref_host = [host[0][:, :, ::2, ::2].contiguous(), host[1], host[2]] if view else host
    for y, gx, goff, gw in (plain, clean, poison):
        assert guarded.same_bits(y, plain[0])
        mask = (y > 0).cpu() if relu else torch.ones_like(gy, dtype=torch.bool)
        t._check_all(ref_host, gy * mask, dg, (gx[:, :, ::2, ::2] if view else gx, goff, gw))
        if view:
            keep = torch.zeros(2 * h - 1, 2 * w - 1, dtype=torch.bool)
            keep[::2, ::2] = True
            assert bool((gx[:, :, ~keep] == 0).all())


@case('deform_bwd[5x7]', 'frh_deform_conv3x3_bwd')
def _deform_bwd_5x7(mp):
    _deform_bwd(mp, (2, 32, 64, 4, 5, 7), 69)


@case('deform_bwd[5x7_relu_128]', 'frh_deform_conv3x3_bwd')
def _deform_bwd_relu(mp):
    _deform_bwd(mp, (2, 32, 128, 4, 5, 7), 133, relu=True)


@case('deform_bwd[stride2_view]', 'frh_deform_conv3x3_bwd')
def _deform_bwd_view(mp):
    _deform_bwd(mp, (2, 32, 64, 4, 5, 7), 24, view=True)


# ----------------------------------------------------------------- BN, bias, FPN merge, BFP
def _bn(c, seed):
    import support
    return [t.to(_dev()) for t in support.bn_params(c, torch.Generator().manual_seed(seed))]


for _shape in ((1, 8, 7, 16), (1, 4, 10, 24), (2, 64, 76, 128)):
    @case('bn_act[{}]'.format('-'.join(map(str, _shape))), 'frh_bn_act')
    def _bn_act(mp, shape=_shape):
        L = _lib()
        n, c, h, w = shape
        g = torch.Generator().manual_seed(c + h)
        x, skip = torch.randn(*shape, generator=g).to(_dev()), torch.randn(*shape, generator=g).to(_dev())
        bn = _bn(c, 5)

        def run(a, relu):
            x, skip, bn = a
            y = torch.empty_like(x)
            L.call('frh_bn_act', L.ptr(x), L.ptr(skip), L.ptr(y), *[L.ptr(t) for t in bn], EPS, n, c, h * w, int(relu),
                   L.stream_of(x))
            return y
        for relu in RELUS:
            guarded.sweep(mp, lambda a: run(a, relu), lambda: (x, skip, bn), ['frh_bn_act'])

    @case('bn_act_maxpool[{}]'.format('-'.join(map(str, _shape))), 'frh_bn_act_maxpool')
    def _bn_act_maxpool(mp, shape=_shape):
        """The stem's BN + ReLU + 3x3 / stride-2 / padding-1 max pool: output ((h - 1) // 2 + 1, w // 2)."""
        L = _lib()
        n, c, h, w = shape
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(c + w)).to(_dev())
        bn = _bn(c, 6)

        def run(a):
            x, bn = a
            y = torch.empty(n, c, (h - 1) // 2 + 1, w // 2, device=x.device)
            L.call('frh_bn_act_maxpool', L.ptr(x), L.ptr(y), *[L.ptr(t) for t in bn], EPS, n, c, h, w, L.stream_of(x))
            return y
        guarded.sweep(mp, run, lambda: (x, bn), ['frh_bn_act_maxpool'])


@case('bias_act_nhwc', 'frh_bias_act_nhwc')
def _bias_act(mp):
    """In place on a channels-last tensor: the shapes of test_conv_bias_relu_bit_exact's small cases."""
    L = _lib()
    for shape in ((2, 256, 10, 16), (1, 64, 7, 9)):
        g = torch.Generator().manual_seed(shape[2])
        y0 = torch.randn(*shape, generator=g).to(_dev()).contiguous(memory_format=CL)
        b = torch.randn(shape[1], generator=g).to(_dev())

        def run(a):
            y, b = a
            n, c, h, w = y.shape
            L.call('frh_bias_act_nhwc', L.ptr(y), L.ptr(b), n * h * w, c, 1, L.stream_of(y))
            return y
        guarded.sweep(mp, run, lambda: (y0.clone(memory_format=torch.preserve_format), b), ['frh_bias_act_nhwc'])


for _name, _shape, _up, _bias in (('up', (2, 64, 25, 38), (13, 19), False), ('no_up', (1, 96, 19, 30), None, False),
                                  ('scalar', (2, 8, 7, 6), (4, 3), False), ('bias_up', (2, 6, 7, 6), (4, 3), True),
                                  ('bias_no_up', (1, 96, 19, 30), None, True)):
    @case('fpn_merge[{}]'.format(_name), 'frh_fpn_merge_nhwc')
    def _fpn_merge(mp, shape=_shape, up_shape=_up, bias=_bias):
        """test_gpu_nhwc.py's shapes: the whole lateral, then its [:, :, :, :w - 1] view (the parent
        is what is copied)."""
        from frcnn_amd import ops
        g = torch.Generator().manual_seed(3)
        lat = torch.randn(*shape, generator=g).to(_dev())
        up = torch.randn(shape[0], shape[1], *up_shape, generator=g).to(_dev()).contiguous(memory_format=CL) \
            if up_shape else None
        b = torch.randn(shape[1], generator=g).to(_dev()) if bias else None
        for cut in (0, 1):
            guarded.sweep(mp, lambda a: ops.fpn_merge_nhwc(a[0][:, :, :, :shape[3] - cut], a[1], a[2]),
                          lambda: (lat, up, b), ['frh_fpn_merge_nhwc'])


def _bfp_case(name):
    import test_gpu_bfp as t
    (c,) = [c for c in t.FWD_CASES if c[0] == name]
    return t, c


for _name in ('ragged', 'scalar_c3', 'ragged_view', 'multi_block'):
    @case('bfp[{}]'.format(_name), 'frh_bfp_fwd', 'frh_bfp_bwd')
    def _bfp(mp, name=_name):
        """Forward with the argmax maps and backward (fixed-order sums: bit for bit).  A view level
        is copied with its own strides."""
        import libra_inputs
        import numpy as np
        from frcnn_amd import ops
        t, (_, sizes, channels, r, how) = _bfp_case(name)
        feats = [t._layout(a, how, _dev(), i == len(sizes) - 1)
                 for i, a in enumerate(libra_inputs.bfp_levels(50, sizes, channels))]
        rng = np.random.default_rng(51)
        gouts = [torch.from_numpy(rng.standard_normal(tuple(f.shape)).astype(np.float32)).to(_dev()) for f in feats]

        def run(a):
            xs = [f.detach().requires_grad_(True) for f in a[0]]
            outs = ops.bfp(xs, r)
            torch.autograd.backward(outs, list(a[1]))
            return [[o.detach() for o in outs], [x.grad for x in xs]]
        guarded.sweep(mp, run, lambda: (feats, gouts), ['frh_bfp_fwd', 'frh_bfp_bwd'])


# ----------------------------------------------------------------- RoIAlign, RoIPool
def _roi_inputs(grids, C, seed, n_rois, patho_level, scales_levels):
    import numpy as np
    import inputs
    import oracle
    import support
    feats = inputs.feature_maps(seed, grids, C, 2)
    rois = np.concatenate([support.rois(seed + 1, n_rois, 2), support.pathological_rois(2)], 0)
    levels = oracle.roi_level_map(rois, 56.0, scales_levels)
    levels[-11:] = patho_level
    return feats, rois, levels


def _roi_align(mp, C, pooled, nhwc, grids=((38, 64), (19, 32), (10, 30)), scales=(1 / 16, 1 / 32, 1 / 4),
               deterministic=True, entries=('frh_roi_align_fwd_strided', 'frh_roi_align_bwd_fixed')):
    """support.rois and support.pathological_rois (on the 10 x 30 level) over three levels, forward
    and backward through ops.roi_align_multilevel."""
    from frcnn_amd import ops
    feats, rois, levels = _roi_inputs(grids, C, 60, 60, len(grids) - 1, len(grids) - 1)
    ft = [torch.from_numpy(f).to(_dev()) for f in feats]
    if nhwc:
        ft = [f.contiguous(memory_format=CL) for f in ft]
    rt, lt = torch.from_numpy(rois).to(_dev()), torch.from_numpy(levels).to(_dev())
    gout = torch.randn(len(rois), C, *pooled, generator=torch.Generator().manual_seed(8)).to(_dev())

    def run(a):
        ft, rt, lt, gout = a
        xs = [f.detach().requires_grad_(True) for f in ft]
        out = ops.roi_align_multilevel(xs, rt, lt, list(scales), pooled, 2)
        out.backward(gout)
        return [out.detach(), [x.grad for x in xs]]
    was = ops._DETERMINISTIC['on']
    ops.set_deterministic_backward(deterministic)
    try:
        if deterministic:
            return guarded.sweep(mp, run, lambda: (ft, rt, lt, gout), entries)
        runs = guarded.sweep(mp, run, lambda: (ft, rt, lt, gout), entries, bits=False)
        _roi_bwd_close(runs, [f.shape for f in feats], rois, levels, scales, gout)
    finally:
        ops.set_deterministic_backward(was)


def _roi_bwd_close(runs, shapes, rois, levels, scales, gout, nhwc_arrays=False):
    """The float-atomic backwards reorder their sums, so every run is held to
    test_roi_align_backward_vs_oracle's own bar against the oracle (rtol 1e-4, atol 2e-5); the
    forward outputs stay bit for bit."""
    import numpy as np
    import oracle
    ref = oracle.roi_align_bwd(list(shapes), rois, levels, list(scales), gout.cpu().numpy(), 2)
    for out, grads in [(r[0], r[1:]) for r in runs]:
        assert guarded.same_bits(out, runs[0][0])
        for g, want in zip(grads, ref):
            got = g.permute(0, 3, 1, 2) if nhwc_arrays else g
            np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-4, atol=2e-5)


for _C, _pooled in ((64, (7, 7)), (192, (7, 7)), (128, (4, 5)), (64, (1, 1))):
    @case('roi_align[cg_C{}_{}x{}]'.format(_C, *_pooled), 'frh_roi_align_fwd_strided', 'frh_roi_align_bwd_fixed')
    def _roi_align_cg(mp, C=_C, pooled=_pooled):
        """The channel-group forward's cases, channels-last, with the deterministic backward."""
        _roi_align(mp, C, pooled, True)


for _C in (16, 40):
    @case('roi_align[quad_C{}]'.format(_C), 'frh_roi_align_fwd_strided', 'frh_roi_align_bwd_strided')
    def _roi_align_quad(mp, C=_C):
        """The standalone channel-quad forward's cases: 4 x 12 bins, C 16 and 40, channels-last (no
        fixed-point backward for 12 bins: the float-atomic one)."""
        _roi_align(mp, C, (4, 12), True, grids=((19, 32), (10, 30)), scales=(1 / 32, 1 / 4), deterministic=False,
                   entries=('frh_roi_align_fwd_strided', 'frh_roi_align_bwd_strided'))


@case('roi_align[nchw_C16]', 'frh_roi_align_fwd_strided', 'frh_roi_align_bwd_fixed')
def _roi_align_nchw(mp):
    _roi_align(mp, 16, (7, 7), False)


for _nhwc in (False, True):
    @case('roi_align[atomic_bwd_{}]'.format('nhwc' if _nhwc else 'nchw'), 'frh_roi_align_bwd_strided')
    def _roi_align_atomic(mp, nhwc=_nhwc):
        _roi_align(mp, 16, (7, 7), nhwc, deterministic=False,
                   entries=('frh_roi_align_fwd_strided', 'frh_roi_align_bwd_strided'))


@case('roi_align[timed]', 'frh_roi_align_fwd_strided_timed')
def _roi_align_timed(mp):
    """The measurement entry: the strided forward launched with two events bound to its dispatch and
    a span slot (FRH_SPAN_SHARDS x FRH_SPAN_STRIDE u64, words {0, 1} of a shard {UINT64_MAX, 0}) that
    one lane per wave updates with atomic min / max.  The slot is guarded and holds clock values; the
    output is the defined part, and equals the strided entry's."""
    from frcnn_amd import ops
    L = _lib()
    grids, scales, C = ((38, 64), (19, 32), (10, 30)), [1 / 16, 1 / 32, 1 / 4], 64
    feats, rois, levels = _roi_inputs(grids, C, 60, 60, 2, 2)
    ft = [torch.from_numpy(f).to(_dev()).contiguous(memory_format=CL) for f in feats]
    rt, lt = torch.from_numpy(rois).to(_dev()), torch.from_numpy(levels).to(_dev())

    def run(a):
        ft, rt, lt = a
        span = torch.zeros(256, 16, dtype=torch.int64, device=rt.device)
        span[:, 0] = -1
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        e1.record()
        out = torch.empty(len(rois), C, 7, 7, device=rt.device)
        hw, st = ops._feat_desc(ft)
        L.call('frh_roi_align_fwd_strided_timed', len(ft), L.ptr_array(ft), hw, st, L.f32_array(scales), 2, C, L.ptr(rt),
               L.ptr(lt), len(rois), 7, 7, 2, 0, L.ptr(out), e0.cuda_event, e1.cuda_event, L.ptr(span), L.stream_of(out))
        torch.cuda.synchronize()
        assert bool((span[:, 0] != -1).any()) and e0.elapsed_time(e1) >= 0
        return out
    runs = guarded.sweep(mp, run, lambda: (ft, rt, lt), ['frh_roi_align_fwd_strided_timed'])
    with torch.no_grad():
        assert guarded.same_bits(runs[0][0], ops.roi_align_multilevel(ft, rt, lt, scales, (7, 7), 2))


for _layout in (0, 1):
    @case('roi_align[dense_layout{}]'.format(_layout), 'frh_roi_align_fwd', 'frh_roi_align_bwd')
    def _roi_align_dense(mp, layout=_layout):
        """The entries without strides (layout 0: NCHW, 1: NHWC): forward bit for bit; the backward
        adds into cleared gradients with float atomics (the tolerance of the case above)."""
        L = _lib()
        grids, C, pooled = ((38, 64), (19, 32), (10, 30)), 16, (7, 7)
        feats, rois, levels = _roi_inputs(grids, C, 60, 60, 2, 2)
        ft = [torch.from_numpy(f).to(_dev()) for f in feats]
        if layout:
            ft = [f.permute(0, 2, 3, 1).contiguous() for f in ft]
        rt, lt = torch.from_numpy(rois).to(_dev()), torch.from_numpy(levels).to(_dev())
        gout = torch.randn(len(rois), C, *pooled, generator=torch.Generator().manual_seed(8)).to(_dev())
        hw = [v for g in grids for v in g]

        def run(a):
            ft, rt, lt, gout = a
            out = torch.empty(len(rois), C, *pooled, device=rt.device)
            common = (L.i32_array(hw), L.f32_array([1 / 16, 1 / 32, 1 / 4]), 2, C, layout, L.ptr(rt), L.ptr(lt), len(rois),
                      pooled[0], pooled[1], 2, 0)
            L.call('frh_roi_align_fwd', len(ft), L.ptr_array(ft), *common, L.ptr(out), L.stream_of(out))
            grads = [torch.zeros_like(f) for f in ft]
            L.call('frh_roi_align_bwd', len(ft), L.ptr_array(grads), *common, L.ptr(gout), L.stream_of(out))
            return [out, grads]

        runs = guarded.sweep(mp, run, lambda: (ft, rt, lt, gout), ['frh_roi_align_fwd', 'frh_roi_align_bwd'], bits=False)
        _roi_bwd_close(runs, [f.shape for f in feats], rois, levels, [1 / 16, 1 / 32, 1 / 4], gout, nhwc_arrays=bool(layout))


for _nhwc in (False, True):
    @case('roi_pool[{}]'.format('nhwc' if _nhwc else 'nchw'), 'frh_roi_pool_fwd', 'frh_roi_pool_bwd')
    def _roi_pool(mp, nhwc=_nhwc):
        """support.rois and support.pathological_rois on a 19 x 30 level, forward (with the argmax
        map; bit for bit) and backward (float atomics into the argmax cells: the bound below)."""
        import numpy as np
        import inputs
        import support
        from frcnn_amd import ops
        feat = torch.from_numpy(inputs.feature_maps(80, [(19, 30)], 24, 2)[0]).to(_dev())
        feat = feat.contiguous(memory_format=CL) if nhwc else feat
        rois = torch.from_numpy(np.concatenate([support.rois(81, 40, 2), support.pathological_rois(2)], 0)).to(_dev())
        gout = torch.randn(len(rois), 24, 7, 7, generator=torch.Generator().manual_seed(9)).to(_dev())

        def run(a):
            x = a[0].detach().requires_grad_(True)
            out = ops.roi_pool(x, a[1], (7, 7), 1 / 32)
            out.backward(a[2])
            return [out.detach(), x.grad]

        # The backward adds with float atomics.  test_gpu_roi_pool.py's bound for a cell with m
        # contributions g_i against the exact sum is (m - 1) 2^-24 sum |g_i| (1 + 2^-20): two runs
        # differ by at most twice that.  m comes from the op's own backward of ones (small
        # integers: exact) and sum |g_i| from its backward of |grad|, itself an f32 sum of m
        # positive terms and so at least (1 - (m - 1) 2^-24) of the exact one: the third factor.
        x = feat.detach().requires_grad_(True)
        out = ops.roi_pool(x, rois, (7, 7), 1 / 32)
        cnt, = torch.autograd.grad(out, x, torch.ones_like(gout), retain_graph=True)
        mag, = torch.autograd.grad(out, x, gout.abs())
        m1 = (cnt.double() - 1).clamp_min(0)
        bound = 2 * m1 * 2.0 ** -24 * mag.double() * (1 + 2.0 ** -20) * (1 + 2 * m1 * 2.0 ** -24)
        runs = guarded.sweep(mp, run, lambda: (feat, rois, gout), ['frh_roi_pool_fwd', 'frh_roi_pool_bwd'], bits=False)
        for out_i, g in runs:
            assert guarded.same_bits(out_i, runs[0][0])
            assert bool(((g.double() - runs[0][1].double()).abs() <= bound).all())
            assert bool((g[cnt == 0] == 0).all())


# ----------------------------------------------------------------- image pipeline
IMAGE_CASES = {'upscale': ([(375, 500), (333, 500), (500, 281)], (1333, 800)), 'identity': ([(600, 1000)], (1000, 600)),
               'half': ([(1200, 1600), (800, 1200)], (800, 600)), 'odd': ([(17, 23), (5, 9), (64, 3)], (101, 37))}

for _name in IMAGE_CASES:
    @case('image_preprocess[{}]'.format(_name), 'frh_image_preprocess')
    def _image_preprocess(mp, name=_name):
        """test_preprocess_matches_oracle's case of this name (its shapes, scale and flips): the
        pipeline's own sizes, the source bytes and the output guarded."""
        import numpy as np
        from frcnn_amd import datasets
        L = _lib()
        shapes, scale = IMAGE_CASES[name]
        rng = np.random.default_rng(list(IMAGE_CASES).index(name))
        imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
        p = datasets.ImagePipeline(img_scale=scale, size_divisor=32)
        sizes = [p._plan(h, w)[:2] for h, w in shapes]
        out_h, out_w = max(p._pad(s[0]) for s in sizes), max(p._pad(s[1]) for s in sizes)
        offs = [int(v) for v in np.cumsum([0] + [h * w * 3 for h, w in shapes[:-1]])]
        src = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(_dev())

        def run(src):
            out = torch.empty(len(imgs), 3, out_h, out_w, device=src.device)
            L.call('frh_image_preprocess', L.ptr(src), len(imgs), L.i64_array(offs),
                   L.i32_array([v for s in shapes for v in s]), L.i32_array([v for s in sizes for v in s]),
                   L.i32_array([i % 2 for i in range(len(imgs))]), L.f32_array(p.mean), L.f32_array(p.std),
                   int(p.to_rgb), L.ptr(out), out_h, out_w, L.stream_of(out))
            return out
        guarded.sweep(mp, run, lambda: src, ['frh_image_preprocess'])


@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_guarded(dev, monkeypatch, name):
    """One case of the table; every entry the case declares (what test_guarded_cpu.py counts as
    swept) must have been called in it."""
    ((entries, fn),) = [c[1:] for c in CASES if c[0] == name]
    with guarded.entry_names(monkeypatch) as called:
        fn(monkeypatch)
    assert set(entries) <= set(called), sorted(set(entries) - set(called))
