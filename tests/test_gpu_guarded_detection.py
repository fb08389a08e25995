"""The detection path through frcnn_amd.ops under the guarded allocator (tests/guarded.py).  Here
ops.py allocates the outputs and the workspaces itself: every case calls the ops function on plain
inputs, then twice on guarded copies of them with the allocator routing ops' torch.empty / zeros /
full / _lib.workspace calls, once 0x00- and once 0xFF-filled (guarded.sweep).  Asserted per case:
every guard band intact, the defined part of every returned tensor poison-free, bit-identical
between the two fills (an element never written, or a workspace word read before it is written,
differs) and bit-identical to the plain call (an over-read of an input picks up the guards' NaN).

Each case names its defined part: the whole tensor unless the header leaves a region open (the
columns of a capacity buffer past counts[s], the rows past num[s]); what lies beyond may hold
anything.  Lists the device sampler fills "in no order" are compared sorted.

Inputs are small and edge-bearing: one image without ground truth and one with 40, 4097 boxes
(one past a 4096 chunk) beside a small count, a five-level pyramid from 19 x 32 down to 2 x 2
(38 x 64 on top for the RPN, so that a level holds more candidates than pre_nms 6000), the
generators of tests/golden/inputs.py at reduced sizes.

test_zero_contract_workspaces_keep_no_state runs A, B, A with another workspace layout in B under
the poisoned allocator: the third result must equal the first bit for bit.

Entries of this file's families that no case guards (NOT_GUARDED):
  frh_rpn_proposals_nms_view  a host-side query: it writes four int64 offsets into the caller's
      host array and touches no device memory
"""
import numpy as np
import pytest
import torch

import guarded

pytestmark = pytest.mark.gpu

NOT_GUARDED = {
    'frh_rpn_proposals_nms_view': 'host-side query: writes four int64 offsets to a host array, no device memory',
}
CASES = []
PYRAMID = [(19, 32), (10, 16), (5, 8), (3, 4), (2, 2)]
PYRAMID_STRIDES = [32, 64, 128, 256, 512]
IMG = (600, 1000)


def case(name, *entries):
    def add(fn):
        CASES.append((name, entries, fn))
        return fn
    return add


def swept_entries():
    return {e for _, entries, _ in CASES for e in entries}


def _dev():
    return torch.device('cuda', 0)


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    return t.to(dtype) if dtype is not None else t


def _boxes(seed, n):
    import inputs
    return T(inputs.random_boxes(seed, n))


def _gt_lists():
    """One image without ground truth, one with 40 boxes (inputs.atss_cases' many-box set)."""
    import inputs
    b, l = inputs.atss_cases()[8]
    assert b.shape == (4, 40)
    return [T(np.zeros((4, 0), np.float32)), T(b)], [T(np.zeros(0, np.int64)), T(l)]


def _counts(vals):
    return torch.tensor(vals, dtype=torch.int32, device=_dev())


def _rows_below(t, num, dim=1):
    """The part of t [S, n, ...] below each segment's count, as a list."""
    return [t[s].narrow(dim - 1, 0, int(k)) for s, k in enumerate(num.tolist())]


# ----------------------------------------------------------------- anchors, IoU, encode / decode
def _anchor_sizes(A=3):
    ws, hs = [], []
    for s in PYRAMID_STRIDES:
        for r in (0.5, 1.0, 2.0)[:A]:
            ws.append(2.0 * s / np.sqrt(r))
            hs.append(2.0 * s * np.sqrt(r))
    return ws, hs


def _anchors(A=3, grids=PYRAMID):
    from frcnn_amd import ops
    ws, hs = _anchor_sizes(A)
    return ops.anchor_grid(grids, [float(s) for s in PYRAMID_STRIDES], ws, hs, A, False, _dev()).contiguous()


@case('anchor_grid', 'frh_anchor_grid')
def _anchor_grid(mp):
    from frcnn_amd import ops
    ws, hs = _anchor_sizes()
    guarded.sweep(mp, lambda a: ops.anchor_grid(PYRAMID, [float(s) for s in PYRAMID_STRIDES], ws, hs, 3, False, _dev()),
                  lambda: (), ['frh_anchor_grid'])


@case('inside_mask', 'frh_inside_mask')
def _inside_mask(mp):
    from frcnn_amd import ops
    anchors = _anchors()
    in_sizes = [(min(h, int(IMG[0] / s) + 1), min(w, int(IMG[1] / s) + 1)) for (h, w), s in zip(PYRAMID, PYRAMID_STRIDES)]
    for border in (0, -1):
        guarded.sweep(mp, lambda a: ops.inside_mask(a, PYRAMID, in_sizes, 3, IMG[0], IMG[1], border), lambda: anchors,
                      ['frh_inside_mask'], written='all')


@case('iou_table', 'frh_iou_table', 'frh_elem_iou')
def _iou(mp):
    from frcnn_amd import ops
    for n, k in ((4097, 40), (130, 1)):
        a, b = _boxes(1, n), _boxes(2, k)
        guarded.sweep(mp, lambda t: ops.iou_table(t[0], t[1]), lambda: (a, b), ['frh_iou_table'])
        c = _boxes(3, n)
        guarded.sweep(mp, lambda t: ops.elem_iou(t[0], t[1]), lambda: (a, c), ['frh_elem_iou'])


@case('bbox2param_param2bbox', 'frh_bbox2param', 'frh_param2bbox')
def _codec(mp):
    from frcnn_amd import ops
    sd = [0.1, 0.1, 0.2, 0.2]
    for n in (4097, 130):
        base, box = _boxes(4, n), _boxes(5, n)
        delta = T(np.random.default_rng(6).standard_normal((4 * 21, n)).astype(np.float32) * 0.5)
        guarded.sweep(mp, lambda t: ops.bbox2param(t[0], t[1], [0.0] * 4, sd), lambda: (base, box), ['frh_bbox2param'])
        guarded.sweep(mp, lambda t: ops.param2bbox(t[0], t[1], [0.0] * 4, sd, IMG), lambda: (base, delta),
                      ['frh_param2bbox'])


# ----------------------------------------------------------------- assignment, sampling, targets
def _assign_inputs(n=4097, small=130):
    """boxes [2, 4, n] (counts n and `small`), gts of _gt_lists packed: image 0 has none."""
    from frcnn_amd import ops
    boxes = torch.stack([_boxes(10, n), _boxes(11, n)]).contiguous()
    gts, glab = _gt_lists()
    gb, gc, gm = ops._pack_boxes(gts, _dev(), 1)
    gl = ops._pack_labels(glab, gm, _dev())
    return boxes, _counts([n, small]), gb, gc, gm, gl


def _assign(t, n, gm):
    from frcnn_amd import ops
    boxes, num, gb, gc = t[:4]
    return ops.maxiou_assign(boxes, boxes.stride(0), num, n, gb, gc, gm, 0.7, 0.3, 0.3)


@case('maxiou_assign', 'frh_maxiou_assign')
def _maxiou(mp):
    """Rows past num_boxes[s] are padding the entry writes (label -1, max_iou 0): all defined."""
    boxes, num, gb, gc, gm, _ = _assign_inputs()
    guarded.sweep(mp, lambda t: _assign(t, 4097, gm), lambda: (boxes, num, gb, gc), ['frh_maxiou_assign'])
    # both images with ground truth, swapped: another (S, max_gts) layout than any other case
    guarded.sweep(mp, lambda t: _assign(t, 4097, gm), lambda: (boxes, num, gb.flip(0).contiguous(), gc.flip(0)),
                  ['frh_maxiou_assign'])


def _labels(seed, S, n):
    rng = np.random.default_rng(seed)
    return T(rng.choice([-1, 0, 1, 2, 3], size=(S, n), p=[0.3, 0.55, 0.05, 0.05, 0.05]).astype(np.int64))


def _sorted_lists(sl):
    """A SampleLists' defined part: the counts, and each list's first count entries, sorted."""
    cnt = sl.sel_counts.tolist()
    return [sl.sel_counts] + [torch.sort(sl.sel[s, k, :cnt[s][k]])[0] for s in range(len(cnt)) for k in (0, 1)]


for _max_num in (256, 6000):
    @case('sample_labels[{}]'.format(_max_num), 'frh_sample_random')
    def _sample(mp, max_num=_max_num):
        """Device sampler, labels out and selection lists out.  Labels: the rows below num[s]."""
        from frcnn_amd import ops
        n = 4097
        lab, num = _labels(20, 2, n), _counts([n, 130])

        def run(t, lists):
            ops.set_sampler_mode('device', seed=77)
            return ops.sample_labels(t[0], t[1], n, max_num, max_num // 2, mode='device', lists=lists)
        try:
            guarded.sweep(mp, lambda t: run(t, False), lambda: (lab, num), ['frh_sample_random'],
                          defined=lambda o: _rows_below(o, num))
            guarded.sweep(mp, lambda t: run(t, True), lambda: (lab, num), ['frh_sample_random'], defined=_sorted_lists)
        finally:
            ops.set_sampler_mode('numpy')


@case('sample_labels[numpy]', 'frh_sample_candidates', 'frh_sample_apply')
def _sample_numpy(mp):
    """The reference-order sampler: candidate lists on the device, the draw on the host."""
    from frcnn_amd import ops
    n = 4097
    lab, num = _labels(21, 2, n), _counts([n, 130])

    def run(t):
        np.random.seed(5)
        return ops.sample_labels(t[0], t[1], n, 256, 128, mode='numpy')
    guarded.sweep(mp, run, lambda: (lab, num), ['frh_sample_candidates', 'frh_sample_apply'],
                  defined=lambda o: _rows_below(o, num))


@case('sample_iou_balanced', 'frh_sample_iou_balanced', 'frh_sample_iou_candidates', 'frh_sample_apply')
def _sample_iou(mp):
    """Rows past an image's count are not written (the header says so): the rows below num[s]."""
    from frcnn_amd import ops
    n = 4097
    lab, num = _labels(22, 2, n), _counts([n, 130])
    iou = T(np.random.default_rng(23).uniform(0, 0.5, (2, n)).astype(np.float32))
    lo, hi = [0.0, 0.1, 0.2], [0.1, 0.2, 0.5]

    def run(t, mode, lists=False):
        ops.set_sampler_mode('device', seed=78)
        np.random.seed(6)
        return ops.sample_iou_balanced(t[0], t[1], t[2], n, 256, 64, lo, hi, mode=mode, lists=lists)
    try:
        guarded.sweep(mp, lambda t: run(t, 'device'), lambda: (lab, iou, num), ['frh_sample_iou_balanced'],
                      defined=lambda o: _rows_below(o, num))
        guarded.sweep(mp, lambda t: run(t, 'device', True), lambda: (lab, iou, num), ['frh_sample_iou_balanced'],
                      defined=_sorted_lists)
        guarded.sweep(mp, lambda t: run(t, 'numpy'), lambda: (lab, iou, num),
                      ['frh_sample_iou_candidates', 'frh_sample_apply'], defined=lambda o: _rows_below(o, num))
    finally:
        ops.set_sampler_mode('numpy')


def _dict_tensors(d):
    return [v for k, v in sorted(d.items()) if torch.is_tensor(v)]


@case('anchor_target_batched', 'frh_anchor_target')
def _anchor_target(mp):
    """From sampled labels (synchronising: outputs cut to the total) and from the device sampler's
    lists without a synchronisation (full capacity; the columns past the total are padding the
    entry writes: all defined)."""
    from frcnn_amd import ops
    n = 4097
    boxes, num, gb, gc, gm, gl = _assign_inputs(n)
    anchors = boxes[0].contiguous()

    def run(t, lists):
        anchors, num, gb, gc, gl = t
        ops.set_sampler_mode('device', seed=79)
        labels, _ = ops.maxiou_assign(anchors, 0, num, n, gb, gc, gm, 0.5, 0.4, 0.3)
        sl = ops.sample_labels(labels, num, n, 256, 128, mode='device', lists=lists)
        return _dict_tensors(ops.anchor_target_batched(sl, num, n, anchors, gb, gl, [0.0] * 4, [1.0] * 4, 256,
                                                       sync=not lists))
    try:
        for lists in (False, True):
            guarded.sweep(mp, lambda t: run(t, lists), lambda: (anchors, num, gb, gc, gl),
                          ['frh_maxiou_assign', 'frh_sample_random', 'frh_anchor_target'])
    finally:
        ops.set_sampler_mode('numpy')


@case('bbox_target_batched', 'frh_prepend_gt_labels', 'frh_bbox_target')
def _bbox_target(mp):
    """bbox.bbox_targets_batched's sequence on 4097 / 130 proposals: assignment, the gt rows
    prepended (rows: those below num_rows[s]), the device sampler, the target gather."""
    from frcnn_amd import ops
    n = 4097
    boxes, num, gb, gc, gm, gl = _assign_inputs(n)
    sd = [0.1, 0.1, 0.2, 0.2]

    def run(t, lists):
        boxes, num, gb, gc, gl = t
        ops.set_sampler_mode('device', seed=80)
        labels, _ = ops.maxiou_assign(boxes, boxes.stride(0), num, n, gb, gc, gm, 0.5, 0.5, 0.5)
        rows, num_rows = ops.prepend_gt_labels(labels, num, gc, gm + n)
        sl = ops.sample_labels(rows, num_rows, gm + n, 512, 128, mode='device', lists=lists)
        r = ops.bbox_target_batched(sl, num_rows, gc, gm + n, boxes, boxes.stride(0), gb, gl, [0.0] * 4, sd, 512,
                                    sync=not lists)
        return [num_rows, _rows_below(rows, num_rows), _dict_tensors(r)]
    try:
        for lists in (False, True):
            guarded.sweep(mp, lambda t: run(t, lists), lambda: (boxes, num, gb, gc, gl),
                          ['frh_prepend_gt_labels', 'frh_sample_random', 'frh_bbox_target'])
    finally:
        ops.set_sampler_mode('numpy')


def _level_maps(seed, channels, nhwc, batch=2):
    import inputs
    maps = [T(m) for m in inputs.feature_maps(seed, PYRAMID, channels, batch)]
    return [m.contiguous(memory_format=torch.channels_last) for m in maps] if nhwc else maps


for _nhwc in (False, True):
    @case('gather_level_outputs[{}]'.format('nhwc' if _nhwc else 'nchw'), 'frh_gather_level_outputs_strided',
          'frh_scatter_level_grads_strided')
    def _gather(mp, nhwc=_nhwc):
        """[B, 4 * 3, H, W] levels, 300 chosen cells over both images and every level, some padding
        columns (seg_of -1: zero output, no gradient), and the adjoint scatter."""
        from frcnn_amd import ops
        lv = _level_maps(30, 12, nhwc)
        total = 3 * sum(h * w for h, w in PYRAMID)
        rng = np.random.default_rng(31)
        # distinct cells and one cell chosen twice by one image: its two gradients add to the same
        # f32 sum in either order, so the scatter's atomics leave the comparison bit for bit
        idx = T(np.concatenate([1 + rng.choice(total - 2, 297, replace=False), [0, total - 1, total - 1]]).astype(np.int64))
        seg = T(np.concatenate([np.where(rng.random(298) < 0.1, -1, rng.integers(0, 2, 298)), [1, 1]]).astype(np.int32))
        gin = T(rng.standard_normal((4, 300)).astype(np.float32))

        def run(t):
            lv = [x.detach().requires_grad_(True) for x in t[0]]
            out = ops.gather_level_outputs(lv, t[1], t[2], 4)
            out.backward(t[3])
            return [out.detach(), [x.grad for x in lv]]
        guarded.sweep(mp, run, lambda: (lv, idx, seg, gin),
                      ['frh_gather_level_outputs_strided', 'frh_scatter_level_grads_strided'])


@case('gather_level_outputs[dense]', 'frh_gather_level_outputs', 'frh_scatter_level_grads')
def _gather_dense(mp):
    """The entries without strides: contiguous [B, C, cells] levels, one anchor per cell."""
    from frcnn_amd import _lib as L
    lv = _level_maps(32, 4, False)
    sizes = [h * w for h, w in PYRAMID]
    offs = [int(v) for v in np.cumsum([0] + sizes[:-1])]
    rng = np.random.default_rng(33)
    idx = T(np.concatenate([1 + rng.choice(sum(sizes) - 2, 298, replace=False), [0, sum(sizes) - 1]]).astype(np.int64))
    seg = T(np.where(rng.random(300) < 0.1, -1, rng.integers(0, 2, 300)).astype(np.int32))
    gin = T(rng.standard_normal((4, 300)).astype(np.float32))

    def run(t):
        lv, idx, seg, gin = t
        out = torch.empty(4, 300, dtype=torch.float32, device=idx.device)
        L.call('frh_gather_level_outputs', len(lv), L.ptr_array(lv), L.i64_array(offs), L.i64_array(sizes), 4, 300,
               L.ptr(idx), L.ptr(seg), L.ptr(out), out.stride(0), L.stream_of(out))
        grads = [torch.zeros_like(x) for x in lv]
        L.call('frh_scatter_level_grads', len(lv), L.ptr_array(grads), L.i64_array(offs), L.i64_array(sizes), 4, 300,
               L.ptr(idx), L.ptr(seg), L.ptr(gin), gin.stride(0), L.stream_of(out))
        return [out, grads]
    guarded.sweep(mp, run, lambda: (lv, idx, seg, gin), ['frh_gather_level_outputs', 'frh_scatter_level_grads'])


# ----------------------------------------------------------------- proposals, NMS, RoI rows
RPN_GRIDS = [(38, 64)] + PYRAMID[:3] + [(2, 2)]


def _proposals_defined(out):
    boxes, scores, counts = out
    k = counts.tolist()
    return [counts] + [boxes[b, :, :k[b]] for b in range(len(k))] + [scores[b, :k[b]] for b in range(len(k))]


for _nhwc, _cls_ch, _pre in ((False, 1, 2000), (True, 1, 6000), (False, 2, 6000), (True, 2, 2000)):
    @case('rpn_proposals[{}_{}ch_pre{}]'.format('nhwc' if _nhwc else 'nchw', _cls_ch, _pre), 'frh_rpn_proposals_strided')
    def _rpn(mp, nhwc=_nhwc, cls_ch=_cls_ch, pre=_pre):
        """Two images, five levels (7296 candidates on the first: more than pre_nms 6000 and than one
        4096 chunk).  Image 1's min_size of 100 empties the first level: its regression deltas are
        zero, so every box there is its anchor (clamped to the image, never larger), and the
        anchors' longer side is 2 * 32 * sqrt(2) = 90.6 < 100; image 0 keeps the level.  Defined:
        counts, and the first counts[b] columns of boxes and scores."""
        import inputs
        from frcnn_amd import ops
        cls, reg = inputs.head_outputs(40 + cls_ch, RPN_GRIDS, 3, cls_ch, batch=2, reg_scale=0.5)
        reg[0][...] = 0.0
        ws, hs = _anchor_sizes()
        assert max(ws[:3] + hs[:3]) < 100.0 <= min(max(w, h) for w, h in zip(ws[3:], hs[3:]))
        cls, reg = [T(c) for c in cls], [T(r) for r in reg]
        if nhwc:
            cls = [c.contiguous(memory_format=torch.channels_last) for c in cls]
            reg = [r.contiguous(memory_format=torch.channels_last) for r in reg]
        anchors = _anchors(3, RPN_GRIDS)
        guarded.sweep(mp, lambda t: ops.rpn_proposals(t[0], t[1], t[2], 3, cls_ch, [0.0] * 4, [1.0] * 4,
                                                      [(600.0, 1000.0)] * 2, [0.0, 100.0], pre, 1000, 1000, 0.7),
                      lambda: (cls, reg, anchors), ['frh_rpn_proposals_strided'], defined=_proposals_defined)


@case('rpn_proposals[dense]', 'frh_rpn_proposals')
def _rpn_dense(mp):
    """The entry without strides (contiguous NCHW levels), through ops.rpn_proposals' own
    allocation with the strides dropped from its argument list."""
    import inputs
    from frcnn_amd import _lib as L, ops
    cls, reg = inputs.head_outputs(45, PYRAMID, 3, 1, batch=2, reg_scale=0.5)
    cls, reg = [T(c) for c in cls], [T(r) for r in reg]
    anchors = _anchors()

    def dense(*a):
        L.call('frh_rpn_proposals', *(a[:4] + a[6:]))
        return 0
    guarded.sweep(mp, lambda t: ops.rpn_proposals(t[0], t[1], t[2], 3, 1, [0.0] * 4, [1.0] * 4, [(600.0, 1000.0)] * 2,
                                                  [0.0, 0.0], 1000, 300, 600, 0.7, _entry=(dense, 'frh_rpn_proposals')),
                  lambda: (cls, reg, anchors), ['frh_rpn_proposals'], defined=_proposals_defined)


@case('nms_sorted', 'frh_nms_sorted')
def _nms(mp):
    """n in {1, 63, 65, 4097}, two segments (n and n // 2 boxes).  Defined: the kept counts and the
    first kc[s] positions of keep."""
    import inputs
    from frcnn_amd import ops
    for n in (1, 63, 65, 4097):
        rows = T(np.stack([inputs.random_boxes(50 + s, n, min_wh=20.0).T for s in range(2)]))
        counts = _counts([n, n // 2])
        guarded.sweep(mp, lambda t: ops.nms_sorted(t[0], t[1], n, 0.6), lambda: (rows, counts), ['frh_nms_sorted'],
                      defined=lambda o: [o[1]] + _rows_below(o[0], o[1]), written='all')


for _i in (0, 3):
    @case('multiclass_nms_batched[{}]'.format(_i), 'frh_mcnms_prepare', 'frh_mcnms_finish')
    def _mcnms(mp, i=_i):
        """inputs.MCNMS_CASES at n = 300: 'official' with shared boxes, 'strict' with per-class
        boxes; two images, the second with 257 rows."""
        import inputs
        from frcnn_amd import ops
        bbox, score, sf, channels = inputs.mcnms_inputs(i)
        assert len(bbox) == 300 and sf is None
        mode = inputs.MCNMS_CASES[i][0]
        b2, s2 = T(np.stack([bbox, bbox[::-1]])), T(np.stack([score, score[::-1]]))
        rows = _counts([300, 257])
        guarded.sweep(mp, lambda t: ops.multiclass_nms_batched(t[0], t[1], channels, 0.5, 0.05, 100, None, mode=mode,
                                                               num_rows=t[2]),
                      lambda: (b2, s2, rows), ['frh_mcnms_prepare', 'frh_mcnms_finish'])


@case('roi_rows', 'frh_roi_rows', 'frh_roi_rows_dev', 'frh_roi_level_map')
def _roi_rows(mp):
    """Flat and per-image boxes with host counts, a fixed-capacity buffer with device counts (the
    rows past the total are padding rows the entry writes: all defined), and the level map."""
    import support
    from frcnn_amd import ops
    flat = _boxes(60, 4097 + 130)
    per_image = torch.stack([_boxes(61, 4100), _boxes(62, 4100)]).contiguous()
    guarded.sweep(mp, lambda t: ops.roi_rows(t, [4097, 130], 56, 4), lambda: flat, ['frh_roi_rows'])
    guarded.sweep(mp, lambda t: ops.roi_rows(t, [4097, 130], 56, 4, seg_stride=t.stride(0), flat=False),
                  lambda: per_image, ['frh_roi_rows'])
    guarded.sweep(mp, lambda t: ops.roi_rows(t, [130], 56, 1)[0], lambda: flat, ['frh_roi_rows'])
    guarded.sweep(mp, lambda t: ops.roi_rows_dev(t[0], t[1], 56, 4), lambda: (flat, _counts([4000, 130])),
                  ['frh_roi_rows_dev'])
    rois = T(np.concatenate([support.rois(63, 4086, 2), support.pathological_rois(2)], 0))
    guarded.sweep(mp, lambda t: ops.roi_level_map(t, 56, 4), lambda: rois, ['frh_roi_level_map'], written='all')


# ----------------------------------------------------------------- one-stage targets and candidates
def _cell_anchors():
    from frcnn_amd import ops
    ws = [8.0 * s for s in PYRAMID_STRIDES]
    return ops.anchor_grid(PYRAMID, [float(s) for s in PYRAMID_STRIDES], ws, ws, 1, False, _dev()).contiguous()


@case('atss_assign', 'frh_atss_assign')
def _atss(mp):
    from frcnn_amd import ops
    anchors = _cell_anchors()
    gts, labels = _gt_lists()
    guarded.sweep(mp, lambda t: ops.atss_assign(t[0], PYRAMID, [float(s) for s in PYRAMID_STRIDES], t[1], t[2],
                                                [IMG] * 2, 9),
                  lambda: (anchors, gts, labels), ['frh_atss_assign'])


@case('fcos_assign', 'frh_fcos_assign')
def _fcos_assign(mp):
    import fcos_inputs
    from frcnn_amd import ops
    gts, labels = _gt_lists()
    guarded.sweep(mp, lambda t: ops.fcos_assign(PYRAMID, [float(s) for s in PYRAMID_STRIDES], t[0], t[1], [IMG] * 2,
                                                fcos_inputs.REAL_THR),
                  lambda: (gts, labels), ['frh_fcos_assign'])


@case('ga_targets', 'frh_ga_targets')
def _ga(mp):
    """The fixture's three images (the second without ground truth) and the 200-box set."""
    import ga_inputs as gi
    from frcnn_amd import ops
    strides = [float(s) for s in gi.STRIDES]
    many_b, many_l = gi.many_case()[:2]
    for boxes, levels, shapes in ((gi.REF_BOXES, gi.REF_LEVELS, gi.IMG_SHAPES),
                                  ([many_b, gi.EMPTY], [many_l, np.zeros(0, np.int64)], gi.IMG_SHAPES[:2])):
        gts, lvs = [T(b) for b in boxes], [T(np.asarray(l, np.int64)) for l in levels]
        guarded.sweep(mp, lambda t: ops.ga_targets(gi.GRIDS, strides, t[0], t[1], shapes, **gi.RATIOS),
                      lambda: (gts, lvs), ['frh_ga_targets'])


for _tag in ('two_chunks', 'filter', 'gfl16_B2', 'retina_A9'):
    @case('dense_candidates[{}]'.format(_tag), 'frh_dense_candidates')
    def _dense(mp, tag=_tag):
        """test_gpu_dense.py's scenario, as its run_op calls it.  Invalid rows are written (zero,
        index -1): all defined."""
        import test_gpu_dense as t
        from frcnn_amd import ops
        sc = t.SCENARIOS[tag]
        cls, reg, ctr = t._inputs(sc)
        dcls, dreg = [T(a) for a in cls], [T(a) for a in reg]
        dctr = [T(a) for a in ctr] if sc['ctr'] else None
        img_hw = [m['img_shape'][:2] for m in sc['metas']]
        mins = [m['scale_factor'] * sc['min_bbox_size'] for m in sc['metas']]
        if sc['kind'] == 'retina':
            head = t._head(sc).to(_dev())
            anchors = head._flat_anchors([tuple(g) for g in sc['grids']], _dev())
            fn = lambda a: ops.dense_candidates(a[0], a[1], None, 'DELTA', img_hw, mins, sc['pre_nms'], num_anchors=sc['A'],
                                                anchors=a[3], means=head.target_means, stds=head.target_stds)
        else:
            anchors = None
            mode = 'DFL' if sc['kind'] == 'gfl' else 'LTRB'
            fn = lambda a: ops.dense_candidates(a[0], a[1], a[2], mode, img_hw, mins, sc['pre_nms'], strides=sc['strides'],
                                                bins=sc['bins'], dfl_stride=0.08, reg_std=sc['reg_std'], reg_mean=0.0)
        guarded.sweep(mp, lambda a: [o for o in fn(a) if o is not None], lambda: (dcls, dreg, dctr, anchors),
                      ['frh_dense_candidates'])


@case('dfl_decode', 'frh_dfl_decode')
def _dfl_decode(mp):
    """gfl_inputs' decode levels, NCHW and channels-last."""
    import gfl_inputs as gi
    from frcnn_amd import ops
    rng = np.random.default_rng(70)
    for cell, (h, w) in gi.DECODE_LEVELS:
        reg = T(rng.standard_normal((2, 4 * gi.DECODE_BINS, h, w)).astype(np.float32) * 2)
        for x in (reg, reg.contiguous(memory_format=torch.channels_last)):
            guarded.sweep(mp, lambda t: ops.dfl_decode(t, gi.DECODE_BINS, gi.DECODE_STRIDE, 1200.0, 0.0, cell, gi.DECODE_IMG),
                          lambda: x, ['frh_dfl_decode'])


# ----------------------------------------------------------------- fused losses
def _with_grad(fn, n_in):
    """fn's outputs (float losses summed with fixed weights) and the gradients of the first n_in inputs."""
    def run(t):
        xs = [v.detach().requires_grad_(True) for v in t[:n_in]]
        out = fn(*xs, *t[n_in:])
        outs = [out] if torch.is_tensor(out) else list(out)
        loss = sum(o * (0.37 + i) for i, o in enumerate(outs) if o.is_floating_point())
        loss.backward()
        return [[o.detach() for o in outs], [x.grad for x in xs]]
    return run


@case('cls_loss', 'frh_cls_loss_fwd', 'frh_cls_loss_bwd')
def _cls_loss(mp):
    """loss_cases.count_case at 257 rows (the last one an ignored padding row), the three kinds."""
    import loss_cases as lc
    from frcnn_amd import ops
    for kind, c in (('focal', 1), ('bce', 1), ('softmax', 3)):
        k = lc.count_case(kind, 257, c)
        assert int(k['lab'][-1]) == -1
        x, lab = T(k['x'].numpy()), T(k['lab'].numpy())
        guarded.sweep(mp, _with_grad(lambda x, lab: ops.cls_loss(x, lab, lc.KIND_ID[kind], k['alpha'], k['gamma']), 1),
                      lambda: (x, lab), ['frh_cls_loss_fwd', 'frh_cls_loss_bwd'])


def _l1_inputs(variant, rows_dim=0):
    import loss_cases as lc
    k = lc.l1_case(1.0 / 9.0, rows_dim, variant)
    assert int(k['lab'][-1]) == -1
    return k, T(k['x'].numpy()), T(k['y'].numpy()), T(k['lab'].numpy())


@case('smooth_l1_loss', 'frh_smooth_l1_fwd', 'frh_smooth_l1_bwd')
def _smooth_l1(mp):
    """loss_cases.l1_case (300 rows, the last a padding row): rows along dim 0 and 1, class select."""
    from frcnn_amd import ops
    for rows_dim in (0, 1):
        k, x, y, lab = _l1_inputs('edges', rows_dim)
        guarded.sweep(mp, _with_grad(lambda x, y, lab: ops.smooth_l1_loss(x, y, k['beta'], lab, rows_dim), 1),
                      lambda: (x, y, lab), ['frh_smooth_l1_fwd', 'frh_smooth_l1_bwd'])
    k, x, y, lab = _l1_inputs('class_select')
    guarded.sweep(mp, _with_grad(lambda x, y, lab: ops.smooth_l1_class_select(x, k['classes'], y, lab, k['beta']), 1),
                  lambda: (x, y, lab), ['frh_smooth_l1_fwd', 'frh_smooth_l1_bwd'])


@case('balanced_l1_loss', 'frh_balanced_l1_fwd', 'frh_balanced_l1_bwd')
def _balanced_l1(mp):
    from frcnn_amd import ops
    k, x, y, lab = _l1_inputs('edges')
    guarded.sweep(mp, _with_grad(lambda x, y, lab: ops.balanced_l1_loss(x, y, 1.0, 0.5, 1.5, lab), 1),
                  lambda: (x, y, lab), ['frh_balanced_l1_fwd', 'frh_balanced_l1_bwd'])
    k, x, y, lab = _l1_inputs('class_select')
    guarded.sweep(mp, _with_grad(lambda x, y, lab: ops.balanced_l1_class_select(x, k['classes'], y, lab, 1.0, 0.5, 1.5), 1),
                  lambda: (x, y, lab), ['frh_balanced_l1_fwd', 'frh_balanced_l1_bwd'])


def _det(cx, rx, clab, ry, rlab, kind, avg):
    from frcnn_amd import ops
    return ops.det_losses(cx, clab, kind, 0.25, 2.0, 1.0, ops._l1_args(rx, ry, rlab, 0), 1.0 / 9.0, 1.0, avg)


def _det_inputs(n_cls, n_reg):
    import loss_cases as lc
    c, r = lc.count_case('focal', n_cls, 3), lc.l1_rows_case(n_reg)
    return [T(c['x'].numpy()), T(r['x'].numpy()), T(c['lab'].numpy()), T(r['y'].numpy()), T(r['lab'].numpy())]


@case('det_losses', 'frh_det_loss_fwd', 'frh_cls_loss_bwd', 'frh_smooth_l1_bwd')
def _det_losses(mp):
    """257 classification rows and 300 regression rows (both end on a padding row), a host and a
    device avg_factor."""
    from frcnn_amd import ops
    t = _det_inputs(257, 300)
    cnt = _counts([37])
    for avg in (37.0, cnt):
        guarded.sweep(mp, _with_grad(lambda cx, rx, clab, ry, rlab: _det(cx, rx, clab, ry, rlab, ops.CLS_FOCAL, avg), 2),
                      lambda: t, ['frh_det_loss_fwd', 'frh_cls_loss_bwd', 'frh_smooth_l1_bwd'])


def _gfl_inputs(tag):
    import gfl_inputs as gi
    c = gi.loss_case(tag)
    assert (c['labels'] < 0).any()
    return gi.loss_kwargs(c), [T(c['cls']), T(c['reg']), T(c['labels']), T(c['ltrb'])]


def _fcos_inputs(tag):
    import fcos_inputs as fi
    c = fi.loss_case(tag)
    assert (c['labels'] < 0).any()
    return fi.loss_kwargs(c), [T(c['cls']), T(c['reg']), T(c['ctr']), T(c['labels']), T(c['ltrb']), T(c['ctr_t'])]


@case('gfl_losses', 'frh_gfl_loss_fwd', 'frh_gfl_loss_bwd')
def _gfl(mp):
    from frcnn_amd import ops
    for tag in ('bins8', 'mixed'):
        kw, t = _gfl_inputs(tag)
        guarded.sweep(mp, _with_grad(lambda cls, reg, lab, ltrb: ops.gfl_losses(cls, reg, lab, ltrb, **kw), 2), lambda: t,
                      ['frh_gfl_loss_fwd', 'frh_gfl_loss_bwd'])


@case('fcos_losses', 'frh_fcos_loss_fwd', 'frh_fcos_loss_bwd')
def _fcos(mp):
    from frcnn_amd import ops
    for tag in ('m257', 'm255'):
        kw, t = _fcos_inputs(tag)
        guarded.sweep(mp, _with_grad(lambda cls, reg, ctr, *rest: ops.fcos_losses(cls, reg, ctr, *rest, **kw), 3),
                      lambda: t, ['frh_fcos_loss_fwd', 'frh_fcos_loss_bwd'])


@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_guarded(dev, monkeypatch, name):
    """One case of the table; every entry the case declares (what test_guarded_cpu.py counts as
    swept) must have been called in it."""
    ((entries, fn),) = [c[1:] for c in CASES if c[0] == name]
    with guarded.entry_names(monkeypatch) as called:
        fn(monkeypatch)
    assert set(entries) <= set(called), sorted(set(entries) - set(called))


# ----------------------------------------------------------------- state in the zero-contract workspaces
def _state_steps():
    """name -> (step A, step B): B has another layout -- other (S, max_gts), other n, other row
    count -- so the persistent workspace is re-laid between the two runs of A."""
    from frcnn_amd import ops
    boxes, num, gb, gc, gm, _ = _assign_inputs(4097)
    b_boxes, b_gts = _boxes(90, 700)[None].contiguous(), _boxes(91, 7)[None].contiguous()
    b_num, b_gc = _counts([700]), _counts([7])
    lab_a, lab_b = _labels(92, 2, 4097), _labels(93, 3, 900)
    num_b3 = _counts([900, 0, 411])
    iou_a = T(np.random.default_rng(94).uniform(0, 0.5, (2, 4097)).astype(np.float32))
    iou_b = T(np.random.default_rng(95).uniform(0, 0.5, (3, 900)).astype(np.float32))
    det_a, det_b = _det_inputs(257, 300), _det_inputs(65537, 3)
    (gkw_a, gfl_a), (gkw_b, gfl_b) = _gfl_inputs('mixed'), _gfl_inputs('bins8')
    (fkw_a, fcos_a), (fkw_b, fcos_b) = _fcos_inputs('m257'), _fcos_inputs('full')

    def sampled(lab, num, n):
        out = ops.sample_labels(lab, num, n, 256, 128, mode='device')
        return _rows_below(out, num)

    def balanced(lab, iou, num, n):
        out = ops.sample_iou_balanced(lab, iou, num, n, 256, 64, [0.0, 0.1, 0.2], [0.1, 0.2, 0.5], mode='device')
        return _rows_below(out, num)
    det = _with_grad(lambda cx, rx, clab, ry, rlab: _det(cx, rx, clab, ry, rlab, ops.CLS_FOCAL, 37.0), 2)
    return {
        'maxiou_assign': (lambda: _assign((boxes, num, gb, gc), 4097, gm),
                          lambda: ops.maxiou_assign(b_boxes, b_boxes.stride(0), b_num, 700, b_gts, b_gc, 7, 0.7, 0.3, 0.3)),
        'sample_labels': (lambda: sampled(lab_a, num, 4097), lambda: sampled(lab_b, num_b3, 900)),
        'sample_iou_balanced': (lambda: balanced(lab_a, iou_a, num, 4097), lambda: balanced(lab_b, iou_b, num_b3, 900)),
        'det_losses': (lambda: det(det_a), lambda: det(det_b)),
        'gfl_losses': (lambda: _with_grad(lambda c, r, l, b: ops.gfl_losses(c, r, l, b, **gkw_a), 2)(gfl_a),
                       lambda: _with_grad(lambda c, r, l, b: ops.gfl_losses(c, r, l, b, **gkw_b), 2)(gfl_b)),
        'fcos_losses': (lambda: _with_grad(lambda c, r, t, *rest: ops.fcos_losses(c, r, t, *rest, **fkw_a), 3)(fcos_a),
                        lambda: _with_grad(lambda c, r, t, *rest: ops.fcos_losses(c, r, t, *rest, **fkw_b), 3)(fcos_b)),
    }


STATE_FUNCTIONS = ('maxiou_assign', 'sample_labels', 'sample_iou_balanced', 'det_losses', 'gfl_losses', 'fcos_losses')


@pytest.mark.parametrize('name', STATE_FUNCTIONS)
def test_zero_contract_workspaces_keep_no_state(dev, monkeypatch, name):
    """A, B, A under the poisoned allocator, the sampler re-seeded before every step, the persistent
    workspaces (ops._ASSIGN_WS, _SAMPLE_WS, _LOSS_WS) born guarded at the first step and kept: the
    third result equals the first bit for bit, and every guard is intact at the end."""
    from frcnn_amd import ops
    step_a, step_b = _state_steps()[name]
    results = []
    try:
        with guarded.allocator(monkeypatch, guarded.POISON, device='cuda') as g:
            for step in (step_a, step_b, step_a):
                ops.set_sampler_mode('device', seed=123)
                results.append(guarded.tensors(step()))
                torch.cuda.synchronize()
            assert g.records
    finally:
        ops.set_sampler_mode('numpy')
    first, _, third = results
    assert len(first) == len(third) and first
    for a, b in zip(first, third):
        assert guarded.same_bits(a, b)
        if a.is_floating_point():
            guarded.assert_written(a)
