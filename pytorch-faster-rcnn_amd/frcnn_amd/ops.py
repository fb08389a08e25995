"""Tensor-level wrappers of the HIP kernels (one function per C-ABI entry).

These take/return torch tensors resident on the HIP device, allocate outputs
and workspaces with the caching allocator and launch on the current stream.
The reference-API modules (anchor, region, bbox, utils, heads) are built on
these.  The torchvision drop-ins the reference imports (`nms`, `roi_align`,
`RoIAlign`, `RoIPool`) live here too.
"""
import ctypes
import os
import warnings

import numpy as np
import torch
from torch import nn

from . import _lib
from ._lib import call as _call, ptr, stream_of, i32_array, i64_array, f32_array, ptr_array, workspace


def call(name, *args):
    """_lib.call; a failed entry point drops the zero-contract workspaces (their counters
    are left zero only by calls that ran to completion), so the next call starts from
    freshly zeroed buffers."""
    try:
        _call(name, *args)
    except RuntimeError:
        _drop_zero_workspaces()
        raise


def _drop_zero_workspaces():
    for ws in (_ASSIGN_WS, _SAMPLE_WS, _LOSS_WS):
        ws.clear()


# ---------------------------------------------------------------- device status word
# include/frcnn_amd.h FRH_DEVERR_*: the one-launch kernels (RPN selection, RPN NMS, device
# sampler) OR a bit into this per-device int32 word when an in-launch wait runs out, and
# end that workgroup's work.  The word is read (one 4-byte copy, a synchronisation) by
# check_device_status(): at the points that synchronise anyway -- the numpy sampler's count
# read, bench.py's loss read after the timed region, the tester -- and after every one-launch
# call when FRCNN_AMD_DEBUG=1.
DEVERR_BITS = {1: 'RPN selection segment barrier (rpn_select_kernel)',
               2: 'RPN NMS mask column wait (nms_fused_kernel)',
               4: 'device sampler image barrier (sampler_fused_kernel)'}
_STATUS = {}
DEBUG = os.environ.get('FRCNN_AMD_DEBUG', '') not in ('', '0')


def _device_key(dev):
    """Device index of `dev`; a bare 'cuda' device means the current device (both the word's
    owner and its checker resolve it this way)."""
    d = torch.device(dev)
    return d.index if d.index is not None else torch.cuda.current_device()


def status_word(dev):
    """The device status word of `dev` (int32 [1], zero until a one-launch kernel flags)."""
    key = _device_key(dev)
    w = _STATUS.get(key)
    if w is None:
        w = _STATUS[key] = torch.zeros(1, dtype=torch.int32, device=torch.device('cuda', key))
    return w


def check_device_status(dev=None):
    """Raise RuntimeError if a one-launch kernel on `dev` (default: every device used) flagged
    a timed-out in-launch wait since the last check.  Synchronises with the word's device.
    The word is cleared and the zero-contract workspaces are dropped (their counters may be
    left dirty by the aborted launch), so later calls start clean."""
    keys = list(_STATUS) if dev is None else [_device_key(dev)]
    for k in keys:
        w = _STATUS.get(k)
        if w is None:
            continue
        v = int(w.item())
        if v:
            w.zero_()
            _drop_zero_workspaces()
            what = ', '.join(m for b, m in DEVERR_BITS.items() if v & b) or 'unknown'
            raise RuntimeError('frcnn_amd: device status 0x{:x} on cuda:{}: an in-launch wait timed out ({}); '
                               'the outputs of that call are undefined'.format(v, k, what))


def _debug_check(dev):
    if DEBUG:
        check_device_status(dev)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError('frcnn_amd: HIP device tensors required (got {})'.format(t.device))


def _f32(t):
    return t if t.dtype == torch.float32 else t.float()


# ---------------------------------------------------------------- anchors (a1/a2)
def anchor_grid(grid_sizes, strides, ws, hs, num_anchors, center_lt, device):
    """All levels' anchors as one [4, N] tensor (reference AnchorCreator per level, concatenated)."""
    L = len(grid_sizes)
    n = sum(num_anchors * int(h) * int(w) for h, w in grid_sizes)
    out = torch.empty(4, max(n, 1), dtype=torch.float32, device=device)[:, :n]
    ws_t = torch.tensor(ws, dtype=torch.float32, device=device)
    hs_t = torch.tensor(hs, dtype=torch.float32, device=device)
    hw = i32_array([v for g in grid_sizes for v in (int(g[0]), int(g[1]))])
    call('frh_anchor_grid', L, hw, f32_array(strides), ptr(ws_t), ptr(hs_t), num_anchors,
         int(bool(center_lt)), ptr(out), out.stride(0), stream_of(out))
    return out


def inside_mask(anchors, grid_sizes, in_sizes, num_anchors, img_h, img_w, allowed_border):
    _need_cuda(anchors)
    n = anchors.shape[1]
    mask = torch.empty(n, dtype=torch.uint8, device=anchors.device)
    hw = i32_array([v for g in grid_sizes for v in (int(g[0]), int(g[1]))])
    ihw = i32_array([v for g in in_sizes for v in (int(g[0]), int(g[1]))])
    call('frh_inside_mask', ptr(anchors), anchors.stride(0), len(grid_sizes), hw, ihw, num_anchors,
         int(img_h), int(img_w), int(allowed_border), ptr(mask), stream_of(anchors))
    return mask


# ---------------------------------------------------------------- IoU (a3)
def iou_table(a, b):
    _need_cuda(a, b)
    a, b = _f32(a), _f32(b)
    if a.stride(1) != 1:
        a = a.contiguous()
    if b.stride(1) != 1:
        b = b.contiguous()
    n, k = a.shape[1], b.shape[1]
    out = torch.empty(n, k, dtype=torch.float32, device=a.device)
    call('frh_iou_table', ptr(a), a.stride(0), n, ptr(b), b.stride(0), k, ptr(out), stream_of(a))
    return out


def elem_iou(a, b):
    _need_cuda(a, b)
    a, b = _f32(a).contiguous(), _f32(b).contiguous()
    n = a.shape[1]
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    call('frh_elem_iou', ptr(a), a.stride(0), ptr(b), b.stride(0), n, ptr(out), stream_of(a))
    return out


# ---------------------------------------------------------------- packing helpers
def device_ints(vals, device, dtype=torch.int32):
    """Small host list -> device tensor without a stream synchronisation
    (pinned staging + non_blocking copy; a pageable copy would block)."""
    t = torch.tensor(list(vals), dtype=dtype)
    if device.type != 'cuda':
        return t
    return t.pin_memory().to(device, non_blocking=True)


_PACKED = []  # (inputs, their versions, key, result): the packs of the last few distinct input lists


def _memo(inputs, key, make):
    """A batch's gt boxes / labels are packed once and reused by the RPN and every RCNN stage:
    hit only for the same tensor objects (held by the entry, so their storage cannot be
    reused) with unchanged version counters, on the same stream (a pack is made on the
    current stream and read in stream order).  Detectors drop the entries at the end of
    each forward_train (release_packs)."""
    dev = key[1]
    if isinstance(dev, torch.device) and dev.type == 'cuda':
        key = key + (torch.cuda.current_stream(dev).cuda_stream,)
    vers = tuple(t._version for t in inputs)
    for ent in _PACKED:
        if ent[2] == key and len(ent[0]) == len(inputs) and all(a is b for a, b in zip(ent[0], inputs)) \
                and ent[1] == vers:
            return ent[3]
    res = make()
    _PACKED.insert(0, (tuple(inputs), vers, key, res))
    del _PACKED[8:]
    return res


def release_packs():
    """Forget the memoised gt packs (end of a forward_train)."""
    del _PACKED[:]


def pack_boxes(box_list, device, min_cols=1):
    """list of [4, n_i] -> ([S, 4, n_max] f32, counts int32 device, n_max)."""
    if all(torch.is_tensor(b) and b.dtype == torch.float32 for b in box_list):
        return _memo(list(box_list), ('boxes', device, min_cols), lambda: _pack_boxes(box_list, device, min_cols))
    return _pack_boxes(box_list, device, min_cols)


def _pack_boxes(box_list, device, min_cols):
    S = len(box_list)
    nmax = max([int(b.shape[1]) for b in box_list] + [min_cols])
    out = torch.zeros(S, 4, nmax, dtype=torch.float32, device=device)
    for s, b in enumerate(box_list):
        if b.shape[1]:
            out[s, :, :b.shape[1]] = b
    counts = device_ints([int(b.shape[1]) for b in box_list], device)
    return out, counts, nmax


def pack_labels(label_list, nmax, device):
    if all(torch.is_tensor(l) for l in label_list):
        return _memo(list(label_list), ('labels', device, nmax), lambda: _pack_labels(label_list, nmax, device))
    return _pack_labels(label_list, nmax, device)


def _pack_labels(label_list, nmax, device):
    S = len(label_list)
    out = torch.zeros(S, max(nmax, 1), dtype=torch.int64, device=device)
    for s, l in enumerate(label_list):
        if l.numel():
            out[s, :l.numel()] = l.to(torch.int64)
    return out


# ---------------------------------------------------------------- MaxIoU assignment (a4)
_ASSIGN_WS = {}


def _assign_workspace(dev, S, mg, max_boxes):
    """One buffer per (device, stream): its leading counters / maxima are zero-filled when
    the (segments, gts) layout changes; every call leaves them zero."""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    need = int(_lib.query('frh_maxiou_assign_workspace', S, mg, max_boxes))
    layout = (S, mg)
    ent = _ASSIGN_WS.get(key)
    if ent is None or ent[1].numel() < need:
        ent = _ASSIGN_WS[key] = [layout, torch.zeros(need, dtype=torch.uint8, device=dev)]
    elif ent[0] != layout:
        ent[1][:int(_lib.query('frh_maxiou_assign_zero_bytes', S, mg))].zero_()
        ent[0] = layout
    return ent[1]

def maxiou_assign(boxes, box_seg_stride, num_boxes, max_boxes, gts, gt_counts, max_gts, pos_iou, neg_iou,
                  min_pos_iou, valid=None, valid_seg_stride=0, num_segs=None):
    """Batched MaxIoUAssigner: boxes [.., 4, ld] (segment stride given), gts [S, 4, Gmax]."""
    _need_cuda(boxes, gts)
    S = num_segs if num_segs is not None else gts.shape[0]
    dev = boxes.device
    labels = torch.empty(S, max(max_boxes, 1), dtype=torch.int64, device=dev)
    max_iou = torch.empty(S, max(max_boxes, 1), dtype=torch.float32, device=dev)
    ws = _assign_workspace(dev, S, max(max_gts, 1), max_boxes)
    call('frh_maxiou_assign', S, ptr(boxes), boxes.stride(-2), box_seg_stride, ptr(num_boxes),
         ptr(valid), valid_seg_stride, ptr(gts), gts.stride(1), gts.stride(0), ptr(gt_counts),
         float(pos_iou), float(neg_iou), float(min_pos_iou), ptr(labels), labels.stride(0), ptr(max_iou),
         max_iou.stride(0), max_boxes, max_gts, ptr(ws), ws.numel(), stream_of(boxes))
    return labels, max_iou


# ---------------------------------------------------------------- sampling (a5)
_SAMPLER = {'mode': 'numpy', 'seed': 0x5eed, 'calls': 0}


def set_sampler_mode(mode, seed=None):
    """'numpy' = the reference's np.random stream (exact parity, host round trip);
    'device' = on-device hash RNG (same distribution, no sync)."""
    if mode not in ('numpy', 'device'):
        raise ValueError("sampler mode must be 'numpy' or 'device'")
    _SAMPLER['mode'] = mode
    if seed is not None:
        _SAMPLER['seed'] = int(seed)
        _SAMPLER['calls'] = 0


def sampler_mode():
    return _SAMPLER['mode']


class SampleLists(object):
    """The device sampler's selection (frh_sample_random's sel / sel_counts): per segment the
    kept positives and negatives, in no order, for the target gathers; `labels` are the
    assignment labels they select from (unchanged)."""

    def __init__(self, labels, sel, sel_counts, max_num):
        self.labels, self.sel, self.sel_counts, self.max_num = labels, sel, sel_counts, int(max_num)


_SAMPLE_WS = {}


def _sample_workspace(dev, S, max_boxes):
    """One buffer per (device, stream) for frh_sample_random: zero-filled once; every call
    leaves its leading frh_sample_zero_bytes(S) bytes zero (the one-launch sampler's counters
    and histograms), so it is reused as is."""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    need = int(_lib.query('frh_sample_workspace', S, max_boxes))
    ws = _SAMPLE_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _SAMPLE_WS[key] = torch.zeros(need, dtype=torch.uint8, device=dev)
    return ws


def sample_labels(labels, num_boxes, max_boxes, max_num, pos_num, mode=None, lists=False, _entry=None):
    """Batched RandomSampler over labels [S, >=max_boxes] (region.py:43-57,112-126).
    lists=True (device mode only): return a SampleLists instead of the sampled labels."""
    mode = mode or _SAMPLER['mode']
    S = labels.shape[0]
    dev = labels.device
    if mode == 'device':
        ws = _sample_workspace(dev, S, max(max_boxes, 1))
        _SAMPLER['calls'] += 1
        seed = (_SAMPLER['seed'] * 0x9E3779B97F4A7C15 + _SAMPLER['calls']) & 0xFFFFFFFFFFFFFFFF
        out = None if lists else torch.empty_like(labels)
        sel = torch.empty(S, 2, max(int(max_num), 1), dtype=torch.int32, device=dev) if lists else None
        sel_cnt = torch.empty(S, 2, dtype=torch.int32, device=dev) if lists else None
        args = (S, ptr(labels), labels.stride(0), ptr(num_boxes), max_boxes, int(max_num), int(pos_num), seed,
                ptr(out), ptr(sel), ptr(sel_cnt), ptr(status_word(dev)), ptr(ws), ws.numel(), stream_of(labels))
        if _entry is None:
            call('frh_sample_random', *args)
        elif _entry[0](*args) != 0:  # tests: the tools library's two-launch sampler
            raise RuntimeError('{} failed'.format(_entry[1]))
        _debug_check(dev)
        return SampleLists(labels, sel, sel_cnt, max_num) if lists else out
    out = torch.empty_like(labels)
    ld = max(max_boxes, 1)
    pos_list = torch.empty(S, ld, dtype=torch.int32, device=dev)
    neg_list = torch.empty(S, ld, dtype=torch.int32, device=dev)
    counts = torch.empty(S, 2, dtype=torch.int32, device=dev)
    ws = workspace(_lib.query('frh_sample_workspace', S, ld), dev)
    call('frh_sample_candidates', S, ptr(labels), labels.stride(0), ptr(num_boxes), max_boxes, ptr(pos_list),
         ptr(neg_list), ld, ptr(counts), ptr(ws), ws.numel(), stream_of(labels))
    cnt = counts.cpu().numpy()  # host round trip, as the reference's .cpu().numpy() (region.py:48,55)
    check_device_status(dev)  # the stream is drained here anyway: a 4-byte read
    keep_ld = max(int(max_num), 1)
    keep = np.zeros((2, S, keep_ld), dtype=np.int32)
    kc = np.zeros((S, 2), dtype=np.int32)
    for s in range(S):
        npos, nneg = int(cnt[s, 0]), int(cnt[s, 1])
        kp = _numpy_keep(npos, pos_num)
        kneg = _numpy_keep(nneg, max_num - min(npos, pos_num))
        kc[s, 0], kc[s, 1] = len(kp), len(kneg)
        keep[0, s, :len(kp)] = kp
        keep[1, s, :len(kneg)] = kneg
    keep_t = torch.from_numpy(keep).to(dev, non_blocking=False)
    kc_t = torch.from_numpy(kc).to(dev)
    call('frh_sample_apply', S, ptr(labels), labels.stride(0), ptr(num_boxes), max_boxes, ptr(pos_list),
         ptr(neg_list), ld, ptr(keep_t[0]), ptr(keep_t[1]), keep_ld, ptr(kc_t), ptr(out), stream_of(labels))
    return out


def _numpy_keep(n, cap):
    """Positions kept by `np.random.choice(cands, n - cap, replace=False)` discarding.

    numpy's legacy choice(replace=False) is permutation(n)[:size]; the kept
    positions are the rest of that permutation, and the global RNG advances
    exactly as in the reference."""
    if n <= cap:
        return np.arange(n, dtype=np.int32)
    perm = np.random.permutation(n)
    return np.sort(perm[n - cap:]).astype(np.int32)


def _numpy_first(n, cap):
    """List positions kept by the reference's `np.random.choice(n, cap, replace=False)`
    (utils.random_select: permutation(n)[:cap], the FIRST cap of the permutation), drawn
    only when the class holds more than its quota (region.py:145,159)."""
    if n <= cap:
        return np.arange(n, dtype=np.int32)
    return np.random.permutation(n)[:cap].astype(np.int32)


def iou_bin_quotas(npos, bin_counts, max_num, pos_num):
    """region.py:145-161: (kept positives, kept negatives per bin in visiting order, highest
    bin first) from the class counts."""
    kp = min(int(npos), pos_num)
    num_neg = max_num - kp
    nb = len(bin_counts)
    per_bin = int(num_neg / nb)
    chosen, takes = 0, []
    for j, c in enumerate(bin_counts):
        allowed = per_bin if j < nb - 1 else num_neg - chosen
        takes.append(min(int(c), allowed))
        chosen += takes[-1]
    return kp, takes


def sample_iou_balanced(labels, ious, num_boxes, max_boxes, max_num, pos_num, bin_lo, bin_hi, iou_offsets=None,
                        mode=None, lists=False):
    """Batched IoUBalancedNegSampler over labels [S, >=max_boxes] (region.py:128-172); row i of
    image s has IoU ious[s, i - iou_offsets[s]] (read for negatives only).  bin_lo / bin_hi:
    the f32 bin edges, ascending.  Returns as sample_labels: the sampled labels (rows past an
    image's count are not written), or with lists=True (device mode) a SampleLists whose
    negatives' list holds every bin's choices."""
    mode = mode or _SAMPLER['mode']
    _need_cuda(labels, ious, num_boxes, iou_offsets)
    if ious.dtype != torch.float32 or ious.stride(-1) != 1 or labels.stride(-1) != 1:
        raise AssertionError('sample_iou_balanced: f32 IoUs and labels with contiguous rows')
    S = labels.shape[0]
    dev = labels.device
    nb = len(bin_lo)
    lo, hi = f32_array(bin_lo), f32_array(bin_hi)
    if mode == 'device':
        _SAMPLER['calls'] += 1
        seed = (_SAMPLER['seed'] * 0x9E3779B97F4A7C15 + _SAMPLER['calls']) & 0xFFFFFFFFFFFFFFFF
        out = None if lists else torch.empty_like(labels)
        sel = torch.empty(S, 2, max(int(max_num), 1), dtype=torch.int32, device=dev) if lists else None
        sel_cnt = torch.empty(S, 2, dtype=torch.int32, device=dev) if lists else None
        call('frh_sample_iou_balanced', S, ptr(labels), labels.stride(0), ptr(ious), ious.stride(0), ptr(iou_offsets),
             ptr(num_boxes), max_boxes, int(max_num), int(pos_num), nb, lo, hi, seed, ptr(out), ptr(sel), ptr(sel_cnt),
             stream_of(labels))
        return SampleLists(labels, sel, sel_cnt, max_num) if lists else out
    out = torch.empty_like(labels)
    ld = max(max_boxes, 1)
    cand = torch.empty(S, 1 + nb, ld, dtype=torch.int32, device=dev)
    counts = torch.empty(S, 1 + nb, dtype=torch.int32, device=dev)
    call('frh_sample_iou_candidates', S, ptr(labels), labels.stride(0), ptr(ious), ious.stride(0), ptr(iou_offsets),
         ptr(num_boxes), max_boxes, nb, lo, hi, ptr(cand), ld, ptr(counts), stream_of(labels))
    cnt = counts.cpu().numpy()  # the one host round trip, as ops.sample_labels
    check_device_status(dev)
    keep_ld = max(int(max_num), 1)
    keep = np.zeros((2, S, keep_ld), dtype=np.int32)
    kc = np.zeros((S, 2), dtype=np.int32)
    for s in range(S):  # draw order: positives, then the bins from the highest down, image by image
        _, takes = iou_bin_quotas(cnt[s, 0], cnt[s, 1:], max_num, pos_num)
        kp = _numpy_first(int(cnt[s, 0]), pos_num)
        kneg = [_numpy_first(int(cnt[s, 1 + j]), takes[j]) + j * ld for j in range(nb)]
        kneg = np.concatenate(kneg).astype(np.int32)
        kc[s, 0], kc[s, 1] = len(kp), len(kneg)
        keep[0, s, :len(kp)] = kp
        keep[1, s, :len(kneg)] = kneg
    keep_t = torch.from_numpy(keep).to(dev)
    kc_t = torch.from_numpy(kc).to(dev)
    call('frh_sample_apply', S, ptr(labels), labels.stride(0), ptr(num_boxes), max_boxes, ptr(cand), ptr(cand[:, 1:]),
         (1 + nb) * ld, ptr(keep_t[0]), ptr(keep_t[1]), keep_ld, ptr(kc_t), ptr(out), stream_of(labels))
    return out


# ---------------------------------------------------------------- target gathers (a6/a12)
def anchor_target_batched(labels, num_boxes, max_boxes, anchors, gts, gt_labels, means, stds, max_out_per_seg,
                          sync=True):
    """labels: the sampled labels [S, n] (chosen = label >= 0) or a SampleLists.
    sync=False (SampleLists only): no read-back of the output size -- every output keeps
    its full capacity S * max_out_per_seg, the columns past the device total being padding
    (seg_of -1, label -1, zero boxes: the gathers and losses ignore them), and 'n_dev' is
    the total as a device int32 [1] (the heads' avg_factor)."""
    if not sync and not isinstance(labels, SampleLists):
        raise AssertionError('sync-free targets need the device sampler lists')
    sl = labels if isinstance(labels, SampleLists) else None
    if sl is not None:
        labels = sl.labels
    S = labels.shape[0]
    dev = labels.device
    cap = max(int(max_out_per_seg), 1)
    T = S * cap
    chosen_idx = torch.empty(T, dtype=torch.int64, device=dev)
    seg_of = torch.empty(T, dtype=torch.int32, device=dev)
    tar_labels = torch.empty(T, dtype=torch.int64, device=dev)
    tars = torch.empty(3, 4, T, dtype=torch.float32, device=dev)
    counts = torch.empty(S + 1, dtype=torch.int32, device=dev)
    ws = None if sl is not None else workspace(_lib.query('frh_anchor_target_workspace', S, max(max_boxes, 1)), dev)
    m = f32_array(means) if means is not None else None
    sd = f32_array(stds) if stds is not None else None
    if sl is not None and sl.max_num != cap:
        raise AssertionError('sampler lists of max_num {} for a cap of {}'.format(sl.max_num, cap))
    call('frh_anchor_target', S, ptr(labels), labels.stride(0), ptr(num_boxes), max_boxes, ptr(anchors),
         anchors.stride(0), 0, ptr(gts), gts.stride(1), gts.stride(0), ptr(gt_labels),
         gt_labels.stride(0) if gt_labels is not None else 0, m, sd, cap, ptr(sl.sel if sl else None),
         ptr(sl.sel_counts if sl else None), ptr(chosen_idx), ptr(seg_of), ptr(tar_labels), ptr(tars[0]),
         ptr(tars[1]), ptr(tars[2]), T, ptr(counts), ptr(ws), ws.numel() if ws is not None else 0,
         stream_of(labels))
    if not sync:
        return dict(chosen_idx=chosen_idx, seg_of=seg_of, tar_labels=tar_labels, tar_anchors=tars[0],
                    tar_bbox=tars[1], tar_param=tars[2], counts=None, counts_dev=counts[:S], n_dev=counts[S:])
    cnt = counts.cpu().tolist()  # output sizes are data dependent: one sync per batch
    n = cnt[S]
    return dict(chosen_idx=chosen_idx[:n], seg_of=seg_of[:n], tar_labels=tar_labels[:n],
                tar_anchors=tars[0][:, :n], tar_bbox=tars[1][:, :n], tar_param=tars[2][:, :n], counts=cnt[:S])


class _GatherLevels(torch.autograd.Function):
    """tar = cat_l(level_out.view(C, -1))[:, chosen] per image, with its adjoint scatter.
    Levels of any layout (NCHW, or the channels-last outputs of an NHWC head): the kernels
    take each level's element strides."""

    @staticmethod
    def forward(ctx, chosen_idx, seg_of, channels, *levels):
        n = chosen_idx.numel()
        offs, hw, st, A = _level_desc(levels, channels)
        out = torch.empty(channels, n, dtype=torch.float32, device=chosen_idx.device)
        if n:
            call('frh_gather_level_outputs_strided', len(levels), ptr_array(levels), i64_array(offs), i32_array(hw),
                 i64_array(st), A, channels, n, ptr(chosen_idx), ptr(seg_of), ptr(out), out.stride(0), stream_of(out))
        ctx.save_for_backward(chosen_idx, seg_of)
        ctx.shapes = [(l.shape, l.stride()) for l in levels]
        ctx.channels = channels
        return out

    @staticmethod
    def backward(ctx, grad):
        chosen_idx, seg_of = ctx.saved_tensors
        # each level's gradient in the level's own layout
        grads = [torch.empty_strided(sh, sd, dtype=torch.float32, device=grad.device).zero_() for sh, sd in ctx.shapes]
        grad = grad.contiguous()
        n = chosen_idx.numel()
        offs, hw, st, A = _level_desc(grads, ctx.channels)
        if n:
            call('frh_scatter_level_grads_strided', len(grads), ptr_array(grads), i64_array(offs), i32_array(hw),
                 i64_array(st), A, ctx.channels, n, ptr(chosen_idx), ptr(seg_of), ptr(grad), grad.stride(0),
                 stream_of(grad))
        return (None, None, None) + tuple(grads)


def _level_desc(levels, channels):
    """(first flat index per level, (H, W) per level, element strides per level, anchors A)."""
    offs, hw, st, acc = [], [], [], 0
    A = levels[0].shape[1] // channels
    for l in levels:
        if l.dim() != 4 or l.shape[1] != channels * A:
            raise AssertionError('head outputs must be [B, C*A, H, W] with one A for every level')
        offs.append(acc)
        hw += [l.shape[2], l.shape[3]]
        st += list(l.stride())
        acc += A * l.shape[2] * l.shape[3]
    return offs, hw, st, A


def gather_level_outputs(levels, chosen_idx, seg_of, channels):
    _need_cuda(chosen_idx)
    return _GatherLevels.apply(chosen_idx, seg_of, channels, *levels)


def prepend_gt_labels(prop_labels, num_props, num_gts, max_rows):
    S = prop_labels.shape[0]
    rows = torch.empty(S, max(max_rows, 1), dtype=torch.int64, device=prop_labels.device)
    num_rows = torch.empty(S, dtype=torch.int32, device=prop_labels.device)
    call('frh_prepend_gt_labels', S, ptr(prop_labels), prop_labels.stride(0), ptr(num_props), ptr(num_gts),
         max_rows, ptr(rows), rows.stride(0), ptr(num_rows), stream_of(prop_labels))
    return rows, num_rows


def bbox_target_batched(rows, num_rows, num_gts, max_rows, props, prop_seg_stride, gts, gt_labels, means, stds,
                        max_out_per_seg, sync=True):
    """rows: the sampled prepended rows [S, n] (chosen = label >= 0) or a SampleLists.
    sync=False: full-capacity outputs with padding columns and device counts, as
    anchor_target_batched."""
    if not sync and not isinstance(rows, SampleLists):
        raise AssertionError('sync-free targets need the device sampler lists')
    sl = rows if isinstance(rows, SampleLists) else None
    if sl is not None:
        rows = sl.labels
    S = rows.shape[0]
    dev = rows.device
    cap = max(int(max_out_per_seg), 1)
    T = S * cap
    tars = torch.empty(3, 4, T, dtype=torch.float32, device=dev)
    lab = torch.empty(2, T, dtype=torch.int64, device=dev)
    counts = torch.empty(S + 1, dtype=torch.int32, device=dev)
    ws = None if sl is not None else workspace(_lib.query('frh_bbox_target_workspace', S, max(max_rows, 1)), dev)
    m = f32_array(means) if means is not None else None
    sd = f32_array(stds) if stds is not None else None
    if sl is not None and sl.max_num != cap:
        raise AssertionError('sampler lists of max_num {} for a cap of {}'.format(sl.max_num, cap))
    call('frh_bbox_target', S, ptr(rows), rows.stride(0), ptr(num_rows), ptr(num_gts), max_rows, ptr(props),
         props.stride(-2), prop_seg_stride, ptr(gts), gts.stride(1), gts.stride(0), ptr(gt_labels),
         gt_labels.stride(0), m, sd, cap, ptr(sl.sel if sl else None), ptr(sl.sel_counts if sl else None),
         ptr(tars[0]), ptr(tars[1]), ptr(lab[0]), ptr(tars[2]), ptr(lab[1]), T, ptr(counts), ptr(ws),
         ws.numel() if ws is not None else 0, stream_of(rows))
    if not sync:
        return dict(tar_props=tars[0], tar_bbox=tars[1], tar_label=lab[0], tar_param=tars[2], tar_is_gt=lab[1],
                    counts=None, counts_dev=counts[:S], n_dev=counts[S:])
    cnt = counts.cpu().tolist()
    n = cnt[S]
    return dict(tar_props=tars[0][:, :n], tar_bbox=tars[1][:, :n], tar_label=lab[0][:n], tar_param=tars[2][:, :n],
                tar_is_gt=lab[1][:n], counts=cnt[:S])


# ---------------------------------------------------------------- encode / decode (a7/a8)
def bbox2param(base, bbox, means=None, stds=None):
    _need_cuda(base, bbox)
    base, bbox = _f32(base), _f32(bbox)
    if base.stride(1) != 1:
        base = base.contiguous()
    if bbox.stride(1) != 1:
        bbox = bbox.contiguous()
    n = base.shape[1]
    out = torch.empty(4, n, dtype=torch.float32, device=base.device)
    call('frh_bbox2param', ptr(base), base.stride(0), ptr(bbox), bbox.stride(0), n,
         f32_array(means) if means is not None else None, f32_array(stds) if stds is not None else None,
         ptr(out), out.stride(0), stream_of(base))
    return out


def param2bbox(base, param, means, stds, img_size=None):
    """base [4, n]; param [4*ncls, n] (coordinate-major classes); out like param."""
    _need_cuda(base, param)
    base, param = _f32(base), _f32(param)
    if base.stride(1) != 1:
        base = base.contiguous()
    if param.stride(1) != 1:
        param = param.contiguous()
    n = base.shape[1]
    ncls = param.shape[0] // 4
    out = torch.empty(param.shape[0], n, dtype=torch.float32, device=base.device)
    h, w = (float(img_size[0]), float(img_size[1])) if img_size is not None else (0.0, 0.0)
    call('frh_param2bbox', ptr(base), base.stride(0), ptr(param), param.stride(0), n, ncls, f32_array(means),
         f32_array(stds), int(img_size is not None), h, w, ptr(out), out.stride(0), stream_of(base))
    return out


# ---------------------------------------------------------------- RPN proposals (a9)
def rpn_proposals(cls_outs, reg_outs, anchors, num_anchors, cls_channels, means, stds, img_hw, min_sizes, pre_nms,
                  post_nms, max_num, nms_iou, _entry=None):
    """All images x levels; returns (boxes [B, 4, cap], scores [B, cap], counts int32 device [B]).
    cls / reg levels of any layout (NCHW or channels-last: the kernels take their strides).
    _entry: (ctypes function, name) taking frh_rpn_proposals_strided's arguments instead of it
    (tests: the tools library's four-launch selection)."""
    _need_cuda(*cls_outs)
    B, L = cls_outs[0].shape[0], len(cls_outs)
    grid = [v for c in cls_outs for v in (c.shape[2], c.shape[3])]
    grid_a = i32_array(grid)
    per_level = [num_anchors * c.shape[2] * c.shape[3] for c in cls_outs]
    P = max(min(pre_nms, n) if pre_nms > 0 else n for n in per_level)
    post = min(post_nms, P) if post_nms > 0 else P
    cap = max_num if max_num > 0 else post * L
    dev = cls_outs[0].device
    boxes = torch.empty(B, 4, cap, dtype=torch.float32, device=dev)
    scores = torch.empty(B, cap, dtype=torch.float32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    wsb = _lib.query('frh_rpn_proposals_workspace', B, L, grid_a, num_anchors, int(pre_nms))
    ws = workspace(wsb, dev)
    args = (B, L, ptr_array(cls_outs), ptr_array(reg_outs),
            i64_array([v for c in cls_outs for v in c.stride()]), i64_array([v for r in reg_outs for v in r.stride()]),
            grid_a, num_anchors, cls_channels, ptr(anchors), anchors.stride(0), f32_array(means), f32_array(stds),
            f32_array([v for hw in img_hw for v in hw]), f32_array(min_sizes), int(pre_nms), int(post_nms),
            int(max_num), float(nms_iou), ptr(boxes), ptr(scores), ptr(counts), ptr(status_word(dev)), ptr(ws),
            ws.numel(), stream_of(boxes))
    if _entry is None:
        call('frh_rpn_proposals_strided', *args)
    elif _entry[0](*args) != 0:
        raise RuntimeError('{} failed'.format(_entry[1]))
    _debug_check(dev)
    if NMS_PROFILE['on']:  # keep this call's per-level NMS input (in the workspace) for a replay
        view = (ctypes.c_int64 * 4)()
        call('frh_rpn_proposals_nms_view', B, L, grid_a, num_anchors, int(pre_nms), view)
        o_box, o_cnt, P_, S_ = list(view)
        rows = ws[o_box:o_box + S_ * P_ * 16].view(torch.float32).view(S_, P_, 4)
        cnt = ws[o_cnt:o_cnt + 4 * S_].view(torch.int32)
        NMS_PROFILE['records'].append((ws, rows, cnt, P_, float(nms_iou), int(post_nms) if post_nms > 0 else -1))
    return boxes, scores, counts


NMS_PROFILE = {'on': False, 'records': []}

def nms_bytes(counts, kept):
    """Algorithmic bytes of one segmented NMS call: per segment of N boxes
    20*N + 16*N*ceil(N/64) + 8*K_keep (boxes + scores read, 64-bit mask written and read once)."""
    n = counts.long()
    return int((20 * n + 16 * n * ((n + 63) // 64) + 8 * kept.long()).sum())


# ---------------------------------------------------------------- NMS (a10)
def nms_sorted(boxes_rows, counts, n_max, iou_thr, max_keep=-1):
    """boxes_rows [S, n_max, 4] pre-sorted; returns keep [S, n_max] int32 positions + counts [S]."""
    S = boxes_rows.shape[0]
    dev = boxes_rows.device
    keep = torch.empty(S, max(n_max, 1), dtype=torch.int32, device=dev)
    kc = torch.empty(S, dtype=torch.int32, device=dev)
    ws = workspace(_lib.query('frh_nms_workspace', S, max(n_max, 1)), dev)
    call('frh_nms_sorted', S, ptr(boxes_rows), boxes_rows.stride(0), ptr(counts), n_max, float(iou_thr),
         int(max_keep), ptr(keep), keep.stride(0), ptr(kc), ptr(ws), ws.numel(), stream_of(boxes_rows))
    return keep, kc


def nms(boxes, scores, iou_threshold):
    """Drop-in for torchvision.ops.nms(boxes[N,4], scores[N], thr) -> int64 keep (score order)."""
    _need_cuda(boxes, scores)
    n = boxes.shape[0]
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=boxes.device)
    order = torch.sort(scores, descending=True, stable=True)[1]
    rows = _f32(boxes).index_select(0, order).contiguous().view(1, n, 4)
    counts = torch.full((1,), n, dtype=torch.int32, device=boxes.device)
    keep, kc = nms_sorted(rows, counts, n, iou_threshold)
    k = int(kc.item())
    return order[keep[0, :k].long()]


# ---------------------------------------------------------------- class-wise batched multiclass NMS (a11)
def multiclass_nms_batched(boxes, scores, nms_channel, nms_iou, min_score=-1, max_num=None, score_factor=None,
                           mode='official', num_rows=None, row_valid=None):
    """utils.multiclass_nms (lib/utils.py:224-269) for B images in one frh_mcnms call.

    boxes [B, n, 4] or [B, n, 4 * C] (viewed (n, 4, C)), scores [B, n, C], score_factor
    [B, n] or [B, n, C] (official) or None, num_rows int32 [B] (device; None = n each),
    row_valid bool [B, n] (False = a row the reference drops before the call) or None.
    Returns per-image lists of (boxes [k, 4], scores [k], labels int64 [k]) in the
    reference's keep order.  Two host syncs per call (segment sizes, output counts)."""
    if mode not in ('official', 'strict'):
        raise AssertionError('unknown mode {}'.format(mode))
    _need_cuda(boxes, scores)
    B, n, C = scores.shape
    dev = scores.device
    boxes, scores = _f32(boxes).contiguous(), _f32(scores).contiguous()
    per_class = int(boxes.shape[2] != 4)
    if per_class and boxes.shape[2] != 4 * C:
        raise AssertionError('boxes must be [B, n, 4] or [B, n, 4 * classes]')
    empty = [(boxes.new_zeros(0, 4), scores.new_zeros(0), torch.zeros(0, dtype=torch.long, device=dev))
             for _ in range(B)]
    if n == 0 or max_num == 0:
        return empty
    if num_rows is None:
        num_rows = torch.full((B,), n, dtype=torch.int32, device=dev)
    chan = torch.zeros(C, dtype=torch.uint8)
    chan[[c for c in nms_channel if 0 <= c < C]] = 1
    chan = chan.to(dev)
    sf, sf_pc = None, 0
    if score_factor is not None:
        sf = _f32(score_factor).contiguous()
        sf_pc = int(sf.dim() == 3)
        if sf_pc and mode == 'strict':
            raise AssertionError('strict mode takes a per-row score factor')
    valid = row_valid.to(torch.uint8).contiguous() if row_valid is not None else None
    ws = workspace(_lib.query('frh_mcnms_workspace', B, C, n), dev)
    st = stream_of(scores)
    info_d = torch.empty(4, dtype=torch.int32, device=dev)
    m = 1 if mode == 'strict' else 0
    for by_class in (1, 0):  # a negative candidate coordinate: the reference's single pass, by image
        call('frh_mcnms_prepare', B, C, n, ptr(num_rows), ptr(boxes), boxes.stride(0), per_class, ptr(scores),
             scores.stride(0), ptr(sf), sf.stride(0) if sf is not None else 0, sf_pc, ptr(valid),
             valid.stride(0) if valid is not None else 0, ptr(chan), m, by_class, float(min_score), ptr(ws),
             ws.numel(), ptr(info_d), st)
        info = info_d.cpu().tolist()  # the call's one sync: segment sizes size the sort and the NMS mask
        if not info[1]:
            break
    P = int(info[0])
    tiles = (info[2] & 0xffffffff) | (info[3] << 32)
    if P == 0:
        return empty
    G = C if by_class else 1
    mx = int(max_num) if max_num is not None else -1
    cap = min(mx, G * P) if mx > 0 else G * P
    ob = torch.empty(B, cap, 4, dtype=torch.float32, device=dev)
    osc = torch.empty(B, cap, dtype=torch.float32, device=dev)
    ol = torch.empty(B, cap, dtype=torch.int64, device=dev)
    oc = torch.empty(B, dtype=torch.int32, device=dev)
    nws = workspace(_lib.query('frh_mcnms_nms_workspace', B, C, P, tiles), dev)
    call('frh_mcnms_finish', B, C, n, P, tiles, ptr(boxes), boxes.stride(0), per_class, ptr(scores),
         scores.stride(0), m, by_class, float(nms_iou), mx, ptr(ob), ptr(osc), ptr(ol), ptr(oc), cap, ptr(ws),
         ws.numel(), ptr(nws), nws.numel(), st)
    counts = oc.cpu().tolist()
    return [(ob[b, :k], osc[b, :k], ol[b, :k]) for b, k in enumerate(counts)]


# ---------------------------------------------------------------- RoI level map + RoIAlign (a13/a14)
def roi_rows(boxes, counts, finest_scale, num_levels, seg_stride=0, flat=True):
    """RoI rows [K, 5] (image, x1, y1, x2, y2) + levels ([K] int64, None for one level) of the
    images' boxes (frh_roi_rows): `boxes` [4, ld] with image b's boxes at columns
    offsets[b]... (flat) or [B, 4, cap] with image b's at boxes[b, :, :counts[b]]."""
    _need_cuda(boxes)
    K = int(sum(counts))
    dev = boxes.device
    rois = torch.empty(K, 5, dtype=torch.float32, device=dev)
    lv = torch.empty(K, dtype=torch.int64, device=dev) if num_levels > 1 else None
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + int(c))
    call('frh_roi_rows', len(counts), ptr(boxes), boxes.stride(-2), seg_stride, int(bool(flat)), i64_array(offs),
         float(finest_scale), int(num_levels), ptr(rois), ptr(lv), stream_of(boxes))
    return rois, lv


def roi_rows_dev(boxes, counts_dev, finest_scale, num_levels):
    """roi_rows for a fixed-capacity flat buffer [4, K] whose per-image counts stay on the
    device (frh_roi_rows_dev): all K rows, those past the total being padding rows."""
    _need_cuda(boxes, counts_dev)
    K = boxes.shape[1]
    dev = boxes.device
    rois = torch.empty(K, 5, dtype=torch.float32, device=dev)
    lv = torch.empty(K, dtype=torch.int64, device=dev) if num_levels > 1 else None
    call('frh_roi_rows_dev', counts_dev.numel(), ptr(boxes), boxes.stride(-2), K, ptr(counts_dev),
         float(finest_scale), int(num_levels), ptr(rois), ptr(lv), stream_of(boxes))
    return rois, lv


def roi_level_map(rois, finest_scale, num_levels):
    _need_cuda(rois)
    rois = _f32(rois).contiguous()
    lv = torch.empty(rois.shape[0], dtype=torch.int64, device=rois.device)
    call('frh_roi_level_map', ptr(rois), rois.shape[0], float(finest_scale), int(num_levels), ptr(lv),
         stream_of(rois))
    return lv


def _feat_desc(feats):
    hw = i32_array([v for f in feats for v in (f.shape[2], f.shape[3])])
    st = i64_array([v for f in feats for v in f.stride()])
    return hw, st


# Optional live timing of the RoIAlign forward launches (bench.py roofline):
# HIP events recorded on the launch stream around each call.  A record keeps the
# feature tensors only to replay the same launch shape for timing; with a graphed
# trunk they alias the graph's output buffers, so a replay reads the newest step's
# values -- never use a record's features for their contents.
ROI_ALIGN_PROFILE = {'on': False, 'records': [], 'events': True, 'timed': None, 'event_pool': [], 'launches': 0}
# 'launches': forward launches so far in this process (tools/roi_dispatch_table.py matches
# them to rocprofv3's dispatches by order).
# 'timed': a list -> each forward launch takes a (start, end, span) triple from 'event_pool'
# (created beforehand; span = device span shards, bench.span_slots), goes through
# frh_roi_align_fwd_strided_timed (the events are bound to the kernel's own dispatch
# timestamps, the span is the kernel's own first-wave-start / last-wave-end on the 100 MHz
# GPU clock: nothing is added to the stream) and appends the triple.


_DETERMINISTIC = {'on': os.environ.get('FRCNN_AMD_DETERMINISTIC', '') not in ('', '0')}


def set_deterministic_backward(on):
    """Force (True) / release (False) the RoIAlign backward's deterministic form."""
    _DETERMINISTIC['on'] = bool(on)


def deterministic_backward():
    """The RoIAlign backward runs its fixed-point form (bit-identical across runs) when
    torch.use_deterministic_algorithms(True) is in effect, FRCNN_AMD_DETERMINISTIC=1 is set, or
    set_deterministic_backward(True) was called; otherwise float atomics (faster)."""
    return _DETERMINISTIC['on'] or torch.are_deterministic_algorithms_enabled()


class _RoIAlignMulti(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rois, levels, scales, output_size, sampling_ratio, aligned, *feats):
        _need_cuda(rois, *feats)
        feats = [_f32(f) for f in feats]
        K = rois.shape[0]
        C = feats[0].shape[1]
        ph, pw = output_size
        out = torch.empty(K, C, ph, pw, dtype=torch.float32, device=rois.device)
        hw, st = _feat_desc(feats)
        ROI_ALIGN_PROFILE['launches'] += 1
        prof = ROI_ALIGN_PROFILE['on']
        e0 = e1 = None
        if prof and ROI_ALIGN_PROFILE['events']:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        timed = ROI_ALIGN_PROFILE['timed']
        if timed is not None and ROI_ALIGN_PROFILE['event_pool']:
            ev = ROI_ALIGN_PROFILE['event_pool'].pop()
            call('frh_roi_align_fwd_strided_timed', len(feats), ptr_array(feats), hw, st, f32_array(scales),
                 feats[0].shape[0], C, ptr(rois), ptr(levels), K, ph, pw, int(sampling_ratio), int(bool(aligned)),
                 ptr(out), ev[0].cuda_event, ev[1].cuda_event, ptr(ev[2]) if len(ev) > 2 else None, stream_of(out))
            timed.append(ev)
        else:
            call('frh_roi_align_fwd_strided', len(feats), ptr_array(feats), hw, st, f32_array(scales),
                 feats[0].shape[0], C, ptr(rois), ptr(levels), K, ph, pw, int(sampling_ratio), int(bool(aligned)),
                 ptr(out), stream_of(out))
        if prof:
            if e1 is not None:
                e1.record()
            ROI_ALIGN_PROFILE['records'].append((e0, e1, rois, levels, [tuple(f.shape) for f in feats], (ph, pw),
                                                 feats, tuple(scales), sampling_ratio))
        ctx.save_for_backward(rois, levels)
        ctx.cfg = (list(scales), output_size, sampling_ratio, aligned, [f.shape for f in feats])
        ctx.formats = [torch.channels_last if (f.stride(1) == 1 and f.shape[1] > 1) else torch.contiguous_format
                       for f in feats]
        return out

    @staticmethod
    def backward(ctx, grad):
        rois, levels = ctx.saved_tensors
        scales, (ph, pw), sr, aligned, shapes = ctx.cfg
        grad = grad.contiguous()
        K, B, C = rois.shape[0], shapes[0][0], shapes[0][1]
        # the gradient keeps each feature map's memory format (NCHW or channels_last)
        if deterministic_backward() and int(sr) == 2 and ph <= 8 and pw <= 8:
            # bit-identical across runs: fixed-point (int64, unit from max|grad|) integer atomics, then one
            # conversion pass that writes every gradient element (frh_roi_align_bwd_fixed)
            grads = [torch.empty(s, dtype=torch.float32, device=grad.device, memory_format=fmt)
                     for s, fmt in zip(shapes, ctx.formats)]
            accs = [torch.empty(s, dtype=torch.int64, device=grad.device, memory_format=fmt).zero_()
                    for s, fmt in zip(shapes, ctx.formats)]
            hw, st = _feat_desc(grads)
            word = torch.empty(1, dtype=torch.int32, device=grad.device)  # the call's max|grad_out| bits
            call('frh_roi_align_bwd_fixed', len(grads), ptr_array(grads), ptr_array(accs), hw, st, f32_array(scales),
                 B, C, ptr(rois), ptr(levels), K, ph, pw, int(sr), int(bool(aligned)), ptr(grad), ptr(word),
                 stream_of(grad))
            return (None, None, None, None, None, None) + tuple(grads)
        if deterministic_backward():
            # the fixed-point form covers sampling 2 with up to 8 x 8 bins (every config); the
            # float-atomic form below is not deterministic, which torch's mode must hear about
            msg = ('frcnn_amd roi_align backward: no deterministic form for sampling_ratio={}, '
                   'output {}x{} (fixed point covers sampling 2 and up to 8x8 bins)'.format(sr, ph, pw))
            if torch.are_deterministic_algorithms_enabled() and torch.is_deterministic_algorithms_warn_only_enabled() \
                    and not _DETERMINISTIC['on']:
                if not _DETERMINISTIC.get('warned'):
                    _DETERMINISTIC['warned'] = True
                    warnings.warn(msg)
            else:
                raise RuntimeError(msg)
        # cleared here and accumulated with float atomics (one per row run of a RoI's taps)
        grads = [torch.empty(s, dtype=torch.float32, device=grad.device, memory_format=fmt).zero_()
                 for s, fmt in zip(shapes, ctx.formats)]
        hw, st = _feat_desc(grads)
        call('frh_roi_align_bwd_strided', len(grads), ptr_array(grads), hw, st, f32_array(scales), B, C,
             ptr(rois), ptr(levels), K, ph, pw, int(sr), int(bool(aligned)), ptr(grad), stream_of(grad))
        return (None, None, None, None, None, None) + tuple(grads)


def roi_align_replay(rec, out=None, events=None):
    """Re-issue a recorded RoIAlign forward launch (same features, RoIs and levels) on the
    current stream; bench.py times back-to-back replays for the per-launch kernel duration.
    events: a (start, end) pair bound to the dispatch (frh_roi_align_fwd_strided_timed)."""
    _, _, rois, levels, shapes, (ph, pw), feats, scales, sr = rec
    K, C = rois.shape[0], shapes[0][1]
    if out is None:
        out = torch.empty(K, C, ph, pw, dtype=torch.float32, device=rois.device)
    hw, st = _feat_desc(feats)
    if events is not None:
        call('frh_roi_align_fwd_strided_timed', len(feats), ptr_array(feats), hw, st, f32_array(scales),
             shapes[0][0], C, ptr(rois), ptr(levels), K, ph, pw, int(sr), 0, ptr(out), events[0].cuda_event,
             events[1].cuda_event, ptr(events[2]) if len(events) > 2 else None, stream_of(out))
    else:
        call('frh_roi_align_fwd_strided', len(feats), ptr_array(feats), hw, st, f32_array(scales), shapes[0][0], C,
             ptr(rois), ptr(levels), K, ph, pw, int(sr), 0, ptr(out), stream_of(out))
    return out


def roi_align_multilevel(feats, rois, levels, scales, output_size, sampling_ratio, aligned=False):
    rois = _f32(rois).contiguous()
    return _RoIAlignMulti.apply(rois, levels, tuple(scales), tuple(output_size), sampling_ratio, aligned, *feats)


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else tuple(int(x) for x in v)


def roi_align(input, boxes, output_size, spatial_scale=1.0, sampling_ratio=-1, aligned=False):
    """Drop-in for torchvision.ops.roi_align with [K, 5] rois."""
    if isinstance(boxes, (list, tuple)):
        raise NotImplementedError('roi_align takes [K, 5] rois')
    return roi_align_multilevel([input], boxes, None, [spatial_scale], _pair(output_size), sampling_ratio, aligned)


class RoIAlign(nn.Module):
    """Drop-in for torchvision.ops.RoIAlign (reference registry lib/builder.py:9,22)."""

    def __init__(self, output_size, spatial_scale, sampling_ratio, aligned=False):
        super().__init__()
        self.output_size = _pair(output_size)
        self.spatial_scale = spatial_scale
        self.sampling_ratio = sampling_ratio
        self.aligned = aligned

    def forward(self, input, rois):
        return roi_align(input, rois, self.output_size, self.spatial_scale, self.sampling_ratio, self.aligned)

    def __repr__(self):
        return '{}(output_size={}, spatial_scale={}, sampling_ratio={}, aligned={})'.format(
            type(self).__name__, self.output_size, self.spatial_scale, self.sampling_ratio, self.aligned)


class _RoIPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, rois, output_size, spatial_scale):
        _need_cuda(feat, rois)
        feat = _f32(feat)
        rois = _f32(rois).contiguous()
        K, C = rois.shape[0], feat.shape[1]
        ph, pw = output_size
        out = torch.empty(K, C, ph, pw, dtype=torch.float32, device=feat.device)
        argmax = torch.empty(K, C, ph, pw, dtype=torch.int32, device=feat.device)
        call('frh_roi_pool_fwd', ptr(feat), i64_array(feat.stride()), feat.shape[2], feat.shape[3], C,
             float(spatial_scale), ptr(rois), K, ph, pw, ptr(out), ptr(argmax), stream_of(out))
        ctx.save_for_backward(rois, argmax)
        ctx.shape = feat.shape
        return out

    @staticmethod
    def backward(ctx, grad):
        rois, argmax = ctx.saved_tensors
        g = torch.zeros(ctx.shape, dtype=torch.float32, device=grad.device)
        grad = grad.contiguous()
        call('frh_roi_pool_bwd', ptr(g), i64_array(g.stride()), g.shape[2], g.shape[3], g.shape[1], ptr(rois),
             rois.shape[0], grad.shape[2], grad.shape[3], ptr(grad), ptr(argmax), stream_of(grad))
        return g, None, None, None


def roi_pool(input, boxes, output_size, spatial_scale=1.0):
    """Drop-in for torchvision.ops.roi_pool with [K, 5] rois."""
    return _RoIPoolFn.apply(input, boxes, _pair(output_size), spatial_scale)


class RoIPool(nn.Module):
    """Drop-in for torchvision.ops.RoIPool.  Accepts and ignores `sampling_ratio`, which the
    reference's C4 config passes (configs/faster_rcnn_r50.py:26) and torchvision rejects
    (documented deviation Q9)."""

    def __init__(self, output_size, spatial_scale, sampling_ratio=None):
        super().__init__()
        self.output_size = _pair(output_size)
        self.spatial_scale = spatial_scale

    def forward(self, input, rois):
        return roi_pool(input, rois, self.output_size, self.spatial_scale)


# ---------------------------------------------------------------- ATSS / LTRB targets (a16)
def atss_assign(anchors, grid_sizes, strides, gt_list, label_list, img_shapes, topk=9):
    """Batched FCOSHead.single_image_targets_atss (fcos_head.py:283-368).
    anchors: [4, N] f32 (one per cell, levels concatenated); gt_list: per image [4, G_i];
    label_list: per image [G_i]; img_shapes: per image (h, w).
    Returns cls i64 [B, N], reg f32 [B, N, 4] (ltrb), ctr f32 [B, N]."""
    _need_cuda(anchors)
    dev = anchors.device
    B = len(gt_list)
    L = len(grid_sizes)
    N = sum(int(h) * int(w) for h, w in grid_sizes)
    if anchors.shape[1] != N or anchors.stride(1) != 1:
        raise AssertionError('anchors must be a [4, N] row-contiguous tensor with one anchor per cell')
    gts, gcnt, gmax, labels, img_hw = _pack_ltrb_gts(gt_list, label_list, img_shapes, dev)
    cls, reg, ctr = _ltrb_targets(B, N, dev)
    ws_n = _lib.query('frh_atss_workspace', B, gmax, L, int(topk), N)
    ws = workspace(ws_n, dev)
    hw = i32_array([int(v) for g in grid_sizes for v in g])
    call('frh_atss_assign', B, L, hw, f32_array(strides), ptr(anchors), anchors.stride(0), ptr(gts), gts.stride(0),
         ptr(gcnt), ptr(labels), gmax, ptr(img_hw), int(topk), ptr(cls), ptr(reg), ptr(ctr), ptr(ws), ws_n,
         stream_of(cls))
    return cls, reg, ctr


def _pack_ltrb_gts(gt_list, label_list, img_shapes, dev):
    """The gt arguments the two LTRB assigners share: boxes [B, 4, gmax], counts, gmax, labels
    [B, gmax] i64 and img_hw [B, 2] on the device, without a synchronisation."""
    gts, gcnt, gmax = pack_boxes([g.float() for g in gt_list], dev)
    labels = pack_labels(label_list, gmax, dev)
    img_hw = device_ints([int(v) for s in img_shapes for v in s[:2]], dev)
    return gts, gcnt, gmax, labels, img_hw


def _ltrb_targets(B, N, dev):
    return (torch.empty(B, N, dtype=torch.int64, device=dev), torch.empty(B, N, 4, dtype=torch.float32, device=dev),
            torch.empty(B, N, dtype=torch.float32, device=dev))


def fcos_assign(grid_sizes, strides, gt_list, label_list, img_shapes, scale_thr):
    """Batched FCOSHead.single_image_targets (fcos_head.py:371-416) in one launch (csrc/fcos.hip).
    grid_sizes / strides: per level; gt_list: per image [4, G_i] on the HIP device; label_list:
    per image [G_i]; img_shapes: per image (h, w); scale_thr: the head's level_scale_thr
    (len(grid_sizes) + 1 bounds).  Returns cls i64 [B, N], reg f32 [B, N, 4] (ltrb), ctr f32 [B, N]
    over the level-concatenated cells, as atss_assign does."""
    _need_cuda(*gt_list)
    if not gt_list:
        raise AssertionError('fcos_assign: at least one image expected')
    dev = gt_list[0].device
    B, L = len(gt_list), len(grid_sizes)
    if len(strides) != L or len(scale_thr) != L + 1 or len(label_list) != B or len(img_shapes) != B:
        raise AssertionError('fcos_assign: a stride per level, one more threshold, a label list and a shape per image')
    N = sum(int(h) * int(w) for h, w in grid_sizes)
    gts, gcnt, gmax, labels, img_hw = _pack_ltrb_gts(gt_list, label_list, img_shapes, dev)
    cls, reg, ctr = _ltrb_targets(B, N, dev)
    hw = i32_array([int(v) for g in grid_sizes for v in g])
    call('frh_fcos_assign', B, L, hw, f32_array(strides), f32_array(scale_thr), ptr(gts), gts.stride(0), ptr(gcnt),
         ptr(labels), gmax, ptr(img_hw), ptr(cls), ptr(reg), ptr(ctr), stream_of(cls))
    return cls, reg, ctr


# ---------------------------------------------------------------- FPN top-down merge (channels-last levels)
class _FpnMerge(torch.autograd.Function):
    """out = (lat + bias) + nearest_upsample(up) as a channels-last tensor (frh_fpn_merge_nhwc);
    lat: any layout; bias: [C] or None; up: the merged coarser level (channels-last) or None."""

    @staticmethod
    def forward(ctx, lat, up, bias):
        B, C, H, W = lat.shape
        out = torch.empty(B, C, H, W, dtype=torch.float32, device=lat.device, memory_format=torch.channels_last)
        uh, uw = (int(up.shape[2]), int(up.shape[3])) if up is not None else (0, 0)
        call('frh_fpn_merge_nhwc', ptr(lat), i64_array(lat.stride()), ptr(bias), ptr(up), uh, uw, ptr(out), B, C, H,
             W, stream_of(out))
        ctx.has_up = up is not None
        if ctx.has_up:
            ctx.save_for_backward(up)
        return out

    @staticmethod
    def backward(ctx, g):
        gup = None
        if ctx.has_up and ctx.needs_input_grad[1]:
            (up,) = ctx.saved_tensors
            with torch.enable_grad():
                u = up.detach().requires_grad_(True)
                y = torch.nn.functional.interpolate(u, size=g.shape[2:], mode='nearest')
                gup, = torch.autograd.grad(y, u, g)
        gb = g.sum((0, 2, 3)) if ctx.needs_input_grad[2] else None
        return g if ctx.needs_input_grad[0] else None, gup, gb


def fpn_merge_nhwc(lat, up=None, bias=None):
    """The FPN's top-down step lat + interpolate(up, size=lat.shape[2:], mode='nearest')
    (lib/necks.py:72-84) as one HIP pass writing a channels-last level; bias: the lateral
    conv's bias when lat was computed without it (its add folded into the pass)."""
    _need_cuda(lat, up, bias)
    if lat.dtype != torch.float32 or (up is not None and (up.dtype != torch.float32 or
                                                          not up.is_contiguous(memory_format=torch.channels_last))):
        raise AssertionError('fpn_merge_nhwc: f32 lateral and a channels-last f32 coarser level')
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != lat.shape[1] or not bias.is_contiguous()):
        raise AssertionError('fpn_merge_nhwc: bias must be a contiguous f32 [C]')
    return _FpnMerge.apply(lat, up, bias)


# ---------------------------------------------------------------- BFP neck (Libra R-CNN)
def _nhwc_empty(shape, dev):
    return torch.empty(tuple(shape), dtype=torch.float32, device=dev, memory_format=torch.channels_last)


def _ptrs_or_null(ts):
    return (_lib.c_vp * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


class _Bfp(torch.autograd.Function):
    """BFP.forward (lib/necks.py:116-141) as two launches (frh_bfp_fwd), channels-last outputs;
    backward two launches (frh_bfp_bwd) from the argmax cells the forward stored."""

    @staticmethod
    def forward(ctx, refine_level, *feats):
        L = len(feats)
        B, C = int(feats[0].shape[0]), int(feats[0].shape[1])
        dev = feats[0].device
        hw = [int(v) for f in feats for v in f.shape[2:]]
        outs = [_nhwc_empty(f.shape, dev) for f in feats]
        refine = torch.empty(B, hw[2 * refine_level], hw[2 * refine_level + 1], C, dtype=torch.float32, device=dev)
        amax, n_arg = None, 0
        if any(ctx.needs_input_grad[1:]):
            n_arg = int(_lib.query('frh_bfp_argmax_elems', L, refine_level, B, C, i32_array(hw)))
            amax = torch.empty(max(n_arg, 1), dtype=torch.int32, device=dev)
        call('frh_bfp_fwd', L, refine_level, B, C, ptr_array(feats), i32_array(hw),
             i64_array([s for f in feats for s in f.stride()]), ptr(refine), ptr_array(outs), ptr(amax), n_arg,
             stream_of(feats[0]))
        ctx.cfg = (refine_level, hw, B, C, n_arg)
        if amax is not None:
            ctx.save_for_backward(amax)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gouts):
        r, hw, B, C, n_arg = ctx.cfg
        (amax,) = ctx.saved_tensors
        dev = amax.device
        L = len(gouts)
        gs = [_f32(g) if g is not None else
              torch.zeros(B, C, hw[2 * i], hw[2 * i + 1], dtype=torch.float32, device=dev).contiguous(
                  memory_format=torch.channels_last) for i, g in enumerate(gouts)]
        gins = [None if i == r else _nhwc_empty((B, C, hw[2 * i], hw[2 * i + 1]), dev) for i in range(L)]
        gref = torch.empty(B, hw[2 * r], hw[2 * r + 1], C, dtype=torch.float32, device=dev)
        call('frh_bfp_bwd', L, r, B, C, ptr_array(gs), i32_array(hw), i64_array([s for g in gs for s in g.stride()]),
             ptr(amax), n_arg, ptr(gref), _ptrs_or_null(gins), stream_of(amax))
        gins[r] = gs[r]  # out[r] = feats[r] + refine, and refine does not depend on feats[r]
        return (None,) + tuple(gins)


def bfp(feats, refine_level):
    """The BFP neck's forward (lib/necks.py:116-141, refine_type=None) on f32 HIP levels of any
    layout; returns channels-last levels."""
    feats = list(feats)
    _need_cuda(*feats)
    if not 2 <= len(feats) <= 8 or not 0 <= refine_level < len(feats):
        raise AssertionError('bfp: 2..8 levels and a refine_level among them')
    b, c = feats[0].shape[:2]
    for f in feats:
        if f.dim() != 4 or f.dtype != torch.float32 or f.shape[0] != b or f.shape[1] != c or f.device != feats[0].device:
            raise AssertionError('bfp: f32 [B, C, H, W] levels of one batch, channel count and device')
    return list(_Bfp.apply(int(refine_level), *feats))


class _BiasAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, bias, relu):
        B, C, H, W = y.shape
        call('frh_bias_act_nhwc', ptr(y), ptr(bias), B * H * W, C, int(bool(relu)), stream_of(y))
        ctx.relu = relu
        ctx.mark_dirty(y)
        ctx.save_for_backward(y if relu else None)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        if ctx.relu:
            g = g * (y > 0)
        return g, (g.sum((0, 2, 3)) if ctx.needs_input_grad[1] else None), None


def conv_bias_relu(conv, x, relu=True):
    """act(conv(x)) for a biased Conv2d: on a HIP device with channels-last f32 input and weights
    the conv runs without its bias (MIOpen NHWC) and frh_bias_act_nhwc adds the bias and applies
    the ReLU in one pass (bit-identical to conv + bias, then relu); otherwise the module ops."""
    ok = (x.is_cuda and x.dtype == torch.float32 and conv.bias is not None and conv.weight.dtype == torch.float32
          and conv.out_channels % 4 == 0 and x.is_contiguous(memory_format=torch.channels_last)
          and conv.weight.is_contiguous(memory_format=torch.channels_last))
    if not ok:
        y = conv(x)
        return torch.relu(y) if relu else y
    y = torch.nn.functional.conv2d(x, conv.weight, None, conv.stride, conv.padding, conv.dilation, conv.groups)
    if not y.is_contiguous(memory_format=torch.channels_last):
        y = y.contiguous(memory_format=torch.channels_last)
    return _BiasAct.apply(y, conv.bias, relu)


# ---------------------------------------------------------------- backbone epilogue (frozen BN + add + ReLU)
class _FrozenBNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, skip, weight, bias, mean, var, eps, relu):
        n, c, h, w = x.shape
        x = x.contiguous()
        skip = skip.contiguous() if skip is not None else None
        y = torch.empty_like(x)
        call('frh_bn_act', ptr(x), ptr(skip), ptr(y), ptr(weight), ptr(bias), ptr(mean), ptr(var), float(eps), n, c,
             h * w, int(bool(relu)), stream_of(x))
        need_x = weight is not None and weight.requires_grad
        ctx.save_for_backward(x if need_x else None, y if relu else None, weight, mean, var)
        ctx.cfg = (eps, relu, skip is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, weight, mean, var = ctx.saved_tensors
        eps, relu, has_skip = ctx.cfg
        g = gy * (y > 0) if relu else gy
        inv = torch.rsqrt(var + eps)
        s = inv * weight if weight is not None else inv
        gx = g * s.view(1, -1, 1, 1) if ctx.needs_input_grad[0] else None
        gskip = g if has_skip and ctx.needs_input_grad[1] else None
        gw = gb = None
        if ctx.needs_input_grad[2]:
            gw = (g * (x - mean.view(1, -1, 1, 1))).sum((0, 2, 3)) * inv
        if ctx.needs_input_grad[3]:
            gb = g.sum((0, 2, 3))
        return gx, gskip, gw, gb, None, None, None, None


# The clauses the *_fused_ok predicates below are made of.
def _f32_hip_4d(x):
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 4


def _conv_is(conv, k, stride, padding):
    """A k x k Conv2d of this stride and zero padding, undilated, ungrouped, with an f32 weight."""
    return (conv.kernel_size == (k, k) and conv.stride == (stride, stride) and conv.padding == (padding, padding)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == 'zeros'
            and conv.weight.dtype == torch.float32)


def _frozen_bn(bn):
    """An eval-mode BN that normalises with running statistics (without them, PyTorch takes the
    batch's even in eval mode: the module path)."""
    return not bn.training and bn.running_mean is not None and bn.running_var is not None


def _aligned16(*tensors):
    return all(t is None or t.data_ptr() % 16 == 0 for t in tensors)


def _needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _bn_args(bn):
    """gamma, beta, mean, var, eps as the frh_* entries take them."""
    return ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var), float(bn.eps)


def _level_geometry(xs):
    """The per-level arrays of the *_levels entries: (h, w) of every level, and its image / row /
    column strides."""
    return (i32_array([v for x in xs for v in x.shape[2:]]),
            i64_array([v for x in xs for v in (x.stride(0), x.stride(2), x.stride(3))]))


def bn_act(x, bn, skip=None, relu=True):
    """act(bn(x) (+ skip)) for an eval-mode BatchNorm2d in one HIP pass (frh_bn_act).
    A BN in training mode (the reference never trains BN statistics), one without running
    statistics, or CPU tensors take the plain module ops."""
    if not (_frozen_bn(bn) and _f32_hip_4d(x)) or (x.shape[2] * x.shape[3]) % 4:
        y = bn(x)
        if skip is not None:
            y = y + skip
        return torch.relu_(y) if relu else y
    return _FrozenBNAct.apply(x, skip, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, relu)


# Channel classes (cin, cout) at which tools/bench_conv1x1.py measured frh_conv1x1_bn_act slower
# than MIOpen / Tensile's 1x1 conv followed by frh_bn_act (the long-sum reductions of stages
# 2 to 4; both times in DESIGN section 4): they keep that path.
_CONV1X1_EXCLUDED = frozenset([(512, 128), (512, 256), (1024, 256), (1024, 512), (2048, 512)])


def _conv_bn_fused_ok(conv, bn, x, k, stride, padding):
    """What the fused conv + frozen-BN entries share: a contiguous NCHW f32 HIP input, a bias-free
    conv of this geometry with a contiguous weight, cin % 16 == 0, cout % 64 == 0, 16-byte
    alignment, and no gradient needed."""
    return (_f32_hip_4d(x) and x.is_contiguous() and _frozen_bn(bn) and conv.bias is None
            and _conv_is(conv, k, stride, padding) and conv.weight.is_contiguous()
            and x.shape[1] == conv.in_channels and conv.in_channels % 16 == 0 and conv.out_channels % 64 == 0
            and _aligned16(x, conv.weight) and not _needs_grad(x, conv.weight, bn.weight, bn.bias))


def conv1x1_fused_ok(conv, bn, x, skip=None):
    """Whether conv1x1_bn_act takes the fused HIP entry for these arguments."""
    if not _conv_bn_fused_ok(conv, bn, x, 1, 1, 0) or (x.shape[2] * x.shape[3]) % 4 \
            or (conv.in_channels, conv.out_channels) in _CONV1X1_EXCLUDED:
        return False
    return skip is None or (skip.is_cuda and skip.dtype == torch.float32 and skip.is_contiguous()
                            and skip.shape == (x.shape[0], conv.out_channels, x.shape[2], x.shape[3])
                            and _aligned16(skip) and not _needs_grad(skip))


# Channel classes (cin, cout) at which tools/bench_conv1x1.py measured frh_conv1x1_bn_act_pre /
# frh_conv1x1_s2_bn_act slower than what they replace (both times in DESIGN section 4).
_CONV1X1_PRE_EXCLUDED = frozenset([(512, 2048)])
_CONV1X1_S2_EXCLUDED = frozenset([(512, 1024), (1024, 2048)])
_CONV1X1_PRE_MAX_CIN = 512


def conv1x1_pre_fused_ok(conv, bn, x, pre_bn, skip=None):
    """Whether conv1x1_bn_act folds pre_bn (+ ReLU) into the fused entry's input side."""
    return (conv1x1_fused_ok(conv, bn, x, skip) and _frozen_bn(pre_bn)
            and pre_bn.num_features == conv.in_channels and conv.in_channels <= _CONV1X1_PRE_MAX_CIN
            and (conv.in_channels, conv.out_channels) not in _CONV1X1_PRE_EXCLUDED
            and not _needs_grad(pre_bn.weight, pre_bn.bias))


def conv1x1_bn_act(conv, bn, x, skip=None, relu=True, pre_bn=None):
    """act(bn(conv(x)) (+ skip)) for a bottleneck's 1x1 / stride-1 conv and its eval-mode BN in
    one HIP launch (frh_conv1x1_bn_act: the BN / residual / ReLU epilogue on the GEMM's
    accumulator, no raw conv output in HBM) when nothing needs a gradient through it (the graphed
    trunk, inference, frozen stages); otherwise bn_act(conv(x), bn, skip, relu).
    pre_bn: x is the raw output of the previous conv and relu(pre_bn(x)) is what this conv reads;
    where the fused conditions hold that BN + ReLU is applied inside the same launch
    (frh_conv1x1_bn_act_pre), otherwise by ops.bn_act first."""
    if pre_bn is not None and not conv1x1_pre_fused_ok(conv, bn, x, pre_bn, skip):
        x, pre_bn = bn_act(x, pre_bn), None
    if not conv1x1_fused_ok(conv, bn, x, skip):
        return bn_act(conv(x), bn, skip=skip, relu=relu)
    n, _, h, w = x.shape
    y = torch.empty(n, conv.out_channels, h, w, dtype=torch.float32, device=x.device)
    if pre_bn is not None:
        call('frh_conv1x1_bn_act_pre', ptr(x), ptr(conv.weight), ptr(skip), ptr(y), *_bn_args(bn), *_bn_args(pre_bn), 1,
             n, conv.in_channels, conv.out_channels, h * w, int(bool(relu)), stream_of(x))
        return y
    call('frh_conv1x1_bn_act', ptr(x), ptr(conv.weight), ptr(skip), ptr(y), *_bn_args(bn), n, conv.in_channels,
         conv.out_channels, h * w, int(bool(relu)), stream_of(x))
    return y


def conv1x1_s2_fused_ok(conv, bn, x):
    """Whether conv1x1_s2_bn_act takes the fused HIP entry for these arguments."""
    return (_conv_bn_fused_ok(conv, bn, x, 1, 2, 0) and x.numel() > 0 and x.shape[3] % 8 == 0
            and (conv.in_channels, conv.out_channels) not in _CONV1X1_S2_EXCLUDED)


def conv1x1_s2_bn_act(conv, bn, x, relu=False):
    """act(bn(conv(x))) for a bottleneck's 1x1 / stride-2 projection and its eval-mode BN in one
    HIP launch (frh_conv1x1_s2_bn_act: the GEMM of conv1x1_bn_act reading x at its even rows and
    columns, output width a multiple of 4) when nothing needs a gradient through it; otherwise
    bn_act(conv(x), bn, relu=relu)."""
    if not conv1x1_s2_fused_ok(conv, bn, x):
        return bn_act(conv(x), bn, relu=relu)
    n, _, h, w = x.shape
    y = torch.empty(n, conv.out_channels, (h + 1) // 2, w // 2, dtype=torch.float32, device=x.device)
    call('frh_conv1x1_s2_bn_act', ptr(x), ptr(conv.weight), None, ptr(y), *_bn_args(bn), n, conv.in_channels,
         conv.out_channels, h, w, int(bool(relu)), stream_of(x))
    return y


_RPN_HEAD1X1_MAX_COUT = 16
_RPN_HEAD1X1_MAX_CIN = 256


def _plain_1x1(conv):
    return (_conv_is(conv, 1, 1, 0) and conv.weight.stride(0) == conv.in_channels and conv.weight.stride(1) == 1
            and _aligned16(conv.weight)
            and (conv.bias is None or (conv.bias.dtype == torch.float32 and conv.bias.is_contiguous())))


def rpn_head1x1_fused_ok(classifier, regressor, hidden):
    """Whether rpn_head1x1_levels takes the fused HIP entry for these arguments."""
    hidden = list(hidden)
    if not hidden or len(hidden) > 8 or not (_plain_1x1(classifier) and _plain_1x1(regressor)):
        return False
    cin = classifier.in_channels
    if regressor.in_channels != cin or cin % 8 or cin > _RPN_HEAD1X1_MAX_CIN \
            or classifier.out_channels + regressor.out_channels > _RPN_HEAD1X1_MAX_COUT:
        return False
    x0 = hidden[0]
    for x in hidden:
        if not (_f32_hip_4d(x) and x.device == x0.device
                and x.shape[0] == x0.shape[0] and x.shape[1] == cin and x.numel() > 0 and x.stride(1) == 1
                and (x.shape[2] * x.shape[3] == 1 or _suggests_channels_last(x))
                and _aligned16(x) and all(s >= 0 and s % 4 == 0 for i, (d, s) in enumerate(zip(x.shape, x.stride())) if i != 1 and d > 1)
                and x.shape[0] * x.shape[2] * x.shape[3] < 1 << 31):
            return False
    return not _needs_grad(classifier.weight, classifier.bias, regressor.weight, regressor.bias, *hidden)


def _suggests_channels_last(t):
    """torch's own stride rule (c10 is_channels_last_strides_4d) for whether a conv returns a
    channels-last output for this 4-d input or weight."""
    least = 0
    if t.stride(1) == 0:
        return False
    for d in (1, 3, 2, 0):
        if t.shape[d] == 0 or t.stride(d) < least or (d == 0 and least == t.stride(1)):
            return False
        least = t.stride(d) * max(t.shape[d], 1)
    return True


def rpn_head1x1_levels(classifier, regressor, hidden):
    """([classifier(h) for h in hidden], [regressor(h) for h in hidden]) for the RPN head's two
    1x1 convs: one HIP launch over every level (frh_rpn_head1x1_levels: each level read once for
    both convs, bias on the accumulator, one fixed-order f32 sum per output) on channels-last f32
    HIP levels when nothing needs a gradient; otherwise the module calls.  The outputs are
    channels-last, as the modules return for a channels-last input."""
    hidden = list(hidden)
    if not rpn_head1x1_fused_ok(classifier, regressor, hidden):
        return [classifier(h) for h in hidden], [regressor(h) for h in hidden]
    n, dev, cin = hidden[0].shape[0], hidden[0].device, classifier.in_channels
    cc, cr = classifier.out_channels, regressor.out_channels
    def out(conv, x):
        # the memory is [n, h, w, c] either way; a one-pixel level is also NCHW-contiguous, and
        # then the modules return it with those strides
        fmt = torch.channels_last if _suggests_channels_last(x) or _suggests_channels_last(conv.weight) \
            else torch.contiguous_format
        return torch.empty((n, conv.out_channels, x.shape[2], x.shape[3]), dtype=torch.float32, device=dev,
                           memory_format=fmt)
    cls = [out(classifier, x) for x in hidden]
    reg = [out(regressor, x) for x in hidden]
    call('frh_rpn_head1x1_levels', len(hidden), ptr_array(hidden), ptr_array(cls), ptr_array(reg),
         ptr(classifier.weight), ptr(classifier.bias), ptr(regressor.weight), ptr(regressor.bias), n, cin, cc, cr,
         *_level_geometry(hidden), stream_of(hidden[0]))
    return cls, reg


def roi_conv3x3_fused_ok(conv, bn, x):
    """Whether roi_conv3x3_bn_act takes the fused HIP entry for these arguments.  No RoI count is
    excluded: tools/bench_roi_conv.py measured the entry faster than the modules at r = 512, 1000
    and 2000 (both times in DESIGN section 4)."""
    return _conv_bn_fused_ok(conv, bn, x, 3, 1, 1) and x.shape[2:] == (7, 7)


def roi_conv3x3_bn_act(conv, bn, x, relu=True):
    """act(bn(conv(x))) for the Double-Head regression branch's 3x3 / stride-1 / padding-1 conv over
    the RoI tiles [R, cin, 7, 7] and its eval-mode BN in one fused launch pair
    (frh_roi_conv3x3_bn_act: NCHW in and out, the BN / ReLU epilogue on the f32-MFMA accumulator)
    when nothing needs a gradient through it (inference); otherwise the module ops, which covers
    training-mode BN (batch statistics), any other stride or padding, and CPU tensors."""
    if not roi_conv3x3_fused_ok(conv, bn, x):
        y = bn(conv(x))
        return torch.relu(y) if relu else y
    r = x.shape[0]
    y = torch.empty(r, conv.out_channels, 7, 7, dtype=torch.float32, device=x.device)
    ws = torch.empty(9 * conv.in_channels * conv.out_channels, dtype=torch.float32, device=x.device)
    call('frh_roi_conv3x3_bn_act', ptr(x), ptr(conv.weight), ptr(y), *_bn_args(bn), r, conv.in_channels,
         conv.out_channels, int(bool(relu)), ptr(ws), stream_of(x))
    return y


# Level sizes (h, w) at which tools/bench_conv3x3.py measured a frh_conv3x3_bias_act call of
# that level alone slower than the MIOpen NHWC conv followed by its bias (+ ReLU) pass (too few
# workgroups for the chip; both times in DESIGN section 4): alone they keep that path, in a
# multi-level launch beside a larger level they ride along.
_CONV3X3_EXCLUDED = frozenset([(38, 64), (19, 32), (10, 16)])


def conv3x3_fused_ok(conv, x, alone=True):
    """Whether conv3x3_bias_act takes the fused HIP entry for these arguments (alone=False:
    as one level of a multi-level launch, where the size exclusions do not apply)."""
    if not (_f32_hip_4d(x) and _conv_is(conv, 3, 1, 1)
            and conv.weight.is_contiguous(memory_format=torch.channels_last)):
        return False
    cout, cin = conv.out_channels, conv.in_channels
    n, c, h, w = x.shape
    sn, sc, sy, sx = x.stride()
    if c != cin or cin % 8 or cout % 64 or n == 0 or h == 0 or w == 0 or (alone and (h, w) in _CONV3X3_EXCLUDED):
        return False
    if sc != 1 or sx < cin or sy < 0 or sn < 0 or (sn | sy | sx) % 4 \
            or (h - 1) * sy + (w - 1) * sx + cin >= 1 << 30:
        return False
    return _aligned16(x, conv.weight, conv.bias) and not _needs_grad(x, conv.weight, conv.bias)


def _conv3x3_ws(cin, cout, dev):
    """The transformed-weight workspace of one call (every call rewrites it)."""
    return torch.empty(16 * cin * cout, dtype=torch.float32, device=dev)


def conv3x3_bias_act(conv, x, relu=False):
    """act(conv(x)) for a 3x3 / stride-1 / padding-1 Conv2d on a channels-last (or channel-stride-1
    strided) f32 HIP input in one fused launch pair (frh_conv3x3_bias_act: Winograd F(2x2, 3x3)
    on the f32 MFMA, bias / ReLU on the accumulators) when nothing needs a gradient through it
    (the graphed trunk, inference); otherwise conv_bias_relu / the module."""
    if not conv3x3_fused_ok(conv, x):
        return conv_bias_relu(conv, x) if relu else conv(x)
    n, _, h, w = x.shape
    sn, _, sy, sx = x.stride()
    y = _nhwc_empty((n, conv.out_channels, h, w), x.device)
    call('frh_conv3x3_bias_act', ptr(x), ptr(conv.weight), ptr(conv.bias), ptr(y),
         ptr(_conv3x3_ws(conv.in_channels, conv.out_channels, x.device)), n, conv.in_channels, conv.out_channels, h, w,
         sn, sy, sx, int(bool(relu)), stream_of(x))
    return y


def conv3x3_bias_act_levels(convs, xs, relu=False):
    """conv3x3_bias_act on every level of a pyramid, convs one shared Conv2d (the RPN head) or one
    per level (the FPN output convs): one weight-transform launch and one convolution launch
    (frh_conv3x3_bias_act_levels) for the levels that can take the fused entry, provided one of
    them would take it alone; conv3x3_bias_act for the others.  Same bits as the per-level calls."""
    xs = list(xs)
    convs = [convs] * len(xs) if isinstance(convs, nn.Module) else list(convs)
    if len(convs) != len(xs):
        raise AssertionError('conv3x3_bias_act_levels: one conv, or one per level')
    fused = [i for i, (c, x) in enumerate(zip(convs, xs)) if conv3x3_fused_ok(c, x, alone=False)]
    if fused:
        c0, x0 = convs[fused[0]], xs[fused[0]]
        fused = [i for i in fused if (convs[i].in_channels, convs[i].out_channels, xs[i].shape[0], xs[i].device)
                 == (c0.in_channels, c0.out_channels, x0.shape[0], x0.device)][:8]
    if len(fused) < 2 or not any(conv3x3_fused_ok(convs[i], xs[i]) for i in fused):
        return [conv3x3_bias_act(c, x, relu) for c, x in zip(convs, xs)]
    outs = [None if i in fused else conv3x3_bias_act(c, x, relu) for i, (c, x) in enumerate(zip(convs, xs))]
    fx, fc = [xs[i] for i in fused], [convs[i] for i in fused]
    n, dev, cin, cout = fx[0].shape[0], fx[0].device, fc[0].in_channels, fc[0].out_channels
    ys = [_nhwc_empty((n, cout, x.shape[2], x.shape[3]), dev) for x in fx]
    distinct = 1 + sum(1 for a, b in zip(fc, fc[1:]) if a.weight.data_ptr() != b.weight.data_ptr())
    ws = _conv3x3_ws(cin, cout * distinct, dev)
    call('frh_conv3x3_bias_act_levels', len(fx), ptr_array(fx), ptr_array([c.weight for c in fc]),
         _ptrs_or_null([c.bias for c in fc]), ptr_array(ys), ptr(ws), ws.numel() * 4, n, cin, cout,
         *_level_geometry(fx), int(bool(relu)), stream_of(fx[0]))
    for i, y in zip(fused, ys):
        outs[i] = y
    return outs


# ---------------------------------------------------------------- VGG16 convolutions
# Classes (cin, cout, pool) of VGG16's convs, the stem as (3, 64, False), at which
# tools/bench_vgg.py measured the fused side slower than the modules on the same channels-last
# input (MIOpen NHWC conv, frh_bias_act_nhwc, max_pool2d; both times in DESIGN section 4): they
# keep that path.
_VGG_CONV_EXCLUDED = frozenset()


def vgg_conv_fused_ok(conv, x, pool):
    """Whether vgg_conv takes the fused HIP entry: conv3x3_fused_ok's conditions without the
    level-size exclusions (measured at 256 channels for the FPN levels), and a class that is
    dispatched."""
    return (conv3x3_fused_ok(conv, x, alone=False)
            and (conv.in_channels, conv.out_channels, bool(pool)) not in _VGG_CONV_EXCLUDED)


def _vgg_conv_call(x, weight, bias, cin, cout, pool):
    """relu(conv3x3(x) + bias), max-pooled 2 x 2 when `pool`, by the fused entries."""
    n, _, h, w = x.shape
    sn, _, sy, sx = x.stride()
    y = _nhwc_empty((n, cout, h // 2, w // 2) if pool else (n, cout, h, w), x.device)
    call('frh_conv3x3_bias_act_pool' if pool else 'frh_conv3x3_bias_act', ptr(x), ptr(weight), ptr(bias), ptr(y),
         ptr(_conv3x3_ws(cin, cout, x.device)), n, cin, cout, h, w, sn, sy, sx, 1, stream_of(x))
    return y


def vgg_conv(conv, x, pool=False):
    """relu(conv(x)), then max_pool2d(., 2) when `pool`, for a 3x3 / stride-1 / padding-1 Conv2d
    of VGG16: one fused launch pair (frh_conv3x3_bias_act, or frh_conv3x3_bias_act_pool with the
    pool on the accumulators) where vgg_conv_fused_ok holds; otherwise conv_bias_relu and
    F.max_pool2d."""
    if vgg_conv_fused_ok(conv, x, pool):
        return _vgg_conv_call(x, conv.weight, conv.bias, conv.in_channels, conv.out_channels, pool)
    y = conv_bias_relu(conv, x)
    return torch.nn.functional.max_pool2d(y, 2) if pool else y


class _PaddedStem(object):
    """What conv3x3_fused_ok reads of a Conv2d, for the stem conv with its cin padded to 8."""

    def __init__(self, conv, weight):
        self.weight, self.bias = weight, conv.bias
        self.in_channels, self.out_channels = 8, conv.out_channels
        for k in ('kernel_size', 'stride', 'padding', 'dilation', 'groups', 'padding_mode'):
            setattr(self, k, getattr(conv, k))


def _stem_weight8(conv):
    """The stem's weight [cout, cin, 3, 3] zero-padded to [cout, 8, 3, 3], channels-last; made
    once per weight version (the memo holds the weight, so its storage is not reused)."""
    w = conv.weight

    def make():
        with torch.no_grad():
            w8 = torch.zeros((w.shape[0], 8, 3, 3), dtype=w.dtype, device=w.device)
            w8 = w8.contiguous(memory_format=torch.channels_last)
            w8[:, :w.shape[1]] = w
            return w8
    return _memo([w], ('vgg_stem_weight8', w.device, w.data_ptr()), make)


def vgg_stem(conv, img):
    """relu(conv(img)) for VGG16's first conv (3 input channels) on a contiguous NCHW f32 HIP
    image: frh_nchw_to_nhwc8 pads the channels to 8 in one pass and frh_conv3x3_bias_act runs on
    it with the zero-padded weight (one cin chunk; the zero channels add exact zeros), under
    vgg_conv_fused_ok's conditions on the padded tensors.  Otherwise the module and a ReLU."""
    cin = conv.in_channels
    ok = (_f32_hip_4d(img) and img.is_contiguous() and 1 <= cin <= 8 and img.shape[1] == cin and img.numel() > 0
          and conv.weight.dim() == 4 and conv.weight.is_cuda and conv.weight.dtype == torch.float32
          and (cin, conv.out_channels, False) not in _VGG_CONV_EXCLUDED
          and _aligned16(img) and not _needs_grad(img, conv.weight, conv.bias))
    if ok:
        n, _, h, w = img.shape
        x8 = torch.empty((n, h, w, 8), dtype=torch.float32, device=img.device).permute(0, 3, 1, 2)
        stem = _PaddedStem(conv, _stem_weight8(conv))
        ok = vgg_conv_fused_ok(stem, x8, False)
    if not ok:
        return torch.relu(conv(img))
    call('frh_nchw_to_nhwc8', ptr(img), ptr(x8), n, cin, h, w, stream_of(img))
    return _vgg_conv_call(x8, stem.weight, stem.bias, 8, conv.out_channels, False)


# ---------------------------------------------------------------- one-stage head convolutions
_CONV3X3_OUT_MAX_COUT = 192

# The parts of a one-stage head at which tools/bench_head_convs.py measured the fused side slower
# than the modules (both times in DESIGN section 4, "One-stage head convolutions"), keyed by what
# was measured: ('tower', cin, cout) for a tower layer over the levels, ('out', cin, c0, c1) for an
# output group.  A part is dispatched only where the fused side's slowest repetition beat the
# modules' fastest; a part listed here keeps the modules for itself, the rest of the head stays
# fused.
_HEAD_CONVS_EXCLUDED = frozenset()


def _conv3x3_plain(conv):
    """A 3x3 / stride-1 / padding-1 Conv2d with a channels-last f32 weight and an f32 bias (or
    none), both 16-byte aligned where the entries read them as vectors."""
    return (isinstance(conv, nn.Conv2d) and _conv_is(conv, 3, 1, 1) and conv.in_channels % 8 == 0
            and conv.weight.is_contiguous(memory_format=torch.channels_last) and _aligned16(conv.weight)
            and (conv.bias is None or (conv.bias.dtype == torch.float32 and conv.bias.is_contiguous()
                                       and _aligned16(conv.bias))))


def _levels_ok(xs, cin):
    """f32 HIP levels of one batch and device with cin channels at stride 1, at most 8, whose other
    strides the *_levels entries take (non-negative multiples of 4)."""
    if not xs or len(xs) > 8:
        return False
    x0 = xs[0]
    for x in xs:
        if not (_f32_hip_4d(x) and x.device == x0.device and x.shape[0] == x0.shape[0] and x.shape[1] == cin
                and x.numel() > 0 and x.stride(1) == 1 and _aligned16(x)
                and all(s >= 0 and s % 4 == 0 for i, (d, s) in enumerate(zip(x.shape, x.stride())) if i != 1 and d > 1)
                and x.shape[0] * x.shape[2] * x.shape[3] < 1 << 27):
            return False
    return True


def _out_group_ok(convs):
    """One or two output convs frh_conv3x3_out_levels takes in one launch."""
    return (1 <= len(convs) <= 2 and all(_conv3x3_plain(c) and c.in_channels == convs[0].in_channels for c in convs)
            and sum(c.out_channels for c in convs) <= _CONV3X3_OUT_MAX_COUT)


def _out_class(convs):
    return ('out', convs[0].in_channels, convs[0].out_channels, convs[1].out_channels if len(convs) > 1 else 0)


def conv3x3_out_fused_ok(convs, xs, scales=None):
    """Whether conv3x3_out_levels takes the fused HIP entry for these arguments."""
    convs, xs = list(convs), list(xs)
    if not (_out_group_ok(convs) and _levels_ok(xs, convs[0].in_channels)) or _out_class(convs) in _HEAD_CONVS_EXCLUDED:
        return False
    flat = []
    for k, conv in enumerate(convs):
        sk = scales[k] if scales is not None else None
        if sk is None:
            continue
        if len(sk) != len(xs):
            return False
        for s in sk:
            if s is not None and not (s.is_cuda and s.dtype == torch.float32 and s.dim() == 1 and s.is_contiguous()
                                      and s.numel() == conv.out_channels):
                return False
        flat += list(sk)
    return not _needs_grad(*(xs + [c.weight for c in convs] + [c.bias for c in convs] + flat))


def _conv_out_empty(conv, x):
    """The output of conv for the level x, as the module would lay it out: the memory is
    [n, h, w, c] either way; a one-pixel level is also NCHW-contiguous, and then the modules return
    it with those strides."""
    fmt = torch.channels_last if _suggests_channels_last(x) or _suggests_channels_last(conv.weight) \
        else torch.contiguous_format
    return torch.empty((x.shape[0], conv.out_channels, x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device,
                       memory_format=fmt)


def conv3x3_out_levels(convs, xs, scales=None, exp=False):
    """The prediction convs of a one-stage head over every level: convs one Conv2d or a list of one
    or two that read the same levels xs (3x3 / stride 1 / padding 1, at most 192 output channels
    together); returns one list of per-level [n, c, h, w] channels-last tensors per conv,
    [exp(conv(x) * scale)] with the scale and the exp optional per conv: scales None, or per conv
    None or a list of per-level f32 [c] tensors (entries may be None); exp a bool, or one per conv.
    One HIP launch (frh_conv3x3_out_levels: a direct f32-MFMA convolution, each level read once
    for both convs, bias / scale / exp on the accumulators, one fixed-order sum per output) on
    channel-stride-1 f32 HIP levels when nothing needs a gradient; otherwise the module
    expressions."""
    convs = [convs] if isinstance(convs, nn.Module) else list(convs)
    xs = list(xs)
    exps = [bool(exp)] * len(convs) if isinstance(exp, (bool, int)) else [bool(e) for e in exp]
    if scales is not None:
        scales = [None if s is None else list(s) for s in scales]
    if len(exps) != len(convs) or (scales is not None and len(scales) != len(convs)):
        raise AssertionError('conv3x3_out_levels: one scale list and one exp flag per conv')
    if not conv3x3_out_fused_ok(convs, xs, scales):
        outs = []
        for k, conv in enumerate(convs):
            ys = []
            for i, x in enumerate(xs):
                y = conv(x)
                s = scales[k][i] if scales is not None and scales[k] is not None else None
                if s is not None:
                    y = y * s.view(-1, 1, 1)
                ys.append(torch.exp(y) if exps[k] else y)
            outs.append(ys)
        return outs
    ys = [[_conv_out_empty(conv, x) for x in xs] for conv in convs]
    two = len(convs) == 2
    c0, c1 = convs[0], convs[1] if two else None
    sc = [None if scales is None or scales[k] is None else _ptrs_or_null(scales[k]) for k in range(len(convs))]
    call('frh_conv3x3_out_levels', len(xs), ptr_array(xs), ptr_array(ys[0]), ptr_array(ys[1]) if two else None,
         ptr(c0.weight), ptr(c0.bias), ptr(c1.weight) if two else None, ptr(c1.bias) if two else None,
         sc[0], sc[1] if two else None, int(exps[0]), int(exps[1]) if two else 0, xs[0].shape[0], c0.in_channels,
         c0.out_channels, c1.out_channels if two else 0, *_level_geometry(xs), stream_of(xs[0]))
    return ys


def _tower_convs(tower):
    """The convs of a head tower (a Sequential of Conv2d, ReLU pairs), or None if it is anything else."""
    mods = list(tower)
    if len(mods) % 2 or not all(isinstance(c, nn.Conv2d) and isinstance(r, nn.ReLU)
                                for c, r in zip(mods[0::2], mods[1::2])):
        return None
    return mods[0::2]


def head_convs_fused_ok(tower_convs, out_convs, xs, extra=()):
    """Whether a one-stage head runs its towers and output convs on the fused HIP entries
    (head_tower_levels, conv3x3_out_levels) for these arguments; all or nothing per head.
    tower_convs: the head's towers (each a Sequential of Conv2d, ReLU pairs); out_convs: one group of
    one or two output convs per tower; xs: the levels; extra: further tensors of the forward
    (FCOSHead's reg_coef).  True only for at most 8 f32 HIP levels with channel stride 1,
    channels-last f32 weights, 3x3 / stride-1 / padding-1 tower convs each followed by a ReLU with
    cin % 8 == 0 and cout % 64 == 0, output groups within frh_conv3x3_out_levels' limits, nothing
    needing a gradient, and a head of which a part is dispatched at all (_HEAD_CONVS_EXCLUDED: a
    listed part keeps its modules inside the fused forward)."""
    xs = list(xs)
    if not xs or not all(torch.is_tensor(x) and x.dim() == 4 for x in xs) or not _levels_ok(xs, xs[0].shape[1]):
        return False
    parts = _head_parts(tower_convs, out_convs, xs[0].shape[1])
    if parts is None or all(p in _HEAD_CONVS_EXCLUDED for p, _ in parts):
        return False
    tensors = xs + list(extra)
    for _, convs in parts:
        for conv in convs:
            tensors += [conv.weight, conv.bias]
    return not _needs_grad(*tensors)


def _head_parts(tower_convs, out_convs, cin):
    """The parts of a head whose layers the fused entries can run on cin-channel levels, as
    (class, convs) pairs in forward order -- ('tower', cin, cout) per tower layer, ('out', cin, c0,
    c1) per output group -- or None where a layer is outside them (the device, the levels and the
    gradients are head_convs_fused_ok's to check)."""
    towers, groups = list(tower_convs), [list(g) for g in out_convs]
    if len(towers) != len(groups):
        return None
    parts = []
    for tower, group in zip(towers, groups):
        convs = _tower_convs(tower)
        if convs is None:
            return None
        c = cin
        for conv in convs:
            if not (_conv3x3_plain(conv) and conv.in_channels == c and conv.out_channels % 64 == 0):
                return None
            parts.append((('tower', conv.in_channels, conv.out_channels), [conv]))
            c = conv.out_channels
        if not _out_group_ok(group) or group[0].in_channels != c:
            return None
        parts.append((_out_class(group), group))
    return parts


def head_tower_levels(tower, xs):
    """[tower(x) for x in xs] for a head tower head_convs_fused_ok accepted: layer by layer, one
    conv3x3_bias_act_levels call (the conv shared over the levels, bias + ReLU on the Winograd
    accumulators); a layer class listed in _HEAD_CONVS_EXCLUDED runs its modules."""
    xs = list(xs)
    for conv in _tower_convs(tower):
        if ('tower', conv.in_channels, conv.out_channels) in _HEAD_CONVS_EXCLUDED:
            xs = [torch.relu(conv(x)) for x in xs]
        else:
            xs = conv3x3_bias_act_levels(conv, xs, relu=True)
    return xs


# Channel classes (cin, cout) at which tools/bench_conv3x3_nchw.py measured frh_conv3x3_nchw_bn_act
# (weight transform included) slower than MIOpen's NCHW 3x3 conv, plus frh_bn_act where the
# entry's epilogue replaces one (both times in DESIGN section 4): they keep the module.  A class
# is dispatched only where the fused side's slowest repetition beat the module's fastest.  Empty
# since the cin-split forms: all four ResNet-50 classes are dispatched.
_CONV3X3_NCHW_EXCLUDED = frozenset()


def conv3x3_nchw_fused_ok(conv, x, bn=None):
    """Whether conv3x3_nchw_bn_act takes the fused HIP entry for these arguments.  Only with grad
    mode off (the graphed trunk, inference): a training step runs the module even through a frozen
    stage, so every training step computes exactly what it computed before this entry existed."""
    if torch.is_grad_enabled():
        return False
    if not (_f32_hip_4d(x) and x.is_contiguous() and _conv_is(conv, 3, 1, 1) and conv.bias is None
            and conv.weight.is_contiguous() and (bn is None or _frozen_bn(bn))):
        return False
    cin, cout = conv.in_channels, conv.out_channels
    n, c, h, w = x.shape
    if c != cin or cin % 4 or cout % 16 or w % 2 or x.numel() == 0 or h * w >= 1 << 27 \
            or max(cin, cout) * h * w >= 1 << 31 or cin * cout >= 1 << 24 or (cin, cout) in _CONV3X3_NCHW_EXCLUDED:
        return False
    return _aligned16(x, conv.weight) and not _needs_grad(x, conv.weight, *((bn.weight, bn.bias) if bn is not None else ()))


def conv3x3_nchw_bn_act(conv, x, bn=None, relu=False):
    """act(bn(conv(x))) for a bottleneck's 3x3 / stride-1 / padding-1 conv on a contiguous NCHW f32
    HIP input (bn None: the raw convolution) in one fused launch pair (frh_conv3x3_nchw_bn_act:
    Winograd F(2x2, 3x3) on the f32 MFMA, the eval-mode BN / ReLU on the accumulators) with grad
    mode off (the graphed trunk, inference); otherwise the module, followed by ops.bn_act where
    there is a BN."""
    if not conv3x3_nchw_fused_ok(conv, x, bn):
        y = conv(x)
        if bn is not None:
            return bn_act(y, bn, relu=relu)
        return torch.relu_(y) if relu else y
    n, _, h, w = x.shape
    cin, cout = conv.in_channels, conv.out_channels
    y = torch.empty(n, cout, h, w, dtype=torch.float32, device=x.device)
    ws = torch.empty(16 * cin * cout, dtype=torch.float32, device=x.device)
    bn_args = _bn_args(bn) if bn is not None else (None, None, None, None, 0.0)
    call('frh_conv3x3_nchw_bn_act', ptr(x), ptr(conv.weight), *bn_args, ptr(y), ptr(ws), n, cin, cout, h, w,
         int(bool(relu)), stream_of(x))
    return y


# ---------------------------------------------------------------- deformable 3x3 conv (GA-RPN)
def deform_conv3x3_torch(x, offset, weight, dg, relu=False):
    """The deformable 3x3 / stride-1 / padding-1 convolution of include/frcnn_amd.h
    (frh_deform_conv3x3_act, DCNv1) restated as a gather and a matmul in torch ops, in x's dtype
    and on x's device: the path autograd differentiates (training), and in f64 the numerics
    reference of the tests.  x [n, cin, h, w], offset [n, 18 dg, h, w], weight [cout, cin, 3, 3]."""
    n, cin, H, W = x.shape
    cout, cpg = weight.shape[0], cin // dg
    if weight.shape[1:] != (cin, 3, 3) or cin % dg or offset.shape != (n, 18 * dg, H, W):
        raise AssertionError('deform_conv3x3: weight [cout, cin, 3, 3] and offset [n, 18 dg, h, w] expected')
    dt, dev = x.dtype, x.device
    off = offset.to(dt).reshape(n, dg, 9, 2, H, W)
    ky = torch.arange(9, device=dev).div(3, rounding_mode='floor').sub(1).to(dt).view(1, 1, 9, 1, 1)
    kx = torch.arange(9, device=dev).remainder(3).sub(1).to(dt).view(1, 1, 9, 1, 1)
    py = (torch.arange(H, dtype=dt, device=dev).view(1, 1, 1, H, 1) + ky) + off[:, :, :, 0]
    px = (torch.arange(W, dtype=dt, device=dev).view(1, 1, 1, 1, W) + kx) + off[:, :, :, 1]
    ok = (py > -1) & (py < H) & (px > -1) & (px < W)  # False for NaN
    py, px = torch.where(ok, py, torch.zeros_like(py)), torch.where(ok, px, torch.zeros_like(px))
    fy, fx = py.floor(), px.floor()
    ly, lx = py - fy, px - fx
    hy, hx = 1 - ly, 1 - lx
    y0, x0 = fy.long(), fx.long()
    xg = x.reshape(n, dg, cpg, H * W)

    def corner(yy, xx, wgt):
        valid = ok & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).view(n, dg, 1, 9 * H * W).expand(-1, -1, cpg, -1)
        v = xg.gather(3, idx).view(n, dg, cpg, 9, H, W)
        return v * (wgt * valid.to(dt)).unsqueeze(2)

    s = ((corner(y0, x0, hy * hx) + corner(y0, x0 + 1, hy * lx)) + corner(y0 + 1, x0, ly * hx)) \
        + corner(y0 + 1, x0 + 1, ly * lx)
    y = torch.matmul(weight.to(dt).reshape(cout, cin * 9), s.reshape(n, cin * 9, H * W)).view(n, cout, H, W)
    return torch.relu(y) if relu else y


def _dc_x_ok(x, cin):
    sn, sc, sy, sx = x.stride()
    return (_f32_hip_4d(x) and x.shape[1] == cin and x.numel() > 0 and sc == 1 and sx >= cin and sy >= 0 and sn >= 0
            and (sn | sy | sx) % 4 == 0)


def deform_conv3x3_fused_ok(x, offset, weight, dg, offset_weight=None):
    """Whether deform_conv3x3 / deform_conv3x3_levels take the HIP entry for these arguments
    (offset_weight given: `offset` is the 2-channel shape map of the guided mode)."""
    return _dc_shapes_ok(x, offset, weight, dg, offset_weight) and not _needs_grad(x, offset, weight, offset_weight)


def _dc_shapes_ok(x, offset, weight, dg, offset_weight=None):
    """deform_conv3x3_fused_ok without the gradient test: what the HIP entries accept."""
    if not (torch.is_tensor(weight) and weight.dim() == 4 and weight.is_cuda and weight.dtype == torch.float32
            and weight.is_contiguous() and weight.shape[2:] == (3, 3)):
        return False
    cout, cin = weight.shape[:2]
    if cin % 16 or cout % 64 or dg < 1 or cin % dg or (cin // dg) % 4:
        return False
    och = 2 if offset_weight is not None else 18 * dg
    if not (_dc_x_ok(x, cin) and _f32_hip_4d(offset)
            and offset.shape == (x.shape[0], och, x.shape[2], x.shape[3])):
        return False
    if offset_weight is not None and not (offset_weight.is_cuda and offset_weight.dtype == torch.float32
                                          and offset_weight.is_contiguous() and offset_weight.numel() == 36 * dg):
        return False
    return _aligned16(x, weight, offset_weight)


def _dc_ws(cin, cout, dev):
    """The repacked-weight workspace of one call (every call rewrites it)."""
    return torch.empty(9 * cin * cout, dtype=torch.float32, device=dev)


def _as_channels_last(x):
    return x if x.stride(1) == 1 else x.contiguous(memory_format=torch.channels_last)


def _dc_act(x, offset, weight, dg, relu, ow):
    """One frh_deform_conv3x3_act call (arguments already checked)."""
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    sn, _, sy, sx = x.stride()
    y = _nhwc_empty((n, cout, h, w), x.device)
    call('frh_deform_conv3x3_act', ptr(x), ptr(offset), ptr(ow), ptr(weight), ptr(y), ptr(_dc_ws(cin, cout, x.device)),
         n, cin, cout, int(dg), h, w, sn, sy, sx, i64_array(offset.stride()), int(bool(relu)), stream_of(x))
    return y


def _dc_act_levels(xs, offsets, weight, dg, relu, ow):
    """One frh_deform_conv3x3_act_levels call (arguments already checked)."""
    n, dev = xs[0].shape[0], xs[0].device
    cout, cin = weight.shape[:2]
    ys = [_nhwc_empty((n, cout, x.shape[2], x.shape[3]), dev) for x in xs]
    call('frh_deform_conv3x3_act_levels', len(xs), ptr_array(xs), ptr_array(offsets), ptr(ow), ptr(weight),
         ptr_array(ys), ptr(_dc_ws(cin, cout, dev)), n, cin, cout, int(dg), *_level_geometry(xs),
         i64_array([v for o in offsets for v in o.stride()]), int(bool(relu)), stream_of(xs[0]))
    return ys


# Level shapes (cin, cout, n, h, w) on which a single-level hip_grad=True call still takes the
# restatement: those where forward + backward on the HIP entries measured slower than the
# restatement's (tools/bench_deform_conv_bwd.py, profiles/ga_rpn_bwd/bench_deform_conv_bwd.json;
# us per forward + backward, median [min, max], HIP against restatement).  A lone small level pays
# the latency floor of the forward (K is not split) and of the data launch by itself.  A pyramid
# call is measured as one unit (17 651 [17 610, 17 697] against 49 787 [49 739, 49 900]) and is
# not subject to this table.
_DEFORM_BWD_EXCLUDED = {
    (256, 256, 2, 19, 32),  # 1622.6 [1619.6, 1622.8] against 1088.5 [1086.8, 1091.5]
    (256, 256, 2, 10, 16),  # 1543.7 [1543.5, 1544.9] against  656.6 [ 655.0,  657.6]
}
_DC_BWD_MAX_COUT = 256  # frh_deform_conv3x3_bwd: FRH_EUNSUPPORTED above


def _dc_hip_grad_ok(xs, offsets, weight, dg, ow):
    """Whether hip_grad=True runs these levels on the HIP forward with frh_deform_conv3x3_bwd as
    its backward: something needs a gradient, the entries accept every level, and the backward
    need not be deterministic (gx is summed with float atomics; the restatement is the
    deterministic form)."""
    if deterministic_backward() or not (1 <= len(xs) <= 8):
        return False
    if not all(_dc_shapes_ok(x, o, weight, dg, ow) for x, o in zip(xs, offsets)):
        return False
    cout, cin = weight.shape[:2]
    if cout > _DC_BWD_MAX_COUT or len({(x.shape[0], x.device) for x in xs}) != 1:
        return False
    if len(xs) == 1 and (cin, cout, xs[0].shape[0], xs[0].shape[2], xs[0].shape[3]) in _DEFORM_BWD_EXCLUDED:
        return False
    return _needs_grad(weight, ow, *xs, *offsets)


class _DeformConv3x3(torch.autograd.Function):
    """act(DeformConv) of one or more levels sharing a weight: the HIP forward (one
    frh_deform_conv3x3_act / _act_levels call) with frh_deform_conv3x3_bwd, one call per level,
    as its backward.  Inputs: dg, relu, weight, ow ([18 dg, 2] or None), the levels' x, then
    their offset (ow None) or shape maps."""

    @staticmethod
    def forward(ctx, dg, relu, weight, ow, *maps):
        L = len(maps) // 2
        xs, offs = list(maps[:L]), list(maps[L:])
        if L == 1:
            ys = [_dc_act(xs[0], offs[0], weight, dg, relu, ow)]
        else:
            ys = _dc_act_levels(xs, offs, weight, dg, relu, ow)
        ctx.dg, ctx.relu, ctx.levels, ctx.guided = int(dg), bool(relu), L, ow is not None
        ctx.save_for_backward(weight, ow, *xs, *offs, *(ys if relu else []))
        return tuple(ys)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gys):
        L, dg, guided = ctx.levels, ctx.dg, ctx.guided
        weight, ow = ctx.saved_tensors[:2]
        xs, offs = ctx.saved_tensors[2:2 + L], ctx.saved_tensors[2 + L:2 + 2 * L]
        ys = ctx.saved_tensors[2 + 2 * L:] if ctx.relu else [None] * L
        need = ctx.needs_input_grad
        cout, cin = weight.shape[:2]
        g_w = g_ow = None
        g_xs, g_offs = [None] * L, [None] * L
        for i in range(L):  # the levels' gw are added in level order
            if gys[i] is None:
                continue
            x, off = xs[i], offs[i]
            n, _, h, w = x.shape
            dev = x.device
            want_off = need[4 + L + i] or (guided and need[3])
            gy = gys[i].float().contiguous(memory_format=torch.channels_last)
            gx = torch.zeros(n, h, w, cin, dtype=torch.float32, device=dev).permute(0, 3, 1, 2) if need[4 + i] else None
            goff = torch.empty(n, 18 * dg, h, w, dtype=torch.float32, device=dev) if want_off else None
            gw = torch.empty_like(weight) if need[2] else None
            ws = workspace(_lib.query('frh_deform_conv3x3_bwd_workspace', n, cin, cout, h, w), dev)
            sn, _, sy, sx = x.stride()
            call('frh_deform_conv3x3_bwd', ptr(x), ptr(off), ptr(ow), ptr(weight), ptr(ys[i]), ptr(gy), ptr(gx),
                 ptr(goff), ptr(gw), ptr(ws), n, cin, cout, dg, h, w, sn, sy, sx, i64_array(off.stride()), stream_of(x))
            g_xs[i] = gx
            if gw is not None:
                g_w = gw if g_w is None else g_w + gw
            if goff is None:
                continue
            if not guided:
                g_offs[i] = goff
                continue
            if need[3]:  # the offset layer is a 1x1 conv without bias: two contractions of goff
                t = torch.einsum('nchw,njhw->cj', goff, off)
                g_ow = t if g_ow is None else g_ow + t
            if need[4 + L + i]:
                g_offs[i] = torch.einsum('cj,nchw->njhw', ow, goff)
        return (None, None, g_w, g_ow, *g_xs, *g_offs)


def deform_conv3x3(x, offset, weight, dg, relu=False, offset_weight=None, hip_grad=False):
    """act(DeformConv(x, offset)) for a 3x3 / stride-1 / padding-1 deformable convolution without
    bias: the HIP entry (frh_deform_conv3x3_act; the result is channels-last) when the tensors
    are f32 on the HIP device, meet its shape conditions and nothing needs a gradient;
    otherwise deform_conv3x3_torch, which autograd differentiates (training).  With
    offset_weight [18 dg, 2(, 1, 1)] (guided mode) `offset` is the 2-channel shape map and the
    offsets are the bias-free 1x1 convolution of it, formed inside the kernel.
    hip_grad=True: where a gradient is needed and the entries accept the tensors, the forward is
    the HIP entry all the same and its backward frh_deform_conv3x3_bwd (gx by float atomics; no
    double backward).  CPU tensors, refused shapes, shapes in _DEFORM_BWD_EXCLUDED and a
    deterministic backward (deterministic_backward()) keep the restatement."""
    ow = None if offset_weight is None else offset_weight.reshape(18 * dg, 2)
    if x.is_cuda and x.dim() == 4:
        x = _as_channels_last(x)
    if hip_grad and _dc_hip_grad_ok([x], [offset], weight, dg, ow):
        return _DeformConv3x3.apply(dg, relu, weight, ow, x, offset)[0]
    if not deform_conv3x3_fused_ok(x, offset, weight, dg, ow):
        if ow is not None:
            offset = nn.functional.conv2d(offset, ow.view(18 * dg, 2, 1, 1))
        return deform_conv3x3_torch(x, offset, weight, dg, relu)
    return _dc_act(x, offset, weight, dg, relu, ow)


def deform_conv3x3_levels(xs, offsets, weight, dg, relu=False, offset_weight=None, hip_grad=False):
    """deform_conv3x3 with one shared weight on every level of a pyramid (at most 8): one repack
    launch and one convolution launch (frh_deform_conv3x3_act_levels) when every level can take
    the HIP entry; the per-level calls otherwise.  Same bits as the per-level calls.
    hip_grad=True, where every level qualifies (deform_conv3x3): that one forward call, and one
    frh_deform_conv3x3_bwd call per level as its backward."""
    xs, offsets = list(xs), list(offsets)
    if len(xs) != len(offsets):
        raise AssertionError('deform_conv3x3_levels: one offset (or shape) map per level')
    ow = None if offset_weight is None else offset_weight.reshape(18 * dg, 2)
    xs = [_as_channels_last(x) if x.is_cuda and x.dim() == 4 else x for x in xs]
    if hip_grad and _dc_hip_grad_ok(xs, offsets, weight, dg, ow):
        return list(_DeformConv3x3.apply(dg, relu, weight, ow, *xs, *offsets))
    if not (1 <= len(xs) <= 8 and all(deform_conv3x3_fused_ok(x, o, weight, dg, ow) for x, o in zip(xs, offsets))
            and len({(x.shape[0], x.device) for x in xs}) == 1):
        return [deform_conv3x3(x, o, weight, dg, relu, offset_weight, hip_grad) for x, o in zip(xs, offsets)]
    return _dc_act_levels(xs, offsets, weight, dg, relu, ow)


def ga_targets(grid_sizes, strides, gt_list, level_list, img_shapes, center_ratio, ignore_ratio, shape_center_ratio):
    """Batched GuidedAnchor.loc_target and the painting of shape_target_single_image_v2
    (guided_head.py:342-397, :195-231) in one launch (csrc/ga.hip).  grid_sizes / strides: per
    level; gt_list: per image [4, G_i] on the HIP device, coordinates >= 0; level_list: per image
    [G_i] integer levels (region.map_gt2level); img_shapes: per image (h, w).  Returns loc i64
    [B, N] (1 / 0 / -1), shape_mask i64 [B, N] and shape_box f32 [B, N, 4] over the
    level-concatenated cells."""
    _need_cuda(*gt_list)
    if not gt_list:
        raise AssertionError('ga_targets: at least one image expected')
    dev = gt_list[0].device
    B, L = len(gt_list), len(grid_sizes)
    if len(strides) != L or len(level_list) != B or len(img_shapes) != B:
        raise AssertionError('ga_targets: a stride per level, a level list and a shape per image')
    N = sum(int(h) * int(w) for h, w in grid_sizes)
    gts, gcnt, gmax = pack_boxes([g.float() for g in gt_list], dev)
    lvls = torch.zeros(B, max(gmax, 1), dtype=torch.int32, device=dev)
    for b, lv in enumerate(level_list):
        if lv.numel() != gt_list[b].shape[1]:
            raise AssertionError('ga_targets: one level per gt')
        if lv.numel():
            lvls[b, :lv.numel()] = lv.to(torch.int32)
    img_hw = device_ints([int(v) for s in img_shapes for v in s[:2]], dev)
    loc = torch.empty(B, N, dtype=torch.int64, device=dev)
    mask = torch.empty(B, N, dtype=torch.int64, device=dev)
    box = torch.empty(B, N, 4, dtype=torch.float32, device=dev)
    hw = i32_array([int(v) for g in grid_sizes for v in g])
    call('frh_ga_targets', B, L, hw, f32_array(strides), ptr(gts), gts.stride(0), ptr(gcnt), ptr(lvls), gmax,
         ptr(img_hw), float(center_ratio), float(ignore_ratio), float(shape_center_ratio), ptr(loc), ptr(mask),
         ptr(box), stream_of(loc))
    return loc, mask, box


def bn_act_maxpool(x, bn, pool):
    """pool(relu(bn(x))) for the ResNet stem (eval-mode BN, MaxPool2d(3, 2, 1)) in one HIP pass
    (frh_bn_act_maxpool) when nothing needs a gradient through it (the reference freezes the
    stem: frozen_stages >= 0); otherwise bn_act then the pool module."""
    fused = (_f32_hip_4d(x) and _frozen_bn(bn) and x.is_contiguous() and x.shape[3] % 8 == 0 and x.shape[3] >= 8
             and (pool.kernel_size, pool.stride, pool.padding, pool.dilation) in ((3, 2, 1, 1), ((3, 3), (2, 2), (1, 1), (1, 1)))
             and not pool.ceil_mode and not pool.return_indices and not _needs_grad(x, bn.weight, bn.bias))
    if not fused:
        return pool(bn_act(x, bn))
    n, c, h, w = x.shape
    y = torch.empty(n, c, (h - 1) // 2 + 1, w // 2, dtype=torch.float32, device=x.device)
    call('frh_bn_act_maxpool', ptr(x), ptr(y), *_bn_args(bn), n, c, h, w, stream_of(x))
    return y


# ---------------------------------------------------------------- f1: fused losses
CLS_FOCAL, CLS_SIGMOID_BCE, CLS_SOFTMAX_CE = 0, 1, 2
_LOSS_WS = {}


def _loss_workspace(x):
    """Zero-filled once per (device, stream): each forward call leaves its arrival counter zero."""
    key = (x.device, torch.cuda.current_stream(x.device).cuda_stream)
    ws = _LOSS_WS.get(key)
    if ws is None:
        ws = _LOSS_WS[key] = torch.zeros(int(_lib.query('frh_loss_workspace')), dtype=torch.uint8, device=x.device)
    return ws


def _loss_fwd(entry, x, out_shape, *args):
    """The tail every fused forward shares: `entry`(*args, status word, out, workspace, its size,
    stream) on x's device and current stream; returns the f32 output of shape `out_shape`."""
    out = torch.empty(out_shape, dtype=torch.float32, device=x.device)
    ws = _loss_workspace(x)
    call(entry, *args, ptr(status_word(x.device)), ptr(out), ptr(ws), ws.numel(), stream_of(x))
    return out


def _cls_call_args(x, target, kind, alpha, gamma):
    n, c = x.shape
    return (kind, ptr(x), n, c, x.stride(0), x.stride(1), ptr(target), int(target.dtype == torch.float32),
            float(alpha), float(gamma))


def _cls_bwd(x, target, cfg, g):
    """frh_cls_loss_bwd: the gradient of the summed loss times the device scalar g."""
    gx = torch.empty_like(x)
    g = _f32(g).contiguous()
    call('frh_cls_loss_bwd', *_cls_call_args(x, target, *cfg), ptr(g), ptr(gx), gx.stride(0), gx.stride(1),
         stream_of(x))
    return gx


class _ClsLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target, kind, alpha, gamma):
        ctx.save_for_backward(x, target)
        ctx.cfg = (kind, alpha, gamma)
        return _loss_fwd('frh_cls_loss_fwd', x, (), *_cls_call_args(x, target, *ctx.cfg))

    @staticmethod
    def backward(ctx, g):
        return _cls_bwd(*ctx.saved_tensors, ctx.cfg, g), None, None, None, None


def cls_loss(x, target, kind, alpha=0.25, gamma=2.0):
    """Summed classification loss of logits x [n, C] (any strides) against target [n]
    (frh_cls_loss_fwd/bwd; kinds CLS_FOCAL / CLS_SIGMOID_BCE / CLS_SOFTMAX_CE)."""
    _need_cuda(x, target)
    if x.dim() != 2 or target.dim() != 1 or target.shape[0] != x.shape[0]:
        raise AssertionError('cls_loss: x [n, C] and target [n] expected')
    if target.is_floating_point():
        target = target.float()
        if x.shape[1] != 1 or kind != CLS_SIGMOID_BCE:
            raise AssertionError('cls_loss: float targets only for single-channel sigmoid BCE')
    elif target.dtype != torch.int64:
        target = target.long()
    return _ClsLoss.apply(_f32(x), target.contiguous(), int(kind), alpha, gamma)


def _l1_call_args(x, y, label, xs, ys, n, m, n_sel, params):
    """The leading arguments of <stem>_fwd / _bwd; params are the element's floats, beta first."""
    return (ptr(x), xs[0], xs[1], xs[2], ptr(y), ys[0], ys[1], ptr(label), n, m, n_sel,
            *(float(p) for p in params))


def _l1_bwd(stem, what, x, y, label, cfg, g):
    """<stem>_bwd into a zero-filled gradient of x's layout: only the selected, unmasked elements
    are written."""
    gx = torch.zeros_like(x)
    if gx.stride() != x.stride():
        raise AssertionError('{}: gradient layout differs from the input'.format(what))
    g = _f32(g).contiguous()
    xs = cfg[0]
    call(stem + '_bwd', *_l1_call_args(x, y, label, *cfg), ptr(g), ptr(gx), xs[0], xs[1], xs[2], stream_of(x))
    return gx


class _L1Loss(torch.autograd.Function):
    """The masked / class-selected regression sum of entry stem `stem` ('frh_smooth_l1' or
    'frh_balanced_l1') with the element parameters `params` ((beta,) or (beta, alpha, gamma))."""

    @staticmethod
    def forward(ctx, x, y, label, xs, ys, n, m, n_sel, stem, params):
        ctx.save_for_backward(x, y, label)
        ctx.stem, ctx.cfg = stem, (xs, ys, n, m, n_sel, params)
        return _loss_fwd(stem + '_fwd', x, (), *_l1_call_args(x, y, label, *ctx.cfg))

    @staticmethod
    def backward(ctx, g):
        return (_l1_bwd(ctx.stem, ctx.stem[len('frh_'):], *ctx.saved_tensors, ctx.cfg, g),) + (None,) * 9


def _l1_args(x, y, label, rows_dim):
    """(x, y, label, x strides, y strides, n, m, n_sel) of a masked smooth-L1 sum."""
    _need_cuda(x, y, label)
    if x.shape != y.shape or x.dim() != 2:
        raise AssertionError('smooth_l1_loss: x and y must be equal 2-D shapes')
    x, y = _f32(x), _f32(y)
    if not (x.is_contiguous() or x.t().is_contiguous()):
        x = x.contiguous()  # the zero-filled gradient must share x's strides
    cd = 1 - rows_dim
    n, m = x.shape[rows_dim], x.shape[cd]
    if label is not None and label.numel() != n:
        raise AssertionError('smooth_l1_loss: one label per row expected')
    lab = label.contiguous().long() if label is not None else None
    return x, y, lab, (x.stride(rows_dim), x.stride(cd), 0), (y.stride(rows_dim), y.stride(cd)), n, m, 1


def smooth_l1_loss(x, y, beta, label=None, rows_dim=0):
    """Summed smooth_l1_loss_v2 of x and y (same shape, 2-D, rows along `rows_dim`),
    counting only rows whose label is > 0 when `label` is given (frh_smooth_l1_fwd/bwd)."""
    return _L1Loss.apply(*_l1_args(x, y, label, rows_dim), 'frh_smooth_l1', (beta,))


def _l1_class_select_args(reg_out, num_classes, target, label):
    _need_cuda(reg_out, target, label)
    n = reg_out.shape[0]
    if reg_out.dim() != 2 or reg_out.shape[1] != 4 * num_classes or target.shape != (n, 4) or label.numel() != n:
        raise AssertionError('smooth_l1_class_select: shape mismatch')
    reg_out, target = _f32(reg_out), _f32(target)
    if reg_out.stride(1) != 1:
        reg_out = reg_out.contiguous()
    xs = (reg_out.stride(0), num_classes, 1)
    return reg_out, target, label.contiguous().long(), xs, (target.stride(0), target.stride(1)), n, 4, num_classes


def smooth_l1_class_select(reg_out, num_classes, target, label, beta):
    """BBoxHead's regression loss: reg_out [n, 4*C] viewed [n, 4, C], the labelled class's
    deltas of the positive rows against target [n, 4] (any strides), summed."""
    return _L1Loss.apply(*_l1_class_select_args(reg_out, num_classes, target, label), 'frh_smooth_l1', (beta,))


def balanced_l1_loss(x, y, beta, alpha, gamma, label=None, rows_dim=0):
    """Summed balanced_l1_loss (lib/losses.py:158-168) of x and y, as smooth_l1_loss."""
    return _L1Loss.apply(*_l1_args(x, y, label, rows_dim), 'frh_balanced_l1', (beta, alpha, gamma))


def balanced_l1_class_select(reg_out, num_classes, target, label, beta, alpha, gamma):
    """smooth_l1_class_select with the balanced-L1 element."""
    return _L1Loss.apply(*_l1_class_select_args(reg_out, num_classes, target, label), 'frh_balanced_l1',
                         (beta, alpha, gamma))


class _DetLoss(torch.autograd.Function):
    """A head's classification and regression losses in one launch (frh_det_loss_fwd),
    each scaled as the heads scale it: (sum * weight) / avg_factor."""

    @staticmethod
    def forward(ctx, x, target, kind, alpha, gamma, wc, rx, ry, rlabel, xs, ys, rn, rm, n_sel, beta, wr, div):
        dcount = div if isinstance(div, torch.Tensor) else None  # device int32 count (sync-free targets)
        hdiv = 1.0 if dcount is not None else float(div)
        cls_cfg, l1_cfg = (kind, alpha, gamma), (xs, ys, rn, rm, n_sel, (beta,))
        out = _loss_fwd('frh_det_loss_fwd', x, 2, *_cls_call_args(x, target, *cls_cfg), float(wc), hdiv,
                        *_l1_call_args(rx, ry, rlabel, *l1_cfg), float(wr), hdiv, ptr(dcount))
        if dcount is not None:
            # backward divides by the count as f32 (count 0: every row is padding, gradients 0)
            div = dcount.float()
        ctx.save_for_backward(x, target, rx, ry, rlabel)
        ctx.cfg = (cls_cfg, wc, l1_cfg, wr, div)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, gc, gr):
        x, target, rx, ry, rlabel = ctx.saved_tensors
        cls_cfg, wc, l1_cfg, wr, div = ctx.cfg
        gx = grx = None
        if gc is not None and ctx.needs_input_grad[0]:
            gx = _cls_bwd(x, target, cls_cfg, (gc / div) * wc)  # the reference's Div then Mul backward
        if gr is not None and ctx.needs_input_grad[6]:
            grx = _l1_bwd('frh_smooth_l1', 'det loss', rx, ry, rlabel, l1_cfg, (gr / div) * wr)
        return (gx,) + (None,) * 5 + (grx,) + (None,) * 10


def det_losses(x, target, kind, alpha, gamma, cls_weight, l1_args, beta, reg_weight, avg_factor):
    """(cls, reg) = (cls_loss(x, target, kind) * cls_weight / avg_factor,
    smooth-L1(*l1_args) * reg_weight / avg_factor) in one launch; l1_args from _l1_args /
    _l1_class_select_args.  avg_factor is a host number (the sampled count) or a device
    int32 [1] count (sync-free targets: rows labelled < 0 are padding and ignored, a count
    of 0 gives zero losses)."""
    _need_cuda(x, target)
    if target.dtype != torch.int64:
        target = target.long()
    rx, ry, rlabel, xs, ys, rn, rm, n_sel = l1_args
    if isinstance(avg_factor, torch.Tensor):
        if avg_factor.dtype != torch.int32 or avg_factor.numel() != 1 or not avg_factor.is_cuda:
            raise AssertionError('a device avg_factor is an int32 [1] count')
    else:
        avg_factor = float(avg_factor)
    return _DetLoss.apply(_f32(x), target.contiguous(), int(kind), alpha, gamma, cls_weight, rx, ry, rlabel, xs, ys,
                          rn, rm, n_sel, beta, reg_weight, avg_factor)


# ---------------------------------------------------------------- f1b: GFL head losses, DFL decode
class _HeadLoss(torch.autograd.Function):
    """Three losses and the positive count of a one-stage head in one launch (<stem>_fwd), one
    launch backward (<stem>_bwd); the positive count and the upstream gradients stay on the device.
    `pack(*ts, cfg)` gives the entries' leading arguments; the first n_out tensors of ts are the
    head's outputs, which get the gradients."""

    @staticmethod
    def forward(ctx, stem, pack, n_out, cfg, *ts):
        out = _loss_fwd(stem + '_fwd', ts[0], 4, *pack(*ts, cfg))
        ctx.save_for_backward(*ts, out)
        ctx.cfg = (stem, pack, n_out, cfg)
        num_pos = out[3].long()
        ctx.mark_non_differentiable(num_pos)
        return out[0], out[1], out[2], num_pos

    @staticmethod
    def backward(ctx, g0, g1, g2, _):
        *ts, out = ctx.saved_tensors
        stem, pack, n_out, cfg = ctx.cfg
        g = _f32(torch.stack([g0, g1, g2])).contiguous()
        grads = [torch.empty_like(t) for t in ts[:n_out]]
        gargs = [a for t in grads for a in (ptr(t),) + t.stride()]
        call(stem + '_bwd', *pack(*ts, cfg), ptr(g), ptr(out), *gargs, stream_of(ts[0]))
        return (None,) * 4 + tuple(grads) + (None,) * (len(ts) - n_out)


def _gfl_args(cls, reg, labels, ltrb, cfg):
    bins, stride, reg_mean, reg_std, norm_prob, beta, wc, wd, wb, avg = cfg
    return (ptr(cls), cls.shape[0], cls.stride(0), cls.stride(1), ptr(reg), bins, reg.stride(0), reg.stride(1),
            ptr(labels), ptr(ltrb), cls.shape[1], reg_mean, reg_std, stride, norm_prob, beta, wc, wd, wb, avg)


def gfl_losses(cls_outs, reg_outs, labels, ltrb, bins, stride, reg_mean=0.0, reg_std=1.0, norm_prob=False, beta=2.0,
               cls_weight=1.0, dfl_weight=1.0, bbox_weight=1.0, dfl_avg_factor=4.0):
    """(cls_loss, dfl_loss, bbox_loss, num_pos) of the GFL head (csrc/gfl.hip; the arguments and
    semantics of losses.gfl_head_losses_torch): cls_outs [C, M] and reg_outs [4*bins, M] f32 logits
    in any strides, labels [M] int64, ltrb [M, 4].  The losses are 0-d tensors, num_pos a 0-d
    int64 device tensor; nothing is read back to the host.  4*bins > 64 raises."""
    _need_cuda(cls_outs, reg_outs, labels, ltrb)
    if cls_outs.dim() != 2 or reg_outs.dim() != 2 or reg_outs.shape[0] != 4 * bins:
        raise AssertionError('gfl_losses: cls_outs [C, M] and reg_outs [4*bins, M] expected')
    m = cls_outs.shape[1]
    if reg_outs.shape[1] != m or labels.shape != (m,) or ltrb.shape != (m, 4):
        raise AssertionError('gfl_losses: labels [M] and ltrb [M, 4] must match the logits')
    if labels.dtype != torch.int64:
        labels = labels.long()
    cfg = (int(bins), float(stride), float(reg_mean), float(reg_std), int(bool(norm_prob)), float(beta),
           float(cls_weight), float(dfl_weight), float(bbox_weight), float(dfl_avg_factor))
    return _HeadLoss.apply('frh_gfl_loss', _gfl_args, 2, cfg, _f32(cls_outs), _f32(reg_outs), labels.contiguous(),
                           _f32(ltrb).contiguous())


# ---------------------------------------------------------------- f1c: FCOS head losses (no GFL)
def _fcos_args(cls, reg, ctr, labels, ltrb, ctr_t, cfg):
    reg_mean, reg_std, alpha, gamma, wc, wb, wt = cfg
    return (ptr(cls), cls.shape[0], cls.stride(0), cls.stride(1), ptr(reg), reg.stride(0), reg.stride(1), ptr(ctr),
            ctr.stride(0), ptr(labels), ptr(ltrb), ptr(ctr_t), cls.shape[1], reg_mean, reg_std, alpha, gamma, wc, wb,
            wt)


def fcos_losses(cls_outs, reg_outs, ctr_outs, labels, ltrb, ctr_tars, reg_mean=0.0, reg_std=1.0, alpha=0.25,
                gamma=2.0, cls_weight=1.0, bbox_weight=1.0, ctr_weight=1.0):
    """(cls_loss, bbox_loss, ctr_loss, num_pos) of the FCOS head without GFL (csrc/fcos.hip; the
    arguments and semantics of losses.fcos_head_losses_torch): cls_outs [C, M] logits, reg_outs
    [4, M] ltrb predictions (the head's exp output) and ctr_outs [M] (or [1, M]) logits, f32 in any
    strides; labels [M] int64, ltrb [M, 4], ctr_tars [M].  The losses are 0-d tensors, num_pos a
    0-d int64 device tensor; nothing is read back to the host."""
    _need_cuda(cls_outs, reg_outs, ctr_outs, labels, ltrb, ctr_tars)
    if cls_outs.dim() != 2 or reg_outs.dim() != 2 or reg_outs.shape[0] != 4:
        raise AssertionError('fcos_losses: cls_outs [C, M] and reg_outs [4, M] expected')
    m = cls_outs.shape[1]
    if ctr_outs.dim() == 2 and ctr_outs.shape[0] == 1:
        ctr_outs = ctr_outs[0]
    if reg_outs.shape[1] != m or ctr_outs.shape != (m,):
        raise AssertionError('fcos_losses: reg_outs [4, M] and ctr_outs [M] must match cls_outs')
    if labels.shape != (m,) or ltrb.shape != (m, 4) or ctr_tars.shape != (m,):
        raise AssertionError('fcos_losses: labels [M], ltrb [M, 4] and ctr_tars [M] must match the outputs')
    if labels.dtype != torch.int64:
        labels = labels.long()
    cfg = (float(reg_mean), float(reg_std), float(alpha), float(gamma), float(cls_weight), float(bbox_weight),
           float(ctr_weight))
    return _HeadLoss.apply('frh_fcos_loss', _fcos_args, 3, cfg, _f32(cls_outs), _f32(reg_outs), _f32(ctr_outs),
                           labels.contiguous(), _f32(ltrb).contiguous(), _f32(ctr_tars).contiguous())


def dfl_decode(reg, bins, stride, reg_std, reg_mean, cell, img_size):
    """Boxes [B, 4, H*W] of one level's DFL regression logits reg [B, 4*bins, H, W] (any strides):
    softmax expectation per side, * reg_std + reg_mean, the box around the cell centre (cell =
    the level's stride), clamped to img_size (h, w) (frh_dfl_decode; fcos_head.py:579-600)."""
    _need_cuda(reg)
    if reg.dim() != 4 or reg.shape[1] != 4 * bins:
        raise AssertionError('dfl_decode: reg [B, 4*bins, H, W] expected')
    reg = _f32(reg)
    B, _, h, w = reg.shape
    out = torch.empty(B, 4, h * w, dtype=torch.float32, device=reg.device)
    call('frh_dfl_decode', ptr(reg), B, int(bins), h, w, reg.stride(0), reg.stride(1), reg.stride(2), reg.stride(3),
         float(stride), float(reg_std), float(reg_mean), float(cell), float(img_size[0]), float(img_size[1]), ptr(out),
         stream_of(reg))
    return out


# ---------------------------------------------------------------- dense-head candidates
DENSE_MODES = {'DELTA': 0, 'LTRB': 1, 'DFL': 2}
DENSE_MAX_ROWS = 16384  # rows of one level the gather launch orders in LDS


def dense_candidates_rows(grid_sizes, num_anchors, pre_nms):
    """k_l = min(pre_nms, n_l) (n_l when pre_nms <= 0) of every level."""
    ns = [num_anchors * int(h) * int(w) for h, w in grid_sizes]
    return [min(int(pre_nms), n) if pre_nms > 0 else n for n in ns]


def dense_candidates(cls_outs, reg_outs, ctr_outs, mode, img_hw, min_sizes, pre_nms, num_anchors=1, anchors=None,
                     means=None, stds=None, strides=None, bins=0, dfl_stride=1.0, reg_std=1.0, reg_mean=0.0):
    """The one-stage heads' NMS input for all images x levels (frh_dense_candidates;
    fcos_head.py:570-621, anchor_head.py:207-250): one memset and four launches, no host sync.

    cls_outs / reg_outs / ctr_outs (or None): per-level [B, C*A, H, W] / [B, 4*A | 4*bins, H, W] /
    [B, 1, H, W] f32 maps of any layout.  mode 'DELTA' (anchors [4, N], means, stds), 'LTRB' or
    'DFL' (strides per level, reg_std, reg_mean; bins, dfl_stride).  img_hw [(h, w)] and
    min_sizes per image.  Returns (boxes [B, cap, 4], scores [B, cap, C], factor [B, cap] or
    None, valid bool [B, cap], index int32 [B, cap]) with cap = sum of the levels' k_l, rows in
    (key descending, column ascending) order per level, invalid rows zero with index -1."""
    ctrs = list(ctr_outs) if ctr_outs is not None else None
    _need_cuda(*cls_outs)
    _need_cuda(*reg_outs)
    if ctrs is not None:
        _need_cuda(*ctrs)
    if mode not in DENSE_MODES:
        raise AssertionError('unknown mode {}'.format(mode))
    for t in list(cls_outs) + list(reg_outs) + (ctrs or []):
        if t.dtype != torch.float32 or t.dim() != 4:
            raise AssertionError('dense_candidates: f32 [B, C, H, W] maps expected')
    B, L = cls_outs[0].shape[0], len(cls_outs)
    A = int(num_anchors)
    C = cls_outs[0].shape[1] // A
    dev = cls_outs[0].device
    grids = [(c.shape[2], c.shape[3]) for c in cls_outs]
    grid_a = i32_array([v for g in grids for v in g])
    cap = sum(dense_candidates_rows(grids, A, pre_nms))
    boxes = torch.empty(B, cap, 4, dtype=torch.float32, device=dev)
    scores = torch.empty(B, cap, C, dtype=torch.float32, device=dev)
    factor = torch.empty(B, cap, dtype=torch.float32, device=dev) if ctrs is not None else None
    valid = torch.empty(B, cap, dtype=torch.uint8, device=dev)
    index = torch.empty(B, cap, dtype=torch.int32, device=dev)
    ws = workspace(_lib.query('frh_dense_candidates_workspace', B, L, grid_a, A, int(pre_nms)), dev)
    strides_of = lambda ts: i64_array([v for t in ts for v in t.stride()])
    call('frh_dense_candidates', B, L, ptr_array(cls_outs), ptr_array(reg_outs),
         ptr_array(ctrs) if ctrs is not None else None, strides_of(cls_outs), strides_of(reg_outs),
         strides_of(ctrs) if ctrs is not None else None, grid_a, A, C, DENSE_MODES[mode],
         ptr(anchors), anchors.stride(0) if anchors is not None else 0,
         f32_array(means) if means is not None else None, f32_array(stds) if stds is not None else None,
         f32_array(strides) if strides is not None else None, int(bins), float(dfl_stride), float(reg_std),
         float(reg_mean), f32_array([v for hw in img_hw for v in hw[:2]]), f32_array(min_sizes), int(pre_nms),
         ptr(boxes), ptr(scores), ptr(factor), ptr(valid), ptr(index), cap, ptr(ws), ws.numel(), stream_of(boxes))
    return boxes, scores, factor, valid.view(torch.bool), index
