"""IoU-balanced negative sampler on the HIP path (csrc/sample.hip: frh_sample_iou_balanced,
frh_sample_iou_candidates; ops.sample_iou_balanced; region.IoUBalancedNegSampler).

numpy mode: the sampled labels equal the reference's (tests/golden/libra_sampler.npz, the
reference's IoUBalancedNegSampler on the CPU after np.random.seed) and the legacy RNG ends
in the same state.  device mode: the per-class counts equal the reference rule's quotas
(restated below from lib/region.py:145-161), every kept row belongs to the class it was
kept for, no duplicates, both output forms agree, the seed decides the set.  Then the
sampler feeding bbox_targets_batched against the reference's bbox_target
(tests/golden/libra_targets.npz)."""
import numpy as np
import pytest
import torch

import inputs
import libra_inputs
from frcnn_amd import _lib, ops, set_sampler_mode
from frcnn_amd.region import IoUBalancedNegSampler, MaxIoUAssigner

pytestmark = pytest.mark.gpu


def _pack(c, dev):
    S = len(c['labels'])
    n = max(len(l) for l in c['labels'])
    lab = torch.full((S, n), -1, dtype=torch.int64)
    iou = torch.zeros(S, n)
    for s in range(S):
        k = len(c['labels'][s])
        lab[s, :k] = torch.from_numpy(c['labels'][s])
        iou[s, :k] = torch.from_numpy(c['ious'][s])
    num = torch.tensor([len(l) for l in c['labels']], dtype=torch.int32)
    return lab.to(dev), iou.to(dev), num.to(dev), n


def _sampler(c):
    return IoUBalancedNegSampler(c['max_num'], c['pos_num'], num_bins=c['num_bins'], max_iou=c['max_iou'],
                                 floor_thr=-1, floor_fraction=0)


@pytest.mark.parametrize('tag', libra_inputs.SAMPLER_FIXTURE_CASES)
def test_numpy_mode_equals_the_reference(dev, tag):
    z = np.load(inputs.golden_path('libra_sampler.npz'))
    c = libra_inputs.sampler_case(tag)
    lab, iou, num, n = _pack(c, dev)
    set_sampler_mode('numpy')
    np.random.seed(c['np_seed'])
    out = _sampler(c).sample(lab, iou, num, n).cpu().numpy()
    st = np.random.get_state()
    for s in range(len(c['labels'])):
        # (rows past an image's count are not written, as by the random sampler)
        np.testing.assert_array_equal(out[s, :len(c['labels'][s])], z['{}_labels_{}'.format(tag, s)])
    np.testing.assert_array_equal(np.asarray(st[1], np.uint32), z['{}_rng_keys'.format(tag)])
    assert int(st[2]) == int(z['{}_rng_pos'.format(tag)])


def test_numpy_mode_single_image_call(dev):
    """The reference signature (labels, overlaps, props_bbox, gt_bbox)."""
    z = np.load(inputs.golden_path('libra_sampler.npz'))
    c = libra_inputs.sampler_case('more_pos')
    set_sampler_mode('numpy')
    np.random.seed(c['np_seed'])
    out = _sampler(c)(torch.from_numpy(c['labels'][0]).to(dev), torch.from_numpy(c['ious'][0]).to(dev), None, None)
    np.testing.assert_array_equal(out.cpu().numpy(), z['more_pos_labels_0'])


def _quotas(lab, iou, c):
    """lib/region.py:145-161 restated: (kept positives, [(bin mask, kept)] from the highest bin down)."""
    starts, ends = libra_inputs.bin_edges(c['num_bins'], c['max_iou'])
    kp = min(int((lab > 0).sum()), c['pos_num'])
    num_neg = c['max_num'] - kp
    per_bin = int(num_neg / c['num_bins'])
    chosen, res = 0, []
    for i, (s, e) in enumerate(zip(starts[::-1], ends[::-1])):
        m = (lab == 0) & (iou >= np.float32(s)) & (iou < np.float32(e))
        allowed = per_bin if i < c['num_bins'] - 1 else num_neg - chosen
        k = min(int(m.sum()), allowed)
        chosen += k
        res.append((m, k))
    return kp, res


@pytest.mark.parametrize('tag', sorted(libra_inputs.SAMPLER_CASES))
def test_device_mode_quotas_classes_and_forms(dev, tag):
    c = libra_inputs.sampler_case(tag)
    lab, iou, num, n = _pack(c, dev)
    s = _sampler(c)
    set_sampler_mode('device', seed=123)
    try:
        out = s.sample(lab, iou, num, n).cpu().numpy()
        set_sampler_mode('device', seed=123)
        sl = s.sample(lab, iou, num, n, lists=True)
        set_sampler_mode('device', seed=123)
        again = s.sample(lab, iou, num, n).cpu().numpy()
        set_sampler_mode('device', seed=124)
        other = s.sample(lab, iou, num, n).cpu().numpy()
    finally:
        set_sampler_mode('numpy')
    assert isinstance(sl, ops.SampleLists)
    sel, cnt = sl.sel.cpu().numpy(), sl.sel_counts.cpu().numpy()
    differs = False
    for i in range(len(c['labels'])):
        l0, u0 = c['labels'][i], c['ious'][i]
        k = len(l0)
        o = out[i, :k]  # rows past the image's count are not written
        np.testing.assert_array_equal(again[i, :k], o)  # the same seed: the same set
        kept = o >= 0
        np.testing.assert_array_equal(o[kept], l0[kept])  # kept rows carry their label
        kp, bins = _quotas(l0, u0, c)
        assert int((kept & (l0 > 0)).sum()) == kp
        for m, q in bins:
            assert int((kept & m).sum()) == q
        in_bins = np.zeros(k, bool)
        for m, _ in bins:
            in_bins |= m
        assert not (kept & ~((l0 > 0) | in_bins)).any()  # ignored rows and negatives beyond max_iou never
        # the list form: same sets, no duplicates, positives and negatives in their own lists
        pos, neg = sel[i, 0, :cnt[i, 0]], sel[i, 1, :cnt[i, 1]]
        assert len(set(pos.tolist())) == len(pos) and len(set(neg.tolist())) == len(neg)
        np.testing.assert_array_equal(np.sort(pos), np.nonzero(kept & (l0 > 0))[0])
        np.testing.assert_array_equal(np.sort(neg), np.nonzero(kept & (l0 == 0))[0])
        # any class cut below its size must change with the seed
        cut = kp < int((l0 > 0).sum()) or any(q < int(m.sum()) for m, q in bins)
        if cut and not np.array_equal(other[i, :k], o):
            differs = True
        if not cut:
            np.testing.assert_array_equal(other[i, :k], o)
    if tag not in ('all_starved', 'no_neg'):
        assert differs


def test_row_capacity_is_unsupported(dev):
    """Above the one-workgroup capacity (16 384 rows) both entries refuse with FRH_EUNSUPPORTED
    before any launch."""
    n = 16385
    lab = torch.zeros(1, n, dtype=torch.int64, device=dev)
    iou = torch.zeros(1, n, device=dev)
    num = torch.tensor([n], dtype=torch.int32, device=dev)
    out = torch.empty_like(lab)
    lo, hi = _lib.f32_array([0.0]), _lib.f32_array([0.5])
    st = _lib.query('frh_sample_iou_balanced', 1, _lib.ptr(lab), n, _lib.ptr(iou), n, None, _lib.ptr(num), n, 8, 4, 1,
                    lo, hi, 1, _lib.ptr(out), None, None, _lib.stream_of(lab))
    assert st == -2
    lists = torch.empty(1, 2, n, dtype=torch.int32, device=dev)
    counts = torch.empty(1, 2, dtype=torch.int32, device=dev)
    st = _lib.query('frh_sample_iou_candidates', 1, _lib.ptr(lab), n, _lib.ptr(iou), n, None, _lib.ptr(num), n, 1,
                    lo, hi, _lib.ptr(lists), n, _lib.ptr(counts), _lib.stream_of(lab))
    assert st == -2
    with pytest.raises(RuntimeError, match='capacity'):
        ops.sample_iou_balanced(lab, iou, num, n, 8, 4, [0.0], [0.5], mode='device')


def _targets(dev, mode):
    from frcnn_amd.bbox import bbox_targets_batched
    case = libra_inputs.target_case()
    s = libra_inputs.TARGET_SAMPLER
    set_sampler_mode(mode, seed=9) if mode == 'device' else set_sampler_mode(mode)
    try:
        np.random.seed(libra_inputs.TARGET_NP_SEED)
        with torch.no_grad():
            return case, bbox_targets_batched(
                [torch.from_numpy(p).to(dev) for p, _, _ in case], [torch.from_numpy(g).to(dev) for _, g, _ in case],
                [torch.from_numpy(l).to(dev) for _, _, l in case], MaxIoUAssigner(*libra_inputs.TARGET_ASSIGNER),
                IoUBalancedNegSampler(s['max_num'], s['pos_num'], num_bins=s['num_bins'], max_iou=s['max_iou']),
                (0.0,) * 4, libra_inputs.TARGET_STDS)
    finally:
        set_sampler_mode('numpy')


def test_sampler_feeds_bbox_targets_numpy_mode(dev):
    """Two images in one call equal the reference's per-image bbox_target with this sampler;
    tar_param within the existing RCNN-target bar (test_gpu_parity: rtol / atol 1e-5, the
    encode's logf)."""
    z = np.load(inputs.golden_path('libra_targets.npz'))
    case, r = _targets(dev, 'numpy')
    for i in range(len(case)):
        for k in ('tar_props', 'tar_bbox', 'tar_label', 'tar_is_gt'):
            np.testing.assert_array_equal(r[k][i].cpu().numpy(), z['{}_{}'.format(i, k)], err_msg=k)
        np.testing.assert_allclose(r['tar_param'][i].cpu().numpy(), z['{}_tar_param'.format(i)], rtol=1e-5, atol=1e-5)


def test_sampler_feeds_bbox_targets_device_mode(dev):
    """Device mode through the same path (sampler lists into frh_bbox_target): as many rows per
    image as the reference kept (the quotas do not depend on the draw), gts first, labels and
    boxes consistent."""
    z = np.load(inputs.golden_path('libra_targets.npz'))
    case, r = _targets(dev, 'device')
    for i, (props, gb, gl) in enumerate(case):
        ref_lab = z['{}_tar_label'.format(i)]
        lab = r['tar_label'][i].cpu().numpy()
        assert lab.shape == ref_lab.shape
        assert int((lab > 0).sum()) == int((ref_lab > 0).sum())
        tb, tl = r['tar_bbox'][i].cpu().numpy(), lab
        for j in np.nonzero(tl > 0)[0][:50]:
            g = np.nonzero((gb == tb[:, j:j + 1]).all(0))[0]
            assert len(g) and gl[g[0]] == tl[j]
