"""tests/support.py itself, without a GPU: the entry spy sees what goes through ops.call and hides
nothing, the thread pin is set and put back, the container helpers keep their containers, and the
shared comparisons fail on everything the per-file loops they replaced failed on."""
import numpy as np
import pytest
import torch

import support


# ----------------------------------------------------------------- spy_entries
def test_spy_records_names_and_args_in_order_and_returns_the_result(monkeypatch):
    from frcnn_amd import ops
    reached = []

    def fake(name, *args):
        reached.append((name, args))
        if name == 'boom':
            raise RuntimeError('entry failed')
        return ('result of', name)
    monkeypatch.setattr(ops, '_call', fake)
    monkeypatch.setattr(ops, '_drop_zero_workspaces', lambda: None)
    spy = support.spy_entries(monkeypatch)
    assert ops._call('a', 1, 'two') == ('result of', 'a')
    ops.call('x', 1)  # ops.call looks _call up as a module global: it goes through the spy
    assert ops._call('b') == ('result of', 'b')
    assert spy.names == ['a', 'x', 'b']
    assert spy.calls == [('a', (1, 'two')), ('x', (1,)), ('b', ())]
    assert reached == spy.calls
    with pytest.raises(RuntimeError, match='entry failed'):
        ops.call('boom', 7)
    assert spy.names[-1] == 'boom' and spy.calls[-1] == ('boom', (7,)) and reached[-1] == ('boom', (7,))
    out, names = spy.ran(lambda: ops._call('c', 3))
    assert out == ('result of', 'c') and names == ['c'] and spy.calls == [('c', (3,))]
    spy.clear()
    assert spy.names == [] and spy.calls == []


def test_count_calls_counts_and_calls_through(monkeypatch):
    from frcnn_amd import ops
    monkeypatch.setattr(ops, 'bn_act', lambda x, scale=1: x * scale)
    monkeypatch.setattr(ops, 'pack_boxes', lambda x: -x)
    count = support.count_calls(monkeypatch, ['bn_act', 'pack_boxes'])
    assert ops.bn_act(3, scale=2) == 6 and ops.bn_act(1) == 1 and ops.pack_boxes(4) == -4
    assert count == {'bn_act': 2, 'pack_boxes': 1}


# ----------------------------------------------------------------- fixture_threads
def test_fixture_threads_sets_8_and_restores():
    before = torch.get_num_threads()
    try:
        for prev in (3, 8, 5):
            torch.set_num_threads(prev)
            with support.fixture_threads():
                assert support.FIXTURE_THREADS == 8 and torch.get_num_threads() == 8
            assert torch.get_num_threads() == prev
            with pytest.raises(KeyError):
                with support.fixture_threads():
                    assert torch.get_num_threads() == 8
                    raise KeyError('body')
            assert torch.get_num_threads() == prev
    finally:
        torch.set_num_threads(before)


# ----------------------------------------------------------------- to, nchw, on_cpu
def test_to_and_nchw_keep_containers_and_pass_non_tensors_through():
    cl = torch.randn(2, 4, 3, 5).contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    marker = object()
    x = [cl, (cl, [cl, None, 3, 'name']), marker, {'k': cl}]
    for fn, y in ((support.to, support.to(x, 'cpu')), (support.nchw, support.nchw(x))):
        assert type(y) is list and type(y[1]) is tuple and type(y[1][1]) is list and len(y) == 4
        assert y[1][1][1:] == [None, 3, 'name'] and y[2] is marker and y[3] is x[3]  # a dict is no container here
        for t in (y[0], y[1][0], y[1][1][0]):
            assert torch.is_tensor(t) and torch.equal(t, cl)
            assert t.is_contiguous() == (fn is support.nchw)
    assert support.to(cl, torch.float64).dtype == torch.float64  # whatever Tensor.to takes
    assert support.nchw(5) == 5 and support.to(None, 'cpu') is None
    assert support.nchw(()) == () and support.to([], 'cpu') == []


@pytest.mark.parametrize('pinned', (True, False))
def test_on_cpu_runs_a_copy_under_the_pin_on_nchw_inputs(pinned):
    seen = {}

    class Probe(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.ones(1))

        def forward(self, xs, flag):
            seen.update(threads=torch.get_num_threads(), contiguous=[x.is_contiguous() for x in xs], flag=flag,
                        grad=torch.is_grad_enabled(), module=self)
            return [x * self.weight for x in xs], flag
    m = Probe()
    before = torch.get_num_threads()
    torch.set_num_threads(3)
    try:
        support.on_cpu(m, 'cpu', pinned=pinned)
        cl = torch.randn(1, 4, 2, 3).contiguous(memory_format=torch.channels_last)
        out, flag = m.forward((cl, cl), 'f')
        assert torch.get_num_threads() == 3
    finally:
        torch.set_num_threads(before)
    assert seen['module'] is not m and seen['flag'] == flag == 'f' and not seen['grad']
    assert seen['threads'] == (8 if pinned else 3) and seen['contiguous'] == [pinned, pinned]
    assert type(out) is list and torch.equal(out[0], cl) and not out[0].requires_grad


# ----------------------------------------------------------------- the comparisons
SCORE_RTOL, BOX_RTOL, BOX_ATOL = 1e-6, 2e-6, 1e-4


def _detections(images=2, k=5):
    """(dets as forward_test returns them, the npz's dict) that match exactly."""
    rng = np.random.default_rng(5)
    dets, z = ([], [], []), {'n': np.array(images)}
    for i in range(images):
        lo = rng.uniform(0, 500, (k, 2)).astype(np.float32)
        boxes = np.concatenate([lo, lo + rng.uniform(1, 300, (k, 2)).astype(np.float32)], 1)
        scores = np.sort(rng.uniform(0.1, 0.9, k).astype(np.float32))[::-1].copy()
        labels = rng.integers(1, 21, k)
        z.update({'boxes_%d' % i: boxes, 'scores_%d' % i: scores, 'labels_%d' % i: labels})
        dets[0].append(torch.from_numpy(boxes).t().contiguous())
        dets[1].append(torch.from_numpy(scores.copy()))
        dets[2].append(torch.from_numpy(labels.copy()))
    return dets, z


def _check_dets(dets, z):
    support.assert_detections_match(dets, z, score_rtol=SCORE_RTOL, box_rtol=BOX_RTOL, box_atol=BOX_ATOL)


def test_detections_match_passes_on_equal_and_within_tolerance():
    dets, z = _detections()
    _check_dets(dets, z)
    _check_dets(dets + ('a fourth output',), z)  # only dets[:3] are compared
    dets[1][1][2] *= 1 + 0.4 * SCORE_RTOL
    dets[0][0][:, 1] += 0.5 * BOX_ATOL
    _check_dets(dets, z)


def test_detections_match_fails_on_a_score_just_outside():
    dets, z = _detections()
    dets[1][1][2] *= 1 + 2 * SCORE_RTOL  # f32 holds 2e-6 relative: ~17 ulps at these scores
    with pytest.raises(AssertionError):
        _check_dets(dets, z)


def test_detections_match_fails_on_a_box_outside():
    dets, z = _detections()
    dets[0][1][3, 4] += 4 * (BOX_ATOL + BOX_RTOL * 800)
    with pytest.raises(AssertionError):
        _check_dets(dets, z)


def test_detections_match_fails_on_a_changed_label():
    dets, z = _detections()
    dets[2][0][0] += 1
    with pytest.raises(AssertionError):
        _check_dets(dets, z)


def test_detections_match_fails_on_another_count_of_detections():
    dets, z = _detections()
    for j in range(3):
        dets[j][1] = dets[j][1][..., :-1]
    with pytest.raises(AssertionError):
        _check_dets(dets, z)


def test_detections_match_fails_on_an_empty_reference_image():
    dets, z = _detections()
    for j, key in enumerate(('boxes_1', 'scores_1', 'labels_1')):
        z[key] = z[key][:0]
        dets[j][1] = dets[j][1][..., :0]
    with pytest.raises(AssertionError):
        _check_dets(dets, z)


def test_detections_match_fails_on_a_wrong_image_count():
    dets, z = _detections()
    with pytest.raises(AssertionError):
        _check_dets(tuple(d[:1] for d in dets), z)
    with pytest.raises(AssertionError):
        _check_dets(dets, dict(z, n=np.array(1)))


LOSSES = {'cls_loss': 1.25, 'ctr_loss': 0.625, 'bbox_loss': 0.03125}


def test_losses_match_passes_and_fails():
    got = {k: torch.tensor(v) for k, v in LOSSES.items()}
    support.assert_losses_match(got, LOSSES, rel=2e-5)
    support.assert_losses_match(got, LOSSES, rel=2e-5, ordered=True)
    support.assert_losses_match(got, got, rel=2e-5)  # a reference of tensors
    near = dict(got, ctr_loss=torch.tensor(0.625 * (1 + 1e-5), dtype=torch.float64))
    support.assert_losses_match(near, LOSSES, rel=2e-5)
    off = dict(got, ctr_loss=torch.tensor(0.625 * (1 + 3e-5), dtype=torch.float64))
    with pytest.raises(AssertionError):
        support.assert_losses_match(off, LOSSES, rel=2e-5)
    missing = {k: v for k, v in got.items() if k != 'bbox_loss'}
    extra = dict(got, dfl_loss=torch.tensor(0.0))
    for ordered in (False, True):
        with pytest.raises(AssertionError):
            support.assert_losses_match(missing, LOSSES, rel=2e-5, ordered=ordered)
        with pytest.raises(AssertionError):
            support.assert_losses_match(extra, LOSSES, rel=2e-5, ordered=ordered)
    swapped = {k: got[k] for k in ('ctr_loss', 'cls_loss', 'bbox_loss')}
    support.assert_losses_match(swapped, LOSSES, rel=2e-5)
    with pytest.raises(AssertionError):
        support.assert_losses_match(swapped, LOSSES, rel=2e-5, ordered=True)


def test_the_comparisons_have_no_default_tolerances():
    dets, z = _detections()
    with pytest.raises(TypeError):
        support.assert_detections_match(dets, z)
    with pytest.raises(TypeError):
        support.assert_losses_match(LOSSES, LOSSES)
