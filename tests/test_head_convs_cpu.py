"""ops.head_convs_fused_ok and the one-stage heads' forward without a GPU: the predicate refuses
what the fused entries cannot run, and on CPU tensors both heads compute the module expressions
bit for bit."""
import pytest
import torch
from torch import nn

import head_convs_cases as hc


def _channels_last_weights(head):
    """The layout the heads' convs have on a HIP device (utils.conv_layout), here on the CPU."""
    for m in head.modules():
        if isinstance(m, nn.Conv2d):
            m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
    return head


def _parts(head, cin):
    from frcnn_amd import ops
    if hasattr(head, 'retina_cls'):
        groups = [[head.retina_cls], [head.retina_reg]]
    else:
        groups = [[head.fcos_cls], [head.fcos_reg, head.fcos_center]]
    return [head.cls_convs, head.reg_convs], groups, ops._head_parts([head.cls_convs, head.reg_convs], groups, cin)


@pytest.mark.parametrize('mode', hc.MODES)
def test_structure_of_a_64_channel_head_is_accepted(mode):
    """The layers alone (device, levels and gradients aside): two towers of two layers and the
    mode's output classes."""
    head = _channels_last_weights(hc.make_head(mode))
    parts = _parts(head, 64)[2]
    assert parts is not None
    classes = [p for p, _ in parts]
    assert classes.count(('tower', 64, 64)) == 4
    outs = {'retina': [('out', 64, 180, 0), ('out', 64, 36, 0)], 'fcos': [('out', 64, 20, 0), ('out', 64, 4, 1)],
            'atss': [('out', 64, 20, 0), ('out', 64, 4, 1)], 'gfl': [('out', 64, 20, 0), ('out', 64, 64, 1)]}[mode]
    assert [c for c in classes if c[0] == 'out'] == outs


@pytest.mark.parametrize('mode', hc.MODES)
def test_predicate_is_false_on_cpu_tensors(mode):
    from frcnn_amd import ops
    head = _channels_last_weights(hc.make_head(mode))
    towers, groups, parts = _parts(head, 64)
    assert parts is not None
    with torch.no_grad():
        assert not ops.head_convs_fused_ok(towers, groups, hc.make_levels('cpu'))


@pytest.mark.parametrize('feat', (8, 16))
@pytest.mark.parametrize('mode', ('retina', 'gfl'))
def test_small_heads_are_refused(mode, feat):
    from frcnn_amd import ops
    head = _channels_last_weights(hc.make_head(mode, feat=feat))
    towers, groups, parts = _parts(head, feat)
    assert parts is None
    with torch.no_grad():
        assert not ops.head_convs_fused_ok(towers, groups, hc.make_levels('cpu', cin=feat))


def _refused(head, cin=64, levels=hc.LEVELS):
    from frcnn_amd import ops
    towers, groups, parts = _parts(head, cin)
    with torch.no_grad():
        assert not ops.head_convs_fused_ok(towers, groups, hc.make_levels('cpu', cin=cin, levels=levels))
    return parts is None


def test_a_tower_conv_without_its_relu_is_refused():
    head = _channels_last_weights(hc.make_head('fcos'))
    head.reg_convs[3] = nn.Identity()
    assert _refused(head)
    head = _channels_last_weights(hc.make_head('retina'))
    head.cls_convs = nn.Sequential(*list(head.cls_convs)[:3])
    assert _refused(head)


def test_a_stride_2_conv_is_refused():
    for name, index in (('cls_convs', 2), ('retina_reg', None)):
        head = hc.make_head('retina')
        if index is None:
            head.retina_reg = nn.Conv2d(64, 36, 3, stride=2, padding=1)
        else:
            getattr(head, name)[index] = nn.Conv2d(64, 64, 3, stride=2, padding=1)
        assert _refused(_channels_last_weights(head))


def test_more_than_192_output_channels_are_refused():
    head = hc.make_head('gfl')
    head.fcos_reg = nn.Conv2d(64, 192, 3, padding=1)  # + centerness: 193
    assert _refused(_channels_last_weights(head))
    head.fcos_reg = nn.Conv2d(64, 191, 3, padding=1)
    assert _parts(_channels_last_weights(head), 64)[2] is not None


def test_nine_levels_are_refused():
    """The layers pass; the levels do not (_levels_ok sees the count before the device)."""
    from frcnn_amd import ops
    head = _channels_last_weights(hc.make_head('retina'))
    assert not _refused(head, levels=((4, 4),) * 9)
    assert not ops._levels_ok([torch.zeros(0)] * 9, 64)


@pytest.mark.parametrize('mode', hc.MODES)
def test_cpu_forward_is_the_module_expressions(mode):
    head, xs = hc.make_head(mode), hc.make_levels('cpu')
    with torch.no_grad():
        got, want = hc.flat(head(xs)), hc.flat(hc.module_forward(head, xs))
    assert len(got) == len(want) == (2 if mode == 'retina' else 3) * len(xs)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.stride() == w.stride() and torch.equal(g, w)
    out = head(xs)  # with gradients, as a training step runs it
    assert all(t.grad_fn is not None for t in hc.flat(out))
    for g, w in zip(hc.flat(out), hc.flat(hc.module_forward(head, xs))):
        assert torch.equal(g, w)
