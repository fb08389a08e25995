"""The shared clauses of ops.py's *_fused_ok predicates (which BN counts as frozen, which Conv2d
has the geometry an entry was written for) and the predicates themselves on CPU tensors: all of
it decided in Python, no library call."""
import pytest
import torch
from torch import nn


@pytest.fixture
def ops(monkeypatch):
    from frcnn_amd import ops

    def no_call(name, *args):
        raise AssertionError('library entry %s called' % name)
    monkeypatch.setattr(ops, 'call', no_call)
    return ops


def test_frozen_bn_truth_table(ops):
    assert not ops._frozen_bn(nn.BatchNorm2d(8))                                    # training
    assert ops._frozen_bn(nn.BatchNorm2d(8).eval())                                 # eval, statistics
    assert not ops._frozen_bn(nn.BatchNorm2d(8, track_running_stats=False).eval())  # eval, batch statistics
    assert ops._frozen_bn(nn.BatchNorm2d(8, affine=False).eval())                   # eval, statistics, no gamma / beta
    assert not ops._frozen_bn(nn.BatchNorm2d(8, affine=False))


def test_conv_is(ops):
    plain = nn.Conv2d(16, 64, 3, padding=1)
    assert ops._conv_is(plain, 3, 1, 1)
    assert not ops._conv_is(plain, 1, 1, 0) and not ops._conv_is(plain, 3, 1, 0) and not ops._conv_is(plain, 3, 2, 1)
    assert ops._conv_is(nn.Conv2d(16, 64, 1), 1, 1, 0)
    strided = nn.Conv2d(16, 64, 3, stride=2, padding=1)
    assert ops._conv_is(strided, 3, 2, 1) and not ops._conv_is(strided, 3, 1, 1)
    assert not ops._conv_is(nn.Conv2d(16, 64, 3, stride=(1, 2), padding=1), 3, 1, 1)
    assert not ops._conv_is(nn.Conv2d(16, 64, 3, padding=1, dilation=2), 3, 1, 1)
    assert not ops._conv_is(nn.Conv2d(16, 64, 3, padding=1, groups=2), 3, 1, 1)
    assert not ops._conv_is(nn.Conv2d(16, 64, 3, padding=1, padding_mode='reflect'), 3, 1, 1)
    assert not ops._conv_is(nn.Conv2d(16, 64, 3, padding=1).double(), 3, 1, 1)


BNS = {'frozen': lambda c: nn.BatchNorm2d(c).eval(),
       'no_stats': lambda c: nn.BatchNorm2d(c, track_running_stats=False).eval()}


@pytest.mark.parametrize('kind', sorted(BNS))
def test_fused_ok_is_false_on_cpu(ops, kind):
    bn, pre_bn = BNS[kind](64), BNS[kind](16)
    x = torch.randn(1, 16, 8, 8)
    conv1 = nn.Conv2d(16, 64, 1, bias=False)
    assert ops.conv1x1_fused_ok(conv1, bn, x) is False
    assert ops.conv1x1_fused_ok(conv1, bn, x, torch.randn(1, 64, 8, 8)) is False
    assert not ops.conv1x1_pre_fused_ok(conv1, bn, x, pre_bn)
    assert not ops.conv1x1_s2_fused_ok(nn.Conv2d(16, 64, 1, stride=2, bias=False), bn, x)
    assert not ops.roi_conv3x3_fused_ok(nn.Conv2d(16, 64, 3, padding=1, bias=False), bn, torch.randn(2, 16, 7, 7))
    x_cl = x.contiguous(memory_format=torch.channels_last)
    conv3 = nn.Conv2d(16, 64, 3, padding=1).to(memory_format=torch.channels_last)
    assert not ops.conv3x3_fused_ok(conv3, x_cl) and not ops.conv3x3_fused_ok(conv3, x_cl, alone=False)
    assert not ops.rpn_head1x1_fused_ok(nn.Conv2d(16, 3, 1), nn.Conv2d(16, 12, 1), [x_cl, x_cl[:, :, :4, :4]])


@pytest.mark.parametrize('kind', sorted(BNS))
def test_cpu_calls_take_the_module_path(ops, kind):
    """On CPU tensors every fused op is its modules (ops.call raises here); a BN without running
    statistics normalises with the batch's."""
    torch.manual_seed(0)
    bn = BNS[kind](64)
    conv = nn.Conv2d(16, 64, 1, bias=False)
    x = torch.randn(2, 16, 8, 8)
    with torch.no_grad():
        ref = torch.relu(bn(conv(x)))
        assert torch.equal(ops.conv1x1_bn_act(conv, bn, x), ref)
        assert torch.equal(ops.bn_act(conv(x), bn), ref)
        pool = nn.MaxPool2d(3, 2, 1)
        assert torch.equal(ops.bn_act_maxpool(conv(x), bn, pool), pool(ref))
