"""ops.conv3x3_nchw_fused_ok / ops.conv3x3_nchw_bn_act where there is no device: on CPU tensors,
and with the library missing, the predicate is False and the op is its modules, decided in Python
with no library call."""
import pytest
import torch
from torch import nn


@pytest.fixture
def ops(monkeypatch):
    from frcnn_amd import ops

    def no_call(name, *args):
        raise AssertionError('library entry %s called' % name)
    monkeypatch.setattr(ops, 'call', no_call)
    monkeypatch.setattr(ops, '_CONV3X3_NCHW_EXCLUDED', frozenset())
    return ops


def test_the_shipped_table_names_only_trunk_classes():
    from frcnn_amd import ops
    assert ops._CONV3X3_NCHW_EXCLUDED <= frozenset([(64, 64), (128, 128), (256, 256), (512, 512)])


@pytest.mark.parametrize('with_bn', (False, True))
def test_cpu_tensors_take_the_modules(ops, with_bn):
    torch.manual_seed(0)
    conv = nn.Conv2d(16, 32, 3, padding=1, bias=False)
    bn = nn.BatchNorm2d(32).eval() if with_bn else None
    x = torch.randn(2, 16, 6, 8)
    with torch.no_grad():
        assert ops.conv3x3_nchw_fused_ok(conv, x, bn) is False
        ref = conv(x) if bn is None else bn(conv(x))
        assert torch.equal(ops.conv3x3_nchw_bn_act(conv, x, bn), ref)
        assert torch.equal(ops.conv3x3_nchw_bn_act(conv, x, bn, relu=True), ref.relu())


def test_missing_library_falls_back(ops, monkeypatch):
    """With no built library the predicate does not try to load it."""
    from frcnn_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', '/nonexistent/libfrcnn_amd.so')
    conv = nn.Conv2d(16, 32, 3, padding=1, bias=False)
    x = torch.randn(1, 16, 4, 8)
    with torch.no_grad():
        assert not ops.conv3x3_nchw_fused_ok(conv, x)
        assert torch.equal(ops.conv3x3_nchw_bn_act(conv, x), conv(x))


def test_bottleneck_on_cpu_is_its_modules(ops):
    from frcnn_amd.backbones import Bottleneck
    torch.manual_seed(1)
    blk = Bottleneck(64, 64).eval()
    x = torch.randn(1, 64, 4, 8)
    with torch.no_grad():
        y = torch.relu(blk.bn1(blk.conv1(x)))
        y = torch.relu(blk.bn2(blk.conv2(y)))
        ref = torch.relu(blk.bn3(blk.conv3(y)) + x)
        assert torch.equal(blk(x), ref)
