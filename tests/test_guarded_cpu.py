"""tests/guarded.py on CPU tensors: the layout it promises, that damage to either guard band is
reported with the allocation and the offset, that the patches leave with the context -- and that
the two GPU sweeps (test_gpu_guarded_convs.py, test_gpu_guarded_detection.py) between them name
every entry of include/frcnn_amd.h that writes device memory."""
import os
import re

import pytest
import torch

import guarded

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _requests():
    return [
        ('contiguous', lambda e: e(2, 3, 5, 7), lambda: torch.empty(2, 3, 5, 7)),
        ('tuple', lambda e: e((3, 5), dtype=torch.int64), lambda: torch.empty((3, 5), dtype=torch.int64)),
        ('channels_last', lambda e: e(2, 3, 5, 7, memory_format=torch.channels_last),
         lambda: torch.empty(2, 3, 5, 7, memory_format=torch.channels_last)),
        ('uint8_odd', lambda e: e(13, dtype=torch.uint8), lambda: torch.empty(13, dtype=torch.uint8)),
        ('empty', lambda e: e(4, 0), lambda: torch.empty(4, 0)),
    ]


@pytest.mark.parametrize('fill', [guarded.CLEAN, guarded.POISON])
def test_payload_has_torchs_strides_alignment_and_fill(monkeypatch, fill):
    want = {name: plain() for name, _, plain in _requests()}
    with guarded.allocator(monkeypatch, fill) as g:
        got = {name: make(torch.empty) for name, make, _ in _requests()}
        strided = torch.empty_strided((2, 3, 4), (40, 12, 2))
        like = torch.empty_like(got['channels_last'])
        view_like = torch.empty_like(got['contiguous'][:, :, ::2])
        zeros = torch.zeros(3, 5, dtype=torch.int32)
        zeros_like = torch.zeros_like(got['channels_last'])
        full = torch.full((2,), 7, dtype=torch.int32)
    assert len(g.records) == len(got) + 6
    for name, t in got.items():
        assert t.shape == want[name].shape and t.stride() == want[name].stride() and t.dtype == want[name].dtype
    assert strided.stride() == (40, 12, 2) and strided.shape == (2, 3, 4)
    assert like.stride() == got['channels_last'].stride() == zeros_like.stride()
    assert view_like.stride() == torch.empty_like(torch.empty(2, 3, 5, 7)[:, :, ::2]).stride()
    for a in g.records:
        assert a.tensor.data_ptr() % 256 == 0
        assert a.start >= guarded.GUARD and a.raw.numel() - a.start - a.nbytes >= guarded.GUARD
        assert a.start % 256 == 0 and a.raw.numel() % 256 == 0
    # the fill: 0xFF bytes are a float NaN and an integer -1; zeros and full keep their values
    if fill == guarded.POISON:
        assert torch.isnan(got['contiguous']).all() and bool((got['tuple'] == -1).all())
        assert bool((got['uint8_odd'] == 0xFF).all())
        assert torch.isnan(strided).all() and torch.isnan(like).all()
    else:
        assert bool((got['contiguous'] == 0).all()) and bool((got['tuple'] == 0).all())
    assert bool((zeros == 0).all()) and bool((zeros_like == 0).all()) and zeros.dtype == torch.int32
    assert full.tolist() == [7, 7] and full.dtype == torch.int32


def test_sentinel_is_a_quiet_nan_and_guards_are_wide_enough():
    s = torch.tensor([guarded.SENTINEL], dtype=torch.int32).view(torch.float32)
    assert torch.isnan(s).all() and guarded.SENTINEL & 0x00400000
    assert guarded.GUARD >= 16384 and guarded.GUARD % 256 == 0 and guarded.GUARD >= 16 * 64 * 16


def _flat(a, dtype=torch.float32):
    """The whole buffer of an allocation as a flat tensor of dtype, and the payload's first index."""
    return a.raw.view(dtype), a.start // a.raw.view(dtype).element_size()


def test_a_store_before_the_payload_is_reported(monkeypatch):
    with pytest.raises(guarded.GuardDamage) as e:
        with guarded.allocator(monkeypatch) as g:
            torch.empty(3, 5)
            flat, guard = _flat(g.records[0])
            flat[guard - 1] = 0.0
    msg = str(e.value)
    assert 'offset -4 ' in msg and '(3, 5)' in msg and 'torch.float32' in msg and 'test_guarded_cpu.py' in msg


def test_a_store_one_element_past_the_end_is_reported(monkeypatch):
    with pytest.raises(guarded.GuardDamage) as e:
        with guarded.allocator(monkeypatch, guarded.POISON) as g:
            t = torch.empty(3, 5)
            flat, guard = _flat(g.records[0])
            flat[guard + t.numel()] = 1.0
    assert 'offset 60 ' in str(e.value) and '(3, 5)' in str(e.value)


def test_a_store_past_an_odd_byte_count_is_reported(monkeypatch):
    with pytest.raises(guarded.GuardDamage) as e:
        with guarded.allocator(monkeypatch) as g:
            torch.empty(13, dtype=torch.uint8)
            flat, guard = _flat(g.records[0], torch.uint8)
            flat[guard + 13] = 0
    assert 'offset 13 ' in str(e.value)


def test_storing_a_nan_into_a_guard_is_reported(monkeypatch):
    with pytest.raises(guarded.GuardDamage) as e:
        with guarded.allocator(monkeypatch) as g:
            t = torch.empty(8)
            flat, guard = _flat(g.records[0])
            flat[guard + t.numel() + 2] = float('nan')
    assert 'offset 40 ' in str(e.value)


def test_the_last_guard_word_is_checked(monkeypatch):
    with pytest.raises(guarded.GuardDamage):
        with guarded.allocator(monkeypatch) as g:
            torch.empty(8)
            flat, _ = _flat(g.records[0])
            flat[-1] = 0.0
    with pytest.raises(guarded.GuardDamage):
        with guarded.allocator(monkeypatch) as g:
            torch.empty(8)
            flat, _ = _flat(g.records[0])
            flat[0] = 0.0


def test_guarded_copy_keeps_values_and_strides_and_reads_nan_behind_the_end(monkeypatch):
    src = torch.arange(24.0).reshape(2, 3, 4).permute(0, 2, 1)
    with guarded.allocator(monkeypatch) as g:
        c = g.copy(src)
        tree = g.copy({'a': [src, None, 3], 'b': (src[:, :0],)})
    assert torch.equal(c, src) and c.stride() == src.stride() and c.data_ptr() % 256 == 0
    assert torch.equal(tree['a'][0], src) and tree['a'][1:] == [None, 3] and tree['b'][0].shape == (2, 0, 3)
    a = g.records[0]
    flat, guard = _flat(a)
    assert torch.isnan(flat[guard + 24]) and torch.isnan(flat[guard - 1])
    lone = guarded.guarded_copy(torch.ones(5, dtype=torch.int64))
    assert lone.tolist() == [1] * 5


def test_assert_written(monkeypatch):
    with guarded.allocator(monkeypatch, guarded.POISON):
        t = torch.empty(4, 6)
        i = torch.empty(5, dtype=torch.int64)
        b = torch.empty(7, dtype=torch.uint8)
    t[:, :5] = 1.0
    t[:3, 5] = float('nan')  # a NaN the kernel computed is not the poison
    with pytest.raises(AssertionError, match='1 of 24 words were never written .first at flat index 23'):
        guarded.assert_written(t)
    t[3, 5] = 2.0
    guarded.assert_written(t)
    guarded.assert_written(t.t())
    i[:] = 3
    i.view(torch.int32)[3] = -1  # half a word of an int64
    with pytest.raises(AssertionError, match='never written'):
        guarded.assert_written(i)
    b[:6] = 1
    with pytest.raises(AssertionError, match='never written'):
        guarded.assert_written(b)
    b[6] = 0
    guarded.assert_written(b)


def test_the_context_restores_torch_also_after_an_exception(monkeypatch):
    before = {n: getattr(torch, n) for n in guarded.Allocator.NAMES}
    with guarded.allocator(monkeypatch):
        assert all(getattr(torch, n) is not f for n, f in before.items())
    assert all(getattr(torch, n) is f for n, f in before.items())
    with pytest.raises(ZeroDivisionError):
        with guarded.allocator(monkeypatch):
            1 / 0
    assert all(getattr(torch, n) is f for n, f in before.items())
    with pytest.raises(guarded.GuardDamage):
        with guarded.allocator(monkeypatch) as g:
            torch.empty(2)
            g.records[0].raw[0] = 0
    assert all(getattr(torch, n) is f for n, f in before.items())
    # patches the test made itself with the same monkeypatch stay
    monkeypatch.setattr(torch, 'empty', before['zeros'])
    with guarded.allocator(monkeypatch):
        pass
    assert torch.empty is before['zeros']


def test_other_devices_and_out_arguments_pass_through(monkeypatch):
    with guarded.allocator(monkeypatch, guarded.POISON, device='cuda') as g:
        t = torch.empty(3)
        m = torch.empty(3, device='meta')
    assert not g.records and m.device.type == 'meta' and t.shape == (3,)
    buf = torch.ones(3)
    with guarded.allocator(monkeypatch, guarded.POISON) as g:
        z = torch.zeros(3, out=buf)
        f = torch.full((3,), 2.0, out=buf)
        e = torch.empty(3, out=buf)
        m = torch.empty(3, device='meta')
    assert not g.records and z is buf and f is buf and e is buf and buf.tolist() == [2.0] * 3
    assert m.device.type == 'meta'


# ----------------------------------------------------------------- the header's entries
def header_entries():
    """{name: return type} of every frh_* function include/frcnn_amd.h declares."""
    text = open(os.path.join(REPO, 'include', 'frcnn_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return {m.group(2): m.group(1).strip() for m in
            re.finditer(r'^\s*((?:const\s+)?\w+\s*\*?)\s*(frh_\w+)\s*\(', text, flags=re.M)}


def test_every_writing_entry_is_swept_or_excused():
    import test_gpu_guarded_convs as convs
    import test_gpu_guarded_detection as det
    declared = header_entries()
    assert len(declared) > 80 and 'frh_conv3x3_bias_act' in declared and 'frh_last_error' in declared
    # by rule: the size queries (they return size_t and touch no device memory) and the two below
    by_rule = {n for n, ret in declared.items() if ret == 'size_t'} | {'frh_last_error', 'frh_abi_version'}
    need = set(declared) - by_rule
    swept = convs.swept_entries() | det.swept_entries()
    excused = dict(convs.NOT_GUARDED, **det.NOT_GUARDED)
    assert all(reason.strip() for reason in excused.values())
    assert not (swept | set(excused)) - set(declared), sorted((swept | set(excused)) - set(declared))
    assert not swept & set(excused), sorted(swept & set(excused))
    missing = sorted(need - swept - set(excused))
    assert not missing, 'entries in no guarded case and not excused: {}'.format(missing)
    for mod in (convs, det):  # the excuses are in the module docstring, where the issue wants them read
        for name in mod.NOT_GUARDED:
            assert name in mod.__doc__, name
