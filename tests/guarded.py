"""A guarded allocator for tests: every tensor it makes is a view into the middle of a larger
flat byte buffer whose two ends (the guard bands) hold one fixed 32-bit pattern, so that a
kernel that stores outside its output, reads past the end of an input, or depends on what an
uninitialised buffer held is seen by a test that otherwise only compares values.

Layout of one allocation (bytes):  [ front guard | payload | back guard ]
  * each guard band is GUARD (16 KiB, a multiple of 256) bytes at least; the back band starts
    on the byte after the payload's last element and is rounded up so the buffer ends on 256;
  * the payload starts 256-byte aligned, so every 16-byte and 256-byte alignment requirement of
    the library's entries holds as it does for a tensor of the caching allocator;
  * the payload has the strides torch would have given it (contiguous, channels_last,
    empty_strided): they are taken from the same call on device='meta' and applied with
    as_strided.

The band size is a condition, not a measurement.  16 KiB is sixteen times a wave's widest access
(64 lanes x 16 bytes), so a stray store or over-read of a tile, a row or a vector past either end
lands in a band.  A store further out than GUARD bytes from the payload is NOT seen.

The guards are filled with SENTINEL (0x7FC0BEEF, a quiet-NaN bit pattern: an over-read of a float
input picks up a NaN, which reaches the result even through a multiplication by zero) and are
checked by comparing the bands as int32 with SENTINEL, never with isnan: a kernel that stores a
NaN of its own into a guard is caught as well.

The payload fill is selectable: 0x00 bytes (the clean run) or 0xFF bytes (the poisoned run: float
NaN, integer -1).  torch.zeros and torch.full keep their values under both fills (the
zero-contract workspaces rely on the first) and are guarded all the same.

guarded_copy / guarded_tree put inputs into guarded buffers, allocator() is the context manager
that reroutes the Python-level allocations, assert_written looks for poison left in an output, and
sweep() is the three-run comparison the two GPU files (test_gpu_guarded_convs.py,
test_gpu_guarded_detection.py) make of every case.  Works on CPU tensors too
(tests/test_guarded_cpu.py)."""
import contextlib
import os
import sys

import torch

GUARD = 16384
ALIGN = 256
SENTINEL = 0x7FC0BEEF
CLEAN, POISON = 0x00, 0xFF
_SENTINEL_BYTES = [(SENTINEL >> (8 * i)) & 0xFF for i in range(4)]  # little endian
_HERE = os.path.abspath(__file__)


class GuardDamage(AssertionError):
    pass


def _round_up(v, m):
    return (v + m - 1) // m * m


def _extent(shape, strides):
    """Elements of storage a (shape, strides) view spans; 0 for an empty tensor."""
    if any(s == 0 for s in shape):
        return 0
    return 1 + sum((s - 1) * st for s, st in zip(shape, strides))


def _call_site():
    """file:line of the nearest frame outside this module (and outside contextlib)."""
    f = sys._getframe(1)
    while f is not None:
        name = f.f_code.co_filename
        if os.path.abspath(name) != _HERE and not name.endswith('contextlib.py'):
            return '{}:{}'.format(os.path.basename(name), f.f_lineno)
        f = f.f_back
    return '?'


class Allocation(object):
    """One guarded buffer: `tensor` is the payload view, `raw` the whole byte buffer."""

    def __init__(self, raw, tensor, start, nbytes, site):
        self.raw, self.tensor, self.start, self.nbytes, self.site = raw, tensor, start, nbytes, site

    def describe(self):
        return 'shape {} dtype {} allocated at {}'.format(tuple(self.tensor.shape), self.tensor.dtype, self.site)

    def _bands(self):
        end = self.start + self.nbytes
        return (0, self.start), (end, self.raw.numel())

    def damage(self):
        """None if both bands are intact, else the first damaged byte's offset relative to the
        payload's first byte (negative in the front band, >= nbytes in the back band)."""
        for lo, hi in self._bands():
            lo4 = _round_up(lo, 4)
            words = self.raw[lo4:hi].view(torch.int32)
            head = self.raw[lo:lo4]
            want = torch.tensor([_SENTINEL_BYTES[(lo + i) % 4] for i in range(lo4 - lo)], dtype=torch.uint8,
                                device=self.raw.device)
            if bool((words != SENTINEL).any()) or bool((head != want).any()):
                pattern = torch.tensor(_SENTINEL_BYTES, dtype=torch.uint8, device=self.raw.device)
                expect = pattern.repeat((hi - lo) // 4 + 2)[lo % 4:lo % 4 + hi - lo]
                bad = torch.nonzero(self.raw[lo:hi] != expect)
                return lo + int(bad[0]) - self.start
        return None

    def check(self):
        off = self.damage()
        if off is not None:
            raise GuardDamage('guard band damaged at byte offset {} of the payload ({} bytes): {}'.format(
                off, self.nbytes, self.describe()))


def _guarded(real_empty, shape, strides, dtype, device, fill, site):
    """The payload view (shape, strides, dtype) on device inside a fresh guarded buffer."""
    itemsize = torch.empty((), dtype=dtype, device='meta').element_size()
    nbytes = _extent(shape, strides) * itemsize
    total = GUARD + _round_up(nbytes, ALIGN) + GUARD  # the back band: GUARD + the round-up
    raw = real_empty(total + ALIGN, dtype=torch.uint8, device=device)
    skew = (-raw.data_ptr()) % ALIGN
    raw = raw[skew:skew + total]
    raw.view(torch.int32).fill_(SENTINEL)
    payload = raw[GUARD:GUARD + nbytes]
    payload.fill_(fill)
    t = payload.view(dtype).as_strided(tuple(shape), tuple(strides)) if nbytes else \
        raw[GUARD:GUARD].view(dtype).as_strided(tuple(shape), tuple(strides))
    return Allocation(raw, t, GUARD, nbytes, site)


def guarded_copy(t, recorder=None):
    """The values and strides of t in a guarded buffer of its own (inputs: activations, weights,
    anchors, boxes, labels, offsets): a read past either end picks up the sentinel NaN.  The view
    spans exactly t's own extent; for a view into a larger parent pass the parent and re-slice.
    With `recorder` (an allocator) its guards are checked on the allocator's exit too."""
    if t is None:
        return None
    a = _guarded(torch.empty if recorder is None else recorder.real['empty'], tuple(t.shape), tuple(t.stride()),
                 t.dtype, t.device, CLEAN, _call_site())
    if a.nbytes:
        a.tensor.copy_(t)
    if recorder is not None:
        recorder.records.append(a)
    return a.tensor


def guarded_tree(x, recorder=None):
    """guarded_copy of every tensor in a (nested) list / tuple / dict; other leaves as they are."""
    if torch.is_tensor(x):
        return guarded_copy(x, recorder)
    if isinstance(x, (list, tuple)):
        return type(x)(guarded_tree(v, recorder) for v in x)
    if isinstance(x, dict):
        return {k: guarded_tree(v, recorder) for k, v in x.items()}
    return x


def assert_written(t, what='output'):
    """No 32-bit word of t still holds the 0xFF poison (an element narrower than 32 bits: no
    element).  For outputs that must be fully defined and in which an all-ones word is no value
    (floats: that word is a NaN; counts, indices and labels that are never -1)."""
    if t.numel() == 0:
        return
    c = t.detach().contiguous().view(-1)
    if c.element_size() >= 4:
        left = c.view(torch.int32) == -1
    else:
        left = c.view(torch.uint8) == 0xFF
    n = int(left.sum())
    assert n == 0, '{}: {} of {} words were never written (first at flat index {}), shape {} dtype {}'.format(
        what, n, left.numel(), int(torch.nonzero(left)[0]), tuple(t.shape), t.dtype)


class Allocator(object):
    """Routes torch.empty / empty_like / empty_strided / zeros / zeros_like / full (what
    frcnn_amd/ops.py and _lib.workspace allocate with; ops._nhwc_empty goes through torch.empty)
    through guarded buffers and records every allocation with its call site."""

    NAMES = ('empty', 'empty_like', 'empty_strided', 'zeros', 'zeros_like', 'full')

    def __init__(self, fill=CLEAN, device=None):
        self.fill = fill
        self.device = None if device is None else torch.device(device)  # guard this device only
        self.records = []
        self.real = {n: getattr(torch, n) for n in self.NAMES}

    # -- helpers
    def _mine(self, k, dev):
        if k.get('out') is not None or k.get('pin_memory') or k.get('names') is not None:
            return False
        if k.get('layout', torch.strided) is not torch.strided:
            return False
        dev = torch.device(dev if dev is not None else 'cpu')
        if dev.type == 'meta':
            return False
        return self.device is None or dev.type == self.device.type

    def _make(self, meta, dev, fill, requires_grad=False):
        a = _guarded(self.real['empty'], tuple(meta.shape), tuple(meta.stride()), meta.dtype, dev, fill, _call_site())
        self.records.append(a)
        return a.tensor.requires_grad_() if requires_grad else a.tensor

    def _factory(self, name, fill_of):
        real = self.real[name]

        def make(*a, **k):
            dev = k.get('device')
            if not self._mine(k, dev):
                return real(*a, **k)
            k2 = dict(k, device='meta')
            rg = k2.pop('requires_grad', False)
            return self._make(real(*a, **k2), dev if dev is not None else 'cpu', fill_of(a, k), rg)
        return make

    def _like(self, name, fill_of):
        real = self.real[name]

        def make(t, *a, **k):
            dev = k.get('device', t.device)
            if not self._mine(k, dev) or a:
                return real(t, *a, **k)
            k2 = dict(k, device='meta')
            rg = k2.pop('requires_grad', False)
            return self._make(real(t, **k2), dev, fill_of(a, k), rg)
        return make

    def patches(self):
        def full(*a, **k):
            real = self.real['full']
            dev = k.get('device')
            if not self._mine(k, dev):
                return real(*a, **k)
            plain = real(*a, **k)  # the values (and the dtype torch infers) from torch itself
            out = self._make(plain, plain.device, CLEAN, k.get('requires_grad', False))
            with torch.no_grad():
                out.copy_(plain)
            return out
        return {
            'empty': self._factory('empty', lambda a, k: self.fill),
            'empty_strided': self._factory('empty_strided', lambda a, k: self.fill),
            'zeros': self._factory('zeros', lambda a, k: CLEAN),
            'empty_like': self._like('empty_like', lambda a, k: self.fill),
            'zeros_like': self._like('zeros_like', lambda a, k: CLEAN),
            'full': full,
        }

    def copy(self, x):
        """guarded_tree of x, the guards checked with this allocator's own."""
        return guarded_tree(x, self)

    def check(self):
        devs = {a.raw.device for a in self.records if a.raw.is_cuda}
        for d in devs:
            torch.cuda.synchronize(d)
        for a in self.records:
            a.check()


def clear_workspaces():
    """Drop the persistent workspaces and the memoised gt packs of frcnn_amd.ops, so that the
    next call allocates them anew (under an allocator: guarded)."""
    from frcnn_amd import ops
    ops._ASSIGN_WS.clear()
    ops._SAMPLE_WS.clear()
    ops._LOSS_WS.clear()
    del ops._PACKED[:]


@contextlib.contextmanager
def allocator(monkeypatch, fill=CLEAN, device=None, clear=True):
    """with allocator(monkeypatch, POISON) as g: ...   Inside, the Python-level allocation calls
    go through guarded buffers (g.records); on exit the patches are undone (also after an
    exception), the device is synchronised and every recorded guard must be intact: GuardDamage
    names the allocation (shape, dtype, call site) and the first damaged byte offset relative to
    the payload.  clear: drop ops' persistent workspaces first (and afterwards, so that nothing
    guarded outlives the check), if frcnn_amd.ops has been imported."""
    g = Allocator(fill, device)

    def drop():
        if clear and 'frcnn_amd.ops' in sys.modules:
            clear_workspaces()
    drop()
    with monkeypatch.context() as m:
        for name, fn in g.patches().items():
            m.setattr(torch, name, fn)
        if 'frcnn_amd.ops' in sys.modules:
            ops = sys.modules['frcnn_amd.ops']
            # patched by name so that the allocation is attributed to its caller in ops, not to
            # the helper's one line, and stays guarded whatever the helper allocates with
            m.setattr(ops, '_nhwc_empty', lambda shape, dev: torch.empty(
                tuple(shape), dtype=torch.float32, device=dev, memory_format=torch.channels_last))
        try:
            yield g
        finally:
            m.undo()
            drop()
    g.check()


# ----------------------------------------------------------------- the sweep both GPU files run
def tensors(x):
    """The tensors of a (nested) list / tuple / dict, in order; None and other leaves dropped."""
    if torch.is_tensor(x):
        return [x]
    if isinstance(x, dict):
        x = list(x.values())
    if isinstance(x, (list, tuple)):
        return [t for v in x for t in tensors(v)]
    return []


def same_bits(a, b):
    """Same shape, dtype and bytes (a NaN equals the same NaN)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(a.detach().contiguous().view(-1).view(torch.uint8), b.detach().contiguous().view(-1).view(torch.uint8))


@contextlib.contextmanager
def entry_names(monkeypatch):
    """The names of the library entries called inside, through _lib.call or ops' own binding."""
    from frcnn_amd import _lib, ops
    names = []
    real = _lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    with monkeypatch.context() as m:
        m.setattr(_lib, 'call', call)
        m.setattr(ops, '_call', call)
        yield names


def sweep(monkeypatch, fn, make, entries, defined=None, written=True, bits=True):
    """Run fn(make()) three times: on plain tensors as the existing tests do, then twice under
    the allocator on guarded copies of the inputs, with outputs and workspaces filled with 0x00
    and with 0xFF.  make() returns the inputs afresh (any tree of tensors and other values); fn
    returns a tree of tensors; defined(out) cuts the part of them the operation defines (default:
    all of it).  Asserts: the entries named were called in every run; every guard intact (the
    allocator's exit); the defined outputs poison-free (written: float outputs only unless
    written == 'all'; an integer output may hold -1 as a value, an element of it left unwritten
    shows in the next comparison) and finite; clean == poisoned == plain bit for bit.  bits=False
    (an entry that sums with float atomics) leaves that last comparison to the caller, who holds
    each run to the entry's own bound.  Returns the runs' defined outputs: plain, clean, poisoned."""
    defined = defined or (lambda out: out)
    runs = []
    for fill in (None, CLEAN, POISON):
        with entry_names(monkeypatch) as names:
            if fill is None:
                out = fn(make())
                torch.cuda.synchronize()
            else:
                with allocator(monkeypatch, fill, device='cuda') as g:
                    out = fn(g.copy(make()))
                    torch.cuda.synchronize()
                    assert g.records, 'nothing was allocated under the allocator'
            out = tensors(defined(out))
        missing = set(entries) - set(names)
        assert not missing, 'entries the case names but did not call: {} (called: {})'.format(sorted(missing), names)
        runs.append(out)
    plain, clean, poison = runs
    assert len(plain) == len(clean) == len(poison) and plain
    for i, (p, c, q) in enumerate(zip(plain, clean, poison)):
        what = 'output {} {} {}'.format(i, tuple(q.shape), q.dtype)
        if written == 'all' or (written and q.is_floating_point()):
            assert_written(q, what + ' (poisoned run)')
        if q.is_floating_point():
            assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(c).all()), what + ': not finite'
        if bits:
            assert same_bits(c, q), what + ': the clean and the poisoned run differ'
            assert same_bits(c, p), what + ': the guarded and the plain run differ'
    return [plain, clean, poison]
