"""Software red zones for the C ABI contract tests (tests/test_gpu_abi_contract.py).

GPU address sanitising is not available to this project, so this module is the instrument: a buffer handed to an
entry point is the PAYLOAD of one device allocation  [front zone | payload | back zone].  The zones carry a
position-dependent pattern (every 4-byte word of the allocation outside the payload is a quiet NaN whose low bits are
the word's index in the allocation, so a copy of a neighbouring zone is caught as well as a stray store), and after the
call `check()` says which bytes outside the payload changed.

Three contracts are checked with it (`run_contract`):
  (a) writes stay inside the outputs and the queried workspaces: every zone is intact after the call;
  (b) results depend on the inputs only: the call is run twice, once on plain pool buffers whose outputs and workspaces
      start as zeros and once on zoned buffers whose outputs and workspaces start as NaN (and whose inputs are
      surrounded by NaN): both runs must agree bit for bit and hold no NaN;
  (c) the value itself: `run_contract` returns the zoned run's outputs for the caller to compare with its reference.

The layout / pattern / checker code works on NumPy byte images and is driven without a GPU by tests/test_host_zoned.py.
"""
import numpy as np

ZONE_BYTES = 4096
NAN_BASE = 0x7FC00000            # quiet NaN; the low 22 bits are free
POISON_WORD = 0x7FD5A5A5         # payload poison: a quiet NaN as float, a huge positive number as int32 / uint32
_IDX_MASK = 0x003FFFFF


# --------------------------------------------------------------------------- #
# layout + pattern + checker on host byte images
# --------------------------------------------------------------------------- #
class Layout(object):
    """Byte geometry of one zoned allocation.  `front` and the back zone are multiples of 256 B, so the payload keeps
    the 256-B alignment of pool blocks unless `shift_bytes` moves it."""

    def __init__(self, payload_bytes, zone_bytes=ZONE_BYTES, shift_bytes=0):
        if zone_bytes <= 0 or zone_bytes % 256:
            raise ValueError('zone_bytes must be a positive multiple of 256')
        if shift_bytes < 0 or shift_bytes >= 256:
            raise ValueError('shift_bytes must be in [0, 256)')
        self.payload_bytes = int(payload_bytes)
        self.zone_bytes = int(zone_bytes)
        self.shift_bytes = int(shift_bytes)
        self.start = self.zone_bytes + self.shift_bytes              # first payload byte
        self.end = self.start + self.payload_bytes                   # first byte of the back zone
        self.total = (self.end + 3) // 4 * 4 + self.zone_bytes       # whole words; the back zone is >= zone_bytes


def pattern_bytes(layout):
    """The whole allocation filled with the zone pattern (uint8)."""
    words = (NAN_BASE | (np.arange(layout.total // 4, dtype=np.uint32) & _IDX_MASK)).astype('<u4')
    return words.view(np.uint8).copy()


def index_pattern_bytes(layout, lo, hi):
    """Zone pattern for int32 INDEX inputs: valid indices in [lo, hi) that differ from their neighbours (a read past the
    row yields a well-formed but wrong index instead of a stray address)."""
    n = layout.total // 4
    span = max(int(hi) - int(lo), 1)
    words = (int(lo) + (np.arange(n, dtype=np.int64) * 7 + 3) % span).astype('<i4')
    return words.view(np.uint8).copy()


def make_image(layout, payload, zone_pattern=None):
    """Byte image of the allocation: pattern everywhere, `payload` (uint8, payload_bytes long) in its place."""
    img = pattern_bytes(layout) if zone_pattern is None else zone_pattern.copy()
    payload = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
    if payload.size != layout.payload_bytes:
        raise ValueError('payload of %d bytes in a layout of %d' % (payload.size, layout.payload_bytes))
    img[layout.start:layout.end] = payload
    return img


def poison_payload(nbytes):
    """nbytes of POISON_WORD (the tail of an odd length is cut from a whole word)."""
    words = np.full((nbytes + 3) // 4, POISON_WORD, '<u4')
    return words.view(np.uint8)[:nbytes].copy()


class Corruption(object):
    """One damaged zone: byte offsets RELATIVE TO THE PAYLOAD (negative: in front of it; >= payload_bytes: behind it)."""

    def __init__(self, name, zone, first, last, count, first_word, last_word, payload_bytes):
        self.name, self.zone, self.first, self.last, self.count = name, zone, first, last, count
        self.first_word, self.last_word, self.payload_bytes = first_word, last_word, payload_bytes

    def __str__(self):
        def val(w):
            return '0x%08x (%r as float, %d as int32)' % (
                w, float(np.array([w], '<u4').view('<f4')[0]), int(np.array([w], '<u4').view('<i4')[0]))
        return ('%s: %s zone corrupted, %d byte(s) changed; first at payload offset %d, last at %d '
                '(payload is %d bytes: its last byte is offset %d); word found at first = %s, at last = %s'
                % (self.name, self.zone, self.count, self.first, self.last, self.payload_bytes,
                   self.payload_bytes - 1, val(self.first_word), val(self.last_word)))


def find_corruption(layout, image, name='buffer', zone_pattern=None):
    """Compares the zones of `image` (uint8, the whole allocation) with the pattern; returns a list of Corruption."""
    image = np.ascontiguousarray(image).view(np.uint8).reshape(-1)
    if image.size != layout.total:
        raise ValueError('image of %d bytes for a layout of %d' % (image.size, layout.total))
    want = pattern_bytes(layout) if zone_pattern is None else zone_pattern
    words = image.view('<u4')
    out = []
    for zone, a, b in (('front', 0, layout.start), ('back', layout.end, layout.total)):
        bad = np.nonzero(image[a:b] != want[a:b])[0]
        if bad.size:
            first, last = a + int(bad[0]), a + int(bad[-1])
            out.append(Corruption(name, zone, first - layout.start, last - layout.start, int(bad.size),
                                  int(words[first // 4]), int(words[last // 4]), layout.payload_bytes))
    return out


# --------------------------------------------------------------------------- #
# device side
# --------------------------------------------------------------------------- #
class ZonedArray(object):
    """[front zone | payload | back zone] in ONE device allocation; `.arr` is the payload as a DeviceArray view.

    host: a NumPy array (its bytes become the payload) or None with `shape`; fill (payload without a host array):
    'poison' (POISON_WORD: NaN) or 'zero'.  index_range=(lo, hi): the zones hold valid int32 indices instead of NaN."""

    def __init__(self, gpu, host=None, shape=None, dtype=np.float32, zone_bytes=ZONE_BYTES, fill='poison', shift_bytes=0,
                 index_range=None, name='buffer'):
        if host is not None:
            host = np.ascontiguousarray(host)
            shape, dtype = host.shape, host.dtype
        self.name = name
        self.shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.layout = Layout(nbytes, zone_bytes, shift_bytes)
        self.zone_pattern = None if index_range is None else index_pattern_bytes(self.layout, *index_range)
        if host is not None:
            payload = host.view(np.uint8).reshape(-1)
        elif fill == 'zero':
            payload = np.zeros(nbytes, np.uint8)
        elif fill == 'poison':
            payload = poison_payload(nbytes)
        else:
            raise ValueError('fill must be "poison" or "zero"')
        self.initial = payload.copy()
        self.block = gpu.DeviceArray((self.layout.total,), np.uint8)
        self.block.set(make_image(self.layout, payload, self.zone_pattern))
        self.arr = gpu.DeviceArray(self.shape, self.dtype, _block=self.block._block, _ptr=self.block.ptr + self.layout.start)

    @property
    def ptr(self):
        return self.arr.ptr

    def get(self):
        return self.arr.get()

    def corruption(self):
        return find_corruption(self.layout, self.block.get(), self.name, self.zone_pattern)

    def check(self):
        bad = self.corruption()
        assert not bad, '\n'.join(str(c) for c in bad)


# --------------------------------------------------------------------------- #
# buffer specifications + the contract runner
# --------------------------------------------------------------------------- #
class Spec(object):
    """role 'in': host array -> device, must not change.  'out': shape / dtype; starts as zeros in the plain run and as
    POISON_WORD in the zoned run unless `init` (the documented caller-initialised content: zeroed maxima words, the addend
    of accumulate = 1, optimizer state) is given.  'ws': nbytes of workspace, treated like an output whose content is
    not compared.  valid: boolean mask of the elements the entry point is documented to write (strided outputs, the
    unwritten half of `gates`): those are compared, the others must keep their initial bits.  exact=False: an entry point
    the header does not call deterministic (float atomics): compared by the caller at its parity bar."""

    def __init__(self, role, host=None, shape=None, dtype=np.float32, init=None, shift=0, index_range=None, valid=None,
                 exact=True, nan_ok=False):
        self.role, self.host, self.init, self.shift = role, host, init, shift
        self.index_range, self.valid, self.exact, self.nan_ok = index_range, valid, exact, nan_ok
        src = host if host is not None else init
        if src is not None:
            src = np.ascontiguousarray(src)
            shape, dtype = src.shape, src.dtype
        self.shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)


def In(host, shift=0, index_range=None):
    return Spec('in', host=np.ascontiguousarray(host), shift=shift, index_range=index_range)


def Out(shape=None, dtype=np.float32, init=None, shift=0, valid=None, exact=True, nan_ok=False):
    return Spec('out', shape=shape, dtype=dtype, init=None if init is None else np.ascontiguousarray(init), shift=shift,
                valid=valid, exact=exact, nan_ok=nan_ok)


def Ws(nbytes):
    return Spec('ws', shape=(int(nbytes),), dtype=np.uint8)


class Bufs(dict):
    """name -> DeviceArray; attribute access; `.ptr(name)` is None-safe."""
    __getattr__ = dict.__getitem__


def _alloc_plain(gpu, spec):
    if spec.shift:
        # the plain run keeps the same pointer class (the dispatch under test must be the same in both runs)
        n = int(np.prod(spec.shape, dtype=np.int64)) * spec.dtype.itemsize
        block = gpu.DeviceArray((n + 256,), np.uint8)
        block.fill_zero()
        arr = gpu.DeviceArray(spec.shape, spec.dtype, _block=block._block, _ptr=block.ptr + spec.shift)
    else:
        arr = gpu.DeviceArray(spec.shape, spec.dtype)
    src = spec.host if spec.role == 'in' else spec.init
    if src is not None:
        arr.set(src)
    else:
        arr.fill_zero()
    return arr


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def run_contract(gpu, fn, specs, zone_bytes=ZONE_BYTES):
    """Runs fn(bufs) once on plain pool buffers and once on zoned ones (see the module docstring) and asserts
    contracts (a) and (b).  Returns {name: host array} of the zoned run's outputs."""
    plain = Bufs((k, _alloc_plain(gpu, s)) for k, s in specs.items())
    fn(plain)
    gpu.synchronize()
    plain_out = dict((k, plain[k].get()) for k, s in specs.items() if s.role == 'out')
    del plain

    zoned = {}
    for k, s in specs.items():
        src = s.host if s.role == 'in' else s.init
        zoned[k] = ZonedArray(gpu, host=src, shape=s.shape, dtype=s.dtype, zone_bytes=zone_bytes, shift_bytes=s.shift,
                              index_range=s.index_range, name=k)
    fn(Bufs((k, z.arr) for k, z in zoned.items()))
    gpu.synchronize()

    problems = []
    for k, z in zoned.items():                                   # (a) every zone intact
        problems += [str(c) for c in z.corruption()]
    assert not problems, 'write outside a buffer:\n' + '\n'.join(problems)

    results = {}
    for k, s in specs.items():
        z = zoned[k]
        if s.role == 'ws':
            continue
        got = z.get()
        if s.role == 'in':
            assert np.array_equal(_bits(got).reshape(-1), _bits(s.host).reshape(-1)), 'input %s was modified' % k
            continue
        results[k] = got
        sel = slice(None) if s.valid is None else np.asarray(s.valid, bool)
        if s.valid is not None:                                  # the elements nobody is documented to write keep their bits
            before = z.initial.view(_bits(got).dtype).reshape(got.shape)
            moved = np.nonzero((_bits(got) != before) & ~sel)
            assert moved[0].size == 0, \
                'output %s: element %s outside the documented extent was written (%d such elements)' % (
                    k, tuple(int(i[0]) for i in moved), moved[0].size)
        g, p = got[sel], plain_out[k][sel]
        if np.issubdtype(s.dtype, np.floating) and not s.nan_ok:
            bad = np.nonzero(~np.isfinite(g.reshape(-1).astype(np.float64)))[0]
            assert bad.size == 0, 'output %s: non-finite at flat index %d (%d in all): an element was not written, or ' \
                'was computed from memory outside the inputs' % (k, int(bad[0]), bad.size)
        if s.exact:                                              # (b) independent of what surrounded and preceded the data
            diff = np.nonzero(_bits(g).reshape(-1) != _bits(p).reshape(-1))[0]
            assert diff.size == 0, \
                'output %s differs between zero-initialised pool buffers and NaN-surrounded ones at flat index %d ' \
                '(%r vs %r; %d elements): the result depends on memory outside the inputs' % (
                    k, int(diff[0]), p.reshape(-1)[diff[0]], g.reshape(-1)[diff[0]], diff.size)
    return results
