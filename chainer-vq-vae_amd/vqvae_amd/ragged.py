"""What the corpus, the ragged front end, the metrics and the latent-rate condition share: N utterances laid end to end in
one device buffer, described by lengths and offsets.  Functions only; LatentCodes, LatentCondition, RaggedFeatures and
ResidentCorpus stay four plain classes that call them."""
import numpy as np

from . import backend
from .backend import DeviceArray


def offsets(sizes, total=False):
    """The int64 exclusive prefix sum of ``sizes``: (N,), or (N + 1,) with the total appended.  The sum is formed in int64
    whatever the input's dtype."""
    off = np.zeros(np.size(sizes) + 1, np.int64)
    np.cumsum(np.asarray(sizes).reshape(-1), dtype=np.int64, out=off[1:])
    return off if total else off[:-1]


def plan_runs(elements, chunk_bytes, cap=None):
    """Cuts utterances 0 .. N - 1 greedily, in input order, into runs [(start, stop), ...].  ``elements``: (S, N) int64,
    the float32 elements of every (stage, utterance).  A run is closed when the next utterance would take
    4 * (the largest running sum over the stages) over ``chunk_bytes`` or, with ``cap``, bring that sum to ``cap``
    elements; an utterance over the byte budget stands alone."""
    elements = np.asarray(elements, np.int64)
    S, N = elements.shape
    runs, start, run = [], 0, np.zeros(S, np.int64)
    for u in range(N):
        new = run + elements[:, u]
        if u > start and (4 * int(new.max()) > int(chunk_bytes) or (cap is not None and new.max() >= cap)):
            runs.append((start, u))
            start, new = u, elements[:, u].copy()
        run = new
    if N > start:
        runs.append((start, N))
    return runs


def check_lengths(tl, who):
    """``tl`` as an array, a ValueError unless it is (N,) integers >= 1 with N >= 1."""
    tl = np.asarray(tl)
    if tl.ndim != 1 or tl.size == 0 or tl.dtype.kind not in 'iu' or (tl < 1).any():
        raise ValueError('%s: tl must be (N,) latent lengths >= 1 with N >= 1, got %r' % (who, tl))
    return tl


def split(flat, offsets, axis=-1):
    """The per-utterance pieces of a host array along ``axis``, as copies: piece i is [offsets[i], offsets[i + 1])."""
    flat = np.moveaxis(flat, axis, -1)
    return [np.moveaxis(flat[..., int(a):int(b)], -1, axis).copy() for a, b in zip(offsets[:-1], offsets[1:])]


def pack_padded(blocks, lengths, C, Tmax):
    """The zero-initialised float32 device array (N, C, Tmax) with block i -- a device array of C rows of lengths[i] -- in
    the first lengths[i] columns of [i]: one batched copy of the N * C rows.  ``blocks`` is walked once, after the output
    has been zeroed."""
    out = backend.zeros((len(lengths), C, Tmax), np.float32)
    backend.copy_many([(out.flat_view((i * C + ch) * Tmax, int(L)), b.flat_view(ch * int(L), int(L)))
                       for i, (b, L) in enumerate(zip(blocks, lengths)) for ch in range(C)])
    return out


def wave_source(waves, who):
    """Where the waves are: (lengths (N,) int64, source), with source(start, stop) -> (device pointer of x, off_in (n,)
    int64, what to keep alive) for a run of utterances.  A ResidentCorpus / CorpusView is read in place through its
    offsets.  Anything else is a list of host or device float32 arrays, each taken whole; a run of them is laid end to
    end on the device (host waves: one upload per run; device waves: one batched copy; both: one of each)."""
    from .corpus import _Utterances
    if isinstance(waves, _Utterances):
        base = waves.corpus
        if getattr(base, 'samples', None) is None:
            raise RuntimeError('%s: this corpus is a description only (nothing on the device)' % who)
        utt = np.asarray(waves.utterances, np.int64)
        return np.asarray(waves.lengths, np.int64), lambda start, stop: (base.samples.ptr, base.offsets[utt[start:stop]], None)
    waves = list(waves)
    for i, w in enumerate(waves):
        if backend.is_device(w):
            if w.dtype != np.float32:
                raise ValueError('%s: wave %d is a %s device array, float32 needed' % (who, i, w.dtype))
        else:
            waves[i] = np.ascontiguousarray(w, np.float32).reshape(-1)
    sizes = np.array([w.size for w in waves], np.int64)

    def source(start, stop):
        offs = offsets(sizes[start:stop], total=True)
        part = waves[start:stop]
        on_device = [backend.is_device(w) for w in part]
        if not any(on_device):
            buf = backend.to_device(np.concatenate(part) if len(part) > 1 else part[0], np.float32)
        elif all(on_device):
            buf = DeviceArray((int(offs[-1]),), np.float32)
        else:
            stage = np.zeros(int(offs[-1]), np.float32)
            for w, o, dev in zip(part, offs, on_device):
                if not dev:
                    stage[int(o):int(o) + w.size] = w
            buf = backend.to_device(stage, np.float32)
        backend.copy_many([(buf.flat_view(int(o), w.size), w.reshape(-1)) for w, o, dev in zip(part, offs, on_device) if dev])
        return buf.ptr, offs[:-1], buf

    return sizes, source
