"""Duration-penalised quantisation on the device: the whole code sequence of an utterance chosen at once, for a ragged list
of utterances and several penalties per call (csrc/segmental.h states the rule, csrc/segmental.hip runs it).

    seg = segment_many(encoder, vq, waves, [0.0, 2.0, 8.0])       # SegmentalCodes
    seg = corpus.segment(encoder, vq, 4.0)                        # ... read in place from a ResidentCorpus / CorpusView
    seg = segment_latents(vq, latents, penalties)                 # from (d, tl_i) float32 latents
    seg.codes[p]                                                  # LatentCodes: condition_many, collapse_many, code_stats
    seg.n_segments, seg.cost, seg.distortion, seg.mean_run, seg.segments_per_second(16000)

``encode_many`` reads a codebook frame by frame: the nearest code of every frame.  A frame between two codes flickers, so
the runs are short and the boundaries say little.  Here the code sequence of an utterance minimises the summed squared
distance to the chosen codes PLUS ``penalty`` for every change of code (the penalised dynamic-programming segmentation
used with VQ-VAE speech units): penalty 0 is the float64 nearest neighbour, a growing penalty gives fewer and longer
units down to a single one.  Several penalties share one distance table, so a rate / distortion curve of a snapshot is
one call.  ``codes[p]`` is a LatentCodes like any other: ``condition_many`` re-synthesises from it, ``collapse_many`` gives
the boundaries and ``code_stats(codes[p], collapsed=True)`` the entropy of the units.

What this is not: no per-code or duration-dependent penalty, no band or beam, no backward pass, no parity with any
toolkit.  The reference has no counterpart.

All arithmetic is float64 ``- * + min`` in one written order, so an utterance's codes, segment count and cost are the same
bits alone, in any list, at any position, for any ``chunk_bytes`` and beside any other penalties; tests/segmental_ref.py
restates them in NumPy.

The entry points are declared in csrc/segmental.h, which is not under include/, so they are bound here (table, Structure,
revision check) on first use and not in _lib.HEADERS.
"""
import ctypes as C

import numpy as np

from . import _lib, backend, ragged
from .backend import DeviceArray

_S = backend.stream
MAX_K = 8192                       # VQVAE_SEG_MAX_K
MAX_PEN = 16                       # VQVAE_SEG_MAX_PEN
WAVE_K = 512                       # VQVAE_SEG_WAVE_K
LANES = 256                        # VQVAE_SEG_LANES
TILE = 64                          # VQVAE_SEG_TILE

HEADER = 'segmental.h'             # under csrc/
REVISION = 1
P = _lib.P


class SegDesc(C.Structure):
    _c_name_ = 'vqvae_seg_desc'
    _fields_ = [(n, C.c_int32) for n in ('n', 'd', 'k', 'n_pen')] + \
               [(n, C.c_int64) for n in ('ttot', 'stride', 'code_stride', 'utt_stride')] + [('lam', C.c_double * MAX_PEN)]


_D = C.POINTER(SegDesc)
# the table IS the list of symbols csrc/segmental.h declares (tests/test_host_segmental.py)
PROTOTYPES = {
    'vqvae_seg_revision': (C.c_int, []),
    'vqvae_seg_workspace_bytes': (C.c_size_t, [_D]),
    'vqvae_seg_distances': (C.c_int, [_D, P, P, P, P]),
    'vqvae_seg_segment': (C.c_int, [_D, P, P, P, P, P, P, P, C.c_size_t, P]),
}
STRUCTS = (SegDesc,)

_bound = None


def load():
    """libvqvae_hip.so with this header's entry points bound (once); another revision of the header is an ImportError."""
    global _bound
    if _bound is not None:
        return _bound
    lib = _lib.load()
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)               # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    has = lib.vqvae_seg_revision()
    if has != REVISION:
        raise ImportError('libvqvae_hip.so at %s has segmental revision %d, this package binds %d: rebuild it '
                          '(__graft_entry__.build())' % (_lib.LIB_PATH, has, REVISION))
    _bound = lib
    return lib


def call(name, *args):
    """Calls an int-returning entry point of the header and raises _lib.HipError on failure."""
    _lib.check(getattr(load(), name)(*args), name)


# --------------------------------------------------------------------------- #
# argument checks and the planner
# --------------------------------------------------------------------------- #
def check_penalties(penalties, who='segment_latents'):
    """``penalties`` as a (P,) float64 array: a scalar means P = 1.  Empty, more than MAX_PEN, negative or non-finite
    penalties are a ValueError."""
    try:
        lam = np.asarray(penalties, np.float64)
    except (TypeError, ValueError):
        raise ValueError('%s: penalties must be a number or a list of numbers, got %r' % (who, penalties))
    if lam.ndim > 1:
        raise ValueError('%s: penalties must be a number or a flat list of numbers, got shape %s' % (who, lam.shape))
    lam = lam.reshape(-1)
    if lam.size == 0:
        raise ValueError('%s: the penalty list is empty' % who)
    if lam.size > MAX_PEN:
        raise ValueError('%s: %d penalties in one call; at most MAX_PEN = %d' % (who, lam.size, MAX_PEN))
    bad = np.nonzero(~(np.isfinite(lam) & (lam >= 0)))[0]
    if bad.size:
        raise ValueError('%s: penalty %d is %r; every penalty must be finite and not negative' % (who, bad[0], float(lam[bad[0]])))
    return np.ascontiguousarray(lam)


def _codebook(vq, who):
    from .frontend import _codebook as device_codebook
    W = device_codebook(vq, who)
    if W.dtype != np.float32 or W.ndim != 2:
        raise ValueError('%s: the codebook must be (k, d) float32, got %s %s' % (who, W.dtype, W.shape))
    if W.shape[0] > MAX_K:
        raise ValueError('%s: k = %d codes; at most MAX_K = %d (a lane of the DP workgroup keeps 32 codes in registers)'
                         % (who, W.shape[0], MAX_K))
    return W


def frame_bytes(k, n_pen):
    """Workspace bytes a frame takes: its row of the float64 table, and per penalty its stay-words and its a."""
    return 8 * int(k) + int(n_pen) * (8 * ((int(k) + 63) // 64) + 4)


def plan_runs(tl, per_frame, chunk_bytes):
    """Cuts utterances 0 .. N - 1 greedily, in order, into runs [(start, stop), ...] of whole utterances whose frames take
    at most ``chunk_bytes`` at ``per_frame`` bytes each; an utterance that is too large alone forms its own run."""
    if int(chunk_bytes) < 1:
        raise ValueError('plan_runs: chunk_bytes must be positive, got %r' % (chunk_bytes,))
    tl = np.asarray(tl, np.int64).reshape(-1)
    runs, start, frames = [], 0, 0
    for u in range(tl.size):
        if u > start and (frames + int(tl[u])) * int(per_frame) > int(chunk_bytes):
            runs.append((start, u))
            start, frames = u, 0
        frames += int(tl[u])
    if tl.size > start:
        runs.append((start, tl.size))
    return runs


# --------------------------------------------------------------------------- #
# the result
# --------------------------------------------------------------------------- #
class SegmentalCodes(object):
    """The segmentations of N utterances under P penalties.  ``penalties`` (P,) float64; ``codes[p]`` a LatentCodes over
    row p of ``indices``, ONE (P, total) int32 device buffer; ``n_segments`` (P, N) int32 and ``cost`` (P, N) float64 host
    arrays: the runs of equal codes and the minimised objective, distortion + penalty * (n_segments - 1).  ``tl`` (N,)."""

    def __init__(self, penalties, tl, k, indices, n_segments, cost):
        from .frontend import LatentCodes
        self.penalties = np.asarray(penalties, np.float64)
        self.tl = np.asarray(tl, np.int32)
        self.k = int(k)
        self.indices = indices
        total = int(self.tl.astype(np.int64).sum())
        self.codes = [LatentCodes(self.tl, indices.flat_view(p * total, total), k) for p in range(len(self.penalties))]
        self.n_segments = np.asarray(n_segments, np.int32)
        self.cost = np.asarray(cost, np.float64)

    def __len__(self):
        return len(self.tl)

    @property
    def distortion(self):
        """(P, N) float64: the summed squared distance to the chosen codes, cost - penalty * (n_segments - 1)."""
        return self.cost - self.penalties[:, None] * (self.n_segments - 1).astype(np.float64)

    @property
    def mean_run(self):
        """(P,) float64: frames per segment over the whole list."""
        return float(self.tl.astype(np.int64).sum()) / self.n_segments.astype(np.int64).sum(axis=1).astype(np.float64)

    def segments_per_second(self, sr, hop=64):
        """(P,) float64: segments per second of audio at ``sr`` samples a second and ``hop`` samples a latent frame."""
        seconds = float(self.tl.astype(np.int64).sum()) * float(hop) / float(sr)
        return self.n_segments.astype(np.int64).sum(axis=1).astype(np.float64) / seconds


class _Job(object):
    """The outputs of one public call and the device calls that fill them."""

    def __init__(self, who, W, lam, tl, chunk_bytes):
        self.who, self.W, self.lam = who, W, lam
        self.k, self.d = W.shape
        self.tl = np.asarray(tl, np.int64).reshape(-1)
        self.off = ragged.offsets(self.tl, total=True)
        self.chunk_bytes = int(chunk_bytes)
        if self.chunk_bytes < 1:
            raise ValueError('%s: chunk_bytes must be positive, got %r' % (who, chunk_bytes))
        self.P, self.N, self.total = len(lam), len(self.tl), int(self.off[-1])
        self.codes = DeviceArray((self.P, self.total), np.int32)
        self.n_seg = DeviceArray((self.P, self.N), np.int32)
        self.cost = DeviceArray((self.P, self.N), np.float64)

    def desc(self, first, count, stride):
        d = SegDesc()
        d.n, d.d, d.k, d.n_pen = int(count), self.d, self.k, self.P
        d.ttot = int(self.off[first + count] - self.off[first])
        d.stride, d.code_stride, d.utt_stride = int(stride), self.total, self.N
        for q, v in enumerate(self.lam):
            d.lam[q] = float(v)
        return d

    def call(self, z_ptr, stride, first, count):
        """One device call: utterances [first, first + count) lie end to end from z_ptr, channel rows ``stride`` apart."""
        d = self.desc(first, count, stride)
        need = load().vqvae_seg_workspace_bytes(C.byref(d))
        if need == C.c_size_t(-1).value:
            raise ValueError('%s: the library refuses this description' % self.who)
        ws = backend.workspace(need)
        frame_off = backend.to_device(self.off[first:first + count + 1] - self.off[first])
        call('vqvae_seg_segment', C.byref(d), z_ptr, self.W.ptr, frame_off.ptr, self.codes.ptr + 4 * int(self.off[first]),
             self.n_seg.ptr + 4 * first, self.cost.ptr + 8 * first, ws.ptr, need, _S())

    def chunk(self, z_ptr, stride, first, count):
        """A chunk of the front end: its own sub-runs of whole utterances, so that every call's workspace fits chunk_bytes."""
        for a, b in plan_runs(self.tl[first:first + count], frame_bytes(self.k, self.P), self.chunk_bytes):
            self.call(z_ptr + 4 * int(self.off[first + a] - self.off[first]), stride, first + a, b - a)

    def result(self):
        return SegmentalCodes(self.lam, self.tl, self.k, self.codes, self.n_seg.get(), self.cost.get())


# --------------------------------------------------------------------------- #
# the public calls
# --------------------------------------------------------------------------- #
def _check_latents(latents, d, who):
    latents = list(latents)
    if not latents:
        raise ValueError('%s: no utterances' % who)
    for i, z in enumerate(latents):
        if not backend.is_device(z):
            z = latents[i] = np.asarray(z)
        if z.dtype != np.float32:
            raise ValueError('%s: the latents of utterance %d are %s, float32 needed' % (who, i, z.dtype))
        if len(z.shape) != 2 or z.shape[0] != d:
            raise ValueError('%s: the latents of utterance %d have shape %s; (d, frames) with d = %d needed'
                             % (who, i, tuple(z.shape), d))
        if z.shape[1] < 1:
            raise ValueError('%s: utterance %d has no frames' % (who, i))
    return latents, np.array([z.shape[1] for z in latents], np.int64)


def _gather(part, d, T):
    """The (d, T) float32 device array of a run of latents laid end to end along the frame axis."""
    if not any(backend.is_device(z) for z in part):
        return backend.to_device(np.concatenate(part, axis=1) if len(part) > 1 else np.ascontiguousarray(part[0]), np.float32)
    buf = DeviceArray((d, T), np.float32)
    pairs, at, keep = [], 0, []
    for z in part:
        if not backend.is_device(z):
            z = backend.to_device(np.ascontiguousarray(z), np.float32)
            keep.append(z)
        n = z.shape[1]
        pairs += [(buf.flat_view(ch * T + at, n), z.flat_view(ch * n, n)) for ch in range(d)]
        at += n
    backend.copy_many(pairs)
    return buf


def segment_latents(vq, latents, penalties, chunk_bytes=1 << 30):
    """The segmentations of a list of latents -- host or device float32 arrays (d, tl_i), the encoder's output as
    ``encode_many(return_latents=True)`` hands it back -- under every penalty: a SegmentalCodes.  ``penalties``: a number
    or up to MAX_PEN of them, finite and not negative.  A run of utterances whose latents, table and stay-words fit
    ``chunk_bytes`` is one upload and two launches; the result does not depend on ``chunk_bytes``."""
    who = 'segment_latents'
    lam = check_penalties(penalties, who)
    W = _codebook(vq, who)
    latents, tl = _check_latents(latents, W.shape[1], who)
    job = _Job(who, W, lam, tl, chunk_bytes)
    for a, b in plan_runs(tl, frame_bytes(job.k, job.P) + 4 * job.d, job.chunk_bytes):
        T = int(job.off[b] - job.off[a])
        z = _gather(latents[a:b], job.d, T)
        job.call(z.ptr, T, a, b - a)
        del z
    return job.result()


def distance_table(vq, latents):
    """Step 1 of the rule alone, for analysis and tests: the float64 table of every utterance, a list of host arrays
    (tl_i, k), from one launch."""
    who = 'distance_table'
    W = _codebook(vq, who)
    latents, tl = _check_latents(latents, W.shape[1], who)
    job_off = ragged.offsets(tl, total=True)
    T = int(job_off[-1])
    z = _gather(latents, W.shape[1], T)
    d = SegDesc()
    d.n, d.d, d.k, d.n_pen = len(tl), W.shape[1], W.shape[0], 1
    d.ttot = d.stride = d.code_stride = T
    d.utt_stride = len(tl)
    table = DeviceArray((T, W.shape[0]), np.float64)
    call('vqvae_seg_distances', C.byref(d), z.ptr, W.ptr, table.ptr, _S())
    return ragged.split(table.get(), job_off, axis=0)


def _from_waves(who, encoder, vq, lengths, source, penalties, chunk_bytes):
    from . import frontend
    lam = check_penalties(penalties, who)
    W = _codebook(vq, who)
    enc = frontend._encoder_params(encoder, who)
    if enc[-1][0].shape[0] != W.shape[1]:
        raise ValueError('%s: the encoder writes %d channels, the codebook has d = %d' % (who, enc[-1][0].shape[0], W.shape[1]))
    lengths, tl = frontend._wave_lengths(lengths, len(enc), who)
    job = _Job(who, W, lam, tl, chunk_bytes)
    frontend._run(who, encoder, vq, None, lengths, source, None, chunk_bytes,
                  hook=lambda z_ptr, stride, tb, first: job.chunk(z_ptr, stride, first, tb.n))
    return job.result()


def segment_many(encoder, vq, waves, penalties, chunk_bytes=1 << 30):
    """``segment_latents`` from waveforms: the ragged encoder of ``encode_many`` (same arguments, same chunks) and, on
    every chunk's z while it is still on the device, the table and the DP in sub-runs of whole utterances that fit
    ``chunk_bytes``.  Nothing but the codes, segment counts and costs comes back."""
    check_penalties(penalties, 'segment_many')
    sizes, source = ragged.wave_source(waves, 'segment_many')
    return _from_waves('segment_many', encoder, vq, sizes, source, penalties, chunk_bytes)


def segment_corpus(corpus, encoder, vq, penalties, chunk_bytes=1 << 30):
    """``ResidentCorpus.segment`` / ``CorpusView.segment``: the utterances are read in place from the corpus buffer."""
    check_penalties(penalties, 'segment')
    lengths, source = ragged.wave_source(corpus, 'segment')
    return _from_waves('segment', encoder, vq, lengths, source, penalties, chunk_bytes)
