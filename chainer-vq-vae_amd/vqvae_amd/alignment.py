"""Time-aligned metrics on the device: dynamic time warping over mel-cepstra for a ragged list of utterance pairs
(include/vqvae_align.h states the rule, csrc/audio_align.hip runs it).

    fa = features_many(targets, cfg)                   # the target speaker's own recordings of the sentences
    fb = features_many(converted, cfg)                 # the converted utterances: other lengths, other timing
    al = align_many(fa, fb)                            # Alignment: mcd_dtw_db, log_mel_mae_dtw, cost, path_len, ...
    ia, ib = al.utterance(3)                           # the warping path of pair 3, ascending from (0, 0)
    al = compare_aligned_many(targets, converted, cfg) # both steps over waves; takes what compare_many takes

Pair i aligns the Fa_i frames of utterance i of ``a`` with the Fb_i frames of utterance i of ``b``; nothing is cut to a
common length.  The local cost of a frame pair is the mel-cepstral distortion of metrics.compare_many (coefficients
1 .. n_mcep, dB); the warp is the plain symmetric one (steps (1, 1), (1, 0), (0, 1), no slope weights, no band), ties to the
diagonal, then to the step along ``a``.  ``mcd_dtw_db`` is the path's cost over its length, the figure usually quoted as
MCD-DTW; NO parity with any toolkit is claimed.

Everything is float64 in one written order, so a pair's results are the same bits alone, in any list, at any position and
for any ``chunk_bytes``; tests/alignment_ref.py restates the rule in NumPy and the device is held to every bit of it.
"""
import ctypes as C

import numpy as np

from . import _lib, backend, ragged
from .backend import DeviceArray
from .metrics import MelConfig, RaggedFeatures, _frames, features_many, tables

_S = backend.stream
MAX_SHORT = _lib.ALIGN_MAX_SHORT   # min(Fa, Fb) of a pair
MAX_MELS = _lib.ALIGN_MAX_MELS
THREADS = _lib.ALIGN_THREADS
REDUCE_LANES = _lib.ALIGN_REDUCE_LANES
MAX_CELLS = 1 << 31                # the direction table of ONE pair


# --------------------------------------------------------------------------- #
# the host side of the rule
# --------------------------------------------------------------------------- #
def check_pairs(frames_a, frames_b, who='align_many'):
    """(Fa, Fb) as int64 (N,) arrays; the refusals, each a ValueError naming the pair: another count on the two sides, a
    shorter side above MAX_SHORT, a direction table above 2^31 cells."""
    fa = np.asarray(frames_a, np.int64).reshape(-1)
    fb = np.asarray(frames_b, np.int64).reshape(-1)
    if fa.size != fb.size:
        raise ValueError('%s: %d utterances on side a and %d on side b' % (who, fa.size, fb.size))
    if fa.size == 0:
        raise ValueError('%s: no utterances' % who)
    empty = np.nonzero((fa < 1) | (fb < 1))[0]
    if empty.size:
        u = int(empty[0])
        raise ValueError('%s: pair %d has %d and %d frames: every side needs one' % (who, u, fa[u], fb[u]))
    long_ = np.nonzero(np.minimum(fa, fb) > MAX_SHORT)[0]
    if long_.size:
        u = int(long_[0])
        raise ValueError('%s: pair %d has %d and %d frames; the shorter side may have at most %d (three anti-diagonals of '
                         'the pair are kept in the 160 KB of LDS of a compute unit)' % (who, u, fa[u], fb[u], MAX_SHORT))
    big = np.nonzero(fa * fb > MAX_CELLS)[0]
    if big.size:
        u = int(big[0])
        raise ValueError('%s: pair %d has %d x %d = %d cells; the direction table of one pair may have at most 2^31'
                         % (who, u, fa[u], fb[u], fa[u] * fb[u]))
    return fa, fb


def plan_chunks(frames_a, frames_b, chunk_bytes, who='align_many'):
    """Runs [(start, stop), ...] of consecutive pairs whose direction tables -- one byte per cell, Fa_i * Fb_i cells --
    stay within ``chunk_bytes`` together (ragged.plan_runs, which counts float32 elements: four cells each); a pair over
    the budget stands alone."""
    if int(chunk_bytes) < 1:
        raise ValueError('%s: chunk_bytes must be positive, got %r' % (who, chunk_bytes))
    fa, fb = check_pairs(frames_a, frames_b, who)
    return ragged.plan_runs((-(-(fa * fb) // 4))[None], chunk_bytes)


class Alignment(object):
    """Per pair, in the caller's order: float64 (N,) ``mcd_dtw_db`` (cost / path_len), ``log_mel_mae_dtw`` (mean absolute
    log-mel difference along the path, nepers of power) and ``cost`` (the path's summed distortion, dB); int64 (N,)
    ``path_len``, ``diagonal_steps``, ``frames_a``, ``frames_b``.  With paths: ``ia`` and ``ib``, device int32 arrays laid
    end to end by the host table ``path_off`` (N + 1,), pair i owning Fa_i + Fb_i - 1 positions of which the first
    path_len[i] are written."""

    def __init__(self, mcd_dtw_db, log_mel_mae_dtw, cost, path_len, diagonal_steps, frames_a, frames_b, ia=None, ib=None,
                 path_off=None):
        self.mcd_dtw_db, self.log_mel_mae_dtw, self.cost = mcd_dtw_db, log_mel_mae_dtw, cost
        self.path_len, self.diagonal_steps, self.frames_a, self.frames_b = path_len, diagonal_steps, frames_a, frames_b
        self.ia, self.ib, self.path_off = ia, ib, path_off
        self._host = None

    def __len__(self):
        return len(self.cost)

    def utterance(self, i):
        """The path of pair i as host int32 arrays (ia, ib) of length path_len[i], ascending from (0, 0) to
        (Fa - 1, Fb - 1): frame ia[k] of ``a`` is aligned with frame ib[k] of ``b``.  The first call copies the whole
        arrays back once."""
        i = int(i)
        if not 0 <= i < len(self.cost):
            raise IndexError('Alignment.utterance: pair %d of %d' % (i, len(self.cost)))
        if self.ia is None:
            raise ValueError('Alignment.utterance: the alignment was computed without paths=True')
        if self._host is None:
            self._host = (self.ia.get(), self.ib.get())
        at, K = int(self.path_off[i]), int(self.path_len[i])
        return self._host[0][at:at + K].copy(), self._host[1][at:at + K].copy()


class _Tables(object):
    """off_a, off_b, cell_off, path_off (n + 1 each) as int64 on the device, uploaded in one copy."""

    def __init__(self, fa, fb):
        n = len(fa)
        self.off_a, self.off_b = ragged.offsets(fa, total=True), ragged.offsets(fb, total=True)
        self.cell_off, self.path_off = ragged.offsets(fa * fb, total=True), ragged.offsets(fa + fb - 1, total=True)
        self.dev = backend.to_device(np.concatenate([self.off_a, self.off_b, self.cell_off, self.path_off]))
        p, step = self.dev.ptr, 8 * (n + 1)
        self.c = _lib.AlignTables(p, p + step, p + 2 * step, p + 3 * step)


def _desc(cfg, fa, fb, stride_a, stride_b):
    return _lib.AlignDesc(len(fa), cfg.n_mels, cfg.n_mcep, int(np.minimum(fa, fb).max()), int(fa.sum()), int(fb.sum()),
                          int(stride_a), int(stride_b), int((fa * fb).sum()), int((fa + fb - 1).sum()))


def _workspace(query, d, who):
    """The bytes a size query asks for; align_many sizes ONE scratch from three of them, so nothing is allocated here."""
    need = getattr(_lib.load(), query)(C.byref(d))
    if need == C.c_size_t(-1).value:
        raise ValueError('%s: the library refuses this description' % who)
    return need


# --------------------------------------------------------------------------- #
# the public calls
# --------------------------------------------------------------------------- #
def align_many(feats_a, feats_b, paths=True, chunk_bytes=1 << 30):
    """Aligns utterance i of ``feats_a`` with utterance i of ``feats_b`` (metrics.RaggedFeatures from features_many, of
    the same MelConfig and the same N) and returns an Alignment.  ``paths``: keep the warping paths on the device.  The
    pairs are cut into chunks whose direction tables (a byte per cell) stay within ``chunk_bytes``; the result does not
    depend on it.  A pair whose shorter side exceeds MAX_SHORT frames, or whose Fa * Fb exceeds 2^31, is a ValueError
    naming it, raised before any device call."""
    who = 'align_many'
    for name, f in (('feats_a', feats_a), ('feats_b', feats_b)):
        if not isinstance(f, RaggedFeatures):
            raise TypeError('%s: %s must be a metrics.RaggedFeatures (features_many), got %r' % (who, name, type(f)))
    cfg = feats_a.cfg
    if cfg.key() != feats_b.cfg.key():
        raise ValueError('%s: the two sides were analysed differently: %r against %r' % (who, cfg, feats_b.cfg))
    if cfg.n_mels > MAX_MELS:
        raise ValueError('%s: n_mels must be at most %d, got %d' % (who, MAX_MELS, cfg.n_mels))
    chunks = plan_chunks(feats_a.frames, feats_b.frames, chunk_bytes, who)
    fa, fb = feats_a.frames.astype(np.int64), feats_b.frames.astype(np.int64)
    N = len(fa)
    if feats_a.log_mel is None or feats_b.log_mel is None:
        raise ValueError('%s: the features are a description only (nothing on the device)' % who)
    dct = backend.to_device(tables(cfg)[2])
    stride_a, stride_b = int(feats_a.frame_off[-1]), int(feats_b.frame_off[-1])
    path_off = ragged.offsets(fa + fb - 1, total=True)
    cost = DeviceArray((N,), np.float64)
    klen = DeviceArray((N,), np.int32)
    diag = DeviceArray((N,), np.int32)
    scores = DeviceArray((N, 2), np.float64)
    ia = DeviceArray((int(path_off[-1]),), np.int32) if paths else None
    ib = DeviceArray((int(path_off[-1]),), np.int32) if paths else None
    Q = cfg.n_mcep
    most_a = max(int(fa[a:b].sum()) for a, b in chunks)
    most_b = max(int(fb[a:b].sum()) for a, b in chunks)
    ca, cb = DeviceArray((most_a * Q,), np.float64), DeviceArray((most_b * Q,), np.float64)
    for start, stop in chunks:
        ta = _Tables(fa[start:stop], fb[start:stop])
        d = _desc(cfg, fa[start:stop], fb[start:stop], stride_a, stride_b)
        db, tc = C.byref(d), C.byref(ta.c)
        la = feats_a.log_mel.ptr + 4 * int(feats_a.frame_off[start])
        lb = feats_b.log_mel.ptr + 4 * int(feats_b.frame_off[start])
        need_c = _workspace('vqvae_align_cepstra_workspace_bytes', d, who)
        need_d = _workspace('vqvae_align_dtw_workspace_bytes', d, who)
        need_p = _workspace('vqvae_align_path_workspace_bytes', d, who) if not paths else 0
        ws = backend.workspace(max(need_c, need_d + need_p, 256))       # the direction table, then the path scratch
        _lib.call('vqvae_align_cepstra', db, 0, la, dct.ptr, ca.ptr, ws.ptr, need_c, _S())
        _lib.call('vqvae_align_cepstra', db, 1, lb, dct.ptr, cb.ptr, ws.ptr, need_c, _S())
        _lib.call('vqvae_align_dtw', db, tc, ca.ptr, cb.ptr, cost.ptr + 8 * start, klen.ptr + 4 * start, diag.ptr + 4 * start,
                  ws.ptr, need_d, _S())
        at = 4 * int(path_off[start])
        _lib.call('vqvae_align_path', db, tc, ws.ptr, cost.ptr + 8 * start, klen.ptr + 4 * start, la, lb,
                  None if ia is None else ia.ptr + at, None if ib is None else ib.ptr + at, scores.ptr + 16 * start,
                  ws.ptr + need_d, need_p, _S())
        del ta
    sc = scores.get()
    return Alignment(sc[:, 0].copy(), sc[:, 1].copy(), cost.get(), klen.get().astype(np.int64), diag.get().astype(np.int64),
                     fa.copy(), fb.copy(), ia, ib, path_off if paths else None)


def compare_aligned_many(reference, test, cfg, paths=False, chunk_bytes=1 << 30):
    """``features_many`` on both sides, then ``align_many``: the time-aligned counterpart of metrics.compare_many for a
    parallel corpus (the same sentences, other lengths and timing).  Both arguments take what ``features_many`` takes --
    host or device lists, a ResidentCorpus / CorpusView read in place; every wave is taken whole."""
    if not isinstance(cfg, MelConfig):
        raise TypeError('compare_aligned_many: cfg must be a MelConfig, got %r' % (type(cfg),))
    len_a, _ = ragged.wave_source(reference, 'compare_aligned_many')
    len_b, _ = ragged.wave_source(test, 'compare_aligned_many')
    if len(len_a) != len(len_b):
        raise ValueError('compare_aligned_many: %d reference and %d test utterances' % (len(len_a), len(len_b)))
    check_pairs(_frames(len_a, cfg, 'compare_aligned_many'), _frames(len_b, cfg, 'compare_aligned_many'), 'compare_aligned_many')
    fa = features_many(reference, cfg, chunk_bytes=chunk_bytes)
    fb = features_many(test, cfg, chunk_bytes=chunk_bytes)
    return align_many(fa, fb, paths, chunk_bytes)
