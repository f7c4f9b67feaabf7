"""Objective audio metrics on the device (include/vqvae_metrics.h, csrc/audio_metrics.hip): a short-time Fourier transform,
log-mel features and three per-utterance distances over a ragged list of waveforms, without taking a wave to the host.

    waves = synthesize_many(encoder, vq, decoder, condition_embed, inputs, speakers)      # T samples for an input of T + 1
    scores = compare_many(inputs, waves, MelConfig())         # reference first; both are cut to their common length
    scores['log_mel_mae'], scores['mcd_db'], scores['spectral_convergence']               # float64 (N,) each
    feats = features_many(corpus, MelConfig(), magnitudes=True)     # a ResidentCorpus / CorpusView is read in place

One STFT resolution, no centring or padding (an utterance of L samples has 1 + (L - n_fft) // hop frames and the samples
behind the last frame belong to none), no time alignment.  The window, the mel filter bank and the cepstral transform are
tables built here in float64, rounded once to float32 and handed to the kernels as inputs (``tables``).  The mel bank is
the Slaney-scale bank of area-normalised triangles (each scaled by 2 / (f[m + 2] - f[m])) -- librosa's defaults as
recalled, written from the formulas; NO parity with librosa or any other toolkit is claimed or tested.

The arithmetic is composition-independent (see the header): a frame's features are a pure function of its own n_fft
samples and the tables, the same bits alone, in any list, at any position and for any ``chunk_bytes``.
"""
import ctypes as C

import numpy as np

from . import _lib, backend, ragged
from .backend import DeviceArray

_S = backend.stream
_TABLE_CACHE = {}


class MelConfig(object):
    """The analysis: sample rate, frame length and hop, mel bands between fmin and fmax (None: sr / 2), cepstral
    coefficients 1 .. n_mcep of the distortion, and the smallest mel power the log is taken of.  Anything outside the
    documented ranges is a ValueError here, before any device call."""

    def __init__(self, sr=16000, n_fft=1024, hop=256, n_mels=80, fmin=0.0, fmax=None, n_mcep=13, floor=1e-10):
        for name, v in (('sr', sr), ('n_fft', n_fft), ('hop', hop), ('n_mels', n_mels), ('n_mcep', n_mcep)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError('MelConfig: %s must be an integer, got %r' % (name, v))
        if sr < 1:
            raise ValueError('MelConfig: sr must be positive, got %r' % (sr,))
        if n_fft % 32 or not 32 <= n_fft <= _lib.METRICS_MAX_NFFT:
            raise ValueError('MelConfig: n_fft must be a multiple of 32 in [32, %d], got %r' % (_lib.METRICS_MAX_NFFT, n_fft))
        if not 1 <= hop <= n_fft:
            raise ValueError('MelConfig: hop must be in [1, n_fft = %d], got %r' % (n_fft, hop))
        if not 1 <= n_mels <= _lib.METRICS_MAX_MELS:
            raise ValueError('MelConfig: n_mels must be in [1, %d], got %r' % (_lib.METRICS_MAX_MELS, n_mels))
        if not 1 <= n_mcep < n_mels:
            raise ValueError('MelConfig: n_mcep must be in [1, n_mels = %d), got %r' % (n_mels, n_mcep))
        floor = float(floor)
        if not floor > 0 or not np.isfinite(floor) or not np.float32(floor) > 0:
            raise ValueError('MelConfig: floor must be a positive float32, got %r' % (floor,))
        fmin = float(fmin)
        fmax = sr / 2.0 if fmax is None else float(fmax)
        if not 0 <= fmin < fmax <= sr / 2.0:
            raise ValueError('MelConfig: 0 <= fmin < fmax <= sr / 2 needed, got fmin = %r, fmax = %r' % (fmin, fmax))
        self.sr, self.n_fft, self.hop, self.n_mels, self.n_mcep = int(sr), int(n_fft), int(hop), int(n_mels), int(n_mcep)
        self.fmin, self.fmax, self.floor = fmin, fmax, floor

    @property
    def nb(self):
        return self.n_fft // 2 + 1

    def key(self):
        return (self.sr, self.n_fft, self.hop, self.n_mels, self.fmin, self.fmax, self.n_mcep, self.floor)

    def __repr__(self):
        return 'MelConfig(sr=%d, n_fft=%d, hop=%d, n_mels=%d, fmin=%r, fmax=%r, n_mcep=%d, floor=%r)' % self.key()


def frame_count(length, cfg):
    """Frames of an utterance of ``length`` samples: 1 + (length - n_fft) // hop; 0 below n_fft."""
    length = np.asarray(length, np.int64)
    return np.where(length >= cfg.n_fft, 1 + (length - cfg.n_fft) // cfg.hop, 0)


def _hz_to_mel(f):
    f = np.asarray(f, np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    logstep = np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def tables(cfg):
    """The three input tables of the kernels as host float32 arrays, built in float64 and rounded once:
    ``dft`` (2 * nb, n_fft): row b is w[k] cos(2 pi b k / n_fft), row nb + b is -w[k] sin(2 pi b k / n_fft), w the periodic
    Hann window divided by its sum (so |re|, |im| <= max |x|);
    ``mel`` (n_mels, nb): Slaney-scale triangles, each normalised by 2 / (f[m + 2] - f[m]) (librosa's defaults as recalled;
    no parity is claimed) -- a configuration that leaves a mel row all zero is a ValueError naming the row;
    ``dct`` (n_mcep, n_mels): rows 1 .. n_mcep of the orthonormal DCT-II (c0 is left out)."""
    hit = _TABLE_CACHE.get(cfg.key())
    if hit is not None:
        return hit
    n, nb = cfg.n_fft, cfg.nb
    k = np.arange(n, dtype=np.int64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * k / n)
    w /= w.sum()
    ang = 2.0 * np.pi * ((np.arange(nb, dtype=np.int64)[:, None] * k[None, :]) % n) / n     # the angle reduced exactly
    dft = np.concatenate([w * np.cos(ang), -w * np.sin(ang)]).astype(np.float32)

    edges = _mel_to_hz(np.linspace(_hz_to_mel(cfg.fmin), _hz_to_mel(cfg.fmax), cfg.n_mels + 2))
    freqs = np.linspace(0.0, cfg.sr / 2.0, nb)
    ramps = edges[:, None] - freqs[None, :]
    width = np.diff(edges)
    lower = -ramps[:-2] / width[:-1, None]
    upper = ramps[2:] / width[1:, None]
    mel = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (edges[2:] - edges[:-2]))[:, None]
    mel = mel.astype(np.float32)
    empty = np.nonzero(~(mel != 0).any(axis=1))[0]
    if empty.size:
        raise ValueError('MelConfig: mel row %d is all zero at n_fft = %d, n_mels = %d (%.1f .. %.1f Hz holds no bin of %.2f Hz '
                         'spacing): fewer mel bands or a longer frame' % (empty[0], n, cfg.n_mels, edges[empty[0]],
                                                                         edges[empty[0] + 2], cfg.sr / float(n)))

    M = cfg.n_mels
    q = np.arange(1, cfg.n_mcep + 1, dtype=np.float64)[:, None]
    dct = (np.sqrt(2.0 / M) * np.cos(np.pi * q * (2.0 * np.arange(M)[None, :] + 1.0) / (2.0 * M))).astype(np.float32)
    out = (dft, mel, dct)
    for t in out:
        t.setflags(write=False)
    _TABLE_CACHE[cfg.key()] = out
    return out


def plan_chunks(frames, width, chunk_bytes):
    """Cuts utterances 0 .. N - 1 greedily, in input order, into runs [(start, stop), ...]: a run is closed when the next
    utterance would take its ``4 * width * frames`` bytes over ``chunk_bytes``; an utterance over the budget stands alone.
    ``width``: float32 values kept per frame (nb for the magnitudes, the largest term)."""
    frames = np.asarray(frames, np.int64).reshape(-1)
    if int(width) < 1 or int(chunk_bytes) < 1:
        raise ValueError('plan_chunks: width and chunk_bytes must be positive, got %r and %r' % (width, chunk_bytes))
    return ragged.plan_runs((int(width) * frames)[None], chunk_bytes)


def _frames(lengths, cfg, who):
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    if lengths.size == 0:
        raise ValueError('%s: no utterances' % who)
    short = np.nonzero(lengths < cfg.n_fft)[0]
    if short.size:
        raise ValueError('%s: utterance %d has %d samples, fewer than one frame (n_fft = %d)'
                         % (who, short[0], lengths[short[0]], cfg.n_fft))
    return frame_count(lengths, cfg).astype(np.int64)


def _desc(cfg, n, ftot, stride):
    d = _lib.MetricsDesc()
    d.n, d.n_fft, d.hop, d.n_mels, d.n_mcep, d.floor = int(n), cfg.n_fft, cfg.hop, cfg.n_mels, cfg.n_mcep, cfg.floor
    d.ftot, d.stride = int(ftot), int(stride)
    return d


def _stft_mel(cfg, tabs, x_ptr, off_in, frames, log_mel_ptr, mag_ptr, stride, mel_ptr=None):
    """One launch over a run of utterances; returns the device frame_off table (kept by the caller while it is read)."""
    frame_off = ragged.offsets(frames, total=True)
    seg = backend.to_device(np.concatenate([np.ascontiguousarray(off_in, np.int64).reshape(-1), frame_off]))
    d = _desc(cfg, len(frames), frame_off[-1], stride)
    ws, need = backend.described_workspace('vqvae_metrics_stft_mel_workspace_bytes', d, 'features_many')
    _lib.call('vqvae_metrics_stft_mel', C.byref(d), x_ptr, seg.ptr, seg.ptr + 8 * len(frames), tabs[0].ptr, tabs[1].ptr,
              log_mel_ptr, mag_ptr, mel_ptr, ws, need, _S())
    return seg


class RaggedFeatures(object):
    """The features of N utterances laid end to end along the frame axis: ``frame_off`` host int64 (N + 1,) with utterance i
    at frames [frame_off[i], frame_off[i + 1]), ``frames`` (N,), ``log_mel`` one channel-major (n_mels, Ftot) float32
    device tensor, ``mag`` (nb, Ftot) or None, ``mel`` the mel powers before floor and log, (n_mels, Ftot), or None."""

    def __init__(self, cfg, frames, log_mel, mag, mel=None):
        self.cfg = cfg
        self.frames = np.asarray(frames, np.int64)
        self.frame_off = ragged.offsets(self.frames, total=True)
        self.log_mel, self.mag, self.mel = log_mel, mag, mel
        self._host = None

    def __len__(self):
        return len(self.frames)

    def utterance(self, i):
        """Host copies of utterance i's blocks: (log_mel (n_mels, F_i), mag (nb, F_i) or None), with ``mel_powers`` a
        third, mel (n_mels, F_i).  The first call copies the whole tensors back once."""
        i = int(i)
        if not 0 <= i < len(self.frames):
            raise IndexError('RaggedFeatures.utterance: utterance %d of %d' % (i, len(self.frames)))
        if self._host is None:
            self._host = [None if t is None else t.get() for t in (self.log_mel, self.mag, self.mel)]
        blocks = tuple(None if t is None else ragged.split(t, self.frame_off[i:i + 2])[0] for t in self._host)
        return blocks if self.mel is not None else blocks[:2]


# --------------------------------------------------------------------------- #
# the public calls
# --------------------------------------------------------------------------- #
def features_many(waves, cfg, magnitudes=False, chunk_bytes=1 << 30, mel_powers=False):
    """Log-mel features (with ``magnitudes`` the STFT magnitudes, with ``mel_powers`` the mel powers the log was taken
    of) of many utterances, one launch per chunk.
    ``waves``: a list of host or device float32 arrays, each taken whole, or a ResidentCorpus / CorpusView, which is read
    in place through its offsets.  Host waves are uploaded with one copy per chunk of at most ``chunk_bytes`` of the
    largest output; the result does not depend on ``chunk_bytes``.  An utterance shorter than n_fft is a ValueError
    naming it."""
    if not isinstance(cfg, MelConfig):
        raise TypeError('features_many: cfg must be a MelConfig, got %r' % (type(cfg),))
    host_tabs = tables(cfg)
    lengths, source = ragged.wave_source(waves, 'features_many')
    frames = _frames(lengths, cfg, 'features_many')
    chunks = plan_chunks(frames, cfg.nb if magnitudes else cfg.n_mels, chunk_bytes)
    feats = RaggedFeatures(cfg, frames, None, None)
    ftot = int(feats.frame_off[-1])
    tabs = [backend.to_device(t) for t in host_tabs[:2]]
    feats.log_mel = DeviceArray((cfg.n_mels, ftot), np.float32)
    feats.mag = DeviceArray((cfg.nb, ftot), np.float32) if magnitudes else None
    feats.mel = DeviceArray((cfg.n_mels, ftot), np.float32) if mel_powers else None
    for start, stop in chunks:
        x_ptr, off_in, keep = source(start, stop)
        at = 4 * int(feats.frame_off[start])
        seg = _stft_mel(cfg, tabs, x_ptr, off_in, frames[start:stop], feats.log_mel.ptr + at,
                        None if feats.mag is None else feats.mag.ptr + at, ftot,
                        None if feats.mel is None else feats.mel.ptr + at)
        del keep, seg
    return feats


def compare_many(reference, test, cfg, chunk_bytes=1 << 30):
    """The three distances of every (reference, test) pair: ``log_mel_mae`` (mean absolute difference of the log-mel
    powers, in nepers of power), ``mcd_db`` (mel-cepstral distortion over coefficients 1 .. n_mcep, dB) and
    ``spectral_convergence`` (Frobenius norm of the magnitude difference over that of the reference), float64 (N,) each,
    and ``frames`` int64 (N,).  Both arguments take what ``features_many`` takes.  The two waves of a pair are cut to their
    common length before framing (synthesize_many returns T samples for an input of T + 1); there is no time alignment.
    A silent reference divides as IEEE divides: spectral_convergence is inf, or nan when the test is silent too.  Lists
    of different length, or a pair whose common length is below n_fft, are a ValueError."""
    if not isinstance(cfg, MelConfig):
        raise TypeError('compare_many: cfg must be a MelConfig, got %r' % (type(cfg),))
    host_tabs = tables(cfg)
    len_a, src_a = ragged.wave_source(reference, 'compare_many')
    len_b, src_b = ragged.wave_source(test, 'compare_many')
    if len(len_a) != len(len_b):
        raise ValueError('compare_many: %d reference and %d test utterances' % (len(len_a), len(len_b)))
    frames = _frames(np.minimum(len_a, len_b), cfg, 'compare_many')
    N = len(frames)
    chunks = plan_chunks(frames, 2 * (cfg.nb + cfg.n_mels), chunk_bytes)
    tabs = [backend.to_device(t) for t in host_tabs]
    out = DeviceArray((N, 3), np.float64)
    most = max(int(frames[a:b].sum()) for a, b in chunks)
    lm = [DeviceArray((cfg.n_mels * most,), np.float32) for _ in range(2)]
    mg = [DeviceArray((cfg.nb * most,), np.float32) for _ in range(2)]
    for start, stop in chunks:
        fr = frames[start:stop]
        ftot = int(fr.sum())
        for side, src in enumerate((src_a, src_b)):
            x_ptr, off_in, keep = src(start, stop)
            seg = _stft_mel(cfg, tabs, x_ptr, off_in, fr, lm[side].ptr, mg[side].ptr, ftot)
            del keep
        d = _desc(cfg, stop - start, ftot, ftot)
        ws, need = backend.described_workspace('vqvae_metrics_distances_workspace_bytes', d, 'compare_many')
        _lib.call('vqvae_metrics_distances', C.byref(d), lm[0].ptr, lm[1].ptr, mg[0].ptr, mg[1].ptr, tabs[2].ptr,
                  seg.ptr + 8 * (stop - start), out.ptr + 24 * start, ws, need, _S())
        del seg
    res = out.get()
    return {'log_mel_mae': res[:, 0].copy(), 'mcd_db': res[:, 1].copy(), 'spectral_convergence': res[:, 2].copy(),
            'frames': frames.copy()}
