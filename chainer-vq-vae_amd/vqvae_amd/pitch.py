"""Pitch and voicing on the device (include/vqvae_pitch.h, csrc/audio_pitch.hip): a per-frame YIN F0 estimator over a
ragged list of waveforms and the per-pair pitch statistics, without taking a wave to the host.

    waves = synthesize_many(encoder, vq, decoder, condition_embed, inputs, speakers)      # T samples for an input of T + 1
    scores = compare_pitch_many(inputs, waves, PitchConfig())   # reference first; both are cut to their common length
    scores['vuv_error'], scores['f0_rmse_cents'], scores['log_f0_mean_test'] - scores['log_f0_mean_ref']
    track = pitch_many(corpus, PitchConfig())                   # a ResidentCorpus / CorpusView is read in place
    f0, aperiodicity = track.utterance(3)                       # host float32 (F_3,) each; f0 == 0 is unvoiced

One frame length, no centring or padding (metrics.frame_count's rule: with frame = n_fft and the same hop, pitch frames
and mel frames coincide), no temporal smoothing, no octave correction, no time alignment.  The rule is the header's; it
is stated so that a float64 NumPy restatement equals the device in every bit, and a frame's result is a pure function of
its own samples: the same bits alone, in any list, at any position and for any ``chunk_bytes``.
"""
import ctypes as C
import math

import numpy as np

from . import _lib, backend, ragged
from .backend import DeviceArray

_S = backend.stream
COLUMNS = ('voiced_ref', 'voiced_test', 'voiced_both', 'vuv_error', 'gross_error', 'f0_rmse_cents', 'log_f0_mean_ref',
           'log_f0_mean_test')


class PitchConfig(object):
    """The analysis: sample rate, frame length and hop, the pitch range looked for, the YIN threshold and the mean power
    below which a frame is unvoiced.  ``tau_min = floor(sr / fmax)``, ``tau_max = ceil(sr / fmin)``, ``W = frame - tau_max``
    (the terms of a difference).  Anything outside the documented ranges is a ValueError here, before any device call."""

    def __init__(self, sr=16000, frame=1024, hop=256, fmin=60.0, fmax=400.0, threshold=0.15, min_power=1e-8):
        for name, v in (('sr', sr), ('frame', frame), ('hop', hop)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError('PitchConfig: %s must be an integer, got %r' % (name, v))
        if not 1 <= sr <= 2 ** 31 - 1:
            raise ValueError('PitchConfig: sr must be positive, got %r' % (sr,))
        if not 1 <= frame <= _lib.PITCH_MAX_FRAME:
            raise ValueError('PitchConfig: frame must be in [1, %d], got %r' % (_lib.PITCH_MAX_FRAME, frame))
        if not 1 <= hop <= frame:
            raise ValueError('PitchConfig: hop must be in [1, frame = %d], got %r' % (frame, hop))
        fmin, fmax, threshold, min_power = float(fmin), float(fmax), float(threshold), float(min_power)
        if not (0 < fmin and np.isfinite(fmin) and 0 < fmax and np.isfinite(fmax)):
            raise ValueError('PitchConfig: fmin and fmax must be positive and finite, got fmin = %r, fmax = %r' % (fmin, fmax))
        if not 0 < threshold < 1:
            raise ValueError('PitchConfig: threshold must be in (0, 1), got %r' % (threshold,))
        if not (min_power >= 0 and np.isfinite(min_power)):
            raise ValueError('PitchConfig: min_power must be finite and not negative, got %r' % (min_power,))
        lo, hi = math.floor(sr / fmax), math.ceil(sr / fmin)
        if not 2 <= lo < hi:
            raise ValueError('PitchConfig: 2 <= tau_min = floor(sr / fmax) < tau_max = ceil(sr / fmin) needed, got tau_min = %d, '
                             'tau_max = %d (sr = %d, fmin = %r, fmax = %r)' % (lo, hi, sr, fmin, fmax))
        if frame - hi < 2:
            raise ValueError('PitchConfig: W = frame - tau_max must be at least 2, got frame = %d, tau_max = %d (fmin = %r): '
                             'a longer frame or a higher fmin' % (frame, hi, fmin))
        self.sr, self.frame, self.hop = int(sr), int(frame), int(hop)
        self.fmin, self.fmax, self.threshold, self.min_power = fmin, fmax, threshold, min_power
        self.tau_min, self.tau_max, self.W = int(lo), int(hi), int(frame - hi)

    def key(self):
        return (self.sr, self.frame, self.hop, self.fmin, self.fmax, self.threshold, self.min_power)

    def __repr__(self):
        return 'PitchConfig(sr=%d, frame=%d, hop=%d, fmin=%r, fmax=%r, threshold=%r, min_power=%r)' % self.key()


def frame_count(length, cfg):
    """Frames of an utterance of ``length`` samples: 1 + (length - frame) // hop; 0 below one frame."""
    length = np.asarray(length, np.int64)
    return np.where(length >= cfg.frame, 1 + (length - cfg.frame) // cfg.hop, 0)


def _frames(lengths, cfg, who):
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    if lengths.size == 0:
        raise ValueError('%s: no utterances' % who)
    short = np.nonzero(lengths < cfg.frame)[0]
    if short.size:
        raise ValueError('%s: utterance %d has %d samples, fewer than one frame (frame = %d)'
                         % (who, short[0], lengths[short[0]], cfg.frame))
    return frame_count(lengths, cfg).astype(np.int64)


def plan_chunks(frames, cfg, chunk_bytes, sides=1):
    """Cuts utterances 0 .. N - 1 greedily, in input order, into runs [(start, stop), ...] (ragged.plan_runs): a run is closed
    when the next utterance would take the samples it stages -- ``frames * hop + frame - hop`` a side, what the frames
    cover -- over ``chunk_bytes``; an utterance over the budget stands alone."""
    if int(chunk_bytes) < 1 or int(sides) < 1:
        raise ValueError('plan_chunks: chunk_bytes and sides must be positive, got %r and %r' % (chunk_bytes, sides))
    frames = np.asarray(frames, np.int64).reshape(-1)
    return ragged.plan_runs((int(sides) * (frames * cfg.hop + (cfg.frame - cfg.hop)))[None], chunk_bytes)


def _desc(cfg, n, ftot):
    d = _lib.PitchDesc()
    d.n, d.sr, d.frame, d.hop, d.ftot = int(n), cfg.sr, cfg.frame, cfg.hop, int(ftot)
    d.fmin, d.fmax, d.threshold, d.min_power = cfg.fmin, cfg.fmax, cfg.threshold, cfg.min_power
    return d


def _yin(cfg, x_ptr, off_in, frames, f0_ptr, ap_ptr, who):
    """One launch over a run of utterances; returns the device table (off_in, then frame_off), kept by the caller while it
    is read."""
    frame_off = ragged.offsets(frames, total=True)
    seg = backend.to_device(np.concatenate([np.ascontiguousarray(off_in, np.int64).reshape(-1), frame_off]))
    d = _desc(cfg, len(frames), frame_off[-1])
    ws, need = backend.described_workspace('vqvae_pitch_yin_workspace_bytes', d, who)
    _lib.call('vqvae_pitch_yin', C.byref(d), x_ptr, seg.ptr, seg.ptr + 8 * len(frames), f0_ptr, ap_ptr, ws, need, _S())
    return seg


class RaggedPitch(object):
    """The tracks of N utterances laid end to end along the frame axis: ``frame_off`` host int64 (N + 1,) with utterance i at
    frames [frame_off[i], frame_off[i + 1]), ``frames`` (N,), ``f0`` (Hz, 0 for an unvoiced frame) and ``aperiodicity``
    float32 (Ftot,) device arrays."""

    def __init__(self, cfg, frames, f0, aperiodicity):
        self.cfg = cfg
        self.frames = np.asarray(frames, np.int64)
        self.frame_off = ragged.offsets(self.frames, total=True)
        self.f0, self.aperiodicity = f0, aperiodicity
        self._host = None

    def __len__(self):
        return len(self.frames)

    def utterance(self, i):
        """Host copies of utterance i's tracks: (f0 (F_i,), aperiodicity (F_i,)).  The first call copies both arrays back
        once."""
        i = int(i)
        if not 0 <= i < len(self.frames):
            raise IndexError('RaggedPitch.utterance: utterance %d of %d' % (i, len(self.frames)))
        if self._host is None:
            self._host = [self.f0.get(), self.aperiodicity.get()]
        return tuple(ragged.split(t, self.frame_off[i:i + 2])[0] for t in self._host)


# --------------------------------------------------------------------------- #
# the public calls
# --------------------------------------------------------------------------- #
def pitch_many(waves, cfg, chunk_bytes=1 << 30):
    """F0 and aperiodicity of every frame of many utterances, one launch per chunk.
    ``waves``: what ``features_many`` takes -- a list of host or device float32 arrays, each taken whole, or a
    ResidentCorpus / CorpusView, which is read in place through its offsets.  Host waves are uploaded with one copy per
    chunk of at most ``chunk_bytes`` of samples; the result does not depend on ``chunk_bytes``.  An utterance shorter
    than one frame is a ValueError naming it."""
    if not isinstance(cfg, PitchConfig):
        raise TypeError('pitch_many: cfg must be a PitchConfig, got %r' % (type(cfg),))
    lengths, source = ragged.wave_source(waves, 'pitch_many')
    frames = _frames(lengths, cfg, 'pitch_many')
    chunks = plan_chunks(frames, cfg, chunk_bytes)
    track = RaggedPitch(cfg, frames, None, None)
    ftot = int(track.frame_off[-1])
    track.f0 = DeviceArray((ftot,), np.float32)
    track.aperiodicity = DeviceArray((ftot,), np.float32)
    for start, stop in chunks:
        x_ptr, off_in, keep = source(start, stop)
        at = 4 * int(track.frame_off[start])
        seg = _yin(cfg, x_ptr, off_in, frames[start:stop], track.f0.ptr + at, track.aperiodicity.ptr + at, 'pitch_many')
        del keep, seg
    return track


def compare_pitch_many(reference, test, cfg, chunk_bytes=1 << 30):
    """The pitch statistics of every (reference, test) pair, float64 (N,) each, and ``frames`` int64 (N,):
    ``voiced_ref``, ``voiced_test``, ``voiced_both`` (frame counts), ``vuv_error`` (share of frames voiced on one side
    only), ``gross_error`` (share of both-voiced frames whose F0 is more than 20 % off the reference's),
    ``f0_rmse_cents`` (over the both-voiced frames) and ``log_f0_mean_ref`` / ``log_f0_mean_test`` (mean natural log of F0
    over each side's own voiced frames: their difference is the register shift).  Both arguments take what
    ``pitch_many`` takes.  The two waves of a pair are cut to their common length before framing; there is no time
    alignment.  An empty set divides as IEEE divides: a pair without a both-voiced frame has nan for gross_error and
    f0_rmse_cents.  Lists of different length, or a pair whose common length is below one frame, are a ValueError."""
    if not isinstance(cfg, PitchConfig):
        raise TypeError('compare_pitch_many: cfg must be a PitchConfig, got %r' % (type(cfg),))
    len_a, src_a = ragged.wave_source(reference, 'compare_pitch_many')
    len_b, src_b = ragged.wave_source(test, 'compare_pitch_many')
    if len(len_a) != len(len_b):
        raise ValueError('compare_pitch_many: %d reference and %d test utterances' % (len(len_a), len(len_b)))
    frames = _frames(np.minimum(len_a, len_b), cfg, 'compare_pitch_many')
    N = len(frames)
    chunks = plan_chunks(frames, cfg, chunk_bytes, sides=2)
    out = DeviceArray((N, len(COLUMNS)), np.float64)
    most = max(int(frames[a:b].sum()) for a, b in chunks)
    f0 = [DeviceArray((most,), np.float32) for _ in range(2)]
    for start, stop in chunks:
        fr = frames[start:stop]
        for side, src in enumerate((src_a, src_b)):
            x_ptr, off_in, keep = src(start, stop)
            seg = _yin(cfg, x_ptr, off_in, fr, f0[side].ptr, None, 'compare_pitch_many')
            del keep
        d = _desc(cfg, stop - start, int(fr.sum()))
        ws, need = backend.described_workspace('vqvae_pitch_compare_workspace_bytes', d, 'compare_pitch_many')
        _lib.call('vqvae_pitch_compare', C.byref(d), f0[0].ptr, f0[1].ptr, seg.ptr + 8 * (stop - start),
                  out.ptr + 8 * len(COLUMNS) * start, ws, need, _S())
        del seg
    res = out.get()
    scores = dict((name, res[:, j].copy()) for j, name in enumerate(COLUMNS))
    scores['frames'] = frames.copy()
    return scores
