"""From WAV files to the waveforms a ResidentCorpus holds, on the device (include/vqvae_ingest.h, csrc/ingest.hip).

The reference decodes, resamples, trims and normalises one file per example on host worker processes, every epoch
(utils.py:56-59: librosa.load(path, sr, res_type='kaiser_fast'), librosa.effects.trim(raw, top_db), raw /= abs(raw).max()).
Here the files are parsed on the host (``read_wav``: RIFF on ``struct``), their raw frames are copied to the device as they
are -- int16 stays int16 -- and three launches per batch decode to mono and resample, find the silence bounds and the peak,
and write the normalised samples where the corpus keeps them.  The rule is normative in the header; ``resample_taps``
computes the filter it takes as an input.  No bit parity with librosa is claimed (the header says why).
"""
import ctypes as C
import math
import os
import pathlib
import struct

import numpy as np

from . import _lib, backend, ragged
from .backend import DeviceArray
from .inputs import _Pinned

FMT_I16, FMT_F32 = 0, 1                            # VQVAE_INGEST_I16 / VQVAE_INGEST_F32
BAD_SAMPLE, ZERO_PEAK, EMPTY = 1, 2, 4             # the status bits of vqvae_ingest_bounds
TOO_SHORT = 8                                      # host only: fewer than MIN_N samples after resampling, nothing launched
FRAME, HOP, MIN_N = 2048, 512, 1025
TILE = 1024                                        # VQVAE_INGEST_TILE
MAX_UTTERANCES = 65535                             # per call
DEFAULT_BATCH_BYTES = 64 << 20

# [resampy-recalled] (Z zero crossings, roll-off rho, Kaiser beta): as remembered, not verified against the package
PRESETS = {'kaiser_fast': (16, 0.85, 8.555504641634386),
           'kaiser_best': (64, 0.9475937167399596, 14.769656459379492)}


# --------------------------------------------------------------------------- #
# files
# --------------------------------------------------------------------------- #
_PCM, _IEEE, _EXTENSIBLE = 1, 3, 0xFFFE


def _wav_layout(path, f):
    """(format tag, channels, sr, bits, block_align, data offset, data bytes) of an open WAV file; ValueError naming it."""
    def bad(what):
        return ValueError('read_wav: %s: %s' % (path, what))

    size = os.fstat(f.fileno()).st_size
    head = f.read(12)
    if len(head) < 12 or head[:4] != b'RIFF' or head[8:12] != b'WAVE':
        raise bad('not a RIFF/WAVE file')
    fmt, at = None, 12
    while True:
        f.seek(at)
        ck = f.read(8)
        if len(ck) < 8:
            raise bad('no data chunk' if fmt else 'no fmt chunk')
        name, n = ck[:4], struct.unpack('<I', ck[4:])[0]
        if name == b'fmt ':
            body = f.read(n)
            if n < 16 or len(body) < n:
                raise bad('truncated fmt chunk')
            tag, channels, sr, _, align, bits = struct.unpack('<HHIIHH', body[:16])
            if tag == _EXTENSIBLE:
                if n < 40:
                    raise bad('truncated WAVE_FORMAT_EXTENSIBLE fmt chunk')
                tag = struct.unpack('<H', body[24:26])[0]            # the first two bytes of SubFormat
            fmt = (tag, channels, sr, bits, align)
        elif name == b'data':
            if fmt is None:
                raise bad('data chunk before the fmt chunk')
            if at + 8 + n > size:
                raise bad('truncated: the data chunk announces %d bytes, the file holds %d' % (n, size - at - 8))
            return fmt + (at + 8, n)
        at += 8 + n + (n & 1)                                        # chunks are padded to even sizes


def _wav_format(path, tag, channels, sr, bits, align):
    if channels < 1 or sr < 1:
        raise ValueError('read_wav: %s: %d channels at %d Hz' % (path, channels, sr))
    if not ((tag == _PCM and bits in (8, 16, 24, 32)) or (tag == _IEEE and bits == 32)):
        raise ValueError('read_wav: %s: unsupported sample format (tag %d, %d bits): PCM 8/16/24/32 and IEEE float32 are read'
                         % (path, tag, bits))
    if align != channels * bits // 8:
        raise ValueError('read_wav: %s: block align %d for %d channels of %d bits' % (path, align, channels, bits))


def wav_info(path):
    """(frames, channels, sr, dtype) from the headers alone: what ``read_wav`` would return, without the samples."""
    path = os.fspath(path)
    with open(path, 'rb') as f:
        tag, channels, sr, bits, align, _, nbytes = _wav_layout(path, f)
    _wav_format(path, tag, channels, sr, bits, align)
    return nbytes // align, channels, sr, np.dtype(np.int16 if (tag == _PCM and bits == 16) else np.float32)


def read_wav(path):
    """(array (frames, channels), sr) of a RIFF/WAVE file.  PCM 16 comes back as int16 and IEEE float32 as float32, both
    as stored; PCM 8 (unsigned, minus 128), 24 and 32 as float32 v / 2^(bits - 1).  WAVE_FORMAT_EXTENSIBLE, unknown
    chunks before ``data`` and the padding of odd-sized chunks are handled; anything else is a ValueError naming the file."""
    path = os.fspath(path)
    with open(path, 'rb') as f:
        tag, channels, sr, bits, align, at, nbytes = _wav_layout(path, f)
        _wav_format(path, tag, channels, sr, bits, align)
        f.seek(at)
        frames = nbytes // align
        data = f.read(frames * align)
    if len(data) < frames * align:
        raise ValueError('read_wav: %s: truncated data chunk' % path)
    if tag == _IEEE:
        wave = np.frombuffer(data, '<f4').astype(np.float32)
    elif bits == 16:
        wave = np.frombuffer(data, '<i2').astype(np.int16)
    elif bits == 8:
        wave = ((np.frombuffer(data, np.uint8).astype(np.float64) - 128.0) / 128.0).astype(np.float32)
    elif bits == 32:
        wave = (np.frombuffer(data, '<i4').astype(np.float64) / 2.0 ** 31).astype(np.float32)
    else:                                                            # 24 bits: three little-endian bytes, sign in the last
        b = np.frombuffer(data, np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = v - ((v & 0x800000) << 1)
        wave = (v.astype(np.float64) / 2.0 ** 23).astype(np.float32)
    return wave.reshape(frames, channels), sr


def write_wav(path, wave, sr):
    """Mono IEEE float32 (generate.py:153 writes its result with librosa.output.write_wav)."""
    wave = np.ascontiguousarray(np.asarray(wave, np.float32).reshape(-1)).astype('<f4')
    data = wave.tobytes()
    fmt = struct.pack('<HHIIHH', _IEEE, 1, int(sr), int(sr) * 4, 4, 32)
    with open(os.fspath(path), 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 4 + 8 + len(fmt) + 8 + len(data)) + b'WAVE')
        f.write(b'fmt ' + struct.pack('<I', len(fmt)) + fmt)
        f.write(b'data' + struct.pack('<I', len(data)) + data)


def corpus_files(root, dataset_type):
    """(files, speaker_ids, speaker_dic) as train.py:39-53 and utils.py:112-128 list them: the files sorted, the
    speakers the sorted names of the speaker directories.  'VCTK': wav48/<speaker>/*.wav; 'ARCTIC': <speaker>/wav/*.wav;
    'vs': <speaker>/*.wav."""
    root = pathlib.Path(root)
    try:
        file_glob, speaker_glob, up = {'VCTK': ('wav48/*/*.wav', 'wav48/*', 1), 'ARCTIC': ('*/wav/*.wav', '*', 2),
                                       'vs': ('*/*.wav', '*', 1)}[dataset_type]
    except KeyError:
        raise ValueError("corpus_files: dataset_type must be 'VCTK', 'ARCTIC' or 'vs', got %r" % (dataset_type,))
    files = sorted(str(p) for p in root.glob(file_glob))
    speakers = sorted(p.name for p in root.glob(speaker_glob) if p.is_dir())
    speaker_dic = dict((name, i) for i, name in enumerate(speakers))
    ids = [speaker_dic[pathlib.Path(f).parents[up - 1].name] for f in files]
    return files, ids, speaker_dic


# --------------------------------------------------------------------------- #
# the filter
# --------------------------------------------------------------------------- #
def resample_plan(sr_in, sr_out, res_type='kaiser_fast'):
    """(L, M, J) and (Z, rho, beta) of the conversion, in integers as the header states them."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in < 1 or sr_out < 1:
        raise ValueError('resample_taps: sample rates must be positive, got %r -> %r' % (sr_in, sr_out))
    if isinstance(res_type, str):
        if res_type not in PRESETS:
            raise ValueError('resample_taps: res_type must be one of %s or a (Z, rho, beta) tuple, got %r'
                             % (sorted(PRESETS), res_type))
        res_type = PRESETS[res_type]
    Z, rho, beta = int(res_type[0]), float(res_type[1]), float(res_type[2])
    if Z < 1 or Z != res_type[0] or not 0 < rho <= 1 or not beta >= 0:
        raise ValueError('resample_taps: (Z, rho, beta) needs an integer Z >= 1, 0 < rho <= 1, beta >= 0, got %r' % (res_type,))
    g = math.gcd(sr_in, sr_out)
    L, M = sr_out // g, sr_in // g
    J = 1 if L == M else (Z if L >= M else -((-Z * M) // L))
    return (L, M, J), (Z, rho, beta)


def resample_taps(sr_in, sr_out, res_type='kaiser_fast'):
    """The tap table float32 (L, 2J) of the header's formula and (L, M, J).  sr_in == sr_out: the table [[1, 0]] with
    J = 1 (the entry point copies and does not read it)."""
    (L, M, J), (Z, rho, beta) = resample_plan(sr_in, sr_out, res_type)
    if L == M:
        return np.array([[1.0, 0.0]], np.float32), (L, M, J)
    s = 1.0 if L >= M else L / M
    p = np.arange(L, dtype=np.float64)[:, None]
    j = np.arange(-J + 1, J + 1, dtype=np.float64)[None, :]
    u = s * (p / L - j)
    v = u / Z
    inside = np.abs(v) < 1
    w = np.where(inside, np.i0(beta * np.sqrt(np.where(inside, 1 - v * v, 0.0))) / np.i0(beta), 0.0)
    h = ((s * rho) * np.sinc(rho * u)) * w
    return np.ascontiguousarray(h.astype(np.float32)), (L, M, J)


def resampled_length(n_in, L, M):
    return (int(n_in) * L + M - 1) // M


# --------------------------------------------------------------------------- #
# the device front end
# --------------------------------------------------------------------------- #
class _Array(object):
    """One utterance given as an array: (frames,) or (frames, channels), int16 or floating."""

    def __init__(self, raw, sr, name):
        a = np.asarray(raw)
        if a.ndim == 1:
            a = a[:, None]
        if a.ndim != 2 or not (a.dtype == np.int16 or a.dtype.kind == 'f'):
            raise ValueError('ingest: %s must be int16 or floating, (frames,) or (frames, channels); got %s %s'
                             % (name, a.dtype, a.shape))
        self.a = a if a.dtype == np.int16 else a.astype(np.float32, copy=False)
        self.name, self.sr = name, int(sr)
        self.frames, self.channels, self.dtype = a.shape[0], a.shape[1], self.a.dtype

    def load(self):
        return self.a


class _File(object):
    """One utterance in a WAV file: the headers are read now, the samples when its batch is staged."""

    def __init__(self, path):
        self.path, self.name = os.fspath(path), 'file %s' % os.fspath(path)
        self.frames, self.channels, self.sr, self.dtype = wav_info(self.path)

    def load(self):
        a, sr = read_wav(self.path)
        if a.shape != (self.frames, self.channels) or sr != self.sr or a.dtype != self.dtype:
            raise ValueError('ingest: %s changed while it was being read' % self.name)
        return a


_REASON = ((BAD_SAMPLE, 'holds a non-finite sample'), (ZERO_PEAK, 'is all zeros (no peak to normalise by)'),
           (EMPTY, 'is empty'), (TOO_SHORT, 'is shorter than %d samples after resampling (nothing to trim by)' % MIN_N))


def status_reason(status):
    for bit, text in _REASON:
        if status & bit:
            return text
    return 'has status %d' % status


class DeviceIngest(object):
    """Decode to mono, resample to ``sr``, trim silence below ``top_db`` and peak-normalise on the device.

    ``run(raws, srs)``: arrays in, device waves out.  ``preprocess_wave(raw, sr_in)``: one wave as ``synthesize``'s
    ``x_enc``.  ``ResidentCorpus.from_arrays`` / ``from_files`` build a corpus with it.  ``timings``: None, or a list that
    receives one dict of device milliseconds ('h2d', 'resample', 'bounds', 'pack') per launch group, taken between
    device events (tools/ingest_bench.py)."""

    def __init__(self, sr=16000, res_type='kaiser_fast', top_db=20):
        if not float(top_db) > 0:
            raise ValueError('DeviceIngest: top_db must be positive, got %r' % (top_db,))
        self.sr, self.res_type, self.top_db = int(sr), res_type, top_db
        self.r = 10.0 ** (-float(top_db) / 10.0)
        resample_plan(self.sr, self.sr, res_type)                    # validates res_type
        self._taps = {}
        self.timings = None

    def taps(self, sr_in):
        """(device tap table, (L, M, J)) of sr_in -> self.sr, uploaded once."""
        if sr_in not in self._taps:
            h, lmj = resample_taps(sr_in, self.sr, self.res_type)
            self._taps[sr_in] = (backend.to_device(h), lmj)
        return self._taps[sr_in]

    # ---- one (sr, channels, format) group of one batch: copy, resample, bounds ----
    def _front(self, items, stage):
        """``items``: _Array / _File of one group.  Returns (y, y_offset_dev, n_out, bounds (U, 4) int32 host, bounds_dev, ms)."""
        st = backend.stream()
        first = items[0]
        fmt = FMT_I16 if first.dtype == np.int16 else FMT_F32
        taps, (L, M, J) = self.taps(first.sr)
        U = len(items)
        n_in = np.array([it.frames for it in items], np.int32)
        in_off = ragged.offsets(n_in)
        n_out = np.array([resampled_length(n, L, M) for n in n_in], np.int32)
        y_off = ragged.offsets(n_out)
        per_frame = first.channels * first.dtype.itemsize
        nbytes = int(n_in.sum(dtype=np.int64)) * per_frame
        flat = stage.array[:nbytes].view(first.dtype)
        for it, off, n in zip(items, in_off, n_in):
            flat[off * it.channels:(off + n) * it.channels] = it.load().reshape(-1)
        raw = DeviceArray((nbytes,), np.uint8)
        marks = [self._mark(st)]
        _lib.call('vqvae_memcpy_h2d_async', raw.ptr, stage.ptr, nbytes, st)
        marks.append(self._mark(st))
        n_in_dev, in_off_dev = backend.to_device(n_in), backend.to_device(in_off)
        n_out_dev, y_off_dev = backend.to_device(n_out), backend.to_device(y_off)
        y = DeviceArray((int(n_out.sum(dtype=np.int64)),), np.float32)
        bounds_dev = DeviceArray((U, 4), np.int32)
        max_n = int(n_out.max())
        ws_bytes = _lib.load().vqvae_ingest_workspace_bytes(U, max_n)
        ws = DeviceArray((ws_bytes,), np.uint8)
        marks.append(self._mark(st))
        _lib.call('vqvae_ingest_resample', raw.ptr, fmt, first.channels, in_off_dev.ptr, n_in_dev.ptr, U, int(n_in.max()),
                  taps.ptr, L, M, J, y.ptr, y_off_dev.ptr, max_n, st)
        marks.append(self._mark(st))
        _lib.call('vqvae_ingest_trim_bounds', y.ptr, y_off_dev.ptr, n_out_dev.ptr, U, max_n, self.r, ws.ptr, ws_bytes,
                  bounds_dev.ptr, st)
        marks.append(self._mark(st))
        bounds = bounds_dev.get()                                    # 16 bytes per utterance; also: the staging buffer is free
        ms = None
        if self.timings is not None:
            ms = {'h2d': _elapsed(marks[0], marks[1]), 'resample': _elapsed(marks[2], marks[3]),
                  'bounds': _elapsed(marks[3], marks[4]), 'h2d_bytes': nbytes, 'utterances': U}
        return y, y_off_dev, n_out, bounds, bounds_dev, ms

    def _mark(self, st):
        return backend.Event().record(st) if self.timings is not None else None

    def _pack(self, front, dst_off, dst):
        y, y_off_dev, n_out, bounds, bounds_dev, ms = front
        st = backend.stream()
        dst_off_dev = backend.to_device(np.asarray(dst_off, np.int64))
        a = self._mark(st)
        _lib.call('vqvae_ingest_pack', y.ptr, y_off_dev.ptr, bounds_dev.ptr, dst_off_dev.ptr, len(n_out), int(n_out.max()),
                  dst.ptr, st)
        b = self._mark(st)
        if ms is not None:
            _lib.call('vqvae_stream_synchronize', st)
            ms['pack'] = _elapsed(a, b)
            self.timings.append(ms)

    # ---- a whole list ----
    def ingest(self, items, batch_bytes=DEFAULT_BATCH_BYTES, skip_bad=False, what='ingest'):
        """``items``: _Array / _File in input order.  Returns (samples DeviceArray of exactly sum(lengths) floats,
        lengths of the kept utterances, their positions in ``items``, skipped [(position, reason)])."""
        status = np.zeros(len(items), np.int64)
        lengths = np.zeros(len(items), np.int64)
        plans = {}
        upper, largest = 0, 1
        for i, it in enumerate(items):
            if it.channels < 1 or it.channels > 8:
                raise ValueError('%s: %s has %d channels; 1..8 are read' % (what, it.name, it.channels))
            if it.frames > 2 ** 31 - 1:
                raise ValueError('%s: %s has more than 2**31 - 1 frames' % (what, it.name))
            if it.sr not in plans:
                plans[it.sr] = resample_plan(it.sr, self.sr, self.res_type)[0]
            L, M, _ = plans[it.sr]
            n = resampled_length(it.frames, L, M)
            if n > 2 ** 31 - 1:
                raise ValueError('%s: %s has more than 2**31 - 1 samples after resampling' % (what, it.name))
            if it.frames == 0:
                status[i] = EMPTY
            elif n < MIN_N:
                status[i] = TOO_SHORT
            else:
                upper += n
                largest = max(largest, it.frames * it.channels * it.dtype.itemsize)
        todo = [i for i in range(len(items)) if status[i] == 0]
        self._raise_or_skip(items, status, skip_bad, what)
        samples = DeviceArray((max(upper, 1),), np.float32)
        stage = _Pinned((max(int(batch_bytes), largest),), np.uint8) if todo else None
        used, at = 0, 0
        while at < len(todo):
            batch, nbytes = [], 0
            while at < len(todo) and len(batch) < MAX_UTTERANCES:
                it = items[todo[at]]
                more = it.frames * it.channels * it.dtype.itemsize
                if batch and nbytes + more > batch_bytes:
                    break
                batch.append(todo[at])
                nbytes, at = nbytes + more, at + 1
            groups = {}
            for i in batch:
                it = items[i]
                groups.setdefault((it.sr, it.channels, it.dtype.str), []).append(i)
            fronts = []
            for idx in groups.values():
                front = self._front([items[i] for i in idx], stage)
                fronts.append((idx, front))
                b = front[3]
                status[idx] = b[:, 3]
                lengths[idx] = np.where(b[:, 3] == 0, b[:, 1] - b[:, 0], 0)
            self._raise_or_skip([items[i] for i in batch], status[batch], skip_bad, what)
            where = {}
            for i in batch:                                          # input order, whatever the grouping
                where[i] = used
                used += int(lengths[i])
            for idx, front in fronts:
                self._pack(front, [where[i] for i in idx], samples)
        keep = [i for i in range(len(items)) if status[i] == 0]
        skipped = [(i, status_reason(int(status[i]))) for i in range(len(items)) if status[i] != 0]
        if not keep:
            raise ValueError('%s: no utterance is left' % what)
        if used < samples.size:
            exact = DeviceArray((used,), np.float32)
            _lib.call('vqvae_memcpy_d2d', exact.ptr, samples.ptr, 4 * used, backend.stream())
            samples = exact
        return samples, lengths[keep].astype(np.int64), keep, skipped

    @staticmethod
    def _raise_or_skip(items, status, skip_bad, what):
        if skip_bad:
            return
        for it, s in zip(items, status):
            if s:
                raise ValueError('%s: %s %s' % (what, it.name, status_reason(int(s))))

    def run(self, raws, srs, batch_bytes=DEFAULT_BATCH_BYTES):
        """``raws``: arrays (frames,) or (frames, channels), int16 or floating; ``srs``: their sample rates (or one for
        all).  Returns (list of device float32 waves, views of one buffer; host int64 lengths).  A wave that cannot be
        processed (all zeros, a non-finite sample, too short to trim) is a ValueError naming its index."""
        raws = list(raws)
        srs = [srs] * len(raws) if np.ndim(srs) == 0 else list(srs)
        if len(srs) != len(raws) or not raws:
            raise ValueError('DeviceIngest.run: %d sample rates for %d waves' % (len(srs), len(raws)))
        items = [_Array(raw, sr, 'wave %d' % i) for i, (raw, sr) in enumerate(zip(raws, srs))]
        samples, lengths, _, _ = self.ingest(items, batch_bytes, False, 'DeviceIngest.run')
        return [samples.flat_view(int(o), int(n)) for o, n in zip(ragged.offsets(lengths), lengths)], lengths

    def preprocess_wave(self, raw, sr_in):
        """One wave as ``synthesize`` takes it: device float32 (1, 1, T, 1) (generate.py:43-50)."""
        waves, _ = self.run([raw], [sr_in])
        return waves[0].reshape(1, 1, waves[0].size, 1)


def _elapsed(a, b):
    ms = C.c_float()
    _lib.call('vqvae_event_synchronize', b.h)
    _lib.call('vqvae_event_elapsed_ms', C.byref(ms), a.h, b.h)
    return float(ms.value)
