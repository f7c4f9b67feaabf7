"""CPU checks of the device ingest (include/vqvae_ingest.h, csrc/ingest.hip, csrc/ingest_rule.h, vqvae_amd.ingest): the tap
tables against the independent restatement (tests/ingest_ref.py), the filter's properties, the trim rule, the very
functions the kernels run compiled for the host into a stand-alone program, the WAV reader and writer, the file lists, the
header against the table Python binds, the entry points' validation and the compiled kernels' resources."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import wave

import numpy as np
import pytest

import ingest_ref as R
import vqvae_amd
from vqvae_amd import _lib
from vqvae_amd import ingest as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'vqvae_ingest.h')
CSRC = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc')
TILE = 1024
CONVERSIONS = [(48000, 'kaiser_fast', (1, 3, 48)), (44100, 'kaiser_fast', (160, 441, 45)), (22050, 'kaiser_fast', (320, 441, 23)),
               (8000, 'kaiser_fast', (2, 1, 16)), (44100, 'kaiser_best', (160, 441, 177))]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


_TAPS = {}


def _taps(sr, res_type='kaiser_fast'):
    if (sr, res_type) not in _TAPS:
        h = R.taps(sr, 16000, res_type)
        h.setflags(write=False)
        _TAPS[(sr, res_type)] = h
    return _TAPS[(sr, res_type)]


# ---- taps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sr,res_type,lmj', CONVERSIONS)
def test_taps_equal_the_restatement(sr, res_type, lmj):
    h, got = G.resample_taps(sr, 16000, res_type)
    assert got == lmj == R.ratio(sr, 16000, res_type)
    assert h.dtype == np.float32 and h.shape == (lmj[0], 2 * lmj[2]) and h.flags.c_contiguous
    np.testing.assert_array_equal(_bits(h), _bits(_taps(sr, res_type)))
    if res_type == 'kaiser_fast':
        gain = h.astype(np.float64).sum(axis=1)
        print('DC gain per phase: %.7f .. %.7f' % (gain.min(), gain.max()))
        assert np.abs(gain - 1).max() <= 1e-4
    else:
        assert h.nbytes == 160 * 354 * 4 and h.nbytes > 80 * 1024          # 221 KB: the global-memory path of the kernel


def test_taps_presets_tuple_identity_and_errors():
    a, _ = G.resample_taps(48000, 16000, 'kaiser_fast')
    b, _ = G.resample_taps(48000, 16000, G.PRESETS['kaiser_fast'])
    np.testing.assert_array_equal(_bits(a), _bits(b))
    assert G.PRESETS == R.FILTERS
    h, lmj = G.resample_taps(16000, 16000)
    assert lmj == (1, 1, 1) and h.tolist() == [[1.0, 0.0]]
    assert G.resample_taps(96000, 32000)[1] == (1, 3, 48)                 # only the ratio counts
    for bad in ('kaiser', (0, 0.9, 8.0), (16, 0.0, 8.0), (16.5, 0.9, 8.0)):
        with pytest.raises(ValueError, match='resample_taps'):
            G.resample_taps(48000, 16000, bad)
    with pytest.raises(ValueError, match='resample_taps'):
        G.resample_taps(0, 16000)
    assert vqvae_amd.resample_taps is G.resample_taps and vqvae_amd.DeviceIngest is G.DeviceIngest


# ---- the filter's properties, on the restatement -----------------------------------------------------------------------------
def _tone(sr, hz, n=6000):
    return (0.5 * np.sin(2 * np.pi * hz * np.arange(n) / sr)).astype(np.float32)


@pytest.mark.parametrize('sr,hz', [(48000, 1000), (48000, 3000), (44100, 3000)])
def test_passband_tone_is_kept(sr, hz):
    """A 0.5-amplitude sine of 6 000 samples; 2J L / M + 2 outputs ignored at each end.  Measured with a NumPy prototype
    of the rule on the CPU: 1.1e-5, 1.5e-5, 1.1e-5; the bound is about three times that."""
    L, M, J = R.ratio(sr, 16000)
    y = R.resample(_tone(sr, hz), _taps(sr), L, M, J)
    edge = 2 * J * L // M + 2
    want = 0.5 * np.sin(2 * np.pi * hz * np.arange(len(y)) / 16000.0)
    err = np.abs(y.astype(np.float64) - want)[edge:-edge].max()
    print('%d -> 16000, %d Hz: max error %.3g' % (sr, hz, err))
    assert len(y) == R.n_out_of(6000, L, M) and err <= 5e-5


def test_stopband_tone_is_removed():
    """12 kHz at 48 kHz would alias to 4 kHz at 16 kHz.  Measured on the CPU prototype: 1.2e-5."""
    L, M, J = R.ratio(48000, 16000)
    y = R.resample(_tone(48000, 12000), _taps(48000), L, M, J)
    edge = 2 * J * L // M + 2
    left = np.abs(y[edge:-edge]).max()
    print('48000 -> 16000, 12 kHz: aliased output %.3g' % left)
    assert left <= 5e-5


# ---- the trim rule, on the restatement -----------------------------------------------------------------------------------------
def trim_signals():
    """The five signals of the trim tests: name -> (y, expected (start, end) or None)."""
    rs = np.random.RandomState(11)

    def burst(n, a, b):
        y = (1e-5 * rs.standard_normal(n)).astype(np.float32)
        y[a:b] = (0.3 * rs.standard_normal(b - a)).astype(np.float32)
        return y

    return {'middle': burst(20000, 6000, 11000), 'from_zero': burst(12000, 0, 4000), 'to_end': burst(10100, 6000, 10100),
            'shortest': burst(1025, 300, 700), 'quiet': (1e-6 * np.sign(rs.standard_normal(9000))).astype(np.float32)}


def test_trim_bounds_of_the_restatement():
    sig = trim_signals()
    r = R.top_db_ratio(20)
    assert r == 10.0 ** (-20 / 10.0) == G.DeviceIngest(top_db=20).r
    s, e, peak, status = R.bounds(sig['middle'], r)
    assert status == 0 and s % 512 == 0 and e % 512 == 0
    assert 6000 - 2048 <= s <= 6000 and 11000 <= e <= 11000 + 2048
    assert peak == np.abs(sig['middle'][s:e]).max() and peak.dtype == np.float32
    s, e, _, status = R.bounds(sig['from_zero'], r)
    assert (s, status) == (0, 0) and 4000 <= e <= 4000 + 2048 and e % 512 == 0
    s, e, _, status = R.bounds(sig['to_end'], r)
    assert 10100 % 512 != 0 and (e, status) == (10100, 0) and s % 512 == 0 and 6000 - 2048 <= s <= 6000
    s, e, _, status = R.bounds(sig['shortest'], r)
    assert status == 0 and 0 <= s < e <= 1025 and len(R.frame_energies(sig['shortest'])) == 3
    with pytest.raises(AssertionError):
        R.frame_energies(np.ones(1024, np.float32))
    assert R.bounds(sig['quiet'], r)[:2] == (0, 9000) and R.frame_energies(sig['quiet']).max() / 2048 < 1e-10   # under amin: kept whole
    assert R.bounds(np.zeros(3000, np.float32), r) == (0, 3000, 0.0, 2)
    nan = sig['middle'].copy()
    nan[7] = np.nan
    assert R.bounds(nan, r) == (0, 20000, 0.0, 1)
    # the energies are the plain sum of squares up to the order of the additions
    y = sig['middle']
    padded = np.pad(y.astype(np.float64), 1024, mode='reflect')
    plain = np.array([np.sum(padded[t * 512:t * 512 + 2048] ** 2) for t in range(1 + len(y) // 512)])
    np.testing.assert_allclose(R.frame_energies(y), plain, rtol=1e-13)


# ---- the rule's own functions, compiled for the host -------------------------------------------------------------------------------
_PROGRAM = r'''
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#define __host__
#define __device__
#define __forceinline__ inline
#include "ingest_rule.h"
static void get(void* p, size_t n, FILE* f) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }
int main(int argc, char** argv) {
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  int32_t cases;
  get(&cases, 4, in);
  for (int c = 0; c < cases; ++c) {
    int32_t k[8];                                      // kind, fmt, channels, L, M, J, n_in, first
    get(k, sizeof k, in);
    if (k[0] == 0) {                                   // resample: every output as its own "thread", exactly sized buffers
      const size_t raw_bytes = (size_t)(k[7] + k[6]) * k[2] * (k[1] == vq::INGEST_FMT_I16 ? 2 : 4), tap_bytes = (size_t)k[3] * 2 * k[5] * 4;
      void* raw = malloc(raw_bytes);
      float* taps = (float*)malloc(tap_bytes);
      get(raw, raw_bytes, in);
      get(taps, tap_bytes, in);
      const int64_t n_out = vq::ingest_n_out(k[6], k[3], k[4]);
      float* y = (float*)malloc((size_t)n_out * 4);
      for (int64_t o = 0; o < n_out; ++o) y[o] = vq::ingest_output_at(raw, k[1], k[2], k[7], k[6], taps, k[3], k[4], k[5], o);
      // the kernel's form: the window staged once, then ingest_dot
      const int64_t q0 = 0, q1 = (n_out - 1) * k[4] / k[3];
      const int window = (int)(q1 - q0) + 2 * k[5];
      float* win = (float*)malloc((size_t)window * 4);
      for (int i = 0; i < window; ++i) win[i] = vq::ingest_mono_at(raw, k[1], k[2], k[7], q0 - k[5] + 1 + i, k[6]);
      for (int64_t o = 0; o < n_out; ++o) {
        const float v = k[3] == k[4] ? win[o] : vq::ingest_dot(win + o * k[4] / k[3], taps + (o * k[4] % k[3]) * 2 * k[5], 2 * k[5]);
        if (v != y[o] && (v == v || y[o] == y[o])) { fprintf(stderr, "case %d output %lld: staged %a, direct %a\n", c, (long long)o, v, y[o]); return 3; }
      }
      int64_t n64 = n_out;
      fwrite(&n64, 8, 1, out);
      fwrite(y, 4, (size_t)n_out, out);
      free(win); free(y); free(taps); free(raw);
    } else {                                           // frame energies + normalisation of a signal of n = k[6] samples
      const int n = k[6];
      float* y = (float*)malloc((size_t)n * 4);
      get(y, (size_t)n * 4, in);
      const int nf = 1 + n / vq::INGEST_HOP;
      int64_t n64 = nf;
      fwrite(&n64, 8, 1, out);
      for (int t = 0; t < nf; ++t) {
        double a[64];
        for (int l = 0; l < 64; ++l) a[l] = vq::ingest_lane_energy(y, n, t, l);
        for (int stride = 32; stride >= 1; stride >>= 1)
          for (int l = 0; l < stride; ++l) a[l] += a[l + stride];
        float hop = 0.0f;
        for (int l = 0; l < 64; ++l) { const float v = vq::ingest_lane_hop_peak(y, n, t, l); if (v > hop) hop = v; }
        const double e[4] = {a[0], vq::ingest_floor_mse(a[0]), (double)hop, vq::ingest_finite_energy(a[0]) ? 1.0 : 0.0};
        fwrite(e, 8, 4, out);
      }
      float peak = 0.0f;
      int32_t bad = 0;
      for (int i = 0; i < n; ++i) { const float v = y[i] < 0 ? -y[i] : y[i]; if (v > peak) peak = v; bad |= !vq::ingest_finite(y[i]); }
      fwrite(&bad, 4, 1, out);
      if (!bad) for (int i = 0; i < n; ++i) { const float v = vq::ingest_normalise(y[i], peak); fwrite(&v, 4, 1, out); }
      free(y);
    }
  }
  fclose(out);
  return 0;
}
'''


def n_in_for(n_out, L, M):
    """The smallest n_in whose n_out is at least ``n_out`` (exactly ``n_out`` when L <= M; when up-sampling not every
    length is reachable and this is the next one)."""
    n = max(1, n_out * M // L - 1)
    while R.n_out_of(n, L, M) < n_out:
        n += 1
    return n


def resample_lengths(L, M, J):
    return [1, 2 * J - 1] + [n_in_for(v, L, M) for v in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)]


def raw_wave(n, channels, dtype, seed):
    rs = np.random.RandomState(seed)
    if dtype == np.int16:
        return rs.randint(-32768, 32768, size=(n, channels)).astype(np.int16)
    return (rs.uniform(-1, 1, size=(n, channels)) * rs.uniform(0.3, 3.0)).astype(np.float32)


def test_rule_functions_compiled_for_the_host_equal_the_restatement(tmp_path):
    """csrc/ingest_rule.h is what the kernels run.  The host compiler builds it into a program of its own, with the address
    and undefined-behaviour sanitisers when the toolchain has them; every buffer is allocated at its exact size, so a read
    outside the utterance, the table or the window is caught.  Both forms of an output are run: straight from the raw
    buffer, and the kernel's staged window + ingest_dot; the program itself checks that they agree."""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    src, exe = str(tmp_path / 'ingest_rule_host.cc'), str(tmp_path / 'ingest_rule_host')
    open(src, 'w').write(_PROGRAM)
    base = [cxx, '-O1', '-std=c++17', '-ffp-contract=off', '-I', CSRC, src, '-o', exe]
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    if subprocess.call(base + san, stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)
    cases, blob = [], []
    for sr, res_type, (L, M, J) in CONVERSIONS + [(16000, 'kaiser_fast', (1, 1, 1))]:
        h = G.resample_taps(sr, 16000, res_type)[0]
        for k, n_in in enumerate(resample_lengths(L, M, J)):
            for channels, dtype in ((1, np.int16), (2, np.float32), (1, np.float32), (3, np.int16)):
                if res_type == 'kaiser_best' and (channels, dtype) not in ((1, np.int16), (2, np.float32)):
                    continue
                first = 3 * (k % 2)                                     # frames of another utterance in front of this one
                raw = raw_wave(first + n_in, channels, dtype, 100 * k + channels)
                cases.append(('resample', sr, res_type, raw[first:], (L, M, J)))
                blob.append(np.array([0, 0 if dtype == np.int16 else 1, channels, L, M, J, n_in, first], np.int32).tobytes()
                            + raw.tobytes() + h.tobytes())
    signals = dict(trim_signals())
    signals['nan'] = signals['middle'].copy()
    signals['nan'][7] = np.nan
    for name, y in sorted(signals.items()):
        cases.append(('energy', name, y))
        blob.append(np.array([1, 0, 0, 0, 0, 0, len(y), 0], np.int32).tobytes() + y.tobytes())
    open(str(tmp_path / 'in.bin'), 'wb').write(struct.pack('<i', len(cases)) + b''.join(blob))
    run = subprocess.run([exe, str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0 and run.stderr == b'', run.stderr.decode()[-2000:]
    out = open(str(tmp_path / 'out.bin'), 'rb').read()
    at = 0
    for case in cases:
        n = struct.unpack_from('<q', out, at)[0]
        at += 8
        if case[0] == 'resample':
            _, sr, res_type, raw, (L, M, J) = case
            got = np.frombuffer(out, np.float32, n, at)
            at += 4 * n
            want = R.resample(R.mono(raw), _taps(sr, res_type) if L != M else None, L, M, J)
            assert n == len(want) == R.n_out_of(len(raw), L, M)
            np.testing.assert_array_equal(_bits(got), _bits(want), str((sr, res_type, raw.shape, raw.dtype)))
        else:
            _, name, y = case
            e = np.frombuffer(out, np.float64, 4 * n, at).reshape(n, 4)
            at += 32 * n
            hops = [np.abs(y[512 * t:512 * (t + 1)]) for t in range(n)]
            np.testing.assert_array_equal(e[:, 3], [float(np.isfinite(h).all() and np.isfinite(y[max(0, 512 * t - 1024):512 * t + 1024]).all())
                                                    for t, h in enumerate(hops)], name)
            bad = struct.unpack_from('<i', out, at)[0]
            at += 4
            assert bad == int(name == 'nan')
            if bad:
                continue
            want = R.frame_energies(y)
            np.testing.assert_array_equal(_bits(e[:, 0]), _bits(want), name)
            np.testing.assert_array_equal(e[:, 2], [h.max() if h.size else 0.0 for h in hops], name)
            np.testing.assert_array_equal(_bits(e[:, 1]), _bits(np.maximum(R.AMIN, want / 2048.0)), name)
            got = np.frombuffer(out, np.float32, len(y), at)
            at += 4 * len(y)
            np.testing.assert_array_equal(_bits(got), _bits(vqvae_amd.inputs.peak_normalise(y)), name)
    assert at == len(out)


# ---- files ------------------------------------------------------------------------------------------------------------------------
def _chunk(name, body):
    return name + struct.pack('<I', len(body)) + body + (b'\0' if len(body) & 1 else b'')


def _riff(*chunks):
    body = b'WAVE' + b''.join(chunks)
    return b'RIFF' + struct.pack('<I', len(body)) + body


def _fmt(tag, channels, sr, bits, extensible=False):
    align = channels * bits // 8
    if not extensible:
        return _chunk(b'fmt ', struct.pack('<HHIIHH', tag, channels, sr, sr * align, align, bits))
    guid = struct.pack('<H', tag) + b'\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71'
    return _chunk(b'fmt ', struct.pack('<HHIIHHHHI', 0xFFFE, channels, sr, sr * align, align, bits, 22, bits, 3) + guid)


def test_read_wav_reads_what_the_wave_module_writes(tmp_path):
    rs = np.random.RandomState(5)
    for channels, sr in ((1, 48000), (2, 44100)):
        a = rs.randint(-32768, 32768, size=(701, channels)).astype(np.int16)
        path = str(tmp_path / ('pcm16_%d.wav' % channels))
        with wave.open(path, 'wb') as w:
            w.setnchannels(channels)
            w.setsampwidth(2)
            w.setframerate(sr)
            w.writeframes(a.astype('<i2').tobytes())
        got, got_sr = G.read_wav(path)
        assert got_sr == sr and got.dtype == np.int16 and got.shape == (701, channels)
        np.testing.assert_array_equal(got, a)
        assert G.wav_info(path) == (701, channels, sr, np.dtype(np.int16))
        assert G.read_wav(tmp_path / ('pcm16_%d.wav' % channels))[1] == sr                  # a pathlib.Path too


def test_read_wav_hand_built_files(tmp_path):
    rs = np.random.RandomState(6)
    f32 = rs.uniform(-1, 1, size=(333, 2)).astype(np.float32)
    i16 = rs.randint(-32768, 32768, size=(335, 1)).astype(np.int16)
    i24 = rs.randint(-2 ** 23, 2 ** 23, size=(100, 1)).astype(np.int32)
    i24[:3, 0] = [-2 ** 23, 2 ** 23 - 1, -1]
    b24 = b''.join(struct.pack('<i', int(v))[:3] for v in i24[:, 0])
    u8 = rs.randint(0, 256, size=(51, 1)).astype(np.uint8)
    i32 = rs.randint(-2 ** 31, 2 ** 31, size=(40, 2)).astype(np.int32)
    files = {
        'float32': (_riff(_fmt(3, 2, 22050, 32), _chunk(b'fact', struct.pack('<I', 333)), _chunk(b'data', f32.tobytes())), f32, 22050),
        'extensible_pcm': (_riff(_fmt(1, 1, 48000, 16, True), _chunk(b'data', i16.tobytes())), i16, 48000),
        'extensible_float': (_riff(_fmt(3, 2, 16000, 32, True), _chunk(b'data', f32.tobytes())), f32, 16000),
        'pcm24': (_riff(_fmt(1, 1, 48000, 24), _chunk(b'data', b24)), (i24 / 2.0 ** 23).astype(np.float32), 48000),
        'pcm8': (_riff(_fmt(1, 1, 8000, 8), _chunk(b'data', u8.tobytes())), ((u8.astype(np.float64) - 128) / 128).astype(np.float32), 8000),
        'pcm32': (_riff(_fmt(1, 2, 16000, 32), _chunk(b'data', i32.tobytes())), (i32 / 2.0 ** 31).astype(np.float32), 16000),
        'list_before_data': (_riff(_fmt(1, 1, 48000, 16), _chunk(b'LIST', b'INFOISFT\x04\x00\x00\x00abc\x00'), _chunk(b'data', i16.tobytes())),
                             i16, 48000),
        'odd_chunk': (_riff(_fmt(1, 1, 48000, 16), _chunk(b'junk', b'\x01\x02\x03'), _chunk(b'data', i16.tobytes())), i16, 48000),
        'odd_data_then_more': (_riff(_fmt(1, 1, 8000, 8), _chunk(b'data', u8.tobytes()), _chunk(b'LIST', b'xy')),
                               ((u8.astype(np.float64) - 128) / 128).astype(np.float32), 8000),
    }
    for name, (blob, want, sr) in files.items():
        path = str(tmp_path / (name + '.wav'))
        open(path, 'wb').write(blob)
        got, got_sr = G.read_wav(path)
        assert got_sr == sr and got.dtype == want.dtype and got.shape == want.shape, name
        np.testing.assert_array_equal(_bits(got) if got.dtype == np.float32 else got, _bits(want) if got.dtype == np.float32 else want, name)
        assert G.wav_info(path) == (want.shape[0], want.shape[1], sr, want.dtype), name


def test_write_wav_round_trip_and_bad_files(tmp_path):
    rs = np.random.RandomState(7)
    w = rs.standard_normal(1001).astype(np.float32)
    w[:3] = [0.0, -0.0, 1e-40]
    path = str(tmp_path / 'out.wav')
    G.write_wav(path, w, 16000)
    got, sr = G.read_wav(path)
    assert sr == 16000 and got.shape == (1001, 1) and got.dtype == np.float32
    np.testing.assert_array_equal(_bits(got[:, 0]), _bits(w))
    whole = open(path, 'rb').read()
    bad = {'truncated.wav': whole[:-10], 'header_only.wav': whole[:30], 'not_riff.wav': b'OggS' + whole[4:],
           'not_wave.wav': whole[:8] + b'AVI ' + whole[12:], 'empty.wav': b'', 'no_data.wav': _riff(_fmt(1, 1, 8000, 16)),
           'adpcm.wav': _riff(_fmt(2, 1, 8000, 16), _chunk(b'data', b'\0\0')),
           'float64.wav': _riff(_fmt(3, 1, 8000, 64), _chunk(b'data', b'\0' * 8)),
           'data_first.wav': _riff(_chunk(b'data', b'\0\0'), _fmt(1, 1, 8000, 16))}
    for name, blob in bad.items():
        p = str(tmp_path / name)
        open(p, 'wb').write(blob)
        for fn in (G.read_wav, G.wav_info):
            with pytest.raises(ValueError) as info:
                fn(p)
            assert p in str(info.value), (name, str(info.value))


def test_corpus_files_follow_sorted_directory_names(tmp_path):
    layout = {'VCTK': ['wav48/p231/p231_002.wav', 'wav48/p231/p231_001.wav', 'wav48/p225/p225_010.wav', 'wav48/p300/p300_001.wav'],
              'ARCTIC': ['cmu_us_slt/wav/a0002.wav', 'cmu_us_bdl/wav/a0001.wav', 'cmu_us_slt/wav/a0001.wav'],
              'vs': ['zed/1.wav', 'amy/2.wav', 'amy/1.wav']}
    for kind, names in layout.items():
        root = tmp_path / kind
        for n in names:
            (root / n).parent.mkdir(parents=True, exist_ok=True)
            G.write_wav(root / n, np.zeros(4, np.float32), 16000)
        (root / ('wav48' if kind == 'VCTK' else '.') / 'README.txt').write_text('not a speaker')
        (root / names[0]).with_suffix('.txt').write_text('not audio')
        files, ids, dic = G.corpus_files(root, kind)
        assert files == sorted(str(root / n) for n in names)
        speakers = sorted(set(n.split('/')[1 if kind == 'VCTK' else 0] for n in names))
        assert dic == dict((s, i) for i, s in enumerate(speakers))
        assert ids == [dic[os.path.relpath(f, str(root)).split(os.sep)[1 if kind == 'VCTK' else 0]] for f in files]
    files, ids, dic = G.corpus_files(tmp_path / 'VCTK', 'VCTK')
    assert ids == [0, 1, 1, 2] and dic == {'p225': 0, 'p231': 1, 'p300': 2}
    with pytest.raises(ValueError, match='dataset_type'):
        G.corpus_files(tmp_path, 'LJ')
    assert vqvae_amd.corpus_files is G.corpus_files and vqvae_amd.read_wav is G.read_wav and vqvae_amd.write_wav is G.write_wav


# ---- the header, the table, the library ---------------------------------------------------------------------------------------------
NAMES = {'vqvae_ingest_abi_version', 'vqvae_ingest_workspace_bytes', 'vqvae_ingest_resample', 'vqvae_ingest_trim_bounds',
         'vqvae_ingest_pack'}


def test_header_exports_are_the_bound_table_and_versions_stand():
    """The header, the library, the versions and _lib's constants: tests/test_host_abi.py, for every header."""
    text = open(HEADER).read()
    assert set(_lib.HEADERS['vqvae_ingest.h'].prototypes) == NAMES
    for macro, value in (('VQVAE_INGEST_I16', G.FMT_I16), ('VQVAE_INGEST_F32', G.FMT_F32), ('VQVAE_INGEST_BAD_SAMPLE', G.BAD_SAMPLE),
                         ('VQVAE_INGEST_ZERO_PEAK', G.ZERO_PEAK), ('VQVAE_INGEST_EMPTY', G.EMPTY)):
        assert int(re.search(r'#define %s\s+(\d+)\s' % macro, text).group(1)) == value, macro
    assert _lib.INGEST_TILE == G.TILE == TILE
    for word in ('[resampy-recalled]', '[librosa-recalled]', 'No bit parity with librosa', '8.555504641634386', '14.769656459379492',
                 '0.9475937167399596'):
        assert word in ' '.join(text.replace('*', ' ').split()), word
    assert 'ingest' not in open(os.path.join(ROOT, 'include', 'vqvae_hip.h')).read()
    assert 'ingest.hip' in open(os.path.join(CSRC, 'Makefile')).read()


def test_c_side_validation_needs_no_device():
    lib = _lib.load()
    fake = 0x10000                                                      # never dereferenced: every call below is rejected first

    def rejected(what, rc):
        assert rc == -1, what
        assert what.encode() in lib.vqvae_last_error_string(), (what, lib.vqvae_last_error_string())

    def resample(raw=fake, fmt=0, channels=1, in_off=fake, n_in=fake, U=3, max_n_in=3000, taps=fake, L=1, M=3, J=48, y=fake,
                 y_off=fake, max_n_out=1000):
        return lib.vqvae_ingest_resample(raw, fmt, channels, in_off, n_in, U, max_n_in, taps, L, M, J, y, y_off, max_n_out, None)

    for name in ('raw', 'in_off', 'n_in', 'taps', 'y', 'y_off'):
        rejected('ingest_resample: null raw, in_offset, n_in, taps, y or y_offset', resample(**{name: None}))
    for U in (0, 65536):
        rejected('ingest_resample: 1..65535 utterances', resample(U=U))
    for ch in (0, 9):
        rejected('ingest_resample: channels must be 1..8', resample(channels=ch))
    rejected('ingest_resample: format must be 0 (int16) or 1 (float32)', resample(fmt=2))
    for kw in (dict(L=0), dict(M=0), dict(J=0)):
        rejected('ingest_resample: L, M and J must be at least 1', resample(**kw))
    rejected('ingest_resample: the tap table has 4194306 entries, the limit is 4194304', resample(L=2097153, J=1))
    rejected('ingest_resample: a tile\'s window of 16465 samples is above the limit of 16384', resample(L=1, M=16, J=48))
    rejected('ingest_resample: n_in must be at least 1', resample(max_n_in=0))
    rejected('ingest_resample: max_n_out is 999, ceil(3000 * 1 / 3) is 1000', resample(max_n_out=999))
    rejected('ingest_resample: max_n_out is 1000, ceil(3001 * 1 / 3) is 1001', resample(max_n_in=3001))
    rejected('at most 2^31 - 1', resample(L=2, M=1, J=16, max_n_in=2 ** 31 - 1, max_n_out=2 ** 31 - 1))

    def trim(y=fake, y_off=fake, n=fake, U=3, max_n=5000, r=0.01, ws=fake, ws_bytes=1 << 20, bounds=fake):
        return lib.vqvae_ingest_trim_bounds(y, y_off, n, U, max_n, r, ws, ws_bytes, bounds, None)

    for name in ('y', 'y_off', 'n', 'ws', 'bounds'):
        rejected('ingest_trim_bounds: null y, y_offset, n, workspace or bounds', trim(**{name: None}))
    for U in (0, 65536):
        rejected('ingest_trim_bounds: 1..65535 utterances', trim(U=U))
    rejected('ingest_trim_bounds: a signal needs at least 1025 samples (got max_n 1024)', trim(max_n=1024))
    for r in (-0.1, 1.0, float('nan')):
        rejected('ingest_trim_bounds: r = 10 ** (-top_db / 10) must be in [0, 1)', trim(r=r))
    assert lib.vqvae_ingest_workspace_bytes(3, 5000) == 3 * (1 + 5000 // 512) * 12
    assert lib.vqvae_ingest_workspace_bytes(1, 1025) == 3 * 12 and lib.vqvae_ingest_workspace_bytes(65535, 2 ** 31 - 1) == 65535 * 2 ** 22 * 12
    assert [lib.vqvae_ingest_workspace_bytes(*a) for a in ((0, 5000), (65536, 5000), (3, 1024))] == [0, 0, 0]
    rejected('ingest_trim_bounds: workspace of 359 bytes, 360 needed', trim(ws_bytes=359))

    def pack(y=fake, y_off=fake, bounds=fake, dst_off=fake, U=3, max_n=5000, dst=fake):
        return lib.vqvae_ingest_pack(y, y_off, bounds, dst_off, U, max_n, dst, None)

    for name in ('y', 'y_off', 'bounds', 'dst_off', 'dst'):
        rejected('ingest_pack: null y, y_offset, bounds, dst_offset or dst', pack(**{name: None}))
    for U in (0, 65536):
        rejected('ingest_pack: 1..65535 utterances', pack(U=U))
    rejected('ingest_pack: max_n must be at least 1', pack(max_n=0))


def test_python_front_end_argument_errors_need_no_device():
    for kw in (dict(top_db=0), dict(top_db=-3), dict(res_type='nearest')):
        with pytest.raises(ValueError):
            G.DeviceIngest(**kw)
    for raw in (np.zeros((3, 2, 2), np.float32), np.zeros(5, np.int32), np.zeros(5, np.uint8)):
        with pytest.raises(ValueError, match='wave 0 must be int16 or floating'):
            G._Array(raw, 16000, 'wave 0')
    a = G._Array(np.zeros((5, 2)), 8000, 'wave 0')
    assert (a.frames, a.channels, a.dtype, a.sr) == (5, 2, np.dtype(np.float32), 8000)
    assert G.status_reason(1) == 'holds a non-finite sample' and G.status_reason(2).startswith('is all zeros') and G.status_reason(4) == 'is empty'
    assert C.sizeof(C.c_int32) * 4 == 16                                # a vqvae_ingest_bounds is read back as four words


# ---- the compiled kernels -----------------------------------------------------------------------------------------------------------
def test_ingest_kernels_compile_without_scratch(tmp_path, record_property):
    """DESIGN 7j's budget: no scratch, no spills, at most 4 KB of static LDS per kernel (the resampler's window and taps are
    dynamic LDS, 80 KB at most, chosen by the entry point)."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    out = str(tmp_path / 'ingest.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', os.path.join(CSRC, 'ingest.hip'), '-o', out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = {}
    for m in re.finditer(r'\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+)'
                         r'.*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)', text, re.S):
        meta[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    kinds = ('ingest_resample_kernelILb1', 'ingest_resample_kernelILb0', 'ingest_copy_kernel', 'ingest_frame_energy_kernel',
             'ingest_bounds_kernel', 'ingest_pack_kernel')
    assert len(meta) == len(kinds), sorted(meta)
    for kind in kinds:
        hits = [v for k, v in meta.items() if kind in k]
        assert len(hits) == 1, (kind, sorted(meta))
        record_property(kind, '%(vgpr)d VGPRs, %(lds)d B static LDS' % hits[0])
        print(kind, hits[0])
        assert (hits[0]['scratch'], hits[0]['spill']) == (0, 0), (kind, hits[0])
        assert hits[0]['lds'] <= 4096 and hits[0]['vgpr'] <= 128, (kind, hits[0])
