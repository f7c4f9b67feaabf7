"""The device ingest (include/vqvae_ingest.h, csrc/ingest.hip, vqvae_amd.ingest) against the independent restatement
tests/ingest_ref.py.  The rule fixes the order of every float64 sum, the taps are an input and the division is correctly
rounded, so every comparison is bit equality; there is no tolerance."""
import os
import wave

import numpy as np
import pytest

import helpers as H
from helpers import _bits, _same
import ingest_ref as R
from test_host_ingest import n_in_for, raw_wave, trim_signals
from zoned import In, Out, ZonedArray, run_contract

pytestmark = pytest.mark.gpu

TILE = 1024


# ---- 1. resample -------------------------------------------------------------------------------------------------------------
RESAMPLE_CASES = [(48000, 'kaiser_fast', np.int16, 1), (44100, 'kaiser_fast', np.float32, 1), (44100, 'kaiser_best', np.int16, 1),
                  (8000, 'kaiser_fast', np.int16, 2), (16000, 'kaiser_fast', np.float32, 2), (22050, 'kaiser_fast', np.float32, 3)]
_RESAMPLE = {}


def _resample_case(sr, res_type, dtype, channels):
    """Five utterances (n_in = 1, 2J - 1 and the lengths whose n_out is TILE - 1, TILE + 1 and 2 TILE + 1, or the next
    reachable length when up-sampling), three frames in front of the first and one frame between two of them, so every
    in_offset is odd; their restatement's outputs.  Computed once and never changed."""
    key = (sr, res_type, dtype, channels)
    if key not in _RESAMPLE:
        L, M, J = R.ratio(sr, 16000, res_type)
        n_in = [1, 2 * J - 1] + [n_in_for(v, L, M) for v in (TILE - 1, TILE + 1, 2 * TILE + 1)]
        raws = [raw_wave(n, channels, dtype, 40 + i) for i, n in enumerate(n_in)]
        gap = np.full((1, channels), 77, dtype)
        in_off, parts, at = [], [np.repeat(gap, 3, axis=0)], 3
        for raw in raws:
            in_off.append(at)
            parts += [raw, gap]
            at += len(raw) + 1
        taps = R.taps(sr, 16000, res_type) if L != M else np.array([[1.0, 0.0]], np.float32)
        want = [R.resample(R.mono(raw), taps, L, M, J) for raw in raws]
        _RESAMPLE[key] = (np.concatenate(parts), np.array(in_off, np.int64), np.array(n_in, np.int32), taps, (L, M, J), want)
        for a in want:
            a.setflags(write=False)
    return _RESAMPLE[key]


@pytest.mark.parametrize('sr,res_type,dtype,channels', RESAMPLE_CASES)
def test_resample_is_the_restatement_under_red_zones(gpu, sr, res_type, dtype, channels):
    from vqvae_amd import _lib
    from vqvae_amd.ingest import resample_taps
    raw, in_off, n_in, taps, (L, M, J), want = _resample_case(sr, res_type, dtype, channels)
    h, lmj = resample_taps(sr, 16000, res_type)
    assert lmj == (L, M, J)
    _same(h, taps)
    n_out = np.array([len(w) for w in want], np.int64)
    assert (2 * J - 1 in n_in) and n_out.max() >= 2 * TILE + 1 and n_out.min() >= 1
    y_off = 1 + np.concatenate(([0], np.cumsum(n_out[:-1])))           # an odd start, the utterances back to back
    total = int(y_off[-1] + n_out[-1])
    valid = np.ones(total, bool)
    valid[0] = False
    specs = {'raw': In(raw.reshape(-1)), 'in_off': In(in_off), 'n_in': In(n_in), 'taps': In(h), 'y_off': In(y_off.astype(np.int64)),
             'y': Out((total,), np.float32, valid=valid)}

    def fn(b):
        _lib.call('vqvae_ingest_resample', b.raw.ptr, 0 if dtype == np.int16 else 1, channels, b.in_off.ptr, b.n_in.ptr, 5,
                  int(n_in.max()), b.taps.ptr, L, M, J, b.y.ptr, b.y_off.ptr, int(n_out.max()), gpu.stream())

    got = run_contract(gpu, fn, specs)['y']
    for u in range(5):
        _same(got[y_off[u]:y_off[u] + n_out[u]], want[u], 'utterance %d (n_in %d)' % (u, n_in[u]))


# ---- 2. bounds -------------------------------------------------------------------------------------------------------------
_SIGNALS = {}


def _signals():
    """The five signals of the host trim test, an all-zero utterance and one that holds a NaN; their restatement's bounds."""
    if not _SIGNALS:
        sig = trim_signals()
        ys = [sig[k] for k in ('middle', 'from_zero', 'to_end', 'shortest', 'quiet')] + [np.zeros(3000, np.float32)]
        nan = sig['middle'][:7000].copy()
        nan[6999] = np.nan
        ys.append(nan)
        r = R.top_db_ratio(20)
        want = np.zeros((len(ys), 4), np.int32)
        for u, y in enumerate(ys):
            s, e, peak, status = R.bounds(y, r)
            want[u] = [s, e, np.float32(peak).view(np.int32), status]
        assert want[:, 3].tolist() == [0, 0, 0, 0, 0, 2, 1]
        want.setflags(write=False)
        _SIGNALS.update(ys=ys, want=want, r=r)
    return _SIGNALS['ys'], _SIGNALS['want'], _SIGNALS['r']


def _bounds_buffers(ys):
    n = np.array([len(y) for y in ys], np.int32)
    y_off = 3 + np.concatenate(([0], np.cumsum(n[:-1] + 2, dtype=np.int64))).astype(np.int64)   # two foreign samples between signals
    flat = np.full(int(y_off[-1] + n[-1]), np.float32(np.inf), np.float32)    # anything read outside a signal would poison its result
    for y, o in zip(ys, y_off):
        flat[o:o + len(y)] = y
    return flat, y_off, n


def test_bounds_are_the_restatement_in_an_exact_poisoned_workspace(gpu):
    from vqvae_amd import _lib
    ys, want, r = _signals()
    flat, y_off, n = _bounds_buffers(ys)
    U, max_n = len(ys), int(n.max())
    ws_bytes = _lib.load().vqvae_ingest_workspace_bytes(U, max_n)
    assert ws_bytes == U * (1 + max_n // 512) * 12
    y_z, off_z, n_z = ZonedArray(gpu, flat, name='y'), ZonedArray(gpu, y_off, name='y_offset'), ZonedArray(gpu, n, name='n')
    results = []
    for fill in ('poison', 'zero'):
        ws = ZonedArray(gpu, shape=(ws_bytes,), dtype=np.uint8, fill=fill, name='workspace')
        out = ZonedArray(gpu, shape=(U, 4), dtype=np.int32, fill=fill, name='bounds')
        _lib.call('vqvae_ingest_trim_bounds', y_z.ptr, off_z.ptr, n_z.ptr, U, max_n, r, ws.ptr, ws_bytes, out.ptr, gpu.stream())
        gpu.synchronize()
        for z in (ws, out, y_z, off_z, n_z):
            z.check()
        results.append(out.get())
    np.testing.assert_array_equal(results[0], results[1])
    np.testing.assert_array_equal(results[0], want)
    _same(y_z.get(), flat, 'y is not modified')


# ---- 3. pack -----------------------------------------------------------------------------------------------------------------
def test_pack_is_peak_normalise_at_unaligned_offsets(gpu):
    from vqvae_amd import _lib
    from vqvae_amd.inputs import peak_normalise
    ys, want, _ = _signals()
    flat, y_off, n = _bounds_buffers(ys)
    U = len(ys)
    lengths = np.where(want[:, 3] == 0, want[:, 1] - want[:, 0], 0).astype(np.int64)
    dst_off = 5 + np.concatenate(([0], np.cumsum(lengths[:-1] + 3))).astype(np.int64)     # three untouched floats between utterances
    total = int(dst_off[-1] + lengths[-1] + 2)
    y_d, off_d, b_d, dst_off_d = gpu.to_device(flat), gpu.to_device(y_off), gpu.to_device(want), gpu.to_device(dst_off)
    dst = ZonedArray(gpu, shape=(total,), dtype=np.float32, fill='poison', name='dst')
    before = dst.get()
    _lib.call('vqvae_ingest_pack', y_d.ptr, off_d.ptr, b_d.ptr, dst_off_d.ptr, U, int(n.max()), dst.ptr, gpu.stream())
    gpu.synchronize()
    dst.check()
    got = dst.get()
    expect = before.copy()
    for u in range(U):
        if want[u, 3] == 0:
            s, e = int(want[u, 0]), int(want[u, 1])
            expect[dst_off[u]:dst_off[u] + e - s] = peak_normalise(ys[u][s:e])
            _same(peak_normalise(ys[u][s:e]), R.normalise(ys[u], s, e, want[u, 2:3].view(np.float32)[0]))
    _same(got, expect, 'the kept ranges normalised, every other element as it was')
    assert np.abs(got[dst_off[0]:dst_off[0] + lengths[0]]).max() == 1.0


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------
_RAWS = {}


def _raws():
    """Seven raw waves of 48 000 bytes each, 48 kHz int16 mono and 22.05 kHz float32 stereo in turn: a loud burst in faint
    noise, so the trim cuts both ends.  With the restatement's waves."""
    if not _RAWS:
        rs = np.random.RandomState(21)
        raws, srs = [], []
        for i in range(7):
            if i % 2 == 0:
                n, a, b = 24000, 6000 + 300 * i, 17000 + 200 * i
                w = 1e-4 * rs.standard_normal((n, 1))
                w[a:b] += 0.2 * (1 + i) / 8 * rs.standard_normal((b - a, 1))
                raws.append(np.clip(np.round(w * 32768), -32768, 32767).astype(np.int16))
                srs.append(48000)
            else:
                n, a, b = 6000, 2800 + 50 * i, 4000 + 40 * i
                w = 1e-4 * rs.standard_normal((n, 2))
                w[a:b] += 0.4 * rs.standard_normal((b - a, 2))
                raws.append(w.astype(np.float32))
                srs.append(22050)
        ref = []
        for raw, sr in zip(raws, srs):
            w, status = R.process(raw, sr)
            assert status == 0 and 1024 <= len(w) <= R.n_out_of(len(raw), *R.ratio(sr, 16000)[:2]) - 1024   # both ends were trimmed
            w.setflags(write=False)
            ref.append(w)
        assert all(r.nbytes == 48000 for r in raws)
        _RAWS.update(raws=raws, srs=srs, ref=ref, speakers=[(3 * i + 1) % 5 for i in range(7)])
    return _RAWS['raws'], _RAWS['srs'], _RAWS['ref'], _RAWS['speakers']


def _corpora_equal(a, b):
    _same(a.samples.get(), b.samples.get(), 'samples')
    for name in ('lengths', 'offsets', 'speakers'):
        _same(getattr(a, name), getattr(b, name), name)
    for name in ('_length_dev', '_offset_dev', '_speaker_dev'):
        _same(getattr(a, name).get(), getattr(b, name).get(), name)


@pytest.mark.parametrize('batch_bytes,fronts', [(3 * 48000, 5), (64 << 20, 2)])
def test_from_arrays_equals_a_corpus_of_the_restatement(gpu, monkeypatch, batch_bytes, fronts):
    """Three batches of 3, 3 and 1 utterances (two groups, two groups, one group: five copy-resample-bounds rounds), then one
    batch of two groups: the same corpus as ResidentCorpus built from the restatement's waves, and the same draw."""
    from vqvae_amd.corpus import ResidentCorpus, ResidentCorpusIterator
    from vqvae_amd.ingest import DeviceIngest
    raws, srs, ref, speakers = _raws()
    calls = []
    front = DeviceIngest._front
    monkeypatch.setattr(DeviceIngest, '_front', lambda self, items, stage: calls.append(len(items)) or front(self, items, stage))
    got = ResidentCorpus.from_arrays(raws, srs, speakers, batch_bytes=batch_bytes)
    assert len(calls) == fronts and sum(calls) == 7 and got.skipped == []
    want = ResidentCorpus(ref, speakers)
    _same(got.samples.get(), np.concatenate(ref), 'the restatement end to end (already peak-normalised)')
    _corpora_equal(got, want)
    a = ResidentCorpusIterator(got, 5, 400, 71).next().arrays
    b = ResidentCorpusIterator(want, 5, 400, 71).next().arrays
    for x, y in zip(a, b):
        _same(x.get(), y.get())


# ---- 5. files and errors ---------------------------------------------------------------------------------------------------------
def test_from_files_skip_bad_and_errors_name_the_file(gpu, tmp_path):
    from vqvae_amd.corpus import ResidentCorpus
    from vqvae_amd.ingest import corpus_files, read_wav
    raws, srs, ref, _ = _raws()
    names = ['wav48/p225/a.wav', 'wav48/p226/a.wav', 'wav48/p226/b.wav', 'wav48/p230/zero.wav', 'wav48/p230/z.wav']
    data = [raws[0], raws[2], raws[4], np.zeros((18000, 1), np.int16), raws[6]]
    for name, a in zip(names, data):
        path = tmp_path / name
        path.parent.mkdir(parents=True, exist_ok=True)
        with wave.open(str(path), 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(48000)
            w.writeframes(a.astype('<i2').tobytes())
    files, ids, dic = corpus_files(tmp_path, 'VCTK')
    assert [os.path.relpath(f, str(tmp_path)) for f in files] == sorted(names) and ids == [0, 1, 1, 2, 2]
    zero = str(tmp_path / 'wav48/p230/zero.wav')
    with pytest.raises(ValueError) as info:
        ResidentCorpus.from_files(files, ids)
    assert zero in str(info.value) and 'is all zeros' in str(info.value)
    got = ResidentCorpus.from_files(files, ids, skip_bad=True, batch_bytes=100000)
    assert got.skipped == [(zero, 'is all zeros (no peak to normalise by)')] and len(got) == 4
    assert got.speakers.tolist() == [0, 1, 1, 2]
    decoded = [read_wav(f) for f in files if f != zero]
    want = ResidentCorpus.from_arrays([a for a, _ in decoded], [sr for _, sr in decoded], [0, 1, 1, 2])
    _corpora_equal(got, want)
    _same(got.samples.get(), np.concatenate([ref[0], ref[2], ref[4], ref[6]]))
    # arrays: the index is named; a NaN and a wave too short to trim
    bad = raws[1].copy()
    bad[100, 1] = np.nan
    with pytest.raises(ValueError, match='wave 1 holds a non-finite sample'):
        ResidentCorpus.from_arrays([raws[0], bad], [48000, 22050], [0, 1])
    with pytest.raises(ValueError, match='wave 0 is shorter than 1025 samples'):
        ResidentCorpus.from_arrays([raws[0][:3000], raws[2]], 48000, [0, 1])
    with pytest.raises(ValueError, match='wave 1 is empty'):
        ResidentCorpus.from_arrays([raws[0], raws[0][:0]], 48000, [0, 1])
    kept = ResidentCorpus.from_arrays([raws[0][:3000], bad, raws[2]], [48000, 22050, 48000], [4, 5, 6], skip_bad=True)
    assert [i for i, _ in kept.skipped] == [0, 1] and kept.speakers.tolist() == [6]
    _same(kept.samples.get(), ref[2])
    with pytest.raises(ValueError, match='no utterance is left'):
        ResidentCorpus.from_arrays([bad], 22050, [0], skip_bad=True)


# ---- 6. preprocess_wave -----------------------------------------------------------------------------------------------------------
def test_preprocess_wave_feeds_synthesize(gpu):
    import vqvae_amd as V
    raws, srs, ref, _ = _raws()
    front = V.DeviceIngest(sr=16000, res_type='kaiser_fast', top_db=20)
    x = front.preprocess_wave(raws[1], srs[1])
    assert gpu.is_device(x) and x.shape == (1, 1, len(ref[1]), 1) and x.dtype == np.float32
    _same(x.get().reshape(-1), ref[1])
    waves, lengths = front.run([raws[0][:, 0], raws[1]], [48000, 22050])              # a (frames,) array too
    assert lengths.tolist() == [len(ref[0]), len(ref[1])]
    _same(waves[0].get(), ref[0])
    _same(waves[1].get(), ref[1])
    cfg = dict(H.SMALL)
    _, model = H.build_model(cfg, seed=31)
    model.to_gpu()
    speaker = np.array([1], np.int32)
    outs = []
    for x_enc in (x, ref[1].reshape(1, 1, -1, 1)):
        wave_out, out = V.synthesize(model.encoder, model.vq, model.decoder, model.condition_embed, x_enc, speaker,
                                     rng=np.random.RandomState(77), n_steps=6)
        outs.append((wave_out, out))
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
