"""Host side of the pitch tracker (vqvae_amd.pitch, include/vqvae_pitch.h): the lag and frame rules, every argument error
(all raised before anything touches a device), the exported symbols, and the NumPy restatement of the rule
(tests/pitch_ref.py) against the truth.

Measured with the restatement on the tone set of ``pitch_ref.tone_set`` (23 three-harmonic tones, geometrically spaced
between 1.15 fmin and 0.9 fmax, 5 frames each, noise 1e-3, seed 0), worst error against the true frequency:
    (16000, 1024, 256, 60, 400)   0.3496 cents
    (8000, 320, 80, 100, 500)     2.4159 cents
    (4000, 160, 40, 100, 400)     9.1914 cents
every frame voiced; 0 of 41 frames of white noise voiced (lowest d' 0.87, 0.80, 0.74); silence unvoiced, aperiodicity 1.
The tests hold the restatement to twice those figures."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pitch_ref as R
from vqvae_amd import _lib, pitch
from vqvae_amd.backend import DeviceArray
from vqvae_amd.corpus import ResidentCorpus
from vqvae_amd.pitch import PitchConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc')
MEASURED_CENTS = {(16000, 1024, 256, 60.0, 400.0): 0.3496, (8000, 320, 80, 100.0, 500.0): 2.4159,
                  (4000, 160, 40, 100.0, 400.0): 9.1914}


def _cfg(c, **kw):
    return PitchConfig(sr=c[0], frame=c[1], hop=c[2], fmin=c[3], fmax=c[4], **kw)


# ---- the lag and frame rules -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', R.CONFIGS + [(2000, 96, 25, 50.0, 400.0), (22050, 2048, 512, 55.0, 880.0)])
def test_lags_and_frame_count_are_the_brute_force_counts(c):
    cfg = _cfg(c)
    assert (cfg.tau_min, cfg.tau_max, cfg.W) == R.lags(c[0], c[1], c[3], c[4]) == R.lags_brute(c[0], c[1], c[3], c[4])
    assert 2 <= cfg.tau_min < cfg.tau_max and cfg.W == cfg.frame - cfg.tau_max >= 2
    for L in range(cfg.frame, cfg.frame + 3 * cfg.hop + 1):
        assert int(pitch.frame_count(L, cfg)) == R.frame_count(L, cfg.frame, cfg.hop) == 1 + (L - cfg.frame) // cfg.hop
    assert int(pitch.frame_count(cfg.frame - 1, cfg)) == 0 == R.frame_count(cfg.frame - 1, cfg.frame, cfg.hop)
    got = pitch.frame_count(np.arange(cfg.frame, cfg.frame + 5), cfg)
    assert got.dtype == np.int64 and got.shape == (5,)


def test_default_configuration():
    cfg = PitchConfig()
    assert cfg.key() == (16000, 1024, 256, 60.0, 400.0, 0.15, 1e-8)
    assert (cfg.tau_min, cfg.tau_max, cfg.W) == (40, 267, 757)
    assert (R.THRESHOLD, R.MIN_POWER) == (cfg.threshold, cfg.min_power)
    from vqvae_amd.metrics import MelConfig, frame_count            # with frame = n_fft and the same hop the frames coincide
    mel = MelConfig()
    for L in (1024, 1279, 1280, 57600):
        assert int(pitch.frame_count(L, cfg)) == int(frame_count(L, mel))


@pytest.mark.parametrize('kw, msg', [
    (dict(sr=0), 'sr must be positive'), (dict(sr=16000.0), 'sr must be an integer'), (dict(frame=4096), 'frame must be in'),
    (dict(frame=0), 'frame must be in'), (dict(frame=True), 'frame must be an integer'), (dict(hop=0), 'hop must be in'),
    (dict(hop=1025), 'hop must be in'), (dict(fmin=0.0), 'fmin and fmax'), (dict(fmax=float('inf')), 'fmin and fmax'),
    (dict(fmin=float('nan')), 'fmin and fmax'), (dict(fmax=-1.0), 'fmin and fmax'), (dict(fmax=9000.0), 'tau_min'),
    (dict(fmin=400.0, fmax=400.0), 'tau_min'), (dict(fmin=500.0), 'tau_min'), (dict(fmin=15.0), 'W = frame - tau_max'),
    (dict(frame=268), 'W = frame - tau_max'), (dict(threshold=0.0), 'threshold'), (dict(threshold=1.0), 'threshold'),
    (dict(threshold=float('nan')), 'threshold'), (dict(min_power=-1e-9), 'min_power'), (dict(min_power=float('inf')), 'min_power'),
    (dict(min_power=float('nan')), 'min_power'),
])
def test_configuration_errors(kw, msg):
    with pytest.raises(ValueError, match=msg):
        PitchConfig(**kw)


def test_the_smallest_accepted_frame():
    assert PitchConfig(frame=269).W == 2 and PitchConfig(frame=2048).W == 2048 - 267
    assert PitchConfig(min_power=0.0).min_power == 0.0 and PitchConfig(fmax=8000.0).tau_min == 2


# ---- argument errors: all before the first device call ---------------------------------------------------------------
def _fake(n):
    """A DeviceArray that owns nothing: the checks below must refuse the call before any pointer is used."""
    return DeviceArray((n,), np.float32, _block=object(), _ptr=0x10000)


def test_argument_errors_name_the_problem():
    cfg = PitchConfig(sr=4000, frame=160, hop=40, fmin=100.0, fmax=400.0)
    ok, short = np.zeros(200, np.float32), np.zeros(159, np.float32)
    with pytest.raises(ValueError, match='pitch_many: utterance 1 has 159 samples, fewer than one frame \\(frame = 160\\)'):
        pitch.pitch_many([ok, short], cfg)
    with pytest.raises(ValueError, match='pitch_many: utterance 1 has 159 samples'):
        pitch.pitch_many([_fake(200), _fake(159)], cfg)
    with pytest.raises(ValueError, match='compare_pitch_many: utterance 0 has 159 samples'):   # the COMMON length counts
        pitch.compare_pitch_many([ok, ok], [short, ok], cfg)
    with pytest.raises(ValueError, match='compare_pitch_many: 2 reference and 1 test utterances'):
        pitch.compare_pitch_many([ok, ok], [ok], cfg)
    with pytest.raises(ValueError, match='no utterances'):
        pitch.pitch_many([], cfg)
    with pytest.raises(ValueError, match='float32 needed'):
        pitch.pitch_many([DeviceArray((200,), np.int32, _block=object(), _ptr=0x10000)], cfg)
    with pytest.raises(TypeError, match='cfg must be a PitchConfig'):
        pitch.pitch_many([ok], dict(frame=160))
    with pytest.raises(TypeError, match='cfg must be a PitchConfig'):
        pitch.compare_pitch_many([ok], [ok], None)
    with pytest.raises(ValueError, match='chunk_bytes'):
        pitch.pitch_many([ok], cfg, chunk_bytes=0)
    with pytest.raises(ValueError, match='chunk_bytes'):
        pitch.compare_pitch_many([ok], [ok], cfg, chunk_bytes=0)
    with pytest.raises(RuntimeError, match='description only'):
        pitch.pitch_many(ResidentCorpus.describe([200, 160], [0, 1]), cfg)
    with pytest.raises(ValueError, match='pitch_many: utterance 1 has 10 samples'):
        c = ResidentCorpus.describe([200, 10], [0, 1])
        c.samples = _fake(210)
        pitch.pitch_many(c, cfg)


def test_chunks_are_planned_by_the_shared_planner():
    from vqvae_amd import ragged
    cfg = PitchConfig(sr=4000, frame=160, hop=40, fmin=100.0, fmax=400.0)
    frames = np.array([1, 5, 2, 40, 3], np.int64)
    samples = frames * 40 + 120                                      # the samples the frames cover
    assert pitch.plan_chunks(frames, cfg, 1) == [(i, i + 1) for i in range(5)]
    assert pitch.plan_chunks(frames, cfg, 1 << 30) == [(0, 5)]
    assert pitch.plan_chunks(frames, cfg, 4 * 600) == ragged.plan_runs(samples[None], 4 * 600) == [(0, 2), (2, 3), (3, 4), (4, 5)]
    assert pitch.plan_chunks(frames, cfg, 4 * 600, sides=2) == ragged.plan_runs(2 * samples[None], 4 * 600)


# ---- the header, the table, the library ------------------------------------------------------------------------------
NAMES = {'vqvae_pitch_abi_version', 'vqvae_pitch_yin_workspace_bytes', 'vqvae_pitch_compare_workspace_bytes',
         'vqvae_pitch_yin', 'vqvae_pitch_compare'}


def test_header_exports_are_the_bound_table():
    import vqvae_amd as V
    for name in ('PitchConfig', 'RaggedPitch', 'pitch_many', 'compare_pitch_many'):
        assert getattr(V, name) is getattr(pitch, name)
    table = _lib.HEADERS['vqvae_pitch.h'].prototypes           # against the header and the library: tests/test_host_abi.py
    assert set(table) == NAMES
    assert [f[0] for f in _lib.PitchDesc._fields_] == ['n', 'sr', 'frame', 'hop', 'fmin', 'fmax', 'threshold', 'min_power', 'ftot']
    for name, n_args in (('vqvae_pitch_yin', 9), ('vqvae_pitch_compare', 8)):
        assert len(table[name][1]) == n_args
    assert R.THREADS == _lib.PITCH_THREADS and R.COLUMNS == pitch.COLUMNS and len(pitch.COLUMNS) == _lib.PITCH_COLUMNS
    for other in ('vqvae_hip.h', 'vqvae_metrics.h'):       # (vqvae_hip.h speaks of the row pitches of a 2-d copy: another thing)
        assert not re.search(r'vqvae_pitch|\byin\b', open(os.path.join(ROOT, 'include', other)).read(), re.I), other
    assert 'pitch' not in open(os.path.join(ROOT, 'include', 'vqvae_metrics.h')).read().lower()
    assert re.search(r'^SRCS = .*\baudio_pitch\.hip\b', open(os.path.join(CSRC, 'Makefile')).read(), re.M)


def test_c_side_validation_needs_no_device():
    lib = _lib.load()
    fake = 0x10000                                           # never dereferenced: every call below is rejected first
    bad = C.c_size_t(-1).value

    def desc(**kw):
        d = _lib.PitchDesc()
        d.n, d.sr, d.frame, d.hop, d.fmin, d.fmax, d.threshold, d.min_power, d.ftot = 2, 4000, 160, 40, 100.0, 400.0, 0.15, 1e-8, 10
        for name, v in kw.items():
            setattr(d, name, v)
        return d

    def yin(d, x=fake, off_in=fake, frame_off=fake, f0=fake, ap=fake, ws=None, ws_bytes=0):
        return lib.vqvae_pitch_yin(None if d is None else C.byref(d), x, off_in, frame_off, f0, ap, ws, ws_bytes, None)

    def cmp(d, fa=fake, fb=fake, frame_off=fake, out=fake):
        return lib.vqvae_pitch_compare(None if d is None else C.byref(d), fa, fb, frame_off, out, None, 0, None)

    def err():
        return lib.vqvae_last_error_string().decode()

    q_yin = lib.vqvae_pitch_yin_workspace_bytes(C.byref(desc()))
    q_cmp = lib.vqvae_pitch_compare_workspace_bytes(C.byref(desc()))
    assert (q_yin, q_cmp) == (0, 0)
    for kw, msg in ((dict(n=0), 'n must be'), (dict(ftot=0), 'ftot')):
        d = desc(**kw)
        assert yin(d) == -1 and msg in err(), kw
        assert cmp(d) == -1 and msg in err(), kw
        assert lib.vqvae_pitch_yin_workspace_bytes(C.byref(d)) == bad
        assert lib.vqvae_pitch_compare_workspace_bytes(C.byref(d)) == bad
    nan, inf = float('nan'), float('inf')
    for kw, msg in ((dict(sr=0), 'sr must be'), (dict(frame=0), 'frame must be'), (dict(frame=2049, fmin=2.0), 'frame must be'),
                    (dict(hop=0), 'hop'), (dict(hop=161), 'hop'), (dict(threshold=0.0), 'threshold'), (dict(threshold=1.0), 'threshold'),
                    (dict(threshold=nan), 'threshold'), (dict(min_power=-1.0), 'min_power'), (dict(min_power=nan), 'min_power'),
                    (dict(min_power=inf), 'min_power'), (dict(fmin=0.0), 'tau_min'), (dict(fmin=nan), 'tau_min'),
                    (dict(fmax=inf), 'tau_min'), (dict(fmax=-3.0), 'tau_min'), (dict(fmax=2001.0), 'tau_min'),
                    (dict(fmin=400.0), 'tau_min'), (dict(fmin=25.0), 'tau_min'), (dict(fmin=1e-300), 'tau_min'),
                    (dict(frame=41), 'tau_min')):
        d = desc(**kw)
        assert yin(d) == -1 and msg in err(), (kw, err())
        assert lib.vqvae_pitch_yin_workspace_bytes(C.byref(d)) == bad, kw
    assert lib.vqvae_pitch_yin_workspace_bytes(C.byref(desc(frame=42))) == 0                # W = 2
    assert lib.vqvae_pitch_yin_workspace_bytes(C.byref(desc(fmax=2000.0))) == 0             # tau_min = 2
    assert lib.vqvae_pitch_yin_workspace_bytes(None) == bad and lib.vqvae_pitch_compare_workspace_bytes(None) == bad
    assert yin(None) == -1 and 'null descriptor' in err()
    assert cmp(None) == -1 and 'null descriptor' in err()
    for name in ('x', 'off_in', 'frame_off'):
        assert yin(desc(), **{name: None}) == -1 and 'null x' in err(), name
    assert yin(desc(), f0=None, ap=None) == -1 and 'both null' in err()
    assert yin(desc(ftot=1 << 40)) == -1 and 'frame tiles' in err()
    for name in ('fa', 'fb', 'frame_off', 'out'):
        assert cmp(desc(), **{name: None}) == -1 and 'null f0_a' in err(), name


# ---- the restatement against the truth -------------------------------------------------------------------------------
@pytest.mark.parametrize('c', R.TRUTH_CONFIGS, ids=lambda c: 'sr%d_frame%d' % c[:2])
def test_restatement_against_the_truth(c, record_property):
    worst, frames = 0.0, 0
    for f, x in R.tone_set(*c):
        f0, ap, lag = R.track(x, *c)
        assert (f0 > 0).all() and (lag >= R.lags(c[0], c[1], c[3], c[4])[0]).all(), f          # every frame voiced
        assert (ap < R.THRESHOLD).all()
        worst = max(worst, float(np.abs(R.cents(f0, f)).max()))
        frames += len(f0)
    record_property('worst_cents', worst)
    print('%r: worst error %.4f cents over %d frames (recorded %.4f)' % (c, worst, frames, MEASURED_CENTS[c]))
    assert frames == 23 * 5 and worst <= 2 * MEASURED_CENTS[c], (worst, MEASURED_CENTS[c])


@pytest.mark.parametrize('c', R.TRUTH_CONFIGS, ids=lambda c: 'sr%d_frame%d' % c[:2])
def test_noise_and_silence_are_unvoiced(c):
    sr, frame, hop = c[:3]
    noise = np.random.RandomState(0).standard_normal(frame + 40 * hop).astype(np.float32)
    f0, ap, lag = R.track(noise, *c)
    assert len(f0) == 41 and (f0 == 0).all() and (lag == 0).all() and (ap >= R.THRESHOLD).all() and (ap < 1).all()
    for min_power in (R.MIN_POWER, 0.0):        # gated by the power, or d = c = 0 everywhere and d' = 1 by the rule
        f0, ap, lag = R.track(np.zeros(frame + 2 * hop, np.float32), *c, min_power=min_power)
        assert len(f0) == 3 and (f0 == 0).all() and (ap == 1).all()
    quiet = R.tone(150.0, frame + hop, sr) * np.float32(1e-5)                                   # power 6.6e-11: under the gate
    f0, ap, lag = R.track(quiet, *c)
    assert (f0 == 0).all() and (ap == 1).all()
    assert (R.track(quiet, *c, min_power=0.0)[0] > 0).all()


def test_a_power_of_two_gain_changes_no_bit_of_f0():
    c = R.CONFIGS[3]
    waves = [w for w in R.utterance_list(*c)[3:8]]
    for x in waves:
        f0, ap, lag = R.track(x, *c, min_power=0.0)
        for k in (-20, -3, 1, 14):
            g0, gp, glag = R.track(x * np.float32(2.0 ** k), *c, min_power=0.0)
            assert np.array_equal(f0.view(np.uint32), g0.view(np.uint32)) and np.array_equal(ap.view(np.uint32), gp.view(np.uint32)), k
            assert np.array_equal(lag, glag)


def test_pair_statistics_of_the_restatement():
    a = np.array([100.0, 0.0, 200.0, 0.0, 150.0, 300.0], np.float32)
    b = np.array([100.0, 120.0, 0.0, 0.0, 190.0, 150.0], np.float32)
    s = dict(zip(R.COLUMNS, R.pair_stats(a, b)))
    assert (s['voiced_ref'], s['voiced_test'], s['voiced_both']) == (4, 4, 3)
    assert s['vuv_error'] == 2 / 6 and s['gross_error'] == 2 / 3
    want = np.sqrt((0.0 + (1200 * np.log2(190 / 150.0)) ** 2 + 1200.0 ** 2) / 3)
    assert abs(s['f0_rmse_cents'] - want) <= 1e-12 * want
    assert abs(s['log_f0_mean_ref'] - np.log([100.0, 200.0, 150.0, 300.0]).mean()) <= 1e-14
    assert abs(s['log_f0_mean_test'] - np.log([100.0, 120.0, 190.0, 150.0]).mean()) <= 1e-14
    none = dict(zip(R.COLUMNS, R.pair_stats(np.zeros(3, np.float32), np.zeros(3, np.float32))))
    assert (none['voiced_ref'], none['voiced_test'], none['voiced_both'], none['vuv_error']) == (0, 0, 0, 0)
    assert all(np.isnan(none[k]) for k in R.COLUMNS[4:])
    assert R.pair_bounds(a, a)[0] == 0 and (R.pair_bounds(a, a)[1:] > 0).all() and (R.pair_bounds(a, b) > 0).all()
