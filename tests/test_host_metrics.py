"""Host side of the audio metrics (vqvae_amd.metrics, include/vqvae_metrics.h): the frame rule, the tables, the chunk
planner, every argument error (all raised before anything touches a device) and the exported symbols."""
import ctypes as C
import os

import numpy as np
import pytest

import metrics_ref as R
from vqvae_amd import _lib, metrics
from vqvae_amd.backend import DeviceArray
from vqvae_amd.corpus import ResidentCorpus
from vqvae_amd.metrics import MelConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'vqvae_metrics.h')
CSRC = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc')


def _cfg(c):
    return MelConfig(n_fft=c[0], hop=c[1], n_mels=c[2], n_mcep=c[3])


# ---- the frame rule --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', R.CONFIGS)
def test_frame_count_is_the_brute_force_count(c):
    cfg = _cfg(c)
    for L in range(cfg.n_fft, cfg.n_fft + 3 * cfg.hop + 1):
        assert int(metrics.frame_count(L, cfg)) == R.frame_count(L, cfg.n_fft, cfg.hop) == 1 + (L - cfg.n_fft) // cfg.hop
    assert int(metrics.frame_count(cfg.n_fft - 1, cfg)) == 0 == R.frame_count(cfg.n_fft - 1, cfg.n_fft, cfg.hop)
    got = metrics.frame_count(np.arange(cfg.n_fft, cfg.n_fft + 5), cfg)
    assert got.dtype == np.int64 and got.shape == (5,)


# ---- the tables ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', R.CONFIGS)
def test_tables(c):
    cfg = _cfg(c)
    dft, mel, dct = metrics.tables(cfg)
    nb = cfg.nb
    assert (dft.shape, mel.shape, dct.shape) == ((2 * nb, cfg.n_fft), (cfg.n_mels, nb), (cfg.n_mcep, cfg.n_mels))
    assert dft.dtype == mel.dtype == dct.dtype == np.float32
    k = np.arange(cfg.n_fft)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * k / cfg.n_fft)
    w /= w.sum()
    assert abs(w.sum() - 1.0) <= 1e-15 and abs(dft[0].astype(np.float64).sum() - 1.0) <= cfg.n_fft * 2.0 ** -25 * w.max() * 2
    assert np.array_equal(dft[0], w.astype(np.float32))                      # row 0 is the window: cos(0) = 1
    assert np.array_equal(dft[nb], np.zeros(cfg.n_fft, np.float32))          # -w sin(0)
    b = min(3, nb - 1)
    assert np.allclose(dft[b], w * np.cos(2 * np.pi * b * k / cfg.n_fft), rtol=0, atol=1e-9)
    assert np.allclose(dft[nb + b], -w * np.sin(2 * np.pi * b * k / cfg.n_fft), rtol=0, atol=1e-9)
    assert np.abs(dft).sum(axis=1).max() <= 1.0 + 1e-6                        # |re|, |im| <= max |x|
    assert (mel >= 0).all() and (mel != 0).any(axis=1).all()                  # no empty mel row
    # orthonormal DCT-II, rows 1 .. n_mcep: in float64 to 1e-12 (the float32 rounding of the table is not the subject)
    M = cfg.n_mels
    q = np.arange(0, M)[:, None]
    full = np.sqrt(2.0 / M) * np.cos(np.pi * q * (2 * np.arange(M)[None, :] + 1) / (2.0 * M))
    full[0] *= np.sqrt(0.5)
    assert np.abs(full @ full.T - np.eye(M)).max() <= 1e-12
    assert np.array_equal(dct, full[1:cfg.n_mcep + 1].astype(np.float32))
    assert metrics.tables(_cfg(c))[0] is dft                                  # built once per configuration


def test_an_empty_mel_row_is_refused():
    with pytest.raises(ValueError, match='mel row 0 is all zero at n_fft = 64, n_mels = 64'):
        metrics.tables(MelConfig(n_fft=64, hop=16, n_mels=64, n_mcep=4))
    with pytest.raises(ValueError, match='mel row 0 is all zero'):
        metrics.features_many([np.zeros(64, np.float32)], MelConfig(n_fft=64, hop=16, n_mels=64, n_mcep=4))


def test_default_configuration():
    cfg = MelConfig()
    assert cfg.key() == (16000, 1024, 256, 80, 0.0, 8000.0, 13, 1e-10) and cfg.nb == 513
    assert MelConfig(fmax=None, sr=22050).fmax == 11025.0


@pytest.mark.parametrize('kw, msg', [
    (dict(n_fft=1000), 'n_fft must be a multiple of 32'), (dict(n_fft=0), 'n_fft'), (dict(n_fft=4096), 'n_fft'),
    (dict(n_fft=64.0), 'n_fft must be an integer'), (dict(hop=0), 'hop must be in'), (dict(hop=1025), 'hop must be in'),
    (dict(n_mels=0), 'n_mels must be in'), (dict(n_mels=129), 'n_mels must be in'), (dict(n_mcep=0), 'n_mcep must be in'),
    (dict(n_mcep=80), 'n_mcep must be in'), (dict(floor=0.0), 'floor'), (dict(floor=-1.0), 'floor'), (dict(floor=1e-60), 'floor'),
    (dict(floor=float('nan')), 'floor'), (dict(fmin=9000.0), 'fmin'), (dict(fmax=9000.0), 'fmax'), (dict(sr=0), 'sr'),
])
def test_configuration_errors(kw, msg):
    with pytest.raises(ValueError, match=msg):
        MelConfig(**kw)


# ---- the chunk planner -----------------------------------------------------------------------------------------------
def test_planner_against_the_restatement():
    rs = np.random.RandomState(3)
    frames = rs.randint(1, 400, 50)
    for width in (80, 513):
        for budget in (1, 4 * width * 400, 4 * width * 1500, 1 << 30):
            chunks = metrics.plan_chunks(frames, width, budget)
            assert chunks == R.plan_chunks(frames.tolist(), width, budget)
            assert chunks[0][0] == 0 and chunks[-1][1] == len(frames)
            assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:])) and all(b > a for a, b in chunks)
            for a, b in chunks:
                if b - a > 1:
                    assert 4 * width * int(frames[a:b].sum()) <= budget
                if b < len(frames):
                    assert 4 * width * int(frames[a:b + 1].sum()) > budget
    assert metrics.plan_chunks(frames, 513, 1) == [(i, i + 1) for i in range(50)]
    assert metrics.plan_chunks(frames, 513, 1 << 30) == [(0, 50)]
    assert metrics.plan_chunks([2, 2, 5000, 2, 2], 10, 4 * 10 * 4) == [(0, 2), (2, 3), (3, 5)]       # an oversize utterance stands alone
    with pytest.raises(ValueError, match='positive'):
        metrics.plan_chunks([1], 10, 0)


# ---- argument errors: all before the first device call ---------------------------------------------------------------
def _fake(n):
    """A DeviceArray that owns nothing: the checks below must refuse the call before any pointer is used."""
    return DeviceArray((n,), np.float32, _block=object(), _ptr=0x10000)


def test_argument_errors_name_the_problem():
    cfg = MelConfig(n_fft=64, hop=16, n_mels=8, n_mcep=4)
    ok, short = np.zeros(100, np.float32), np.zeros(63, np.float32)
    with pytest.raises(ValueError, match='features_many: utterance 1 has 63 samples, fewer than one frame \\(n_fft = 64\\)'):
        metrics.features_many([ok, short], cfg)
    with pytest.raises(ValueError, match='features_many: utterance 1 has 63 samples'):
        metrics.features_many([_fake(100), _fake(63)], cfg)
    with pytest.raises(ValueError, match='compare_many: utterance 0 has 63 samples'):        # the COMMON length counts
        metrics.compare_many([ok, ok], [short, ok], cfg)
    with pytest.raises(ValueError, match='compare_many: 2 reference and 1 test utterances'):
        metrics.compare_many([ok, ok], [ok], cfg)
    with pytest.raises(ValueError, match='no utterances'):
        metrics.features_many([], cfg)
    with pytest.raises(ValueError, match='float32 needed'):
        metrics.features_many([DeviceArray((100,), np.int32, _block=object(), _ptr=0x10000)], cfg)
    with pytest.raises(TypeError, match='cfg must be a MelConfig'):
        metrics.features_many([ok], dict(n_fft=64))
    with pytest.raises(TypeError, match='cfg must be a MelConfig'):
        metrics.compare_many([ok], [ok], None)
    with pytest.raises(ValueError, match='chunk_bytes'):
        metrics.features_many([ok], cfg, chunk_bytes=0)
    with pytest.raises(RuntimeError, match='description only'):
        metrics.features_many(ResidentCorpus.describe([200, 64], [0, 1]), cfg)
    with pytest.raises(ValueError, match='features_many: utterance 1 has 10 samples'):
        c = ResidentCorpus.describe([200, 10], [0, 1])
        c.samples = _fake(210)
        metrics.features_many(c, cfg)


# ---- the header, the table, the library ------------------------------------------------------------------------------
NAMES = {'vqvae_metrics_abi_version', 'vqvae_metrics_stft_mel_workspace_bytes', 'vqvae_metrics_distances_workspace_bytes',
         'vqvae_metrics_stft_mel', 'vqvae_metrics_distances'}


def test_header_exports_are_the_bound_table():
    import vqvae_amd as V
    for name in ('MelConfig', 'RaggedFeatures', 'features_many', 'compare_many'):
        assert getattr(V, name) is getattr(metrics, name)
    table = _lib.HEADERS['vqvae_metrics.h'].prototypes         # against the header and the library: tests/test_host_abi.py
    assert set(table) == NAMES
    for name, n_args in (('vqvae_metrics_stft_mel', 12), ('vqvae_metrics_distances', 11)):
        assert len(table[name][1]) == n_args
    assert repr(R.DB) in open(HEADER).read() and R.DB == 10.0 / np.log(10.0) and R.THREADS == _lib.METRICS_THREADS
    assert 'metrics' not in open(os.path.join(ROOT, 'include', 'vqvae_hip.h')).read()
    assert 'audio_metrics.hip' in open(os.path.join(CSRC, 'Makefile')).read()


def test_c_side_validation_needs_no_device():
    lib = _lib.load()
    fake = 0x10000                                           # never dereferenced: every call below is rejected first
    bad = C.c_size_t(-1).value

    def desc(**kw):
        d = _lib.MetricsDesc()
        d.n, d.n_fft, d.hop, d.n_mels, d.n_mcep, d.floor, d.ftot, d.stride = 2, 64, 16, 8, 4, 1e-10, 10, 10
        for name, v in kw.items():
            setattr(d, name, v)
        return d

    def stft(d, x=fake, off_in=fake, frame_off=fake, dft=fake, mel=fake, log_mel=fake, mag=fake, mel_pw=None, ws=None,
             ws_bytes=0):
        return lib.vqvae_metrics_stft_mel(None if d is None else C.byref(d), x, off_in, frame_off, dft, mel, log_mel, mag,
                                          mel_pw, ws, ws_bytes, None)

    def dist(d, **kw):
        args = dict(la=fake, lb=fake, ma=fake, mb=fake, dct=fake, frame_off=fake, out=fake)
        args.update(kw)
        return lib.vqvae_metrics_distances(None if d is None else C.byref(d), args['la'], args['lb'], args['ma'], args['mb'],
                                           args['dct'], args['frame_off'], args['out'], None, 0, None)

    def err():
        return lib.vqvae_last_error_string().decode()

    q_stft = lib.vqvae_metrics_stft_mel_workspace_bytes(C.byref(desc()))
    q_dist = lib.vqvae_metrics_distances_workspace_bytes(C.byref(desc()))
    assert q_stft != bad and q_dist != bad
    for kw, msg in ((dict(n=0), 'n must be'), (dict(ftot=0), 'ftot'), (dict(n_fft=48), 'multiple of 32'), (dict(n_fft=0), 'multiple of 32'),
                    (dict(n_fft=4096), 'multiple of 32'), (dict(hop=0), 'hop'), (dict(hop=65), 'hop'), (dict(n_mels=0), 'n_mels'),
                    (dict(n_mels=129), 'n_mels'), (dict(floor=0.0), 'floor'), (dict(stride=9), 'stride')):
        d = desc(**kw)
        assert stft(d) == -1 and msg in err(), kw
        assert dist(d) == -1 and msg in err(), kw
        assert lib.vqvae_metrics_stft_mel_workspace_bytes(C.byref(d)) == bad
        assert lib.vqvae_metrics_distances_workspace_bytes(C.byref(d)) == bad
    for kw in (dict(n_mcep=0), dict(n_mcep=8)):
        assert dist(desc(**kw)) == -1 and 'n_mcep' in err()
        assert lib.vqvae_metrics_distances_workspace_bytes(C.byref(desc(**kw))) == bad
    assert lib.vqvae_metrics_stft_mel_workspace_bytes(None) == bad
    assert stft(None) == -1 and 'null descriptor' in err()
    assert dist(None) == -1 and 'null descriptor' in err()
    for name in ('x', 'off_in', 'frame_off', 'dft', 'mel'):
        assert stft(desc(), **{name: None}) == -1 and 'null x' in err(), name
    assert stft(desc(), log_mel=None, mag=None) == -1 and 'all null' in err()
    assert stft(desc(), dft=fake + 4) == -1 and '16-byte aligned' in err()
    assert stft(desc(ftot=1 << 40, stride=1 << 40)) == -1 and 'frame tiles' in err()
    for name in ('la', 'lb', 'ma', 'mb', 'dct', 'frame_off', 'out'):
        assert dist(desc(), **{name: None}) == -1 and 'null log_mel_a' in err(), name
    # a workspace below the query: both plans are empty today, so the refusal can only be shown where a query is not 0
    if q_stft:
        assert stft(desc(), ws=fake, ws_bytes=q_stft - 1) == -1 and 'workspace' in err()
        assert stft(desc(), ws=None, ws_bytes=q_stft) == -1 and 'workspace' in err()
    assert (q_stft, q_dist) == (0, 0)
