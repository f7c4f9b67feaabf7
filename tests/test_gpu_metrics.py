"""Audio metrics on the device (vqvae_amd.metrics, include/vqvae_metrics.h) against the float64 restatement of the rule
(tests/metrics_ref.py), with DERIVED error bounds; bit equality of an utterance's features in every arrangement; the
distance kernel against the exact restatement of its own order; red zones round every output of both entry points.

Bounds (eps = 2^-24, A_f = sum_k |w[k] x[f hop + k]| in float64):
  d_mag = 2 (n_fft + 4) eps A_f                      the standard dot-product bound, valid for any summation order
  d_mel = sum_b mel[m, b] (2 mag d_mag + d_mag^2 + 4 eps pw) + (nb + 3) eps mel
  d_log = 2 d_mel / mel + 2^-21 max(1, |log mel|)    wherever mel >= 2 d_mel (everywhere, with the signals' noise floor)
and, because these are loose, the RMS error over all elements is at most 4 x that of a float32 NumPy evaluation of the
same rule (the margin covers the matrix pipe's different summation order).  Measured ratios are recorded as properties.
"""
import ctypes as C

import numpy as np
import pytest

import metrics_ref as R
import zoned as Z
from vqvae_amd import _lib, metrics
from vqvae_amd.corpus import ResidentCorpus
from vqvae_amd.metrics import MelConfig

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


class Ref(object):
    """Float64 features of one wave and the bounds that go with them."""

    def __init__(self, x, tabs, cfg, with_f32=False):
        n_fft, hop, nb = cfg.n_fft, cfg.hop, cfg.nb
        self.mag, self.mel, self.log_mel, self.pw = R.features(x, tabs, n_fft, hop, cfg.floor)
        A = R.window_l1(x, tabs, n_fft, hop)
        self.d_mag = 2 * (n_fft + 4) * EPS * A[None, :] * np.ones((nb, 1))
        melw = tabs[1].astype(np.float64)
        self.d_mel = melw @ (2 * self.mag * self.d_mag + self.d_mag ** 2 + 4 * EPS * self.pw) + (nb + 3) * EPS * self.mel
        self.log_ok = self.mel >= 2 * self.d_mel
        with np.errstate(divide='ignore', invalid='ignore'):
            self.d_log = 2 * self.d_mel / self.mel + 2.0 ** -21 * np.maximum(1.0, np.abs(np.log(self.mel)))
        if with_f32:
            self.mag32, self.mel32 = R.features(x, tabs, n_fft, hop, cfg.floor, np.float32)[:2]


class Case(object):
    pass


@pytest.fixture(scope='module', params=R.CONFIGS, ids=lambda c: 'nfft%d_hop%d_mel%d' % c[:3])
def case(request, gpu):
    """Per configuration, computed once and left unchanged: the list, its float64 reference and the device's features of
    the list in one call."""
    n_fft, hop, n_mels, n_mcep = request.param
    c = Case()
    c.cfg = MelConfig(n_fft=n_fft, hop=hop, n_mels=n_mels, n_mcep=n_mcep)
    c.tabs = metrics.tables(c.cfg)
    c.waves = R.utterance_list(n_fft, hop)
    c.ref = [Ref(x, c.tabs, c.cfg, with_f32=True) for x in c.waves]
    c.feats = metrics.features_many(c.waves, c.cfg, magnitudes=True, mel_powers=True)
    c.blocks = [c.feats.utterance(i) for i in range(len(c.waves))]
    return c


def _same(a, b):
    return all(np.array_equal(np.ascontiguousarray(p).view(np.uint32), np.ascontiguousarray(q).view(np.uint32)) for p, q in zip(a, b))


# ---- values ----------------------------------------------------------------------------------------------------------
def test_frames_and_layout(case):
    f = case.feats
    assert f.frames.tolist() == R.FRAME_COUNTS and f.frame_off.tolist() == np.concatenate([[0], np.cumsum(R.FRAME_COUNTS)]).tolist()
    ftot = sum(R.FRAME_COUNTS)
    assert f.log_mel.shape == (case.cfg.n_mels, ftot) and f.mag.shape == (case.cfg.nb, ftot) and f.mel.shape == f.log_mel.shape
    assert f.frame_off.dtype == np.int64 and len(f) == 8
    for (lm, mg, ml), F in zip(case.blocks, R.FRAME_COUNTS):
        assert lm.shape == (case.cfg.n_mels, F) and mg.shape == (case.cfg.nb, F) and ml.shape == lm.shape
    with pytest.raises(IndexError):
        f.utterance(8)


def test_values_within_the_derived_bounds(case, record_property):
    worst = dict(mag=0.0, mel=0.0, log=0.0)
    outside = total = 0
    sq = dict(mag_dev=0.0, mag_np=0.0, mel_dev=0.0, mel_np=0.0)
    for (lm, mg, ml), r in zip(case.blocks, case.ref):
        e_mag = np.abs(mg.astype(np.float64) - r.mag)
        e_mel = np.abs(ml.astype(np.float64) - r.mel)
        e_log = np.abs(lm.astype(np.float64) - np.log(r.mel))
        worst['mag'] = max(worst['mag'], (e_mag / r.d_mag).max())
        worst['mel'] = max(worst['mel'], (e_mel / r.d_mel).max())
        worst['log'] = max(worst['log'], (e_log[r.log_ok] / r.d_log[r.log_ok]).max())
        outside += int((~r.log_ok).sum())
        total += r.log_ok.size
        sq['mag_dev'] += (e_mag ** 2).sum()
        sq['mel_dev'] += (e_mel ** 2).sum()
        sq['mag_np'] += ((r.mag32.astype(np.float64) - r.mag) ** 2).sum()
        sq['mel_np'] += ((r.mel32.astype(np.float64) - r.mel) ** 2).sum()
    ratio_mag, ratio_mel = np.sqrt(sq['mag_dev'] / sq['mag_np']), np.sqrt(sq['mel_dev'] / sq['mel_np'])
    for k, v in worst.items():
        record_property('device_over_bound_%s' % k, float(v))
    record_property('device_over_numpy_float32_rms_mag', float(ratio_mag))
    record_property('device_over_numpy_float32_rms_mel', float(ratio_mel))
    record_property('log_elements_outside_the_condition', '%d of %d' % (outside, total))
    print('n_fft %d: device / bound mag %.4f mel %.4f log %.4f; device / numpy float32 RMS mag %.3f mel %.3f; %d of %d outside'
          % (case.cfg.n_fft, worst['mag'], worst['mel'], worst['log'], ratio_mag, ratio_mel, outside, total))
    assert worst['mag'] <= 1.0 and worst['mel'] <= 1.0 and worst['log'] <= 1.0, worst
    assert outside <= 0.01 * total
    assert ratio_mag <= 4.0 and ratio_mel <= 4.0, (ratio_mag, ratio_mel)


def test_the_longest_frame_reads_its_samples_directly(gpu):
    """n_fft 2048: the power spectrum takes 131 KB of LDS and no window can be staged beside it, so EVERY tile reads its
    samples from global memory, the tiles inside one utterance too.  Same bounds, same bit equalities."""
    cfg = MelConfig(n_fft=2048, hop=512, n_mels=80, n_mcep=13)
    tabs = metrics.tables(cfg)
    rs = np.random.RandomState(2)
    waves = []
    for F in (1, 34, 2):
        L = cfg.n_fft + cfg.hop * (F - 1) + 7
        t = np.arange(L) / 16000.0
        x = 0.5 * np.sin(2 * np.pi * 440 * t) + 0.25 * np.sin(2 * np.pi * 2900 * t + 1) + 0.1 * rs.randn(L)
        waves.append((x / np.abs(x).max()).astype(np.float32))
    feats = metrics.features_many(waves, cfg, magnitudes=True, mel_powers=True)
    assert feats.frames.tolist() == [1, 34, 2]
    for i, x in enumerate(waves):
        lm, mg, ml = feats.utterance(i)
        r = Ref(x, tabs, cfg)
        assert r.log_ok.all()
        assert (np.abs(mg.astype(np.float64) - r.mag) <= r.d_mag).all()
        assert (np.abs(ml.astype(np.float64) - r.mel) <= r.d_mel).all()
        assert (np.abs(lm.astype(np.float64) - np.log(r.mel)) <= r.d_log).all()
        assert _same(metrics.features_many([x], cfg, magnitudes=True, mel_powers=True).utterance(0), (lm, mg, ml)), i


# ---- bit equalities --------------------------------------------------------------------------------------------------
def test_an_utterance_is_the_same_bits_in_every_arrangement(case, gpu):
    cfg, waves, blocks = case.cfg, case.waves, case.blocks
    n = len(waves)
    kw = dict(magnitudes=True, mel_powers=True)
    for i, x in enumerate(waves):                                                   # alone
        assert _same(metrics.features_many([x], cfg, **kw).utterance(0), blocks[i]), i
    rev = metrics.features_many(waves[::-1], cfg, **kw)                             # the reversed list
    assert all(_same(rev.utterance(n - 1 - i), blocks[i]) for i in range(n))
    loud = [np.float32(1e3) * np.random.RandomState(9 + i).randn(cfg.n_fft + 3 * cfg.hop + 5).astype(np.float32) for i in range(n + 1)]
    mixed = [loud[0]]
    for i, x in enumerate(waves):
        mixed += [x, loud[i + 1]]
    mix = metrics.features_many(mixed, cfg, **kw)                                   # between neighbours of amplitude 1e3
    assert all(_same(mix.utterance(2 * i + 1), blocks[i]) for i in range(n))
    one = metrics.features_many(waves, cfg, chunk_bytes=1, **kw)                    # one utterance per chunk
    assert metrics.plan_chunks(case.feats.frames, cfg.nb, 1) == [(i, i + 1) for i in range(n)]
    assert all(_same(one.utterance(i), blocks[i]) for i in range(n))
    assert metrics.plan_chunks(case.feats.frames, cfg.nb, 1 << 30) == [(0, n)]     # ... and the fixture's call was one chunk
    dev = metrics.features_many([gpu.to_device(x) for x in waves], cfg, **kw)       # device arrays
    assert all(_same(dev.utterance(i), blocks[i]) for i in range(n))
    half = [gpu.to_device(x) if i % 2 else x for i, x in enumerate(waves)]          # host and device arrays mixed
    assert all(_same(metrics.features_many(half, cfg, chunk_bytes=4 * cfg.nb * 40, **kw).utterance(i), blocks[i]) for i in range(n))
    only = metrics.features_many(waves, cfg)                                        # log_mel alone (mag and mel_pw NULL)
    assert only.mag is None and only.mel is None
    assert all(_same(only.utterance(i)[:1], blocks[i][:1]) and only.utterance(i)[1] is None for i in range(n))


def test_a_resident_corpus_is_read_in_place(case, gpu):
    cfg, waves, blocks = case.cfg, case.waves, case.blocks
    n = len(waves)
    kw = dict(magnitudes=True, mel_powers=True)
    corpus = ResidentCorpus(waves, list(range(n)))              # the waves' peak is exactly 1: stored as they are
    held = corpus.samples.get()
    assert all(np.array_equal(held[int(o):int(o) + len(x)], x) for o, x in zip(corpus.offsets, waves))
    got = metrics.features_many(corpus, cfg, **kw)
    assert all(_same(got.utterance(i), blocks[i]) for i in range(n))
    order = [5, 0, 7, 7, 2]
    view = metrics.features_many(corpus.subset(order), cfg, chunk_bytes=4 * cfg.nb * 34, **kw)
    assert view.frames.tolist() == [R.FRAME_COUNTS[i] for i in order]
    assert all(_same(view.utterance(j), blocks[i]) for j, i in enumerate(order))
    if cfg.n_fft == 1024:                                       # from raw audio (ingest needs 1025 samples: the default's list has them)
        raw = ResidentCorpus.from_arrays(waves, 16000, list(range(n)), top_db=80)
        host = raw.samples.get()
        own = [host[int(o):int(o) + int(L)].copy() for o, L in zip(raw.offsets, raw.lengths)]
        assert min(len(x) for x in own) >= cfg.n_fft
        a, b = metrics.features_many(raw, cfg, **kw), metrics.features_many(own, cfg, **kw)
        assert a.frames.tolist() == b.frames.tolist()
        assert all(_same(a.utterance(i), b.utterance(i)) for i in range(len(own)))


def test_trailing_samples_and_silence(case):
    cfg, waves, blocks = case.cfg, case.waves, case.blocks
    kw = dict(magnitudes=True, mel_powers=True)
    changed = []
    for x, F in zip(waves, R.FRAME_COUNTS):
        used = cfg.n_fft + cfg.hop * (F - 1)
        y = x.copy()
        y[used:] = 1e6                                           # belongs to no frame
        changed.append(y)
    assert any(len(x) > cfg.n_fft + cfg.hop * (F - 1) for x, F in zip(waves, R.FRAME_COUNTS))
    got = metrics.features_many(changed, cfg, **kw)
    assert all(_same(got.utterance(i), blocks[i]) for i in range(len(waves)))
    silent = [waves[3], np.zeros(cfg.n_fft + 2 * cfg.hop, np.float32), waves[6]]
    lm, mg, ml = metrics.features_many(silent, cfg, **kw).utterance(1)
    # mel is exactly 0, so every element is logf(floor): ONE value, the device's logf of the float32 floor.  That function
    # is accurate to 1 ulp, not correctly rounded (at 1e-10 it returns the neighbour of the rounded logarithm), so the
    # value is pinned to within one ulp of log(floor) and every element to that value's bits.
    assert (mg == 0).all() and (ml == 0).all() and not np.signbit(ml).any()
    want = np.float32(np.log(np.float64(np.float32(cfg.floor))))
    assert lm.shape == (cfg.n_mels, 3) and (lm.view(np.uint32) == lm.view(np.uint32)[0, 0]).all(), (lm.min(), lm.max())
    assert abs(float(lm[0, 0]) - float(want)) <= float(np.spacing(np.abs(want))), (lm[0, 0], want)
    again = metrics.features_many([np.zeros(cfg.n_fft, np.float32)], cfg).utterance(0)[0]      # alone, one frame: the same bits
    assert again.shape == (cfg.n_mels, 1) and (again.view(np.uint32) == lm.view(np.uint32)[0, 0]).all()


# ---- distances -------------------------------------------------------------------------------------------------------
def _perturbed(waves, cut=1):
    rs = np.random.RandomState(4)
    return [(x[:len(x) - cut] + np.float32(0.05) * rs.randn(len(x) - cut).astype(np.float32)).astype(np.float32) for x in waves]


def test_distances_are_the_exact_restatement_of_the_kernels_order(case):
    cfg, waves = case.cfg, case.waves
    test = _perturbed(waves)
    got = metrics.compare_many(waves, test, cfg)
    common = [min(len(a), len(b)) for a, b in zip(waves, test)]
    frames = [1 + (L - cfg.n_fft) // cfg.hop for L in common]
    assert got['frames'].tolist() == frames and got['frames'].dtype == np.int64
    assert frames != R.FRAME_COUNTS                                               # an even frame count lost its last frame
    for k in ('log_mel_mae', 'mcd_db', 'spectral_convergence'):
        assert got[k].dtype == np.float64 and got[k].shape == (len(waves),) and np.isfinite(got[k]).all() and (got[k] > 0).all()
    cut_a, cut_b = [a[:L] for a, L in zip(waves, common)], [b[:L] for b, L in zip(test, common)]
    fa = metrics.features_many(cut_a, cfg, magnitudes=True)
    fb = metrics.features_many(cut_b, cfg, magnitudes=True)
    for i in range(len(waves)):
        (la, ma), (lb, mb) = fa.utterance(i), fb.utterance(i)
        want = R.distances_exact(la, lb, ma, mb, case.tabs[2])
        have = np.array([got['log_mel_mae'][i], got['mcd_db'][i], got['spectral_convergence'][i]])
        assert np.array_equal(have.view(np.uint64), want.view(np.uint64)), (i, have, want)
    pre = metrics.compare_many(cut_a, cut_b, cfg)                                 # the common prefix, cut by the caller
    chunked = metrics.compare_many(waves, test, cfg, chunk_bytes=1)
    for k in got:
        assert np.array_equal(got[k], pre[k]) and np.array_equal(got[k], chunked[k]), k
    swapped = metrics.compare_many(test, waves, cfg)                              # the longer wave on the other side
    assert np.array_equal(swapped['log_mel_mae'], got['log_mel_mae']) and np.array_equal(swapped['frames'], got['frames'])


def test_identical_waves_and_a_gain_of_two(case, gpu):
    cfg, waves = case.cfg, case.waves
    same = metrics.compare_many(waves, [x.copy() for x in waves], cfg)
    for k in ('log_mel_mae', 'mcd_db', 'spectral_convergence'):
        assert (same[k] == 0).all() and not np.signbit(same[k]).any(), (k, same[k])
    assert same['frames'].tolist() == R.FRAME_COUNTS
    twice = [np.float32(2) * x for x in waves]                                    # exact in float32
    got = metrics.compare_many(waves, twice, cfg)
    for i, r in enumerate(case.ref):
        # the log bound of both sides (the test side's mel is 4 x the reference's and so are its bounds: the relative part
        # is the same, the absolute part is taken at log mel + ln 4)
        d_log_b = 2 * r.d_mel / r.mel + 2.0 ** -21 * np.maximum(1.0, np.abs(np.log(4 * r.mel)))
        tol = (r.d_log + d_log_b).mean() * (1 + 1e-12)
        assert abs(got['log_mel_mae'][i] - 2 * np.log(2.0)) <= tol, (i, got['log_mel_mae'][i], tol)
        assert 0 <= got['mcd_db'][i] < 1e-3                                        # a gain moves only c0, which is left out
        assert abs(got['spectral_convergence'][i] - 1.0) <= 1e-6                   # |2 m - m| / |m|, both from exact doublings
    quiet = metrics.compare_many([np.zeros_like(waves[2]), np.zeros_like(waves[2])], [waves[2], np.zeros_like(waves[2])], cfg)
    assert np.isposinf(quiet['spectral_convergence'][0]) and np.isnan(quiet['spectral_convergence'][1])   # as IEEE divides
    assert quiet['log_mel_mae'][1] == 0 and quiet['mcd_db'][1] == 0


def test_scores_agree_with_float64_from_the_waves(case, record_property):
    """Tolerances derived from the per-element bounds (e = d_log of both sides added; g = d_mag):
      log_mel_mae  | |x + dx| - |x| | <= |dx|                     ->  mean(e)
      mcd_db       c_q moves by at most 0.5 sum_m |dct[q, m]| e[m]; the 2-norm over q by at most the 2-norm of that
                   (triangle inequality); times C sqrt(2), mean over the frames
      spectral_convergence = N / D with N, D Frobenius norms: |dN| <= |g_a|_F + |g_b|_F, |dD| <= |g_a|_F
                   ->  (|dN| + sc |dD|) / (D - |dD|)
    each with a relative 1e-12 for the float64 sums of either side."""
    cfg, waves = case.cfg, case.waves
    test = _perturbed(waves, cut=0)
    got = metrics.compare_many(waves, test, cfg)
    dct = case.tabs[2].astype(np.float64)
    worst = np.zeros(3)
    for i, (ra, y) in enumerate(zip(case.ref, test)):
        rb = Ref(y, case.tabs, cfg)
        assert ra.log_ok.all() and rb.log_ok.all()
        want = R.distances(ra.log_mel, rb.log_mel, ra.mag, rb.mag, dct)
        e = ra.d_log + rb.d_log
        ga, gb = np.sqrt((ra.d_mag ** 2).sum()), np.sqrt((rb.d_mag ** 2).sum())
        D = np.sqrt((ra.mag ** 2).sum())
        tol = np.array([e.mean(),
                        (R.DB * np.sqrt(2.0) * np.sqrt(((0.5 * np.abs(dct) @ e) ** 2).sum(axis=0))).mean(),
                        ((ga + gb) + want[2] * ga) / (D - ga)]) * (1 + 1e-12) + 1e-12 * np.abs(want)
        have = np.array([got['log_mel_mae'][i], got['mcd_db'][i], got['spectral_convergence'][i]])
        worst = np.maximum(worst, np.abs(have - want) / tol)
        assert (np.abs(have - want) <= tol).all(), (i, have, want, tol)
    record_property('score_error_over_tolerance', [float(w) for w in worst])
    print('n_fft %d: score error / tolerance (mae, mcd, sc) %s' % (cfg.n_fft, worst))


# ---- red zones -------------------------------------------------------------------------------------------------------
def _desc(cfg, n, ftot):
    d = _lib.MetricsDesc()
    d.n, d.n_fft, d.hop, d.n_mels, d.n_mcep, d.floor, d.ftot, d.stride = n, cfg.n_fft, cfg.hop, cfg.n_mels, cfg.n_mcep, cfg.floor, ftot, ftot
    return d


@pytest.mark.parametrize('outputs', ['all', 'log_mel', 'mag'])
def test_stft_mel_writes_inside_its_outputs(case, gpu, outputs):
    """The list holds tiles inside one utterance (staged samples) and tiles that span several (direct reads)."""
    cfg, waves = case.cfg, case.waves
    n, ftot = len(waves), sum(R.FRAME_COUNTS)
    off_in = np.concatenate([[0], np.cumsum([len(x) for x in waves])[:-1]]).astype(np.int64)
    d = _desc(cfg, n, ftot)
    lib = _lib.load()
    need = lib.vqvae_metrics_stft_mel_workspace_bytes(C.byref(d))
    assert need != C.c_size_t(-1).value
    specs = dict(x=Z.In(np.concatenate(waves)), off_in=Z.In(off_in), frame_off=Z.In(case.feats.frame_off),
                 dft=Z.In(case.tabs[0]), mel=Z.In(case.tabs[1]), ws=Z.Ws(max(need, 256)))
    if outputs in ('all', 'log_mel'):
        specs['log_mel'] = Z.Out((cfg.n_mels, ftot))
    if outputs in ('all', 'mag'):
        specs['mag'] = Z.Out((cfg.nb, ftot))
    if outputs == 'all':
        specs['mel_pw'] = Z.Out((cfg.n_mels, ftot))

    def run(b):
        _lib.call('vqvae_metrics_stft_mel', C.byref(d), b.x.ptr, b.off_in.ptr, b.frame_off.ptr, b.dft.ptr, b.mel.ptr,
                  b['log_mel'].ptr if 'log_mel' in b else None, b['mag'].ptr if 'mag' in b else None,
                  b['mel_pw'].ptr if 'mel_pw' in b else None, b.ws.ptr, need, gpu.stream())

    out = Z.run_contract(gpu, run, specs)
    whole = [np.concatenate([blk[j] for blk in case.blocks], axis=1) for j in range(3)]
    for name, j in (('log_mel', 0), ('mag', 1), ('mel_pw', 2)):
        if name in out:
            assert _same([out[name]], [whole[j]]), name


def test_distances_write_inside_their_output(case, gpu):
    cfg, waves = case.cfg, case.waves
    n, ftot = len(waves), sum(R.FRAME_COUNTS)
    other = metrics.features_many(_perturbed(waves, cut=0), cfg, magnitudes=True)
    d = _desc(cfg, n, ftot)
    need = _lib.load().vqvae_metrics_distances_workspace_bytes(C.byref(d))
    assert need != C.c_size_t(-1).value
    la, ma = case.feats.log_mel.get(), case.feats.mag.get()
    lb, mb = other.log_mel.get(), other.mag.get()
    specs = dict(la=Z.In(la), lb=Z.In(lb), ma=Z.In(ma), mb=Z.In(mb), dct=Z.In(case.tabs[2]), frame_off=Z.In(case.feats.frame_off),
                 out=Z.Out((n, 3), np.float64), ws=Z.Ws(max(need, 256)))

    def run(b):
        _lib.call('vqvae_metrics_distances', C.byref(d), b.la.ptr, b.lb.ptr, b.ma.ptr, b.mb.ptr, b.dct.ptr, b.frame_off.ptr,
                  b.out.ptr, b.ws.ptr, need, gpu.stream())

    out = Z.run_contract(gpu, run, specs)['out']
    fo = case.feats.frame_off
    for i in range(n):
        a, b = int(fo[i]), int(fo[i + 1])
        want = R.distances_exact(la[:, a:b], lb[:, a:b], ma[:, a:b], mb[:, a:b], case.tabs[2])
        assert np.array_equal(out[i].view(np.uint64), want.view(np.uint64)), i
