"""The speaker-identity kernels (csrc/speaker_id.hip) against tests/speakerid_ref.py: everything the device computes is float64
+ - * in one written order, so every comparison here is an equality of bits, at the smallest shapes that still cross each
edge: utterances of 1, 2 and 3 frames (both delta edges coincide), lists that cross the 256-frame tiles of the features
kernel, frame counts on both sides of the 256 lanes of the reduce, D of 1, 12, 26 and 48 (one to many accumulator tiles, the
three instantiations of the score kernel), 1, 8, 9 and 109 models (one tile, a tile + 1, many)."""
import ctypes as C

import numpy as np
import pytest

import speakerid_ref as R
import zoned as Z
from vqvae_amd import _lib, metrics, speakerid
from vqvae_amd.corpus import ResidentCorpus
from vqvae_amd.metrics import MelConfig, RaggedFeatures

pytestmark = pytest.mark.gpu

N_MELS = 32
LANE_EDGES = [1, 255, 256, 257, 1000]
DIMS = {1: (1, False), 12: (6, True), 26: (13, True), 48: (24, True)}        # D: (n_mcep, deltas)
NAN = np.uint64(0x7ff8000000000000)


def _cfg(n_mcep, n_mels=N_MELS):
    return MelConfig(n_fft=256, hop=64, n_mels=n_mels, n_mcep=n_mcep)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _log_mel(frames, seed, quiet=0.0):
    """Random log-mel blocks (n_mels, F) float32; a share ``quiet`` of the frames lies 10 nepers a band below the rest."""
    rs = np.random.RandomState(seed)
    blocks = []
    for F in frames:
        loud = rs.uniform(size=F) >= quiet
        blocks.append(np.where(loud[None, :], rs.uniform(-1.0, 0.0, (N_MELS, F)), rs.uniform(-12.0, -10.0, (N_MELS, F))).astype(np.float32))
    return blocks


def _feats(gpu, cfg, blocks):
    """The blocks as features_many would have left them: one channel-major device tensor."""
    return RaggedFeatures(cfg, [b.shape[1] for b in blocks], gpu.to_device(np.ascontiguousarray(np.concatenate(blocks, axis=1))), None)


def _sf(gpu, D, xs, keeps):
    """A RaggedSpeakerFeatures over given host blocks: the statistics and score kernels take any x."""
    n_mcep, deltas = DIMS[D]
    return speakerid.RaggedSpeakerFeatures(_cfg(n_mcep), [len(x) for x in xs], deltas, None,
                                           gpu.to_device(np.concatenate(xs)), gpu.to_device(np.concatenate(keeps).astype(np.uint8)))


def _blocks(D, frames, seed, scale=1.0):
    rs = np.random.RandomState(seed)
    xs = [scale * rs.standard_normal((F, D)) for F in frames]
    keeps = [rs.uniform(size=F) < 0.8 for F in frames]
    for k in keeps:
        k[rs.randint(len(k))] = True
    return xs, keeps


def _gaussians(D, G, seed):
    rs = np.random.RandomState(seed)
    mu = rs.standard_normal((G, D))
    linv = np.tril(rs.standard_normal((G, D, D))) * 0.3
    linv[:, np.arange(D), np.arange(D)] = rs.uniform(0.5, 2.0, (G, D))
    return mu, linv


# ---- features ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('deltas', [True, False], ids=['deltas', 'static'])
@pytest.mark.parametrize('n_mcep', [1, 6, 13, 24])
@pytest.mark.parametrize('frames', [[1, 2, 3, 70], [300, 1, 255, 257, 2]], ids=['edges', 'tiles'])
def test_features_equal_the_restatement(gpu, frames, n_mcep, deltas):
    cfg = _cfg(n_mcep)
    dct = metrics.tables(cfg)[2]
    blocks = _log_mel(frames, 10 * n_mcep + len(frames), quiet=0.3)
    feats = _feats(gpu, cfg, blocks)
    for gate_db in (None, 20.0):
        sf = speakerid.speaker_features(feats, deltas, gate_db)
        assert (sf.D, sf.x.shape, sf.keep.shape, sf.keep.dtype) == (n_mcep * (2 if deltas else 1), (sum(frames), sf.D), (sum(frames),), np.uint8)
        assert sf.frames.tolist() == frames and sf.frame_off.tolist() == np.concatenate([[0], np.cumsum(frames)]).tolist()
        thr = R.threshold(N_MELS, gate_db)
        for i, b in enumerate(blocks):
            x, keep = sf.utterance(i)
            wx, wk = R.features(b, dct, deltas, thr)
            assert _same(x, wx), (i, gate_db)
            assert np.array_equal(keep, wk) and keep.any(), (i, gate_db)
            if gate_db is not None and frames[i] >= 70:
                assert not keep.all()                                    # the planted quiet frames are dropped
    # the static half is vqvae_align_cepstra's output
    ftot = sum(frames)
    c = gpu.DeviceArray((ftot, n_mcep), np.float64)
    d = _lib.AlignDesc(len(frames), N_MELS, n_mcep, 1, ftot, ftot, ftot, ftot, ftot, ftot)
    _lib.call('vqvae_align_cepstra', C.byref(d), 0, feats.log_mel.ptr, gpu.to_device(dct).ptr, c.ptr, None, 0, gpu.stream())
    assert _same(sf.x.get()[:, :n_mcep], c.get())


def test_a_resident_corpus_read_in_place_equals_host_waves(gpu):
    cfg = MelConfig(**R.VOICE_CFG)
    ew, es, _, _ = R.voices()
    corpus = ResidentCorpus(ew, es)
    held = corpus.samples.get()
    own = [held[int(o):int(o) + int(L)].copy() for o, L in zip(corpus.offsets, corpus.lengths)]
    a = speakerid.speaker_features(metrics.features_many(corpus, cfg), gate_db=20.0)
    b = speakerid.speaker_features(metrics.features_many(own, cfg), gate_db=20.0)
    assert _same(a.x.get(), b.x.get()) and np.array_equal(a.keep.get(), b.keep.get())
    ma = corpus.fit_speakers(cfg, gate_db=20.0)
    mb = speakerid.fit_speakers(b, es)
    assert ma.G == 4 and ma.gate_db == 20.0 and np.array_equal(ma.count, mb.count) and _same(ma.S1, mb.S1) and _same(ma.S2, mb.S2)
    order = [7, 0, 3, 10]
    view = corpus.subset(order).fit_speakers(cfg, n_speakers=4, ridge=1e-6, gate_db=20.0)
    part = speakerid.fit_speakers(metrics.features_many([own[i] for i in order], cfg), es[order], 4, gate_db=20.0, ridge=1e-6)
    assert _same(view.S2, part.S2) and _same(view.linv, part.linv)


# ---- statistics --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', sorted(DIMS))
def test_statistics_equal_the_restatement(gpu, D):
    xs, keeps = _blocks(D, LANE_EDGES, 40 + D)
    cnt, s1, s2 = speakerid.speaker_stats(_sf(gpu, D, xs, keeps))
    assert s1.shape == (5, D) and s2.shape == (5, D * (D + 1) // 2) and cnt.dtype == np.int64
    for i, (x, k) in enumerate(zip(xs, keeps)):
        wc, w1, w2 = R.stats(x, k)
        assert cnt[i] == wc and _same(s1[i], w1) and _same(s2[i], w2), i


def test_statistics_do_not_depend_on_the_list(gpu):
    D = 26
    xs, keeps = _blocks(D, LANE_EDGES, 77)
    cnt, s1, s2 = speakerid.speaker_stats(_sf(gpu, D, xs, keeps))
    for i in (0, 3, 4):                                                  # alone
        c, a, b = speakerid.speaker_stats(_sf(gpu, D, xs[i:i + 1], keeps[i:i + 1]))
        assert c[0] == cnt[i] and _same(a[0], s1[i]) and _same(b[0], s2[i]), i
    c, a, b = speakerid.speaker_stats(_sf(gpu, D, xs[::-1], keeps[::-1]))     # reversed
    assert np.array_equal(c[::-1], cnt) and _same(a[::-1], s1) and _same(b[::-1], s2)
    loud, lk = _blocks(D, [3, 300, 256, 1, 700, 2], 78, scale=1e3)       # beside neighbours a thousand times larger
    mix_x = [v for pair in zip(loud, xs + xs[:1]) for v in pair]
    mix_k = [v for pair in zip(lk, keeps + keeps[:1]) for v in pair]
    c, a, b = speakerid.speaker_stats(_sf(gpu, D, mix_x, mix_k))
    assert np.array_equal(c[1::2][:5], cnt) and _same(a[1::2][:5], s1) and _same(b[1::2][:5], s2)


# ---- score -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,G', [(1, 1), (1, 109), (12, 8), (12, 9), (26, 1), (26, 9), (26, 109), (48, 1), (48, 9)])
def test_scores_equal_the_restatement(gpu, D, G):
    xs, keeps = _blocks(D, LANE_EDGES, 50 + D + G)
    mu, linv = _gaussians(D, G, 60 + D + G)
    q, cnt = speakerid.score_raw(_sf(gpu, D, xs, keeps), mu, speakerid.pack_lower(linv))
    assert q.shape == (5, G) and cnt.tolist() == [int(k.sum()) for k in keeps]
    for i, (x, k) in enumerate(zip(xs, keeps)):
        want, n = R.score(x, k, mu, linv)
        assert n == cnt[i] and _same(q[i], want), (i, np.abs(q[i] - want).max())


def test_scores_do_not_depend_on_the_list_or_the_table(gpu):
    D, G = 26, 19
    xs, keeps = _blocks(D, LANE_EDGES, 91)
    mu, linv = _gaussians(D, G, 92)
    packed = speakerid.pack_lower(linv)
    q, cnt = speakerid.score_raw(_sf(gpu, D, xs, keeps), mu, packed)
    perm = np.random.RandomState(93).permutation(G)                      # a model moved in the table, into another tile
    qp, _ = speakerid.score_raw(_sf(gpu, D, xs, keeps), mu[perm], packed[perm])
    assert _same(qp, q[:, perm])
    qs, _ = speakerid.score_raw(_sf(gpu, D, xs, keeps), mu[11:12], packed[11:12])    # a model alone
    assert _same(qs[:, 0], q[:, 11])
    for i in (0, 2, 4):                                                  # an utterance alone
        qa, ca = speakerid.score_raw(_sf(gpu, D, xs[i:i + 1], keeps[i:i + 1]), mu, packed)
        assert ca[0] == cnt[i] and _same(qa[0], q[i]), i
    loud, lk = _blocks(D, [5, 400, 256, 1, 30], 94, scale=1e3)
    mix_x = [v for pair in zip(loud, xs[::-1]) for v in pair]
    mix_k = [v for pair in zip(lk, keeps[::-1]) for v in pair]
    qm, cm = speakerid.score_raw(_sf(gpu, D, mix_x, mix_k), mu, packed)
    assert _same(qm[1::2][::-1], q) and np.array_equal(cm[1::2][::-1], cnt)


@pytest.mark.parametrize('gate_db', [None, 20.0], ids=['every_frame', 'gated'])
def test_identify_many_on_the_synthetic_voices(gpu, gate_db):
    cfg = MelConfig(**R.VOICE_CFG)
    dct = metrics.tables(cfg)[2]
    ew, es, tw, ts = R.voices()
    sc = speakerid.identify_many(ew, es, tw, cfg, gate_db=gate_db)
    m = sc.models
    assert (m.G, m.D, m.gate_db, sc.q.shape) == (4, 12, gate_db, (8, 4))
    thr = R.threshold(cfg.n_mels, gate_db)
    # the models' raw sums: the restatement over the device's own log-mel, summed per speaker in list order
    fe, ft = metrics.features_many(ew, cfg), metrics.features_many(tw, cfg)
    per = [R.stats(*R.features(fe.utterance(i)[0], dct, True, thr)) for i in range(len(ew))]
    Cn, S1, S2 = R.speaker_sums(per, es, 4)
    assert np.array_equal(m.count, Cn) and _same(m.S1, S1) and _same(m.S2, S2)
    # the scores: the restatement fed the same linv
    q = np.stack([R.score(*R.features(ft.utterance(i)[0], dct, True, thr), m.mu, m.linv)[0] for i in range(len(tw))])
    assert _same(sc.q, q) and _same(sc.ll, R.log_likelihood(q, m.logdet, 12))
    assert np.array_equal(sc.identified, ts) and sc.accuracy(ts) == 1.0 and (sc.llr(ts) > 0).all()
    again = speakerid.score_speakers(m, speakerid.speaker_features(ft, True, gate_db))
    assert _same(again.q, sc.q) and np.array_equal(again.count, sc.count)


# ---- contracts -----------------------------------------------------------------------------------------------------------------
def test_every_entry_point_writes_inside_its_outputs(gpu):
    n_mcep, D, G = 6, 12, 9
    frames = [1, 257, 40, 2]
    ftot, N, T = sum(frames), len(frames), D * (D + 1) // 2
    cfg = _cfg(n_mcep)
    dct = metrics.tables(cfg)[2]
    blocks = _log_mel(frames, 5, quiet=0.3)
    off = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    thr = R.threshold(N_MELS, 20.0)
    d = speakerid.SpkDesc(N, N_MELS, n_mcep, 1, D, G, 1, 0, ftot, ftot, float(thr))
    lib, st = speakerid.load(), gpu.stream

    def run_features(b):
        speakerid.call('vqvae_spk_features', C.byref(d), b.log_mel.ptr, b.dct.ptr, b.off.ptr, b.x.ptr, b.keep.ptr, st())

    out = Z.run_contract(gpu, run_features, dict(log_mel=Z.In(np.concatenate(blocks, axis=1)), dct=Z.In(dct), off=Z.In(off),
                                                 x=Z.Out((ftot, D), np.float64), keep=Z.Out((ftot,), np.uint8)))
    want = [R.features(b, dct, True, thr) for b in blocks]
    x, keep = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
    assert _same(out['x'], x) and np.array_equal(out['keep'], keep.astype(np.uint8))

    def run_stats(b):
        speakerid.call('vqvae_spk_stats', C.byref(d), b.x.ptr, b.keep.ptr, b.off.ptr, b.s1.ptr, b.s2.ptr, b.cnt.ptr, st())

    ins = dict(x=Z.In(x), keep=Z.In(keep.astype(np.uint8)), off=Z.In(off))
    out = Z.run_contract(gpu, run_stats, dict(ins, s1=Z.Out((N, D), np.float64), s2=Z.Out((N, T), np.float64), cnt=Z.Out((N,), np.int64)))
    for i, (wx, wk) in enumerate(want):
        wc, w1, w2 = R.stats(wx, wk)
        assert out['cnt'][i] == wc and _same(out['s1'][i], w1) and _same(out['s2'][i], w2), i

    mu, linv = _gaussians(D, G, 6)

    def run_score(b):
        speakerid.call('vqvae_spk_score', C.byref(d), b.x.ptr, b.keep.ptr, b.off.ptr, b.mu.ptr, b.linv.ptr, b.q.ptr, b.cnt.ptr, st())

    out = Z.run_contract(gpu, run_score, dict(ins, mu=Z.In(mu), linv=Z.In(speakerid.pack_lower(linv)), q=Z.Out((N, G), np.float64),
                                              cnt=Z.Out((N,), np.int64)))
    for i, (wx, wk) in enumerate(want):
        wq, wc = R.score(wx, wk, mu, linv)
        assert out['cnt'][i] == wc and _same(out['q'][i], wq), i
    assert lib.vqvae_spk_revision() == 1


def test_a_bad_descriptor_is_refused_without_a_launch(gpu):
    lib = speakerid.load()
    N, D, G, ftot = 2, 12, 3, 10
    bufs = dict((n, Z.ZonedArray(gpu, shape=s, dtype=t, name=n)) for n, s, t in (
        ('x', (ftot, D), np.float64), ('keep', (ftot,), np.uint8), ('s1', (N, D), np.float64), ('s2', (N, 78), np.float64),
        ('cnt', (N,), np.int64), ('q', (N, G), np.float64)))
    lm, dct = gpu.to_device(np.zeros((N_MELS, ftot), np.float32)), gpu.to_device(np.zeros((6, N_MELS), np.float32))
    off = gpu.to_device(np.array([0, 4, 10], np.int64))
    mu, lp = gpu.to_device(np.zeros((G, D))), gpu.to_device(np.ones((G, 78)))
    st = gpu.stream()
    p = dict((n, z.ptr) for n, z in bufs.items())
    calls = {'spk_features': lambda d, **kw: lib.vqvae_spk_features(d, lm.ptr, dct.ptr, off.ptr, kw.get('x', p['x']), p['keep'], st),
             'spk_stats': lambda d, **kw: lib.vqvae_spk_stats(d, p['x'], p['keep'], off.ptr, p['s1'], kw.get('s2', p['s2']), p['cnt'], st),
             'spk_score': lambda d, **kw: lib.vqvae_spk_score(d, p['x'], p['keep'], off.ptr, mu.ptr, lp.ptr, kw.get('q', p['q']), p['cnt'], st)}
    good = lambda: speakerid.SpkDesc(N, N_MELS, 6, 1, D, G, 1, 0, ftot, ftot, 50.0)

    def refused(who, rc, words):
        msg = lib.vqvae_last_error_string().decode()
        assert rc != 0 and who in msg and words in msg, (who, rc, msg, words)

    for who, entry in calls.items():
        for field, value, words in (('n', 0, 'n must be at least 1'), ('n_mels', 129, 'n_mels must be in'), ('n_mcep', 32, 'n_mcep must be in'),
                                    ('deltas', -1, 'deltas must be 0 or 1'), ('dim', 13, 'dim must be n_mcep * (1 + deltas)'),
                                    ('n_models', 524281, 'n_models must be in'), ('use_gate', 2, 'use_gate must be 0 or 1'),
                                    ('reserved', 7, 'reserved must be 0'), ('ftot', 1, 'ftot must be at least n'),
                                    ('stride', 9, 'stride must be at least ftot'), ('thr', float('nan'), 'thr must be finite')):
            d = good()
            setattr(d, field, value)
            refused(who, entry(C.byref(d)), words)
        refused(who, entry(None), 'null descriptor')
    refused('spk_features', calls['spk_features'](C.byref(good()), x=None), 'null log_mel')
    refused('spk_stats', calls['spk_stats'](C.byref(good()), s2=None), 'null x, keep')
    refused('spk_score', calls['spk_score'](C.byref(good()), q=None), 'null x, keep')
    none = good()
    none.n_models = 0
    refused('spk_score', calls['spk_score'](C.byref(none)), 'n_models must be at least 1')
    gpu.synchronize()
    for name, z in bufs.items():                            # nothing ran: every payload still holds its poison, every zone its pattern
        z.check()
        assert np.array_equal(z.arr.get().view(np.uint8).reshape(-1), z.initial), name


def test_a_contradicting_frame_off_is_skipped_and_marked(gpu):
    """Utterance 1 of [0, 50, 30, 90] ends before it begins: it is marked and its neighbours' results stand, 0 over frames
    [0, 50) and 2 over [30, 90).  A table whose total is not ftot marks every utterance."""
    n_mcep, D, G, ftot = 6, 12, 3, 90
    cfg = _cfg(n_mcep)
    dct = metrics.tables(cfg)[2]
    lm = _log_mel([ftot], 8, quiet=0.3)[0]
    thr = R.threshold(N_MELS, 20.0)
    mu, linv = _gaussians(D, G, 9)
    lm_d, dct_d = gpu.to_device(lm), gpu.to_device(dct)
    mu_d, lp_d = gpu.to_device(mu), gpu.to_device(speakerid.pack_lower(linv))
    d = speakerid.SpkDesc(3, N_MELS, n_mcep, 1, D, G, 1, 0, ftot, ftot, float(thr))

    def run(table):
        off = gpu.to_device(np.array(table, np.int64))
        x, keep = gpu.DeviceArray((ftot, D), np.float64), gpu.DeviceArray((ftot,), np.uint8)
        s1, s2, cnt = gpu.DeviceArray((3, D), np.float64), gpu.DeviceArray((3, 78), np.float64), gpu.DeviceArray((3,), np.int64)
        q, cq = gpu.DeviceArray((3, G), np.float64), gpu.DeviceArray((3,), np.int64)
        speakerid.call('vqvae_spk_features', C.byref(d), lm_d.ptr, dct_d.ptr, off.ptr, x.ptr, keep.ptr, gpu.stream())
        speakerid.call('vqvae_spk_stats', C.byref(d), x.ptr, keep.ptr, off.ptr, s1.ptr, s2.ptr, cnt.ptr, gpu.stream())
        speakerid.call('vqvae_spk_score', C.byref(d), x.ptr, keep.ptr, off.ptr, mu_d.ptr, lp_d.ptr, q.ptr, cq.ptr, gpu.stream())
        return x.get(), keep.get().astype(bool), s1.get(), s2.get(), cnt.get(), q.get(), cq.get()

    x, keep, s1, s2, cnt, q, cq = run([0, 50, 30, 90])
    x0, k0 = R.features(lm[:, :50], dct, True, thr)         # frames [0, 50) are found in utterance 0, [50, 90) in utterance 2
    x2, k2 = R.features(lm[:, 30:], dct, True, thr)
    assert _same(x[:50], x0) and np.array_equal(keep[:50], k0) and _same(x[50:], x2[20:]) and np.array_equal(keep[50:], k2[20:])
    assert cnt.tolist() == cq.tolist() == [int(keep[:50].sum()), 0, int(keep[30:].sum())]
    assert (_bits(s1[1]) == NAN).all() and (_bits(s2[1]) == NAN).all() and (_bits(q[1]) == NAN).all()
    for i, (a, b) in ((0, (0, 50)), (2, (30, 90))):
        wc, w1, w2 = R.stats(x[a:b], keep[a:b])
        wq, _ = R.score(x[a:b], keep[a:b], mu, linv)
        assert _same(s1[i], w1) and _same(s2[i], w2) and _same(q[i], wq), i
    for table in ([0, 50, 70, 100], [0, 50, 70, 80], [1, 50, 70, 90]):
        x, keep, s1, s2, cnt, q, cq = run(table)
        assert (_bits(x) == NAN).all() and not keep.any() and cnt.tolist() == cq.tolist() == [0, 0, 0], table
        assert (_bits(s1) == NAN).all() and (_bits(s2) == NAN).all() and (_bits(q) == NAN).all(), table
