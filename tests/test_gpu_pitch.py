"""Pitch and voicing on the device (vqvae_amd.pitch, include/vqvae_pitch.h) against the NumPy restatement of the rule
(tests/pitch_ref.py): f0 and aperiodicity equal it in EVERY bit, in every arrangement of the list; the pair statistics
equal the restatement of their own order where they are exact and stay within a derived bound where the device's log and
log2 enter; red zones round every output of both entry points.

The bound of the three log-based columns (pitch_ref.pair_bounds): the ROCm documentation installed beside the compiler
states no accuracy for the float64 log and log2 of the device library, so 4 ulp per term is taken, summed over the terms,
plus one ulp of the largest partial sum per addition (an addition may round the other way once its inputs differ).
Measured on an MI355X: the device uses at most 0.07 of that bound on the lists below (recorded as a property)."""
import ctypes as C

import numpy as np
import pytest

import pitch_ref as R
import zoned as Z
from vqvae_amd import _lib, pitch
from vqvae_amd.corpus import ResidentCorpus
from vqvae_amd.pitch import PitchConfig

pytestmark = pytest.mark.gpu
SEMITONE = 2.0 ** (1.0 / 12.0)


def _cfg(c, **kw):
    return PitchConfig(sr=c[0], frame=c[1], hop=c[2], fmin=c[3], fmax=c[4], **kw)


class Case(object):
    pass


@pytest.fixture(scope='module', params=R.CONFIGS, ids=lambda c: 'sr%d_frame%d_hop%d' % c[:3])
def case(request, gpu):
    """Per configuration, computed once and left unchanged: the list and the same list a semitone up, the restatement's
    tracks of both and the device's tracks of both, each in one call."""
    c = Case()
    c.c = request.param
    c.cfg = _cfg(c.c)
    c.waves = R.utterance_list(*c.c)
    c.up = R.utterance_list(*c.c, shift=SEMITONE)
    c.ref = [R.track(x, *c.c) for x in c.waves]
    c.ref_up = [R.track(x, *c.c) for x in c.up]
    c.track = pitch.pitch_many(c.waves, c.cfg)
    c.track_up = pitch.pitch_many(c.up, c.cfg)
    c.blocks = [c.track.utterance(i) for i in range(len(c.waves))]
    c.blocks_up = [c.track_up.utterance(i) for i in range(len(c.up))]
    return c


def _same(a, b):
    return all(p.dtype == q.dtype == np.float32 and p.shape == q.shape and np.array_equal(p.view(np.uint32), q.view(np.uint32))
               for p, q in zip(a, b))


# ---- the tracker -----------------------------------------------------------------------------------------------------
def test_frames_and_layout(case):
    t = case.track
    assert t.frames.tolist() == R.FRAME_COUNTS and t.frame_off.tolist() == np.concatenate([[0], np.cumsum(R.FRAME_COUNTS)]).tolist()
    assert t.f0.shape == t.aperiodicity.shape == (sum(R.FRAME_COUNTS),) and t.f0.dtype == np.float32
    assert t.frame_off.dtype == np.int64 and len(t) == 8
    for (f0, ap), F in zip(case.blocks, R.FRAME_COUNTS):
        assert f0.shape == ap.shape == (F,)
    with pytest.raises(IndexError):
        t.utterance(8)


def test_the_list_holds_the_cases_it_is_there_for(case):
    """On the restatement: the last lag without refinement, the first lag, silence, noise, an onset, two pitches."""
    tau_min, tau_max, W = R.lags(case.c[0], case.c[1], case.c[3], case.c[4])
    ref = case.ref
    assert ref[0][2].tolist() == [tau_max] and ref[0][0][0] == np.float32(case.c[0] / np.float64(tau_max))      # tau* = tau
    assert ref[1][2].tolist() == [tau_min]
    assert (ref[2][0] == 0).all() and (ref[2][1] == 1).all()
    assert (ref[4][0] == 0).all() and (ref[4][1] >= R.THRESHOLD).all() and (ref[4][1] < 1).all()
    assert (ref[3][0] > 0).all() and (ref[7][0] > 0).all()
    assert ref[5][0][0] == 0 and ref[5][1][0] == 1 and ref[5][0][-1] > 0 and 0 < (ref[5][0] > 0).sum() < len(ref[5][0])
    assert len(set(ref[6][2].tolist()) - {0}) >= 2


def test_f0_and_aperiodicity_equal_the_restatement_in_every_bit(case):
    for i, ((f0, ap), (rf0, rap, lag)) in enumerate(zip(case.blocks, case.ref)):
        assert _same((f0, ap), (rf0, rap)), (i, f0, rf0, ap, rap)
    for i, ((f0, ap), (rf0, rap, lag)) in enumerate(zip(case.blocks_up, case.ref_up)):
        assert _same((f0, ap), (rf0, rap)), (i, f0, rf0, ap, rap)


def test_an_utterance_is_the_same_bits_in_every_arrangement(case, gpu):
    cfg, waves, blocks = case.cfg, case.waves, case.blocks
    n = len(waves)
    for i, x in enumerate(waves):                                                   # alone
        assert _same(pitch.pitch_many([x], cfg).utterance(0), blocks[i]), i
    rev = pitch.pitch_many(waves[::-1], cfg)                                        # the reversed list
    assert all(_same(rev.utterance(n - 1 - i), blocks[i]) for i in range(n))
    loud = [np.float32(1e3) * np.random.RandomState(9 + i).randn(cfg.frame + 3 * cfg.hop + 5).astype(np.float32) for i in range(n + 1)]
    mixed = [loud[0]]
    for i, x in enumerate(waves):
        mixed += [x, loud[i + 1]]
    mix = pitch.pitch_many(mixed, cfg)                                              # between neighbours of amplitude 1e3
    assert all(_same(mix.utterance(2 * i + 1), blocks[i]) for i in range(n))
    one = pitch.pitch_many(waves, cfg, chunk_bytes=1)                               # one utterance per chunk
    assert pitch.plan_chunks(case.track.frames, cfg, 1) == [(i, i + 1) for i in range(n)]
    assert all(_same(one.utterance(i), blocks[i]) for i in range(n))
    assert pitch.plan_chunks(case.track.frames, cfg, 1 << 30) == [(0, n)]      # ... and the fixture's call was one chunk
    dev = pitch.pitch_many([gpu.to_device(x) for x in waves], cfg)                  # device arrays
    assert all(_same(dev.utterance(i), blocks[i]) for i in range(n))
    half = [gpu.to_device(x) if i % 2 else x for i, x in enumerate(waves)]          # host and device arrays mixed, three chunks
    some = pitch.pitch_many(half, cfg, chunk_bytes=4 * (cfg.frame + 40 * cfg.hop))
    assert all(_same(some.utterance(i), blocks[i]) for i in range(n))


def test_a_resident_corpus_is_read_in_place(case, gpu):
    """The corpus peak-normalises what it stores (and takes no silent wave): its own samples, read back, are the list that
    the in-place reading must agree with."""
    cfg = case.cfg
    keep = [i for i in range(len(case.waves)) if i != 2]
    corpus = ResidentCorpus([case.waves[i] for i in keep], list(range(len(keep))))
    held = corpus.samples.get()
    own = [held[int(o):int(o) + int(L)].copy() for o, L in zip(corpus.offsets, corpus.lengths)]
    assert [len(x) for x in own] == [len(case.waves[i]) for i in keep]
    want = pitch.pitch_many(own, cfg)
    got = pitch.pitch_many(corpus, cfg)
    assert got.frames.tolist() == [R.FRAME_COUNTS[i] for i in keep]
    assert all(_same(got.utterance(j), want.utterance(j)) for j in range(len(keep)))
    assert any((want.utterance(j)[0] > 0).any() for j in range(len(keep)))
    order = [5, 0, 6, 6, 2]
    view = pitch.pitch_many(corpus.subset(order), cfg, chunk_bytes=4 * (cfg.frame + 33 * cfg.hop))
    assert view.frames.tolist() == [want.frames[j] for j in order]
    assert all(_same(view.utterance(k), want.utterance(j)) for k, j in enumerate(order))


def test_samples_behind_the_last_frame_change_nothing(case):
    cfg, waves = case.cfg, case.waves
    changed = []
    for x, F in zip(waves, R.FRAME_COUNTS):
        y = x.copy()
        y[cfg.frame + cfg.hop * (F - 1):] = 1e6                   # belongs to no frame
        changed.append(y)
    assert sum(len(x) > cfg.frame + cfg.hop * (F - 1) for x, F in zip(waves, R.FRAME_COUNTS)) >= 5
    got = pitch.pitch_many(changed, cfg)
    assert all(_same(got.utterance(i), case.blocks[i]) for i in range(len(waves)))


@pytest.mark.parametrize('c', [(4000, 151, 25, 90.0, 410.0), (4000, 152, 25, 90.0, 410.0), (16000, 2048, 512, 8.0, 400.0),
                               (16000, 2048, 512, 7.8203, 400.0)], ids=['W106', 'W107', 'frame2048_tau2000', 'frame2048_tau2046'])
def test_the_other_tails_and_the_largest_tile(gpu, c):
    """W = 106 and 107 leave two and three terms behind the last group of four (the four configurations above leave none
    or one); frame 2048 with tau_max 2000 takes 157 KB of LDS for its four frames, which must be asked for, and with
    tau_max 2046 (W = 2: the tail alone) all 160 KB of a CU."""
    cfg = _cfg(c)
    assert (cfg.W % 4 in (2, 3)) or 64 + 4 * (16 * (cfg.tau_max + 1) + 4 * cfg.frame) > 64 * 1024
    rs = np.random.RandomState(5)
    waves = [R.tone(150.0, cfg.frame, c[0], rs), R.tone(210.0, cfg.frame + 5 * cfg.hop + 3, c[0], rs, noise=0.05),
             np.zeros(cfg.frame + cfg.hop, np.float32), (0.2 * rs.standard_normal(cfg.frame + 2 * cfg.hop)).astype(np.float32)]
    got = pitch.pitch_many(waves, cfg)
    assert got.frames.tolist() == [1, 6, 2, 3]
    for i, x in enumerate(waves):
        f0, ap, lag = R.track(x, *c)
        assert _same(got.utterance(i), (f0, ap)), (i, got.utterance(i), f0, ap)


# ---- red zones -------------------------------------------------------------------------------------------------------
def _desc(cfg, n, ftot):
    return pitch._desc(cfg, n, ftot)


@pytest.mark.parametrize('outputs', ['both', 'f0', 'aperiodicity'])
def test_yin_writes_inside_its_outputs(case, gpu, outputs):
    cfg, waves = case.cfg, case.waves
    n, ftot = len(waves), sum(R.FRAME_COUNTS)
    off_in = np.concatenate([[0], np.cumsum([len(x) for x in waves])[:-1]]).astype(np.int64)
    d = _desc(cfg, n, ftot)
    need = _lib.load().vqvae_pitch_yin_workspace_bytes(C.byref(d))
    assert need != C.c_size_t(-1).value
    specs = dict(x=Z.In(np.concatenate(waves)), off_in=Z.In(off_in), frame_off=Z.In(case.track.frame_off), ws=Z.Ws(max(need, 256)))
    if outputs in ('both', 'f0'):
        specs['f0'] = Z.Out((ftot,))
    if outputs in ('both', 'aperiodicity'):
        specs['aperiodicity'] = Z.Out((ftot,))

    def run(b):
        _lib.call('vqvae_pitch_yin', C.byref(d), b.x.ptr, b.off_in.ptr, b.frame_off.ptr, b['f0'].ptr if 'f0' in b else None,
                  b['aperiodicity'].ptr if 'aperiodicity' in b else None, b.ws.ptr, need, gpu.stream())

    out = Z.run_contract(gpu, run, specs)
    whole = [np.concatenate([blk[j] for blk in case.blocks]) for j in range(2)]
    for name, j in (('f0', 0), ('aperiodicity', 1)):
        if name in out:
            assert _same([out[name]], [whole[j]]), name


def test_compare_writes_inside_its_output(case, gpu):
    n, ftot = len(case.waves), sum(R.FRAME_COUNTS)
    d = _desc(case.cfg, n, ftot)
    need = _lib.load().vqvae_pitch_compare_workspace_bytes(C.byref(d))
    assert need != C.c_size_t(-1).value
    fa, fb = case.track.f0.get(), case.track_up.f0.get()
    specs = dict(fa=Z.In(fa), fb=Z.In(fb), frame_off=Z.In(case.track.frame_off), out=Z.Out((n, 8), np.float64, nan_ok=True),
                 ws=Z.Ws(max(need, 256)))

    def run(b):
        _lib.call('vqvae_pitch_compare', C.byref(d), b.fa.ptr, b.fb.ptr, b.frame_off.ptr, b.out.ptr, b.ws.ptr, need, gpu.stream())

    out = Z.run_contract(gpu, run, specs)['out']
    fo = case.track.frame_off
    for i in range(n):
        want = R.pair_stats(fa[int(fo[i]):int(fo[i + 1])], fb[int(fo[i]):int(fo[i + 1])])
        assert np.array_equal(out[i, :5].view(np.uint64), want[:5].view(np.uint64)), (i, out[i], want)


# ---- the pair statistics ---------------------------------------------------------------------------------------------
def _rows(scores):
    return np.stack([scores[k] for k in R.COLUMNS], axis=1)


def test_pair_statistics_against_the_restatement(case, record_property):
    """The test side is a semitone up and one sample short, as synthesize_many's waves are: an even frame count loses its
    last frame.  Counts, vuv_error and gross_error in every bit; the log-based three within pair_bounds."""
    cfg, waves = case.cfg, case.waves
    test = [x[:-1] for x in case.up]
    got = pitch.compare_pitch_many(waves, test, cfg)
    common = [min(len(a), len(b)) for a, b in zip(waves, test)]
    frames = [1 + (L - cfg.frame) // cfg.hop for L in common]
    assert got['frames'].tolist() == frames != R.FRAME_COUNTS and got['frames'].dtype == np.int64
    rows = _rows(got)
    assert rows.dtype == np.float64 and rows.shape == (len(waves), 8)
    worst = 0.0
    for i, F in enumerate(frames):
        fa, fb = case.blocks[i][0][:F], case.blocks_up[i][0][:F]       # a frame's track does not depend on what follows it
        want, bound = R.pair_stats(fa, fb), R.pair_bounds(fa, fb)
        assert np.array_equal(rows[i, :5].view(np.uint64), want[:5].view(np.uint64)), (i, rows[i], want)
        for k in range(3):
            have, ref = rows[i, 5 + k], want[5 + k]
            assert np.isnan(have) == np.isnan(ref), (i, k, have, ref)
            if not np.isnan(ref):
                print('pair %d %s: device %.17g restatement %.17g bound %.3g' % (i, R.COLUMNS[5 + k], have, ref, bound[k]))
                assert abs(have - ref) <= bound[k], (i, R.COLUMNS[5 + k], have, ref, bound[k])
                worst = max(worst, abs(have - ref) / bound[k])
    record_property('log_columns_over_bound', float(worst))
    print('sr %d frame %d: log-based columns use %.4f of their bound' % (cfg.sr, cfg.frame, worst))
    pre = pitch.compare_pitch_many([a[:L] for a, L in zip(waves, common)], test, cfg)             # cut by the caller
    chunked = pitch.compare_pitch_many(waves, test, cfg, chunk_bytes=1)
    for k in got:
        assert np.array_equal(got[k], pre[k], equal_nan=True) and np.array_equal(got[k], chunked[k], equal_nan=True), k
    assert np.array_equal(_rows(pre).view(np.uint64), rows.view(np.uint64)) and np.array_equal(_rows(chunked).view(np.uint64), rows.view(np.uint64))
    swapped = pitch.compare_pitch_many(test, waves, cfg)                                         # the longer wave on the other side
    assert np.array_equal(swapped['voiced_ref'], got['voiced_test']) and np.array_equal(swapped['frames'], got['frames'])
    assert np.array_equal(swapped['log_f0_mean_test'].view(np.uint64), got['log_f0_mean_ref'].view(np.uint64))


def test_identical_waves_a_semitone_and_no_voiced_frame(case):
    cfg, waves = case.cfg, case.waves
    same = pitch.compare_pitch_many(waves, [x.copy() for x in waves], cfg)
    assert same['frames'].tolist() == R.FRAME_COUNTS
    assert (same['vuv_error'] == 0).all() and np.array_equal(same['voiced_ref'], same['voiced_test'])
    assert np.array_equal(same['voiced_ref'], same['voiced_both'])
    assert same['voiced_ref'].tolist() == [float((b[0] > 0).sum()) for b in case.blocks]
    voiced = same['voiced_both'] > 0
    assert voiced.tolist() == [True, True, False, True, False, True, True, True]
    for k in ('gross_error', 'f0_rmse_cents'):
        assert (same[k][voiced] == 0).all() and not np.signbit(same[k][voiced]).any(), (k, same[k])
    assert np.array_equal(same['log_f0_mean_ref'].view(np.uint64), same['log_f0_mean_test'].view(np.uint64))
    # no voiced frame (silence, noise): the empty sets divide as IEEE divides
    for k in ('gross_error', 'f0_rmse_cents', 'log_f0_mean_ref', 'log_f0_mean_test'):
        assert np.isnan(same[k][~voiced]).all() and np.isfinite(same[k][voiced]).all(), (k, same[k])
    assert (same['voiced_ref'][~voiced] == 0).all() and (same['vuv_error'][~voiced] == 0).all()
    # silence against a tone: every frame is a voicing error, nothing is voiced on both sides
    one = pitch.compare_pitch_many([waves[2]], [np.resize(waves[3], len(waves[2]))], cfg)
    assert one['vuv_error'][0] == 1 and one['voiced_ref'][0] == 0 and one['voiced_test'][0] == one['frames'][0] == 2
    assert np.isnan(one['gross_error'][0]) and np.isnan(one['f0_rmse_cents'][0]) and np.isnan(one['log_f0_mean_ref'][0])
    assert np.isfinite(one['log_f0_mean_test'][0])
    # a semitone up: each frame's interval is within the two sides' truth errors of 100 cents, and so is their RMS
    up = pitch.compare_pitch_many(waves, case.up, cfg)
    for i, f in R.list_tones(case.c[3], case.c[4]).items():
        e_ref = np.abs(R.cents(case.ref[i][0], f)).max()
        e_up = np.abs(R.cents(case.ref_up[i][0], f * SEMITONE)).max()
        assert up['voiced_both'][i] == R.FRAME_COUNTS[i] and up['gross_error'][i] == 0 and up['vuv_error'][i] == 0
        print('utterance %d: rmse %.4f cents, truth errors %.4f + %.4f' % (i, up['f0_rmse_cents'][i], e_ref, e_up))
        assert abs(up['f0_rmse_cents'][i] - 100.0) <= e_ref + e_up + 1e-9, (i, up['f0_rmse_cents'][i], e_ref, e_up)
        shift = up['log_f0_mean_test'][i] - up['log_f0_mean_ref'][i]
        assert abs(1200.0 * shift / np.log(2.0) - 100.0) <= e_ref + e_up + 1e-9, (i, shift)
