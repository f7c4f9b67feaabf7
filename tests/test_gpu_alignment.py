"""Time alignment on the device (vqvae_amd.alignment, include/vqvae_align.h, csrc/audio_align.hip) against the NumPy
restatement of the rule (tests/alignment_ref.py): every score, the path length, the diagonal count and the whole path
equal it in EVERY bit, in every arrangement of the list; answers known by construction; red zones round every output and
round exactly-sized, poisoned workspaces of the three entry points.

The restatement starts from the device's own float32 log-mel features (tests/test_gpu_metrics.py holds those to their own
restatement); everything after them is float64 +, -, *, /, sqrt, min and integer work, so no tolerance is needed or used.
The DP kernel has one path: a workgroup of 256 threads per pair, cepstra from global memory.  The rows below take it
through a single cell, a single row and column, a diagonal inside one wavefront, across a wavefront (64), across the
workgroup (a shorter side above 256, in each direction, so a diagonal is looped over) and a 1100 x 1300 pair."""
import ctypes as C

import numpy as np
import pytest

import alignment_ref as R
import zoned as Z
from vqvae_amd import _lib, alignment, metrics
from vqvae_amd.corpus import ResidentCorpus
from vqvae_amd.metrics import MelConfig

pytestmark = pytest.mark.gpu
CFG = MelConfig(sr=16000, n_fft=64, hop=16, n_mels=12, n_mcep=5)
PAIRS = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (9, 5), (64, 64), (63, 65), (300, 340), (340, 300), (257, 700), (1100, 1300)]
SMALL = list(range(8))                       # the pairs the arrangement tests move around


def _wave(F, seed, cfg=CFG, extra=0):
    """Seeded noise of exactly F frames (and ``extra`` samples that belong to none)."""
    rs = np.random.RandomState(seed)
    n = cfg.n_fft + cfg.hop * (F - 1) + extra
    return (0.3 * rs.standard_normal(n) * (0.2 + rs.uniform(size=n).cumsum() / n)).astype(np.float32)


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


class Case(object):
    pass


@pytest.fixture(scope='module')
def case(gpu):
    """Computed once and left unchanged: the waves, their features, the device's alignment in one call and the
    restatement of every pair from the device's log-mel blocks."""
    c = Case()
    c.a = [_wave(fa, 100 + i, extra=i % 3) for i, (fa, fb) in enumerate(PAIRS)]
    c.b = [_wave(fb, 200 + i, extra=(i + 1) % 4) for i, (fa, fb) in enumerate(PAIRS)]
    c.fa, c.fb = metrics.features_many(c.a, CFG), metrics.features_many(c.b, CFG)
    c.al = alignment.align_many(c.fa, c.fb)
    c.dct = metrics.tables(CFG)[2]
    c.la = [c.fa.utterance(i)[0] for i in range(len(PAIRS))]
    c.lb = [c.fb.utterance(i)[0] for i in range(len(PAIRS))]
    c.ref = [R.align(la, lb, c.dct) for la, lb in zip(c.la, c.lb)]
    c.paths = [c.al.utterance(i) for i in range(len(PAIRS))]
    return c


def _same_pair(al, i, other, j):
    """Pair i of ``al`` and pair j of ``other`` hold the same bits in every quantity."""
    ok = all(_bits(getattr(al, k)[i]) == _bits(getattr(other, k)[j]) for k in ('cost', 'mcd_dtw_db', 'log_mel_mae_dtw'))
    ok = ok and all(getattr(al, k)[i] == getattr(other, k)[j] for k in ('path_len', 'diagonal_steps', 'frames_a', 'frames_b'))
    if ok and al.ia is not None and other.ia is not None:
        p, q = al.utterance(i), other.utterance(j)
        ok = np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1])
    return ok


# ---- bits against the restatement -------------------------------------------------------------------------------------------
def test_the_layout_of_the_result(case):
    al = case.al
    assert len(al) == len(PAIRS) and al.frames_a.tolist() == [p[0] for p in PAIRS] and al.frames_b.tolist() == [p[1] for p in PAIRS]
    for k in ('mcd_dtw_db', 'log_mel_mae_dtw', 'cost'):
        assert getattr(al, k).dtype == np.float64 and getattr(al, k).shape == (len(PAIRS),), k
    for k in ('path_len', 'diagonal_steps', 'frames_a', 'frames_b'):
        assert getattr(al, k).dtype == np.int64 and getattr(al, k).shape == (len(PAIRS),), k
    cap = [fa + fb - 1 for fa, fb in PAIRS]
    assert al.path_off.tolist() == np.concatenate([[0], np.cumsum(cap)]).tolist() and al.path_off.dtype == np.int64
    assert al.ia.dtype == al.ib.dtype == np.int32 and al.ia.shape == al.ib.shape == (sum(cap),)
    with pytest.raises(IndexError):
        al.utterance(len(PAIRS))


@pytest.mark.parametrize('i', range(len(PAIRS)), ids=['%dx%d' % p for p in PAIRS])
def test_every_quantity_equals_the_restatement_in_every_bit(case, i):
    al, r = case.al, case.ref[i]
    ia, ib = case.paths[i]
    Fa, Fb = PAIRS[i]
    print('pair %s: device cost %.17g K %d diagonal %d mcd %.17g mae %.17g; restatement cost %.17g K %d diagonal %d mcd %.17g mae %.17g'
          % (PAIRS[i], al.cost[i], al.path_len[i], al.diagonal_steps[i], al.mcd_dtw_db[i], al.log_mel_mae_dtw[i],
             r['cost'], r['path_len'], r['diagonal_steps'], r['mcd_dtw_db'], r['log_mel_mae_dtw']))
    assert al.path_len[i] == r['path_len'] and al.diagonal_steps[i] == r['diagonal_steps']
    assert ia.dtype == ib.dtype == np.int32 and np.array_equal(ia, r['ia']) and np.array_equal(ib, r['ib'])
    assert _bits(al.cost[i]) == _bits(r['cost']), (al.cost[i], r['cost'])
    assert _bits(al.mcd_dtw_db[i]) == _bits(r['mcd_dtw_db']), (al.mcd_dtw_db[i], r['mcd_dtw_db'])
    assert _bits(al.log_mel_mae_dtw[i]) == _bits(r['log_mel_mae_dtw']), (al.log_mel_mae_dtw[i], r['log_mel_mae_dtw'])
    # the path is a warping path, and the cost is the local cost summed along it in ascending order
    steps = set(zip(np.diff(ia).tolist(), np.diff(ib).tolist()))
    assert (ia[0], ib[0]) == (0, 0) and (ia[-1], ib[-1]) == (Fa - 1, Fb - 1) and steps <= {(1, 1), (1, 0), (0, 1)}
    assert _bits(R.path_sum(r['d'], ia, ib)) == _bits(al.cost[i])
    assert max(Fa, Fb) <= al.path_len[i] <= Fa + Fb - 1 and al.cost[i] > 0


def test_the_small_pairs_agree_with_the_plain_loops_too(case):
    for i in SMALL:
        r = R.dtw_loops(case.ref[i]['d'])
        assert _bits(r[0]) == _bits(case.al.cost[i]) and r[1:3] == (case.al.path_len[i], case.al.diagonal_steps[i])
        assert np.array_equal(r[3], case.paths[i][0]) and np.array_equal(r[4], case.paths[i][1])


# ---- composition independence -----------------------------------------------------------------------------------------------
def test_a_pair_is_the_same_bits_in_every_arrangement(case, gpu):
    a, b, al = case.a, case.b, case.al
    idx = SMALL + [8]
    sa, sb = [a[i] for i in idx], [b[i] for i in idx]
    n = len(idx)
    for k, i in enumerate(idx):                                                     # alone
        assert _same_pair(alignment.compare_aligned_many([a[i]], [b[i]], CFG, paths=True), 0, al, i), i
    rev = alignment.compare_aligned_many(sa[::-1], sb[::-1], CFG, paths=True)        # the reversed list
    assert all(_same_pair(rev, n - 1 - k, al, i) for k, i in enumerate(idx))
    other_a = [_wave(11 + k, 900 + k) * np.float32(50) for k in range(n + 1)]
    other_b = [_wave(17 - k, 950 + k) * np.float32(50) for k in range(n + 1)]
    ma, mb = [other_a[0]], [other_b[0]]
    for k in range(n):
        ma += [sa[k], other_a[k + 1]]
        mb += [sb[k], other_b[k + 1]]
    mix = alignment.compare_aligned_many(ma, mb, CFG, paths=True)                    # between other, louder pairs
    assert all(_same_pair(mix, 2 * k + 1, al, i) for k, i in enumerate(idx))
    frames = ([PAIRS[i][0] for i in idx], [PAIRS[i][1] for i in idx])
    assert alignment.plan_chunks(frames[0], frames[1], 1) == [(k, k + 1) for k in range(n)]
    assert alignment.plan_chunks(case.al.frames_a, case.al.frames_b, 1 << 30) == [(0, len(PAIRS))]   # the fixture's call was one chunk
    one = alignment.compare_aligned_many(sa, sb, CFG, paths=True, chunk_bytes=1)      # one pair per chunk
    assert all(_same_pair(one, k, al, i) for k, i in enumerate(idx))
    some = alignment.align_many(metrics.features_many(sa, CFG), metrics.features_many(sb, CFG), chunk_bytes=64 * 64 + 63 * 65)
    assert all(_same_pair(some, k, al, i) for k, i in enumerate(idx))                 # several pairs to a chunk, several chunks
    dev = alignment.compare_aligned_many([gpu.to_device(x) for x in sa], [gpu.to_device(x) for x in sb], CFG, paths=True)
    assert all(_same_pair(dev, k, al, i) for k, i in enumerate(idx))
    half_a = [gpu.to_device(x) if k % 2 else x for k, x in enumerate(sa)]             # host and device arrays mixed
    half_b = [x if k % 2 else gpu.to_device(x) for k, x in enumerate(sb)]
    half = alignment.compare_aligned_many(half_a, half_b, CFG, paths=True, chunk_bytes=3000)
    assert all(_same_pair(half, k, al, i) for k, i in enumerate(idx))


def test_a_resident_corpus_is_read_in_place(case, gpu):
    """The corpus peak-normalises what it stores: its own samples, read back, are the list the in-place reading must
    agree with."""
    idx = SMALL + [8]
    corpus = ResidentCorpus([case.a[i] for i in idx], list(range(len(idx))))
    held = corpus.samples.get()
    own = [held[int(o):int(o) + int(L)].copy() for o, L in zip(corpus.offsets, corpus.lengths)]
    sb = [case.b[i] for i in idx]
    want = alignment.compare_aligned_many(own, sb, CFG, paths=True)
    got = alignment.compare_aligned_many(corpus, sb, CFG, paths=True)
    assert got.frames_a.tolist() == [PAIRS[i][0] for i in idx]
    assert all(_same_pair(got, k, want, k) for k in range(len(idx)))
    order = [5, 0, 8, 8, 2]
    view = alignment.compare_aligned_many([sb[j] for j in order], corpus.subset(order), CFG, paths=True, chunk_bytes=2000)
    back = alignment.compare_aligned_many([sb[j] for j in order], [own[j] for j in order], CFG, paths=True)
    assert all(_same_pair(view, k, back, k) for k in range(len(order)))


# ---- answers known by construction ------------------------------------------------------------------------------------------
def test_repeated_frames_give_the_repetition_map(gpu):
    """hop == n_fft: frames do not overlap, so a test wave made of whole frames of the reference, some repeated, has the
    reference's feature bits in the repeated order."""
    cfg = MelConfig(sr=16000, n_fft=64, hop=64, n_mels=12, n_mcep=5)
    ref, test, maps = [], [], []
    for u, reps in enumerate(([1, 3, 1, 2, 1, 1, 4, 1, 2], [2], [1] * 70 + [5] + [1] * 20 + [3], [1, 1, 1])):
        x = _wave(len(reps), 300 + u, cfg)
        src = np.repeat(np.arange(len(reps)), reps)
        ref.append(x)
        test.append(x.reshape(-1, 64)[src].reshape(-1).copy())
        maps.append(src)
    al = alignment.compare_aligned_many(ref, test, cfg, paths=True)
    for u, src in enumerate(maps):
        ia, ib = al.utterance(u)
        assert al.mcd_dtw_db[u] == 0.0 and al.cost[u] == 0.0 and al.log_mel_mae_dtw[u] == 0.0, u
        assert al.path_len[u] == al.frames_b[u] == len(src) and al.diagonal_steps[u] == al.frames_a[u] - 1
        assert ia.tolist() == src.tolist() and ib.tolist() == list(range(len(src))), u
    swapped = alignment.compare_aligned_many(test, ref, cfg, paths=True)
    for u, src in enumerate(maps):
        ia, ib = swapped.utterance(u)
        assert swapped.cost[u] == 0.0 and ia.tolist() == list(range(len(src))) and ib.tolist() == src.tolist(), u


@pytest.mark.parametrize('shape', [(3, 7), (7, 3), (5, 5), (1, 4), (300, 2)], ids=lambda s: '%dx%d' % s)
def test_silence_gives_the_tie_break_path(gpu, shape):
    Fa, Fb = shape
    silent = lambda F: np.zeros(CFG.n_fft + CFG.hop * (F - 1), np.float32)
    al = alignment.compare_aligned_many([silent(Fa)], [silent(Fb)], CFG, paths=True)
    ia, ib = al.utterance(0)
    want = R.tie_break_path(Fa, Fb)
    assert ia.tolist() == want[0].tolist() and ib.tolist() == want[1].tolist()
    assert al.cost[0] == 0.0 and al.mcd_dtw_db[0] == 0.0 and al.log_mel_mae_dtw[0] == 0.0
    assert al.path_len[0] == max(Fa, Fb) and al.diagonal_steps[0] == min(Fa, Fb) - 1


def test_identical_lists_align_on_the_diagonal(case):
    al = alignment.align_many(case.fa, case.fa)
    assert (al.cost == 0.0).all() and (al.mcd_dtw_db == 0.0).all() and (al.log_mel_mae_dtw == 0.0).all()
    assert not np.signbit(al.cost).any() and al.path_len.tolist() == al.frames_a.tolist()
    assert al.diagonal_steps.tolist() == (al.frames_a - 1).tolist()
    for i in range(len(PAIRS)):
        ia, ib = al.utterance(i)
        assert ia.tolist() == ib.tolist() == list(range(PAIRS[i][0])), i


def test_a_diagonal_path_scores_what_the_unaligned_distance_scores(gpu):
    """An equal-length pair whose path is the diagonal: the test wave is the reference plus noise a thousandth of its
    size.  mcd_dtw_db is then compare_many's mcd_db up to the order of a float64 sum of at most 128 terms of the same
    float32 inputs: 1e-12 relative."""
    frames = [128, 90, 33, 1]
    ref = [_wave(F, 400 + F) for F in frames]
    test = [(x + 1e-3 * _wave(F, 500 + F)).astype(np.float32) for x, F in zip(ref, frames)]
    al = alignment.compare_aligned_many(ref, test, CFG, paths=True)
    plain = metrics.compare_many(ref, test, CFG)
    assert plain['frames'].tolist() == frames
    for u, F in enumerate(frames):
        ia, ib = al.utterance(u)
        assert ia.tolist() == ib.tolist() == list(range(F)) and al.path_len[u] == F, u
        print('pair %d: mcd_dtw_db %.17g, mcd_db %.17g' % (u, al.mcd_dtw_db[u], plain['mcd_db'][u]))
        assert al.mcd_dtw_db[u] > 0 and abs(al.mcd_dtw_db[u] - plain['mcd_db'][u]) <= 1e-12 * plain['mcd_db'][u], u
        assert abs(al.log_mel_mae_dtw[u] - plain['log_mel_mae'][u]) <= 1e-12 * plain['log_mel_mae'][u], u


def test_without_paths_nothing_is_kept_and_the_scores_are_the_same(case):
    al = alignment.align_many(case.fa, case.fb, paths=False)
    assert al.ia is None and al.ib is None and al.path_off is None
    assert all(_same_pair(al, i, case.al, i) for i in range(len(PAIRS)))
    with pytest.raises(ValueError, match='without paths=True'):
        al.utterance(0)


# ---- red zones, exactly-sized and poisoned workspaces ------------------------------------------------------------------------
ZONED = [0, 1, 2, 4, 5, 7, 8]                # pairs of the fixture handed to the entry points directly


def _chunk(case):
    fa = np.array([PAIRS[i][0] for i in ZONED], np.int64)
    fb = np.array([PAIRS[i][1] for i in ZONED], np.int64)
    la = np.concatenate([case.la[i] for i in ZONED], axis=1)
    lb = np.concatenate([case.lb[i] for i in ZONED], axis=1)
    d = alignment._desc(CFG, fa, fb, la.shape[1], lb.shape[1])
    off = [np.concatenate([[0], np.cumsum(v)]).astype(np.int64) for v in (fa, fb, fa * fb, fa + fb - 1)]
    return fa, fb, la, lb, d, off


def _tables(b):
    return _lib.AlignTables(b.off_a.ptr, b.off_b.ptr, b.cell_off.ptr, b.path_off.ptr)


def _need(query, d):
    need = getattr(_lib.load(), query)(C.byref(d))
    assert need != C.c_size_t(-1).value
    return need


def test_cepstra_write_inside_their_output(case, gpu):
    fa, fb, la, lb, d, off = _chunk(case)
    need = _need('vqvae_align_cepstra_workspace_bytes', d)
    assert need == 0
    for side, lm in ((0, la), (1, lb)):
        specs = dict(lm=Z.In(lm), dct=Z.In(case.dct), c=Z.Out((lm.shape[1], CFG.n_mcep), np.float64), ws=Z.Ws(256))

        def run(b):
            _lib.call('vqvae_align_cepstra', C.byref(d), side, b.lm.ptr, b.dct.ptr, b.c.ptr, b.ws.ptr, need, gpu.stream())

        out = Z.run_contract(gpu, run, specs)['c']
        assert np.array_equal(_bits(out), _bits(R.cepstra(lm, case.dct))), side


def test_dtw_and_path_write_inside_their_outputs_and_workspaces(case, gpu):
    fa, fb, la, lb, d, off = _chunk(case)
    n = len(fa)
    ca, cb = R.cepstra(la, case.dct), R.cepstra(lb, case.dct)
    need = _need('vqvae_align_dtw_workspace_bytes', d)
    assert need == -(-int((fa * fb).sum()) // 256) * 256
    tabs = dict(off_a=Z.In(off[0]), off_b=Z.In(off[1]), cell_off=Z.In(off[2]), path_off=Z.In(off[3]))
    specs = dict(tabs, ca=Z.In(ca), cb=Z.In(cb), cost=Z.Out((n,), np.float64), klen=Z.Out((n,), np.int32), diag=Z.Out((n,), np.int32),
                 ws=Z.Out((need,), np.uint8, valid=np.arange(need) < int((fa * fb).sum())))
    def run(b):
        t = _tables(b)
        _lib.call('vqvae_align_dtw', C.byref(d), C.byref(t), b.ca.ptr, b.cb.ptr, b.cost.ptr, b.klen.ptr, b.diag.ptr,
                  b.ws.ptr, need, gpu.stream())

    out = Z.run_contract(gpu, run, specs)                   # the direction table: an output here, every cell written, the same from zeros and poison
    for k, i in enumerate(ZONED):
        assert _bits(out['cost'][k]) == _bits(case.al.cost[i]) and out['klen'][k] == case.al.path_len[i]
        assert out['diag'][k] == case.al.diagonal_steps[i]
    assert set(np.unique(out['ws'][:int((fa * fb).sum())]).tolist()) <= {0, 1, 2, 3}
    assert (out['ws'][off[2][:-1]] == 3).all() and (out['ws'] == 3).sum() == n      # one start cell a pair, first in its table

    ptot = int((fa + fb - 1).sum())
    need_p = _need('vqvae_align_path_workspace_bytes', d)
    assert need_p == -(-8 * ptot // 256) * 256
    written = np.zeros(ptot, bool)
    for k in range(n):
        written[int(off[3][k]):int(off[3][k]) + int(out['klen'][k])] = True
    for paths in (True, False):
        specs = dict(tabs, dirs=Z.In(out['ws']), cost=Z.In(out['cost']), klen=Z.In(out['klen']), la=Z.In(la), lb=Z.In(lb),
                     scores=Z.Out((n, 2), np.float64), ws=Z.Ws(need_p))
        if paths:
            specs.update(ia=Z.Out((ptot,), np.int32, valid=written), ib=Z.Out((ptot,), np.int32, valid=written))

        def run_path(b):
            t = _tables(b)
            _lib.call('vqvae_align_path', C.byref(d), C.byref(t), b.dirs.ptr, b.cost.ptr, b.klen.ptr, b.la.ptr, b.lb.ptr,
                      b.ia.ptr if paths else None, b.ib.ptr if paths else None, b.scores.ptr, b.ws.ptr, need_p, gpu.stream())

        got = Z.run_contract(gpu, run_path, specs)
        for k, i in enumerate(ZONED):
            assert _bits(got['scores'][k, 0]) == _bits(case.al.mcd_dtw_db[i]), (paths, i)
            assert _bits(got['scores'][k, 1]) == _bits(case.al.log_mel_mae_dtw[i]), (paths, i)
            if paths:
                at, K = int(off[3][k]), int(out['klen'][k])
                assert np.array_equal(got['ia'][at:at + K], case.paths[i][0]) and np.array_equal(got['ib'][at:at + K], case.paths[i][1])


# ---- the C side refuses a bad descriptor before any launch -------------------------------------------------------------------
def test_a_bad_descriptor_is_refused_without_a_launch(case, gpu):
    fa, fb, la, lb, good, off = _chunk(case)
    n = len(fa)
    lib = _lib.load()
    need = _need('vqvae_align_dtw_workspace_bytes', good)
    bufs = dict(cost=Z.ZonedArray(gpu, shape=(n,), dtype=np.float64, name='cost'), klen=Z.ZonedArray(gpu, shape=(n,), dtype=np.int32, name='klen'),
                diag=Z.ZonedArray(gpu, shape=(n,), dtype=np.int32, name='diag'), ws=Z.ZonedArray(gpu, shape=(need,), dtype=np.uint8, name='ws'),
                scores=Z.ZonedArray(gpu, shape=(n, 2), dtype=np.float64, name='scores'), c=Z.ZonedArray(gpu, shape=(la.shape[1], CFG.n_mcep), dtype=np.float64, name='c'))
    ins = dict((k, gpu.to_device(v)) for k, v in (('off_a', off[0]), ('off_b', off[1]), ('cell_off', off[2]), ('path_off', off[3]),
                                                 ('ca', R.cepstra(la, case.dct)), ('cb', R.cepstra(lb, case.dct)), ('la', la), ('lb', lb),
                                                 ('dct', case.dct)))
    t = _lib.AlignTables(ins['off_a'].ptr, ins['off_b'].ptr, ins['cell_off'].ptr, ins['path_off'].ptr)
    st = gpu.stream()

    need_p = _need('vqvae_align_path_workspace_bytes', good)
    assert need_p <= need

    def cepstra(d, side=0):
        return 'align_cepstra', lib.vqvae_align_cepstra(C.byref(d), side, ins['la'].ptr, ins['dct'].ptr, bufs['c'].ptr, None, 0, st)

    def dtw(d, ws_bytes=need, tables=t):
        return 'align_dtw', lib.vqvae_align_dtw(C.byref(d), None if tables is None else C.byref(tables), ins['ca'].ptr, ins['cb'].ptr,
                                                bufs['cost'].ptr, bufs['klen'].ptr, bufs['diag'].ptr, bufs['ws'].ptr, ws_bytes, st)

    def path(d, ws_bytes=need_p, tables=t, ia=None):
        return 'align_path', lib.vqvae_align_path(C.byref(d), None if tables is None else C.byref(tables), bufs['ws'].ptr, bufs['cost'].ptr,
                                                  bufs['klen'].ptr, ins['la'].ptr, ins['lb'].ptr, ia, None, bufs['scores'].ptr,
                                                  bufs['ws'].ptr, ws_bytes, st)

    def refused(result, words):
        who, rc = result
        msg = lib.vqvae_last_error_string().decode()
        assert rc != 0 and who in msg and words in msg, (who, rc, msg, words)

    for field, value, words in (('n', 0, 'n must be at least 1'), ('n_mels', 129, 'n_mels must be in'), ('n_mcep', 12, 'n_mcep must be in'),
                                ('max_short', alignment.MAX_SHORT + 1, 'max_short must be in'), ('max_short', 0, 'max_short must be in'),
                                ('fb_tot', 0, 'fa_tot and fb_tot'), ('stride_a', 1, 'strides must be'), ('cells', 0, 'cells and ptot')):
        bad = alignment._desc(CFG, fa, fb, la.shape[1], lb.shape[1])
        setattr(bad, field, value)
        for entry in (cepstra, dtw, path):
            refused(entry(bad), words)
    refused(dtw(good, ws_bytes=need - 1), 'workspace of')    # a workspace one byte short
    refused(path(good, ws_bytes=need_p - 1), 'workspace of') # ... which the path entry point needs when it must keep the paths itself
    refused(dtw(good, tables=None), 'null tables')
    refused(path(good, tables=None), 'null tables')
    refused(path(good, ia=bufs['ws'].ptr), 'both be given or both be null')
    refused(cepstra(good, side=2), 'side must be 0 or 1')
    gpu.synchronize()
    for k, z in bufs.items():                               # nothing ran: every payload still holds its poison, every zone its pattern
        z.check()
        assert np.array_equal(z.arr.get().view(np.uint8).reshape(-1), z.initial), k
