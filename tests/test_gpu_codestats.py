"""Code statistics on the device (vqvae_amd.codestats, include/vqvae_codes.h, csrc/code_stats.hip) against the NumPy restatement
of the rule (tests/codestats_ref.py).  Everything the device does here is integer arithmetic, so EVERY comparison is an
equality: runs, count tables, agreement, edit distance and substitutions, in every arrangement of the list; answers known
by construction; red zones round every output of the four entry points.

The edit kernel has one path: a workgroup of 256 threads per pair over the anti-diagonals.  The rows below take it through
a single cell, a single row and column, a diagonal inside one wavefront, across a wavefront (64), across the workgroup (a
shorter side above 256, in each direction, so a diagonal is looped over), a 1100 x 1300 pair and one pair at the bound of
the shorter side (6143 x 6200: the LDS opt-in).  The runs kernel scans in passes of 256: the lengths straddle 64 and 256."""
import ctypes as C

import numpy as np
import pytest

import codestats_ref as R
import zoned as Z
from vqvae_amd import _lib, codestats
from vqvae_amd.frontend import LatentCodes

pytestmark = pytest.mark.gpu
PAIRS = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (9, 5), (63, 65), (64, 64), (40, 33),
         (255, 257), (256, 256), (257, 255), (300, 700), (700, 300), (1100, 1300)]
ALPHABETS = [3, 128]                           # 3: tie-rich, and long runs for the collapse
SMALL = list(range(9))                         # the pairs the arrangement tests move around
RUN_LENGTHS = [1, 63, 64, 65, 255, 256, 257, 1000]


def _string(n, k, seed):
    return np.random.RandomState(seed).randint(0, k, n).astype(np.int32)


def _codes(utts, k, gpu=None):
    """LatentCodes of a list of host arrays; with ``gpu`` the buffer is handed over on the device (no host check of
    the codes against k)."""
    tl = np.array([len(u) for u in utts], np.int32)
    flat = np.concatenate([np.asarray(u, np.int32).reshape(-1) for u in utts])
    return LatentCodes(tl, flat if gpu is None else gpu.to_device(flat), k)


class Case(object):
    pass


@pytest.fixture(scope='module')
def case(gpu):
    """Computed once and left unchanged: per alphabet the two sides, the device's comparison raw and collapsed in one call
    each, and the restatement of every pair."""
    out = {}
    for k in ALPHABETS:
        c = Case()
        c.a = [_string(la, k, 100 + 7 * i + k) for i, (la, lb) in enumerate(PAIRS)]
        c.b = [_string(lb, k, 200 + 7 * i + k) for i, (la, lb) in enumerate(PAIRS)]
        c.ca, c.cb = _codes(c.a, k), _codes(c.b, k)
        c.raw = codestats.compare_codes_many(c.ca, c.cb, collapse=False)
        c.col = codestats.compare_codes_many(c.ca, c.cb, collapse=True)
        c.ref_raw = [R.edit_diagonals(a, b) for a, b in zip(c.a, c.b)]
        c.ref_col = [R.edit_diagonals(R.runs(a)[0], R.runs(b)[0]) for a, b in zip(c.a, c.b)]
        out[k] = c
    return out


FIELDS = ('distance', 'subs', 'ins', 'dels', 'matches', 'len_a', 'len_b', 'agree', 'overlap')


def _same_pair(cmp, i, other, j):
    return all(getattr(cmp, f)[i] == getattr(other, f)[j] for f in FIELDS)


# ---- the edit distance ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', ALPHABETS)
@pytest.mark.parametrize('i', range(len(PAIRS)), ids=['%dx%d' % p for p in PAIRS])
def test_every_quantity_equals_the_restatement(case, i, k):
    c = case[k]
    La, Lb = PAIRS[i]
    for cmp, ref, sa, sb in ((c.raw, c.ref_raw[i], c.a[i], c.b[i]), (c.col, c.ref_col[i], R.runs(c.a[i])[0], R.runs(c.b[i])[0])):
        dist, subs = ref
        dels, ins, matches = R.derive(dist, subs, len(sa), len(sb))
        print('pair %s k %d: device dist %d subs %d ins %d dels %d over %d x %d; restatement dist %d subs %d ins %d dels %d over %d x %d'
              % (PAIRS[i], k, cmp.distance[i], cmp.subs[i], cmp.ins[i], cmp.dels[i], cmp.len_a[i], cmp.len_b[i],
                 dist, subs, ins, dels, len(sa), len(sb)))
        assert (cmp.len_a[i], cmp.len_b[i]) == (len(sa), len(sb))
        assert (cmp.distance[i], cmp.subs[i]) == (dist, subs)
        assert (cmp.dels[i], cmp.ins[i], cmp.matches[i]) == (dels, ins, matches)
        assert (cmp.agree[i], cmp.overlap[i]) == R.agreement(c.a[i], c.b[i])          # raw frames on both
        assert cmp.error_rate[i] == dist / len(sa) and cmp.normalised[i] == dist / max(len(sa), len(sb))
        assert cmp.agreement[i] == cmp.agree[i] / min(La, Lb)
    if k == 3 and min(La, Lb) >= 40:
        assert c.col.len_a[i] < La and c.col.len_b[i] < Lb                              # the collapse had something to do


@pytest.mark.parametrize('k', ALPHABETS)
def test_the_small_pairs_agree_with_the_plain_loops_too(case, k):
    c = case[k]
    for i in SMALL:
        assert R.edit_loops(c.a[i], c.b[i]) == (c.raw.distance[i], c.raw.subs[i]), PAIRS[i]
    for f in FIELDS:
        assert getattr(c.raw, f).dtype == np.int64 and getattr(c.raw, f).shape == (len(PAIRS),), f
    assert len(c.raw) == len(PAIRS) and c.raw.collapse is False and c.col.collapse is True


@pytest.mark.parametrize('collapse', [False, True], ids=['raw', 'collapsed'])
def test_a_pair_is_the_same_in_every_arrangement(case, gpu, collapse):
    c = case[3]
    whole = c.col if collapse else c.raw
    idx = SMALL + [9, 12]
    sa, sb = [c.a[i] for i in idx], [c.b[i] for i in idx]
    n = len(idx)
    for i in idx:                                                                   # alone
        assert _same_pair(codestats.compare_codes_many(_codes([c.a[i]], 3), _codes([c.b[i]], 3), collapse), 0, whole, i), i
    rev = codestats.compare_codes_many(_codes(sa[::-1], 3), _codes(sb[::-1], 3), collapse)          # the reversed list
    assert all(_same_pair(rev, n - 1 - j, whole, i) for j, i in enumerate(idx))
    ma, mb = [_string(11, 3, 900)], [_string(17, 3, 950)]                           # beside neighbours that end and begin
    for j in range(n):                                                              # with this pair's own boundary codes
        ma += [sa[j], np.full(5 + j, sa[j][-1], np.int32)]
        mb += [sb[j], np.full(3 + j, sb[j][-1], np.int32)]
        ma[-3] = np.concatenate([ma[-3], sa[j][:1]])
        mb[-3] = np.concatenate([mb[-3], sb[j][:1]])
    mix = codestats.compare_codes_many(_codes(ma, 3, gpu), _codes(mb, 3, gpu), collapse)            # device buffers
    assert all(_same_pair(mix, 2 * j + 1, whole, i) for j, i in enumerate(idx))


@pytest.mark.parametrize('collapse', [False, True], ids=['raw', 'collapsed'])
def test_answers_known_by_construction(gpu, collapse):
    a = np.arange(300, dtype=np.int32) % 11                                         # no two neighbours equal: nothing collapses
    third = a[np.arange(300) % 3 != 2]
    assert len(R.runs(third)[0]) == len(third) == 200
    shapes = [(5, 9), (9, 5), (64, 64), (300, 257)]
    sa = [a, a, third, a] + [_string(la, 3, la) * 2 for la, lb in shapes]
    sb = [a, third, a, a[::-1].copy()] + [_string(lb, 3, lb) * 2 + 1 for la, lb in shapes]
    for j in range(4, len(sa)):                                                     # (nothing to collapse there either)
        sa[j], sb[j] = sa[j] + 2 * (np.arange(len(sa[j])) % 2 * 3), sb[j] + 2 * (np.arange(len(sb[j])) % 2 * 3)
    cmp = codestats.compare_codes_many(_codes(sa, 16), _codes(sb, 16), collapse)
    assert (cmp.distance[0], cmp.subs[0], cmp.matches[0], cmp.agreement[0]) == (0, 0, 300, 1.0)            # identical
    assert (cmp.distance[1], cmp.subs[1], cmp.dels[1], cmp.ins[1], cmp.matches[1]) == (100, 0, 100, 0, 200)  # every third removed
    assert (cmp.distance[2], cmp.subs[2], cmp.dels[2], cmp.ins[2], cmp.matches[2]) == (100, 0, 0, 100, 200)  # ... and put back
    assert (cmp.distance[3], cmp.subs[3]) == R.edit_diagonals(a, a[::-1])
    for j, (la, lb) in enumerate(shapes, start=4):                                  # disjoint alphabets (even against odd)
        assert (cmp.len_a[j], cmp.len_b[j]) == (la, lb)
        assert (cmp.distance[j], cmp.subs[j], cmp.agree[j]) == (max(la, lb), min(la, lb), 0), (la, lb)


def test_one_pair_at_the_bound_of_the_shorter_side(gpu):
    """6143 x 6200: 147432 bytes of dynamic LDS, the opt-in above 64 KiB; 24 passes of a diagonal per thread."""
    M = codestats.MAX_SHORT
    a, b = _string(M, 5, 61), _string(6200, 5, 62)
    cmp = codestats.compare_codes_many(_codes([a[:40], a], 5), _codes([b[:50], b], 5), collapse=False)
    want = R.edit_diagonals(a, b)
    print('device dist %d subs %d; restatement dist %d subs %d' % (cmp.distance[1], cmp.subs[1], want[0], want[1]))
    assert (cmp.distance[1], cmp.subs[1]) == want and (cmp.len_a[1], cmp.len_b[1]) == (M, 6200)
    assert (cmp.distance[0], cmp.subs[0]) == R.edit_diagonals(a[:40], b[:50])      # a small pair beside it, in the large LDS
    assert (cmp.agree[1], cmp.overlap[1]) == R.agreement(a, b)


# ---- runs -----------------------------------------------------------------------------------------------------------------
def _run_list():
    utts = [_string(n, 3, 300 + n) for n in RUN_LENGTHS]
    utts.append(np.full(300, 2, np.int32))                                          # all equal: one run
    utts.append((np.arange(301) % 2).astype(np.int32))                              # alternating: nothing collapses
    crossing = (np.arange(300) % 2).astype(np.int32)
    crossing[250:261] = 2                                                           # one run over positions 250 .. 260
    utts.append(crossing)
    for n in (5, 256, 7):                                                           # neighbours sharing their boundary code
        utts.append(np.concatenate([utts[-1][-1:], _string(n, 3, 400 + n), [1]]).astype(np.int32))
        assert utts[-1][0] == utts[-2][-1]
    return utts


def test_runs_equal_the_restatement(gpu):
    utts = _run_list()
    runs = codestats.collapse_many(_codes(utts, 3), max_run=8)
    want = [R.runs(u) for u in utts]
    got = runs.to_host()
    assert runs.lengths.tolist() == [len(w[0]) for w in want] and runs.lengths.dtype == np.int64
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0].dtype == g[1].dtype == np.int32 and np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), i
        assert g[1].sum() == len(utts[i])
    n = len(RUN_LENGTHS)
    assert runs.lengths[n] == 1 and got[n][1].tolist() == [300] and runs.lengths[n + 1] == 301
    at = int(np.nonzero(got[n + 2][1] == 11)[0][0])
    assert got[n + 2][0][at] == 2 and got[n + 2][1][:at].sum() == 250
    hist = R.run_hist([w[1] for w in want], 8)
    assert np.array_equal(runs.histogram, hist) and runs.histogram.dtype == np.int64 and hist[7] >= 2 and hist.sum() == runs.lengths.sum()
    assert runs.mean_run == sum(len(u) for u in utts) / float(hist.sum())
    one = codestats.collapse_many(_codes(utts, 3, gpu), max_run=1)                  # every run in the clamp bucket
    assert one.histogram.tolist() == [hist.sum()] and np.array_equal(one.u.get()[:1], utts[0][:1])
    bare = codestats.collapse_many(_codes(utts, 3), max_run=None)                   # the nullable histogram
    assert bare.run_hist is None and bare.lengths.tolist() == runs.lengths.tolist()
    assert all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) for p, q in zip(bare.to_host(), got))
    with pytest.raises(ValueError, match='max_run=None'):
        bare.histogram
    rev = codestats.collapse_many(_codes(utts[::-1], 3), max_run=8)                 # the reversed list
    assert all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) for p, q in zip(rev.to_host()[::-1], got))
    assert np.array_equal(rev.histogram, hist)


# ---- counts ---------------------------------------------------------------------------------------------------------------
def _same_tables(st, want, bigrams=True):
    uni, big, invalid = want
    assert st.uni.dtype == np.int64 and np.array_equal(st.uni, uni) and st.invalid == invalid
    if bigrams:
        assert st.big.dtype == np.int64 and np.array_equal(st.big, big)
    else:
        assert st.big is None


@pytest.mark.parametrize('k', [1, 5, 128])
def test_counts_equal_the_restatement(gpu, k):
    lengths = [1, 2, 63, 64, 65, 257, 1000, 300]
    utts = [_string(n, k, 500 + n + k) for n in lengths]
    N = len(utts)
    codes = _codes(utts, k)
    st = codestats.code_stats(codes, max_run=4)                                     # G = 1
    _same_tables(st, R.counts_loops(utts, [0] * N, k, 1))
    assert st.uni.shape == (1, k) and st.big.shape == (k, k) and st.n_speakers == 1 and st.mi_bits == 0.0
    assert st.uni.sum() == sum(lengths) == st.positions and st.big.sum() == sum(lengths) - N == st.transitions
    spk = np.array([0, 2, 2, 0, 2, 0, 2, 0], np.int32)                              # G = 3, group 1 empty
    st3 = codestats.code_stats(codes, spk, 3)
    want = R.counts_loops(utts, spk, k, 3)
    _same_tables(st3, want)
    assert np.array_equal(want[0], R.counts_add_at(utts, spk, k, 3)[0]) and st3.uni[1].sum() == 0
    assert np.array_equal(st3.big, st.big) and np.array_equal(st3.uni.sum(axis=0), st.uni[0])
    order = [5, 0, 7, 2, 1, 6, 3, 4]                                                # the tables do not depend on the list's order
    stp = codestats.code_stats(_codes([utts[j] for j in order], k, gpu), spk[order], 3)
    _same_tables(stp, want)
    runs = [R.runs(u) for u in utts]
    assert np.array_equal(st.run_hist, R.run_hist([r[1] for r in runs], 4)) and st.runs == sum(len(r[0]) for r in runs)
    assert st.mean_run == sum(lengths) / float(st.runs)
    stc = codestats.code_stats(codes, spk, 3, collapsed=True)                       # runs instead of positions
    _same_tables(stc, R.counts_loops([r[0] for r in runs], spk, k, 3))
    assert (np.diag(stc.big) == 0).all() and stc.uni.sum() == st.runs and stc.big.sum() == st.runs - N
    for name, v in codestats.figures(want[0], want[1]).items():                     # the figures are the host's, of these tables
        assert np.array_equal(getattr(st3, name), v, equal_nan=True), name


def test_a_large_codebook_counts_unigrams_only(gpu):
    k = 8192
    utts = [_string(n, k, 700 + n) for n in (1, 300, 1000)] + [np.array([0, k - 1, k - 1], np.int32)]
    with pytest.raises(ValueError, match='ask for bigrams=False'):
        codestats.code_stats(_codes(utts, k))
    st = codestats.code_stats(_codes(utts, k), [1, 0, 1, 1], bigrams=False)
    _same_tables(st, R.counts_add_at(utts, [1, 0, 1, 1], k, 2, bigrams=False), bigrams=False)
    assert st.uni[1, k - 1] >= 2 and not hasattr(st, 'self_share')


def test_boundaries_leak_nothing(gpu):
    one = codestats.code_stats(_codes([[3]], 5))                                    # a single position: no transition
    assert one.big.sum() == 0 and one.uni.tolist() == [[0, 0, 0, 1, 0]] and np.isnan(one.self_share)
    k = 12
    utts = [np.full(1 + 40 * i, i, np.int32) for i in range(k)]                     # utterance i constant at code i
    st = codestats.code_stats(_codes(utts, k), np.arange(k) % 2, 2)
    assert np.array_equal(st.big, np.diag([40 * i for i in range(k)]))              # anything off the diagonal crossed a boundary
    assert st.self_share == 1.0 and st.next_entropy_bits == 0.0 and st.runs == k
    assert st.uni.sum() == sum(len(u) for u in utts) and st.big.sum() == st.uni.sum() - k


def test_contention_on_one_code(gpu):
    n = 1 << 20
    st = codestats.code_stats(_codes([np.full(n, 3, np.int32), np.full(9, 3, np.int32)], 4), max_run=2)
    assert st.uni.tolist() == [[0, 0, 0, n + 9]] and st.big[3, 3] == n + 9 - 2 == st.big.sum() and st.invalid == 0
    assert st.run_hist.tolist() == [0, 2] and st.runs == 2


def test_invalid_codes_and_groups_count_as_invalid_only(gpu):
    k = 6
    utts = [_string(n, k, 800 + n) for n in (70, 300, 9, 4)]
    utts[0][35], utts[1][256] = -1, k                                               # planted in the middle
    codes = _codes(utts, k, gpu)                                                    # a device buffer: not checked on the host
    st = codestats.code_stats(codes, [0, 1, 1, 0], 2)
    want = R.counts_loops(utts, [0, 1, 1, 0], k, 2)
    assert want[2] == 2 and want[1].sum() == sum(len(u) for u in utts) - 4 - 4
    _same_tables(st, want)
    # a group outside [0, G) is the C side's rule (the Python call refuses it): the whole utterance is invalid positions
    tl = np.array([len(u) for u in utts], np.int32)
    start = np.concatenate([[0], np.cumsum(tl)[:-1]]).astype(np.int64)
    for groups in ([0, 2, 1, 0], [0, 1, -1, 0]):
        uni, big, invalid = gpu.DeviceArray((2, k), np.int64), gpu.DeviceArray((k, k), np.int64), gpu.DeviceArray((1,), np.int64)
        keep, (s, n_, g) = codestats._upload(start, tl, np.array(groups, np.int32))
        codestats._count('test', codes.indices, int(tl.sum()), s, n_, g, 4, k, 2, uni, big, invalid)
        want = R.counts_loops(utts, groups, k, 2)
        assert want[2] in (300 + 1, 9 + 2)
        assert np.array_equal(uni.get(), want[0]) and np.array_equal(big.get(), want[1]) and invalid.get()[0] == want[2]


def test_accumulate_adds_and_its_absence_clears(gpu):
    k = 5
    utts = [_string(n, k, 850 + n) for n in (33, 300)]
    codes = _codes(utts, k)
    tl = codes.tl
    keep, (s, n_, g) = codestats._upload(codes.offsets[:-1].astype(np.int64), tl, np.array([1, 0], np.int32))
    uni, big, invalid = gpu.DeviceArray((2, k), np.int64), gpu.DeviceArray((k, k), np.int64), gpu.DeviceArray((1,), np.int64)
    for arr in (uni, big, invalid):
        arr.set(np.full(arr.shape, 7, np.int64))
    want = R.counts_loops(utts, [1, 0], k, 2)
    args = ('test', codes.indices, int(tl.sum()), s, n_, g, 2, k, 2, uni, big, invalid)
    codestats._count(*args, accumulate=True)
    assert np.array_equal(uni.get(), want[0] + 7) and np.array_equal(big.get(), want[1] + 7) and invalid.get()[0] == 7
    codestats._count(*args, accumulate=True)
    assert np.array_equal(uni.get(), 2 * want[0] + 7) and np.array_equal(big.get(), 2 * want[1] + 7)
    codestats._count(*args)                                                         # cleared first, on the stream
    assert np.array_equal(uni.get(), want[0]) and np.array_equal(big.get(), want[1]) and invalid.get()[0] == 0


# ---- red zones --------------------------------------------------------------------------------------------------------------
def _need(query, d):
    need = getattr(_lib.load(), query)(C.byref(d))
    assert need == 0
    return need


def test_every_entry_point_writes_inside_its_outputs(gpu):
    k = 7
    utts = [_string(n, k, 900 + n) for n in (1, 64, 257, 300, 5)]
    other = [_string(n, k, 950 + n) for n in (3, 64, 300, 257, 5)]
    N = len(utts)
    tl, tlb = np.array([len(u) for u in utts], np.int32), np.array([len(u) for u in other], np.int32)
    start = np.concatenate([[0], np.cumsum(tl)[:-1]]).astype(np.int64)
    startb = np.concatenate([[0], np.cumsum(tlb)[:-1]]).astype(np.int64)
    flat, flatb, total, totalb = np.concatenate(utts), np.concatenate(other), int(tl.sum()), int(tlb.sum())
    st = gpu.stream

    # runs: the slots behind an utterance's runs are not written
    want = [R.runs(u) for u in utts]
    written = np.zeros(total, bool)
    for o, w in zip(start, want):
        written[int(o):int(o) + len(w[0])] = True
    d = _lib.CodesRunsDesc(N, 4, total)
    need = _need('vqvae_codes_runs_workspace_bytes', d)
    specs = dict(codes=Z.In(flat), start=Z.In(start), len=Z.In(tl), u=Z.Out((total,), np.int32, valid=written),
                 dur=Z.Out((total,), np.int32, valid=written), m=Z.Out((N,), np.int32), hist=Z.Out((4,), np.int64), ws=Z.Ws(256))

    def run_runs(b):
        _lib.call('vqvae_codes_runs', C.byref(d), b.codes.ptr, b.start.ptr, b.len.ptr, b.u.ptr, b.dur.ptr, b.m.ptr,
                  b.hist.ptr, b.ws.ptr, need, st())

    out = Z.run_contract(gpu, run_runs, specs)
    assert out['m'].tolist() == [len(w[0]) for w in want] and np.array_equal(out['hist'], R.run_hist([w[1] for w in want], 4))
    assert np.array_equal(out['u'][written], np.concatenate([w[0] for w in want]))
    assert np.array_equal(out['dur'][written], np.concatenate([w[1] for w in want]))

    # counts, with and without the nullable table
    groups = np.array([0, 1, 1, 0, 1], np.int32)
    for bigrams in (1, 0):
        dh = _lib.CodesHistDesc(N, k, 2, bigrams, 0, 0, total)
        need = _need('vqvae_codes_hist_workspace_bytes', dh)
        specs = dict(codes=Z.In(flat), start=Z.In(start), len=Z.In(tl), group=Z.In(groups), uni=Z.Out((2, k), np.int64),
                     invalid=Z.Out((1,), np.int64), ws=Z.Ws(256))
        if bigrams:
            specs['big'] = Z.Out((k, k), np.int64)

        def run_hist(b):
            _lib.call('vqvae_codes_hist', C.byref(dh), b.codes.ptr, b.start.ptr, b.len.ptr, b.group.ptr, b.uni.ptr,
                      b.big.ptr if bigrams else None, b.invalid.ptr, b.ws.ptr, need, st())

        out = Z.run_contract(gpu, run_hist, specs)
        wu, wb, wi = R.counts_loops(utts, groups, k, 2)
        assert np.array_equal(out['uni'], wu) and out['invalid'][0] == wi == 0 and (not bigrams or np.array_equal(out['big'], wb))

    # the two pair entry points
    dp = _lib.CodesPairDesc(N, int(np.minimum(tl, tlb).max()), total, totalb)
    specs = dict(a=Z.In(flat), b=Z.In(flatb), sa=Z.In(start), na=Z.In(tl), sb=Z.In(startb), nb=Z.In(tlb), ws=Z.Ws(256))

    def run_agree(b):
        t = _lib.CodesPairTables(b.sa.ptr, b.na.ptr, b.sb.ptr, b.nb.ptr)
        _lib.call('vqvae_codes_agree', C.byref(dp), C.byref(t), b.a.ptr, b.b.ptr, b.agree.ptr, b.ws.ptr,
                  _need('vqvae_codes_agree_workspace_bytes', dp), st())

    def run_edit(b):
        t = _lib.CodesPairTables(b.sa.ptr, b.na.ptr, b.sb.ptr, b.nb.ptr)
        _lib.call('vqvae_codes_edit', C.byref(dp), C.byref(t), b.a.ptr, b.b.ptr, b.dist.ptr, b.subs.ptr, b.ws.ptr,
                  _need('vqvae_codes_edit_workspace_bytes', dp), st())

    out = Z.run_contract(gpu, run_agree, dict(specs, agree=Z.Out((N,), np.int32)))
    assert out['agree'].tolist() == [R.agreement(x, y)[0] for x, y in zip(utts, other)]
    out = Z.run_contract(gpu, run_edit, dict(specs, dist=Z.Out((N,), np.int32), subs=Z.Out((N,), np.int32)))
    assert list(zip(out['dist'].tolist(), out['subs'].tolist())) == [R.edit_diagonals(x, y) for x, y in zip(utts, other)]


def test_contradicting_tables_are_skipped_on_the_device(gpu):
    """An entry that contradicts the descriptor writes what the header says and nothing else: its neighbours' results stand."""
    k = 4
    utts = [_string(n, k, 970 + n) for n in (20, 30, 40)]
    flat = gpu.to_device(np.concatenate(utts))
    tl = np.array([20, 30, 40], np.int32)
    start = np.array([0, 20, 50], np.int64)
    bad_len, bad_start = np.array([20, 0, 40], np.int32), np.array([0, 20, 51], np.int64)     # no code; one code past the end
    N, total = 3, 90
    for s_, n_, skipped in ((start, bad_len, 1), (bad_start, tl, 2)):
        keep, (sp, np_) = codestats._upload(s_, n_)
        keep2, (sg, ng) = codestats._upload(start, tl)
        m, hist = gpu.DeviceArray((N,), np.int32), gpu.DeviceArray((4,), np.int64)
        u, dur = gpu.DeviceArray((total,), np.int32), gpu.DeviceArray((total,), np.int32)
        d = _lib.CodesRunsDesc(N, 4, total)
        _lib.call('vqvae_codes_runs', C.byref(d), flat.ptr, sp, np_, u.ptr, dur.ptr, m.ptr, hist.ptr, None, 0, gpu.stream())
        want = [0 if i == skipped else len(R.runs(x)[0]) for i, x in enumerate(utts)]
        assert m.get().tolist() == want and hist.get().sum() == sum(want)
        out = gpu.DeviceArray((2, N), np.int32)
        dp = _lib.CodesPairDesc(N, 40, total, total)
        t = _lib.CodesPairTables(sp, np_, sg, ng)
        _lib.call('vqvae_codes_edit', C.byref(dp), C.byref(t), flat.ptr, flat.ptr, out.ptr, out.ptr + 4 * N, None, 0, gpu.stream())
        assert out.get().tolist() == [[-1 if i == skipped else 0 for i in range(N)], [0, 0, 0]]
        _lib.call('vqvae_codes_agree', C.byref(dp), C.byref(t), flat.ptr, flat.ptr, out.ptr, None, 0, gpu.stream())
        assert out.get()[0].tolist() == [-1 if i == skipped else int(tl[i]) for i in range(N)]
    short = _lib.CodesPairDesc(N, 25, total, total)                                 # a shorter side above max_short: skipped
    keep, (sg, ng) = codestats._upload(start, tl)
    out = gpu.DeviceArray((2, N), np.int32)
    t = _lib.CodesPairTables(sg, ng, sg, ng)
    _lib.call('vqvae_codes_edit', C.byref(short), C.byref(t), flat.ptr, flat.ptr, out.ptr, out.ptr + 4 * N, None, 0, gpu.stream())
    assert out.get()[0].tolist() == [0, -1, -1]


def test_a_bad_descriptor_is_refused_without_a_launch(gpu):
    lib = _lib.load()
    N, k, total = 2, 4, 10
    bufs = dict((n, Z.ZonedArray(gpu, shape=s, dtype=t, name=n)) for n, s, t in (
        ('u', (total,), np.int32), ('dur', (total,), np.int32), ('m', (N,), np.int32), ('hist', (4,), np.int64),
        ('uni', (1, k), np.int64), ('big', (k, k), np.int64), ('invalid', (1,), np.int64), ('dist', (N,), np.int32), ('subs', (N,), np.int32)))
    flat = gpu.to_device(_string(total, k, 1))
    keep, (s, n_, g) = codestats._upload(np.array([0, 4], np.int64), np.array([4, 6], np.int32), np.zeros(N, np.int32))
    tabs = _lib.CodesPairTables(s, n_, s, n_)
    st = gpu.stream()

    def runs(d, m=bufs['m'].ptr):
        return 'codes_runs', lib.vqvae_codes_runs(C.byref(d), flat.ptr, s, n_, bufs['u'].ptr, bufs['dur'].ptr, m, bufs['hist'].ptr, None, 0, st)

    def hist(d, big=bufs['big'].ptr):
        return 'codes_hist', lib.vqvae_codes_hist(C.byref(d), flat.ptr, s, n_, g, bufs['uni'].ptr, big, bufs['invalid'].ptr, None, 0, st)

    def agree(d, t=tabs):
        return 'codes_agree', lib.vqvae_codes_agree(C.byref(d), None if t is None else C.byref(t), flat.ptr, flat.ptr, bufs['dist'].ptr, None, 0, st)

    def edit(d, t=tabs, subs=bufs['subs'].ptr):
        return 'codes_edit', lib.vqvae_codes_edit(C.byref(d), None if t is None else C.byref(t), flat.ptr, flat.ptr, bufs['dist'].ptr, subs, None, 0, st)

    def refused(result, words):
        who, rc = result
        msg = lib.vqvae_last_error_string().decode()
        assert rc != 0 and who in msg and words in msg, (who, rc, msg, words)

    for field, value, words in (('n', 0, 'n must be at least 1'), ('max_run', 0, 'max_run must be at least 1'), ('total', 1, 'total must be at least n')):
        d = _lib.CodesRunsDesc(N, 4, total)
        setattr(d, field, value)
        refused(runs(d), words)
    for field, value, words in (('n', 0, 'n must be at least 1'), ('k', 0, 'k and groups'), ('groups', 0, 'k and groups'), ('bigrams', 2, 'must be 0 or 1'),
                                ('accumulate', 2, 'must be 0 or 1'), ('reserved', 1, 'reserved 0'), ('k', 4097, 'bigrams need k of at most 4096'),
                                ('total', 1, 'total must be at least n')):
        d = _lib.CodesHistDesc(N, k, 1, 1, 0, 0, total)
        setattr(d, field, value)
        refused(hist(d), words)
    for field, value, words in (('n', 0, 'n must be at least 1'), ('max_short', 0, 'max_short must be in'),
                                ('max_short', codestats.MAX_SHORT + 1, 'max_short must be in'), ('total_b', 1, 'total_a and total_b')):
        for entry in (agree, edit):
            d = _lib.CodesPairDesc(N, 6, total, total)
            setattr(d, field, value)
            refused(entry(d), words)
    refused(runs(_lib.CodesRunsDesc(N, 4, total), m=None), 'null codes')
    refused(hist(_lib.CodesHistDesc(N, k, 1, 1, 0, 0, total), big=None), 'big must be given')
    refused(hist(_lib.CodesHistDesc(N, k, 1, 0, 0, 0, total)), 'big must be given')
    refused(agree(_lib.CodesPairDesc(N, 6, total, total), t=None), 'null tables')
    refused(edit(_lib.CodesPairDesc(N, 6, total, total), t=None), 'null tables')
    refused(edit(_lib.CodesPairDesc(N, 6, total, total), subs=None), 'null a, b, dist or subs')
    gpu.synchronize()
    for name, z in bufs.items():                            # nothing ran: every payload still holds its poison, every zone its pattern
        z.check()
        assert np.array_equal(z.arr.get().view(np.uint8).reshape(-1), z.initial), name


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_encoded_utterances_end_to_end(gpu):
    """encode_many on a small model feeds the calls; they must equal the restatement over codes.to_host()."""
    import vqvae_amd as V
    from vqvae_amd.net import Encoder
    from vqvae_amd.utils import VQ
    rs = np.random.RandomState(77)
    d, k = 16, 24
    enc, vq = Encoder(d), VQ(k, d)
    vq.W.data = (0.02 * rs.standard_normal((k, d))).astype(np.float32)
    enc.to_gpu()
    vq.to_gpu()
    waves = [(0.5 * rs.standard_normal(64 * tl + 13) * np.sin(np.arange(64 * tl + 13) / 50.0)).astype(np.float32) for tl in (30, 41, 7, 64, 22, 35)]
    speakers = np.array([0, 1, 2, 0, 1, 2], np.int32)
    codes = V.encode_many(enc, vq, waves)
    host = codes.to_host()
    assert [len(h) for h in host] == [30, 41, 7, 64, 22, 35]
    st = V.code_stats(codes, speakers, 3, permutations=3, seed=5)
    _same_tables(st, R.counts_loops(host, speakers, k, 3))
    assert st.used == len(np.unique(np.concatenate(host))) and abs(st.mi_bits - R.mi_bits(st.uni)) <= 1e-12
    perm = np.random.RandomState(5)
    for p in range(3):                                                              # the restated relabelings, one call each
        relabeled = V.code_stats(codes, speakers[perm.permutation(len(host))], 3, bigrams=False)
        assert np.array_equal(relabeled.uni.sum(axis=0), st.uni.sum(axis=0))
        assert st.mi_permuted[p] == relabeled.mi_bits, p
    assert st.mi_permuted.shape == (3,) and st.mi_permuted.dtype == np.float64

    corpus = V.ResidentCorpus(waves, speakers)
    view = corpus.subset([4, 0, 5, 1])
    vcodes = view.encode(enc, vq)
    got, want = view.code_stats(vcodes, n_speakers=3, max_run=5), V.code_stats(vcodes, view.speakers, 3, max_run=5)
    _same_tables(got, (want.uni, want.big, want.invalid))
    assert np.array_equal(got.run_hist, want.run_hist) and got.mi_bits == want.mi_bits and got.n_speakers == 3
    _same_tables(got, R.counts_loops(vcodes.to_host(), view.speakers, k, 3))

    other = V.encode_many(enc, vq, [w[::-1].copy() for w in waves[::-1]])          # another list of the same N
    oh = other.to_host()
    for collapse in (True, False):
        cmp = V.compare_codes_many(codes, other, collapse)
        for i in range(len(host)):
            a, b = (R.runs(host[i])[0], R.runs(oh[i])[0]) if collapse else (host[i], oh[i])
            assert (cmp.distance[i], cmp.subs[i]) == R.edit_diagonals(a, b) and (cmp.len_a[i], cmp.len_b[i]) == (len(a), len(b))
            assert (cmp.agree[i], cmp.overlap[i]) == R.agreement(host[i], oh[i])
    again = V.compare_codes_many(codes, V.encode_many(enc, vq, waves))              # the same waves encode to the same codes
    assert (again.distance == 0).all() and (again.agreement == 1.0).all()
