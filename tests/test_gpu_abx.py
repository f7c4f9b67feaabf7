"""ABX distances on the device (vqvae_amd.abx, csrc/abx.h, csrc/abx.hip) against the NumPy restatement of the rule
(tests/abx_ref.py).  The rule is float64 in one written order, so EVERY comparison with the restatement is a bit equality:
the norms, the local-cost tables, the codebook's table, cost, path_len and distance in every arrangement of the list;
answers known without the restatement; red zones round every output and exactly sized, poisoned workspaces.

The local kernel tiles 16 x 16 frames and stages 32 channels at a time: items of 1, 63, 64 and 65 frames and D of 1, 3, 512,
513 and 4096 straddle both.  The DP has two forms split at a shorter side of 64: the pair shapes stand on both sides of
that and reach the bound of 1024; integer-valued features make exact ties common, so the candidate order is exercised."""
import ctypes as C

import numpy as np
import pytest

import abx_ref as R
import zoned as Z
from vqvae_amd import abx
from vqvae_amd.utils import VQ

pytestmark = pytest.mark.gpu
METRICS = ['cosine', 'euclidean']


def _vq(W):
    W = np.ascontiguousarray(W, np.float32)
    vq = VQ(W.shape[0], W.shape[1])
    vq.W.data = W.copy()
    vq.to_gpu()
    return vq


def _whole(lengths):
    """One item per utterance."""
    n = len(lengths)
    return abx.Items(np.arange(n), np.zeros(n, int), np.array(lengths), np.zeros(n, int))


# ---- steps 1 and 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [1, 3, 512, 513, 4096])
def test_norms_local_costs_and_the_code_table_equal_the_restatement(gpu, D):
    rs = np.random.default_rng(D)
    lengths = [1, 63, 64, 65]
    x = [rs.standard_normal((D, F)).astype(np.float32) for F in lengths]
    x[1] = (1e3 * x[1]).astype(np.float32)                     # scaled by 1e3 and 1e-3 beside each other
    x[2] = (1e-3 * x[2]).astype(np.float32)
    x[1][:, 5] = 0.0                                           # a zero frame
    x[3][:, 64] = 0.0
    fr = abx.Frames.from_latents([x[0], gpu.to_device(x[1]), x[2], x[3]])         # a device array beside host ones
    assert np.array_equal(fr.norms().get(), np.concatenate([R.norms(v) for v in x]))
    ia = np.array([0, 0, 1, 2, 3, 3, 2, 1])
    ib = np.array([0, 3, 2, 2, 1, 3, 0, 1])
    W = rs.standard_normal((33, D)).astype(np.float32)
    W[7] = 0.0
    W[8] *= np.float32(1e3)
    vq = _vq(W)
    for metric in METRICS:
        got = abx.local_costs(fr, _whole(lengths), ia, ib, metric)
        for p, (a, b) in enumerate(zip(ia, ib)):
            want = R.local(x[a], x[b], metric)
            assert got[p].dtype == np.float64 and got[p].shape == want.shape
            assert np.array_equal(got[p], want), (D, metric, p, np.abs(got[p] - want).max())
        if metric == 'cosine':
            assert (got[2][5] == 1.0).all() and (np.diag(got[5])[:64] == 0.0).all() and got[5][64, 64] == 1.0
        table = abx.code_table(vq, metric)
        assert table.shape == (33, 33) and table.dtype == np.float64
        assert np.array_equal(table.get(), R.code_table(W, metric)), (D, metric)


# ---- step 3 ---------------------------------------------------------------------------------------------------------------------
class Case(object):
    pass


ITEMS = [(0, 0, 1), (0, 10, 50), (0, 100, 164), (0, 130, 195), (0, 100, 1600), (0, 200, 500), (0, 495, 502), (1, 0, 1024),
         (1, 300, 1400), (0, 64, 128)]                         # overlapping; the last of utterance 1 ends at the buffer's end
PAIRS = [(0, 0), (0, 1), (1, 0), (2, 9), (2, 3), (2, 4), (3, 3), (3, 2), (5, 6), (6, 5), (7, 8), (2, 9), (3, 9), (8, 6)]
SHAPES = [(1, 1), (1, 40), (40, 1), (64, 64), (64, 65), (64, 1500), (65, 65), (65, 64), (300, 7), (7, 300), (1024, 1100),
          (64, 64), (65, 64), (1100, 7)]


@pytest.fixture(scope='module')
def case(gpu):
    """Computed once and left unchanged: integer-valued features of three channels, the items and pairs above, and the
    restatement of every pair under both metrics."""
    c = Case()
    rs = np.random.RandomState(42)
    c.x = [rs.randint(0, 3, (3, T)).astype(np.float32) for T in (1600, 1400)]
    c.fr = abx.Frames.from_latents(c.x)
    u, a, b = (np.array(v) for v in zip(*ITEMS))
    c.items = abx.Items(u, a, b, np.zeros(len(ITEMS), int))
    c.ia, c.ib = (np.array(v) for v in zip(*PAIRS))
    cut = [c.x[uu][:, aa:bb] for uu, aa, bb in ITEMS]
    assert [(cut[i].shape[1], cut[j].shape[1]) for i, j in PAIRS] == SHAPES
    c.want = dict((m, [R.pair(cut[i], cut[j], m) for i, j in PAIRS]) for m in METRICS)
    c.got = dict((m, abx.pair_distances(c.fr, c.items, c.ia, c.ib, m)) for m in METRICS)
    return c


def _same(pd, want, where=None, what=''):
    assert pd.distance.dtype == pd.cost.dtype == np.float64 and pd.path_len.dtype == np.int32
    for p in range(len(pd)):
        dist, cost, K = want[p if where is None else where[p]]
        assert (pd.cost[p], pd.path_len[p], pd.distance[p]) == (cost, K, dist), (what, p, pd.cost[p], cost, pd.path_len[p], K)


@pytest.mark.parametrize('metric', METRICS)
def test_cost_path_length_and_distance_equal_the_restatement(case, metric):
    _same(case.got[metric], case.want[metric], what=metric)
    pd = case.got[metric]
    # an item against itself: the diagonal, at no cost -- but for its zero frames, which cost 1.0 each under the cosine
    if metric == 'euclidean':
        assert pd.cost[6] == 0.0 and pd.path_len[6] == 65 and pd.distance[6] == 0.0
    else:
        assert pd.cost[6] <= (np.abs(case.x[0][:, 130:195]).sum(axis=0) == 0).sum() and pd.path_len[6] >= 65
    assert pd.cost[8] == pd.cost[9]                                         # both orders of one pair: the cost is symmetric
    assert (pd.cost[3], pd.path_len[3]) == (pd.cost[11], pd.path_len[11])   # a repeated pair
    print('%s: path lengths %r' % (metric, pd.path_len.tolist()))


@pytest.mark.parametrize('metric', METRICS)
def test_a_pair_is_the_same_in_every_arrangement(case, gpu, metric):
    c, want = case, case.want[metric]
    for p in (0, 5, 8, 10):                                                 # alone
        _same(abx.pair_distances(c.fr, c.items, c.ia[p:p + 1], c.ib[p:p + 1], metric), want, [p], 'alone %d' % p)
    order = np.random.RandomState(1).permutation(len(PAIRS))               # shuffled
    _same(abx.pair_distances(c.fr, c.items, c.ia[order], c.ib[order], metric), want, order, 'shuffled')
    assert len(abx.plan_chunks([a * b for a, b in SHAPES], 1)) == len(PAIRS)
    _same(abx.pair_distances(c.fr, c.items, c.ia, c.ib, metric, chunk_bytes=1), want, what='every pair alone')
    _same(abx.pair_distances(c.fr, c.items, c.ia, c.ib, metric, chunk_bytes=8 * 64 * 70), want, what='a few pairs a call')
    # the two sides in different buffers, side b scaled beside nothing of side a's
    other = abx.Frames.from_latents([c.x[1], c.x[0]])
    u, a, b = (np.array(v) for v in zip(*ITEMS))
    swapped = abx.Items(1 - u, a, b, np.zeros(len(ITEMS), int))
    _same(abx.pair_distances((c.fr, other), (c.items, swapped), c.ia, c.ib, metric), want, what='two buffers')


# ---- the codes form -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 2, 128, 8192])
def test_the_codes_form_equals_the_dense_form_over_the_gathered_rows(gpu, k):
    import vqvae_amd as V
    rs = np.random.RandomState(k)
    d = 4 if k == 8192 else 16
    W = rs.randn(k, d).astype(np.float32)
    used = np.array([0, 1, 63, 64, 4097, 8191]) if k == 8192 else np.arange(k)
    tl = [90, 7, 70]
    flat = used[rs.randint(0, used.size, sum(tl))]
    flat[3:9] = flat[3]                                                     # a run of one code: exact ties
    codes = V.LatentCodes(tl, flat, k)
    vq = _vq(W)
    lat = [np.ascontiguousarray(W[h].T) for h in codes.to_host()]
    items = abx.Items([0, 0, 1, 2, 2, 0], [0, 20, 0, 0, 3, 5], [64, 85, 7, 70, 68, 6], np.zeros(6, int))
    ia, ib = np.array([0, 1, 2, 3, 4, 5, 3]), np.array([1, 0, 3, 1, 4, 2, 3])
    for metric in METRICS:
        by_codes = abx.pair_distances(abx.Frames.from_codes(codes, vq), items, ia, ib, metric)
        dense = abx.pair_distances(abx.Frames.from_latents(lat), items, ia, ib, metric)
        assert np.array_equal(by_codes.cost, dense.cost) and np.array_equal(by_codes.path_len, dense.path_len)
        assert np.array_equal(by_codes.distance, dense.distance), (k, metric)
        if k <= 128:
            cut = [lat[u][:, a:b] for u, a, b in zip(items.utterance, items.start, items.stop)]
            _same(by_codes, [R.pair(cut[i], cut[j], metric) for i, j in zip(ia, ib)], what='codes k %d %s' % (k, metric))
    del vq


def test_a_caller_s_own_table_is_honoured(gpu):
    import vqvae_amd as V
    rs = np.random.RandomState(9)
    k, tl = 5, [80, 66]
    table = rs.randint(0, 3, (k, k)).astype(np.float64)                     # not symmetric, integer-valued: ties
    codes = V.LatentCodes(tl, rs.randint(0, k, sum(tl)), k)
    host = codes.to_host()
    items = abx.Items([0, 0, 1, 1], [0, 10, 0, 1], [10, 80, 66, 2], np.zeros(4, int))
    ia, ib = np.array([0, 1, 2, 3, 1]), np.array([1, 2, 1, 0, 0])
    cut = [host[u][a:b] for u, a, b in zip(items.utterance, items.start, items.stop)]
    want = [R.dtw(R.local_codes(cut[i], cut[j], table)) for i, j in zip(ia, ib)]
    for own in (table, gpu.to_device(table)):
        fr = abx.Frames.from_codes(codes, table=own)
        _same(abx.pair_distances(fr, items, ia, ib, 'euclidean'), want, what='own table')
        got = abx.local_costs(fr, items, ia, ib)
        assert all(np.array_equal(g, R.local_codes(cut[i], cut[j], table)) for g, i, j in zip(got, ia, ib))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def _desc(n, d, metric, max_short, ftot, cells, form=0, k=0):
    s = abx.AbxDesc()
    s.n, s.d, s.metric, s.form, s.k, s.max_short = n, d, metric, form, k, max_short
    s.ftot_a = s.ftot_b = s.stride_a = s.stride_b = ftot
    s.cells = cells
    return s


def _tables(b):
    t = abx.AbxTables()
    t.a_start, t.b_start, t.a_len, t.b_len, t.cell_off = b.a_start.ptr, b.b_start.ptr, b.a_len.ptr, b.b_len.ptr, b.cell_off.ptr
    return t


@pytest.mark.parametrize('shapes', [[(1, 1), (64, 70), (5, 3), (17, 64)], [(65, 66), (5, 3), (70, 65)]])
def test_every_entry_point_writes_inside_its_outputs(gpu, shapes):
    """Red zones round every output and round a workspace of exactly the queried size, poisoned; both DP forms."""
    lib = abx.load()
    rs = np.random.RandomState(len(shapes))
    D, ftot = 5, 200
    x = rs.randint(0, 3, (D, ftot)).astype(np.float32)
    a_start = np.array([7 * i for i in range(len(shapes))], np.int64)
    b_start = np.array([ftot - fb for fa, fb in shapes], np.int64)          # every side b ends at the buffer's last frame
    fa, fb = (np.array(v, np.int32) for v in zip(*shapes))
    cell_off = np.concatenate([[0], np.cumsum(fa.astype(np.int64) * fb)]).astype(np.int64)
    n, cells = len(shapes), int(cell_off[-1])
    st = gpu.stream
    for metric in (0, 1):
        d = _desc(n, D, metric, int(np.minimum(fa, fb).max()), ftot, cells)
        need = lib.vqvae_abx_workspace_bytes(C.byref(d))
        assert need == (8 * cells + 255) // 256 * 256

        def run(b):
            t = _tables(b)
            abx.call('vqvae_abx_norms', C.byref(d), 0, b.x.ptr, b.norms.ptr, st())
            abx.call('vqvae_abx_local', C.byref(d), C.byref(t), b.x.ptr, b.x.ptr, b.norms.ptr, b.norms.ptr, None, b.ws.ptr, 8 * cells, st())
            abx.call('vqvae_abx_dtw', C.byref(d), C.byref(t), b.ws.ptr, 8 * cells, b.cost.ptr, b.path_len.ptr, b.distance.ptr, st())

        out = Z.run_contract(gpu, run, dict(x=Z.In(x), a_start=Z.In(a_start), b_start=Z.In(b_start), a_len=Z.In(fa), b_len=Z.In(fb),
                                            cell_off=Z.In(cell_off[:-1]), norms=Z.Out((ftot,), np.float64), cost=Z.Out((n,), np.float64),
                                            path_len=Z.Out((n,), np.int32), distance=Z.Out((n,), np.float64), ws=Z.Ws(8 * cells)))
        name = METRICS[metric]
        assert np.array_equal(out['norms'], R.norms(x))
        for p in range(n):
            dist, cost, K = R.pair(x[:, a_start[p]:a_start[p] + fa[p]], x[:, b_start[p]:b_start[p] + fb[p]], name)
            assert (out['cost'][p], out['path_len'][p], out['distance'][p]) == (cost, K, dist), (name, p)


def test_a_contradicting_table_entry_marks_its_pair_alone(gpu):
    rs = np.random.RandomState(31)
    D, ftot = 4, 120
    x = rs.randint(0, 3, (D, ftot)).astype(np.float32)
    xd = gpu.to_device(x)
    a_start, b_start = np.array([0, 30, 60], np.int64), np.array([10, 50, 100], np.int64)
    fa, fb = np.array([20, 9, 15], np.int32), np.array([12, 30, 20], np.int32)
    cell_off = np.array([0, 240, 510], np.int64)
    n, cells = 3, 810
    want = [R.pair(x[:, a_start[p]:a_start[p] + fa[p]], x[:, b_start[p]:b_start[p] + fb[p]], 'euclidean') for p in range(n)]
    poison = np.array([Z.POISON_WORD, Z.POISON_WORD], '<u4').view(np.float64)[0]

    def run(change, max_short=20):
        tabs = dict(a_start=a_start.copy(), b_start=b_start.copy(), a_len=fa.copy(), b_len=fb.copy(), cell_off=cell_off.copy())
        for name, value in change.items():
            tabs[name][1] = value
        dev = abx.Items.__new__(abx.Items)                                  # a plain holder of the device tables
        for name, host in tabs.items():
            setattr(dev, name, gpu.to_device(host))
        d = _desc(n, D, 1, max_short, ftot, cells)
        ws = Z.ZonedArray(gpu, shape=(cells,), dtype=np.float64, name='ws')
        outs = dict((name, Z.ZonedArray(gpu, shape=(n,), dtype=t, name=name)) for name, t in
                    (('cost', np.float64), ('path_len', np.int32), ('distance', np.float64)))
        t = _tables(dev)
        abx.call('vqvae_abx_local', C.byref(d), C.byref(t), xd.ptr, xd.ptr, None, None, None, ws.ptr, 8 * cells, gpu.stream())
        abx.call('vqvae_abx_dtw', C.byref(d), C.byref(t), ws.ptr, 8 * cells, outs['cost'].ptr, outs['path_len'].ptr,
                 outs['distance'].ptr, gpu.stream())
        gpu.synchronize()
        for zb in list(outs.values()) + [ws]:
            zb.check()
        return outs['cost'].get(), outs['path_len'].get(), outs['distance'].get(), ws.get()

    cost, K, dist, ws = run({})                                             # the table that agrees
    assert [(dd, c, k) for dd, c, k in zip(dist, cost, K)] == want
    whole = ws.copy()
    for change in (dict(a_start=112), dict(a_start=-1), dict(b_start=91), dict(a_len=0), dict(b_len=-3), dict(cell_off=541),
                   dict(cell_off=-8), dict(a_len=21, b_len=30)):             # the last: the shorter side above max_short
        cost, K, dist, ws = run(change)
        assert np.isnan(cost[1]) and np.isnan(dist[1]) and K[1] == 0, change
        for p in (0, 2):                                                    # the neighbours' bits
            assert (dist[p], cost[p], K[p]) == want[p], (change, p)
        assert np.array_equal(ws[:240], whole[:240]) and np.array_equal(ws[510:], whole[510:])
        assert (ws[240:510].view(np.uint64) == poison.view(np.uint64)).all(), change      # nothing else is written for it


def test_a_bad_descriptor_is_refused_without_a_launch(gpu):
    lib = abx.load()
    bufs = dict((name, Z.ZonedArray(gpu, shape=s, dtype=t, name=name)) for name, s, t in (
        ('cost', (2,), np.float64), ('path_len', (2,), np.int32), ('distance', (2,), np.float64), ('ws', (200,), np.float64),
        ('norms', (40,), np.float64)))
    x = gpu.to_device(np.zeros((8, 40), np.float32))
    holder = abx.Items.__new__(abx.Items)
    for name, host in (('a_start', np.array([0, 5], np.int64)), ('b_start', np.array([10, 20], np.int64)),
                       ('a_len', np.array([10, 10], np.int32)), ('b_len', np.array([10, 10], np.int32)),
                       ('cell_off', np.array([0, 100], np.int64))):
        setattr(holder, name, gpu.to_device(host))
    t = _tables(holder)
    good = lambda: _desc(2, 8, 0, 10, 40, 200)

    def refused(rc, who, words):
        msg = lib.vqvae_last_error_string().decode()
        assert rc != 0 and who in msg and words in msg, (who, rc, msg, words)

    for field, value, words in (('n', 0, 'n must be at least 1'), ('d', 4097, 'd must be in [1, 4096]'), ('metric', 5, 'metric must be'),
                                ('form', 3, 'form must be'), ('max_short', 1025, 'align whole utterances with align_many'),
                                ('stride_a', 39, 'stride_a must be at least ftot_a'), ('cells', 0, 'cells must be in')):
        d = good()
        setattr(d, field, value)
        refused(lib.vqvae_abx_norms(C.byref(d), 0, x.ptr, bufs['norms'].ptr, gpu.stream()), 'abx_norms', words)
        refused(lib.vqvae_abx_local(C.byref(d), C.byref(t), x.ptr, x.ptr, bufs['norms'].ptr, bufs['norms'].ptr, None, bufs['ws'].ptr,
                                    1600, gpu.stream()), 'abx_local', words)
        refused(lib.vqvae_abx_dtw(C.byref(d), C.byref(t), bufs['ws'].ptr, 1600, bufs['cost'].ptr, bufs['path_len'].ptr,
                                  bufs['distance'].ptr, gpu.stream()), 'abx_dtw', words)
    refused(lib.vqvae_abx_dtw(C.byref(good()), C.byref(t), bufs['ws'].ptr, 1599, bufs['cost'].ptr, bufs['path_len'].ptr,
                              bufs['distance'].ptr, gpu.stream()), 'abx_dtw', 'the workspace must hold 1600 bytes')
    refused(lib.vqvae_abx_table(8193, 8, 0, x.ptr, bufs['ws'].ptr, bufs['norms'].ptr, 320, gpu.stream()), 'abx_table', 'k must be in')
    gpu.synchronize()
    for name, zb in bufs.items():                           # nothing ran: every payload still holds its poison, every zone its pattern
        zb.check()
        assert np.array_equal(zb.arr.get().view(np.uint8).reshape(-1), zb.initial), name


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _equal_scores(got, want):
    assert got.error == want.error and got.by_label_pair == want.by_label_pair
    assert np.array_equal(got.groups, want.groups) and np.array_equal(got.rates, want.rates)
    for name in ('triples', 'errors', 'ties'):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    for name in ('distance', 'cost', 'path_len', 'ia', 'ib'):
        assert np.array_equal(getattr(got.pairs, name), getattr(want.pairs, name)), name


@pytest.mark.parametrize('noise', [0.05, 3.0])
def test_abx_on_the_constructed_sets(gpu, noise):
    feats, label, speaker = R.constructed(noise)
    M = len(feats)
    items = abx.Items(np.arange(M), np.zeros(M, int), [f.shape[1] for f in feats], label, speaker)
    sc = abx.abx(abx.Frames.from_latents(feats), items)
    memo = {}

    def distance(a, x):
        if (a, x) not in memo:
            memo[(a, x)] = R.pair(feats[a], feats[x], 'cosine')[0]
        return memo[(a, x)]

    error, by_label_pair, groups = R.scores(R.triples(label, speaker), distance)
    assert sc.error == error and sc.by_label_pair == by_label_pair
    assert dict((tuple(int(v) for v in g), (int(n), int(e), int(t)))
                for g, n, e, t in zip(sc.groups, sc.triples, sc.errors, sc.ties)) == groups
    assert np.array_equal(sc.pairs.distance, [distance(a, x) for a, x in zip(sc.plan.pairs_a, sc.plan.pairs_b)])
    assert sc.triples.sum() == 576 and len(sc.pairs) == 264
    print('noise %r: error %.4f' % (noise, sc.error))
    if noise == 0.05:
        assert sc.error == 0.0 and sc.errors.sum() == 0 and sc.ties.sum() == 0
        _equal_scores(abx.abx(abx.Frames.from_latents(feats), items, plan=sc.plan), sc)       # a plan made once and handed over
    else:
        assert 0.0 < sc.error < 0.5
        across = abx.abx(abx.Frames.from_latents(feats), items, across_speakers=True, metric='euclidean', max_per_group=5, seed=2)
        want = R.scores([(a, b, x, tuple(int(v) for v in across.plan.groups[g])) for a, b, x, g in
                         zip(across.plan.tri_a, across.plan.tri_b, across.plan.tri_x, across.plan.tri_group)],
                        lambda a, x: R.pair(feats[a], feats[x], 'euclidean')[0])
        assert across.error == want[0] and across.by_label_pair == want[1] and (across.triples <= 5).all()


def test_waves_end_to_end(gpu):
    import vqvae_amd as V
    from vqvae_amd.net import Encoder
    rs = np.random.RandomState(77)
    d, k = 16, 24
    enc, vq = Encoder(d), VQ(k, d)
    vq.W.data = (0.02 * rs.standard_normal((k, d))).astype(np.float32)
    enc.to_gpu()
    vq.to_gpu()
    tl = (30, 41, 7, 64)
    waves = [(0.5 * rs.standard_normal(64 * t + 13) * np.sin(np.arange(64 * t + 13) / 50.0)).astype(np.float32) for t in tl]
    utt, start, stop, label, speaker = [], [], [], [], []
    for u, t in enumerate(tl):                                              # items of 3 to 7 frames, end to end
        at, m = 0, 0
        while at + 3 <= t:
            F = min(3 + (m + u) % 5, t - at)
            utt.append(u), start.append(at), stop.append(at + F), label.append(m % 3), speaker.append(u % 2)
            at, m = at + F, m + 1
    items = abx.Items(utt, start, stop, label, speaker)
    codes, latents = V.encode_many(enc, vq, waves, return_latents=True)
    corpus = V.ResidentCorpus(waves, np.array([0, 1, 0, 1], np.int32))
    flat = corpus.samples.get()
    own = [flat[int(o):int(o) + int(L)].copy() for o, L in zip(corpus.offsets, corpus.lengths)]
    for what, fr in (('latents', abx.Frames.from_latents(latents)), ('codes', abx.Frames.from_codes(codes, vq))):
        want = abx.abx(fr, items)
        _equal_scores(abx.abx_many(enc, vq, waves, items, what=what), want)
        _equal_scores(abx.abx_many(enc, vq, waves, items, what=what, chunk_bytes=20000), want)      # several chunks of the front end
        _equal_scores(corpus.abx(enc, vq, items, what=what), abx.abx_many(enc, vq, own, items, what=what))
        print('%s: error %.4f over %d triples, %d pairs' % (what, want.error, want.triples.sum(), len(want.pairs)))
    view = corpus.subset([3, 1])
    sub = abx.Items([0, 0, 1, 1], [0, 8, 2, 9], [6, 13, 7, 15], [0, 1, 0, 1], [0, 0, 0, 0])
    _equal_scores(view.abx(enc, vq, sub), abx.abx_many(enc, vq, [own[3], own[1]], sub))
    with pytest.raises(ValueError, match='feature_bytes allows 100'):
        abx.abx_many(enc, vq, waves, items, feature_bytes=100)


def test_features_are_read_in_place(gpu):
    from vqvae_amd import metrics
    from vqvae_amd.metrics import MelConfig
    rs = np.random.RandomState(5)
    cfg = MelConfig(sr=16000, n_fft=64, hop=16, n_mels=12, n_mcep=5)
    waves = [(0.3 * rs.standard_normal(n)).astype(np.float32) for n in (64 + 16 * 39, 64 + 16 * 69, 64 + 16 * 4)]
    feats = metrics.features_many(waves, cfg)
    fr = abx.Frames.from_features(feats)
    assert fr.x is feats.log_mel and fr.d == 12 and fr.tl.tolist() == feats.frames.tolist() and fr.stride == feats.log_mel.shape[1]
    mel = [feats.utterance(i)[0] for i in range(3)]
    items = abx.Items([0, 1, 1, 2], [0, 0, 5, 0], [int(feats.frames[0]), 66, int(feats.frames[1]), int(feats.frames[2])], np.zeros(4, int))
    ia, ib = np.array([0, 1, 3, 2]), np.array([1, 2, 0, 2])
    cut = [mel[u][:, a:b] for u, a, b in zip(items.utterance, items.start, items.stop)]
    for metric in METRICS:
        _same(abx.pair_distances(fr, items, ia, ib, metric), [R.pair(cut[i], cut[j], metric) for i, j in zip(ia, ib)], what='log-mel ' + metric)
