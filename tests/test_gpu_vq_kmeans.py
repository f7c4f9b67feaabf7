"""k-means initialisation of the codebook on the device (include/vqvae_kmeans.h, vqvae_amd/codebook_init.py): the entry
points against the NumPy restatement of tests/vq_kmeans_ref.py bit for bit, inside red zones (tests/zoned.py), then through
the Python object: a whole run, what it does to the optimizer, an EMACodebook, a monitor and a recorded step, and the
data-parallel form with two real processes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import vq_ema_ref as E
import vq_kmeans_ref as R
from test_gpu_codebook import CFG, _assert_same_bits, _batches, _bits, _It, _params
from zoned import In, Out, Ws, run_contract

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _lib():
    from vqvae_amd import _lib as L
    return L


def _pool(rs, d, N, kind='normal'):
    if kind == 'dup':                      # a handful of distinct rows, each many times: the total == 0 rounds
        base = rs.standard_normal((d, 5)).astype(np.float32)
        return np.ascontiguousarray(base[:, rs.randint(0, 5, N)])
    if kind == 'blobs':
        return (rs.standard_normal((d, N)) * 0.05 + rs.randint(-4, 5, (d, N // 64 + 1)).repeat(64, 1)[:, :N]).astype(np.float32)
    return (rs.standard_normal((d, N)) * rs.choice([1e-2, 1.0, 30.0], (d, 1))).astype(np.float32)


# --------------------------------------------------------------------------- #
# collect
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('B,d,T,N,row0,count', [
    (2, 64, 960, 1920, 0, 1920), (3, 5, 37, 301, 17, 111), (1, 512, 120, 7680, 7560, 120), (4, 3, 50, 333, 100, 131),
    (5, 1, 1, 9, 4, 5), (2, 7, 33, 40, 39, 1),
])
def test_collect_contract(gpu, B, d, T, N, row0, count):
    rs = np.random.RandomState(B + d + T)
    z = rs.standard_normal((B, d, T)).astype(np.float32)
    before = rs.standard_normal((d, N)).astype(np.float32)
    specs = dict(z=In(z), pool=Out(init=before))
    got = run_contract(gpu, lambda a: _lib().call('vqvae_kmeans_collect', a.z.ptr, B, d, T, count, a.pool.ptr, N, row0,
                                                  gpu.stream()), specs)['pool']
    want = before.copy()
    want[:, row0:row0 + count] = z.transpose(0, 2, 1).reshape(B * T, d)[:count].T
    np.testing.assert_array_equal(_bits(got), _bits(want))


# --------------------------------------------------------------------------- #
# seeding
# --------------------------------------------------------------------------- #
SEED_SHAPES = [
    # N, d, k, seed, kind, shift of the pool in bytes
    (1000, 64, 16, 0, 'normal', 0),            # N no multiple of the block
    (100, 1, 8, 1, 'normal', 0),               # smaller than one block, d = 1
    (256, 128, 1, 2, 'normal', 0),             # k = 1
    (257, 3, 5, 3, 'normal', 0),
    (7680, 512, 12, 0x1234567890ABCDEF, 'normal', 0),      # the default model's pool
    (30720, 64, 24, 5, 'blobs', 0),            # configs[1]'s pool
    (5, 4, 9, 6, 'normal', 0),                 # k > N
    (300, 6, 12, 7, 'dup', 0),                 # five distinct rows: rounds 5.. meet total == 0
    (262144, 8, 6, 8, 'normal', 0),            # four rows a thread (1 024 blocks, N % 4 == 0)
    (262144, 8, 6, 8, 'normal', 4),            # the same pool 4 bytes off a 16-byte boundary: one row a thread, same bits
    (525056, 2, 4, 9, 'normal', 0),            # 2 051 blocks: two chunks in the pick kernel's tree
    (524289, 2, 3, 10, 'normal', 0),           # N % 4 != 0 beyond one chunk
]


def _seed(gpu, a, N, d, k, seed):
    _lib().call('vqvae_kmeans_seed', a.pool.ptr, N, d, k, seed, a.W.ptr, a.rows.ptr, a.mind.ptr, a.ws.ptr, a.ws.nbytes,
                gpu.stream())


@pytest.mark.parametrize('N,d,k,seed,kind,shift', SEED_SHAPES)
def test_seed_contract(gpu, N, d, k, seed, kind, shift):
    """rows, W and mind bit for bit against the restatement; run_contract runs the call twice (plain buffers, then red
    zones with a poisoned workspace and outputs) and compares the two runs' bits."""
    pool = _pool(np.random.RandomState(N + d + k), d, N, kind)
    need = _lib().load().vqvae_kmeans_workspace_bytes(N, d, k)
    assert need > 0
    specs = dict(pool=In(pool, shift=shift), W=Out((k, d)), rows=Out((k,), np.int32), mind=Out((N,)), ws=Ws(need))
    got = run_contract(gpu, lambda a: _seed(gpu, a, N, d, k, seed), specs)
    W, rows, mind, totals = R.seed(pool, k, seed)
    np.testing.assert_array_equal(got['rows'], rows)
    np.testing.assert_array_equal(_bits(got['W']), _bits(W))
    np.testing.assert_array_equal(_bits(got['mind']), _bits(mind))
    if kind == 'dup':
        assert totals[4:] == [0.0] * (k - 5) and len(np.unique(pool[:, rows[:5]], axis=1).T) == 5
    if k > N:
        assert totals[N - 1:] == [0.0] * (k - N)
    if kind == 'normal' and k <= N:
        assert len(set(rows.tolist())) == k and (mind[rows] == 0).all()


def test_seed_spreads_over_well_separated_blobs(gpu):
    """k blobs, 64 rows each: D^2 sampling puts one seed into every blob (the blobs are 1 apart, 1e-3 wide)."""
    k, d = 48, 16
    rs = np.random.RandomState(0)
    centres = rs.standard_normal((k, d)).astype(np.float32) * 3
    pool = np.ascontiguousarray((centres.repeat(64, 0) + rs.standard_normal((k * 64, d)) * 1e-3).astype(np.float32).T)
    N = k * 64
    a = dict(pool=gpu.to_device(pool), W=gpu.empty((k, d)), rows=gpu.empty((k,), np.int32), mind=gpu.empty((N,)),
             ws=gpu.DeviceArray((_lib().load().vqvae_kmeans_workspace_bytes(N, d, k),), np.uint8))
    _lib().call('vqvae_kmeans_seed', a['pool'].ptr, N, d, k, 3, a['W'].ptr, a['rows'].ptr, a['mind'].ptr, a['ws'].ptr,
                a['ws'].nbytes, gpu.stream())
    rows = a['rows'].get()
    assert sorted((rows // 64).tolist()) == list(range(k))
    assert a['mind'].get().max() < 1e-3


# --------------------------------------------------------------------------- #
# update, inertia
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('N,d,k,empty', [(1000, 64, 16, True), (1000, 64, 16, False), (77, 3, 130, True), (30720, 64, 512, True),
                                         (7680, 512, 128, False), (525056, 2, 4, False)])
def test_update_and_inertia_contract(gpu, N, d, k, empty):
    rs = np.random.RandomState(N + k)
    pool = _pool(rs, d, N)
    live = rs.choice(k, max(k // 3, 1), replace=False) if empty else np.arange(k)
    idx = live[rs.randint(0, live.size, N)].astype(np.int32)
    if not empty:
        idx[:k] = np.arange(k)[:N]
    n, S = E.accumulate(idx[None], pool[None], k)
    stats = E.stats_of(n, S)
    seed, it = 0xABCDEF0123456789, 3
    specs = dict(pool=In(pool), stats=In(stats), W=Out((k, d)), n_empty=Out((1,), np.int32))
    got = run_contract(gpu, lambda a: _lib().call('vqvae_kmeans_update', a.pool.ptr, N, d, k, a.stats.ptr, seed, it, a.W.ptr,
                                                  a.n_empty.ptr, gpu.stream()), specs)
    W, n_empty = R.update(pool, n, S, seed, it)
    assert int(got['n_empty'][0]) == n_empty == int((n == 0).sum()) and (n_empty > 0) == (empty or k > N)
    np.testing.assert_array_equal(_bits(got['W']), _bits(W))
    # the inertia of that codebook under the same assignment, with a few indices outside the codebook
    idx2 = idx.copy()
    idx2[::13] = -1
    idx2[5 % N] = k
    need = _lib().load().vqvae_kmeans_workspace_bytes(N, d, k)
    specs = dict(pool=In(pool), W=In(W), idx=In(idx2, index_range=(0, k)), out=Out((1,), np.float64), ws=Ws(need))
    got = run_contract(gpu, lambda a: _lib().call('vqvae_kmeans_inertia', a.pool.ptr, a.W.ptr, a.idx.ptr, N, d, k, a.out.ptr,
                                                  a.ws.ptr, a.ws.nbytes, gpu.stream()), specs)
    want = R.inertia(pool, W, idx2)
    assert _bits(got['out'])[0] == _bits(np.array([want]))[0], (got['out'][0], want)


# --------------------------------------------------------------------------- #
# the Python object
# --------------------------------------------------------------------------- #
def _vq(gpu, k, d, seed=0):
    import vqvae_amd as V
    vq = V.VQ(k, d)
    vq.W.data = (np.random.RandomState(seed).standard_normal((k, d)) * 0.01).astype(np.float32)
    vq.to_gpu()
    return vq


def _reference_run(pool, k, seed, iters):
    W, rows, _, _ = R.seed(pool, k, seed)
    inertia, empty = [], []
    for it in range(iters):
        idx = R.argmin_exact(pool, W)
        inertia.append(R.inertia(pool, W, idx))
        n, S = E.accumulate(idx[None], pool[None], k)
        W, ne = R.update(pool, n, S, seed, it)
        empty.append(ne)
    idx = R.argmin_exact(pool, W)
    inertia.append(R.inertia(pool, W, idx))
    return W, rows, inertia, empty, np.bincount(idx, minlength=k).astype(np.float32)


@pytest.mark.parametrize('k,d,B,T,calls,iters,kind', [(24, 16, 2, 100, 5, 4, 'normal'), (40, 32, 3, 67, 4, 3, 'dup'),
                                                      (8, 64, 1, 300, 1, 0, 'normal')])
def test_run_equals_the_restatement(gpu, k, d, B, T, calls, iters, kind):
    import vqvae_amd as V
    from vqvae_amd import core
    rs = np.random.RandomState(k + d)
    rows = B * T * calls - 7 if calls > 1 else B * T              # the last collect() is cut
    zs = [np.ascontiguousarray(_pool(rs, d, B * T, kind).T.reshape(B, T, d).transpose(0, 2, 1)) for _ in range(calls)]
    pool = np.concatenate([z.transpose(0, 2, 1).reshape(B * T, d) for z in zs])[:rows].T.copy()
    vq = _vq(gpu, k, d)
    addr = vq.W.data.ptr
    init = V.KMeansCodebookInit(vq, rows=rows, iters=iters, seed=11)
    left = rows
    for i, z in enumerate(zs):
        left = init.collect(core.Variable(gpu.to_device(z[..., None])) if i % 2 else gpu.to_device(z))
        assert left == max(rows - (i + 1) * B * T, 0)
    np.testing.assert_array_equal(_bits(init.pool.get()), _bits(pool))
    e0 = core.param_epoch('load')
    rep = init.run()
    W, seeds, inertia, empty, counts = _reference_run(pool, k, 11, iters)
    assert vq.W.data.ptr == addr and core.param_epoch('load') == e0 + 1 and vq._cache is None and init.pool is None
    np.testing.assert_array_equal(_bits(vq.W.data.get()), _bits(W))
    np.testing.assert_array_equal(rep['rows'], seeds)
    np.testing.assert_array_equal(rep['counts'], counts)
    assert rep['empty'] == empty and [float(x).hex() for x in rep['inertia']] == [float(x).hex() for x in inertia]
    assert len(rep['inertia']) == iters + 1 and rep['counts'].sum() == rows
    for i in range(iters):
        if empty[i] == 0:
            assert rep['inertia'][i + 1] <= rep['inertia'][i] * (1 + 1e-6)
    if kind == 'dup' and iters:
        assert sum(empty) > 0 and (counts == 0).any()            # 20 distinct rows, 40 codes: clusters stay empty
    with pytest.raises(RuntimeError, match='rows are missing'):
        init.run()


def test_run_on_blobs_uses_every_code_and_beats_random_rows(gpu):
    """k blobs of 64 rows, 0.02 wide and several units apart (D^2 sampling then misses a blob with a probability of about
    1e-3 over all rounds): every code ends with its blob's 64 rows, far below a random-row initialisation's inertia."""
    import vqvae_amd as V
    k, d = 32, 24
    rs = np.random.RandomState(5)
    centres = rs.standard_normal((k, d)).astype(np.float32) * 4
    pool = np.ascontiguousarray((centres.repeat(64, 0) + rs.standard_normal((k * 64, d)) * 0.02).astype(np.float32)[rs.permutation(k * 64)].T)
    N = k * 64
    vq = _vq(gpu, k, d)
    init = V.KMeansCodebookInit(vq, rows=N, iters=5, seed=0)
    assert init.collect(gpu.to_device(pool[None])) == 0
    rep = init.run()
    assert rep['counts'].tolist() == [64.0] * k and rep['empty'] == [0] * 5
    Wr = np.ascontiguousarray(pool[:, rs.choice(N, k, replace=False)].T)
    random_init = R.inertia(pool, Wr, R.argmin_exact(pool, Wr))
    assert rep['inertia'][-1] < 0.25 * random_init and rep['inertia'][-1] <= rep['inertia'][0]
    np.testing.assert_allclose(np.sort(vq.W.data.get(), 0), np.sort(centres, 0), atol=0.02)


def test_lazily_shaped_codebook_and_argument_errors(gpu):
    import vqvae_amd as V
    vq = V.VQ(12)
    init = V.KMeansCodebookInit(vq, rows=50, iters=1)
    z = gpu.to_device(np.random.RandomState(0).standard_normal((1, 6, 50)).astype(np.float32))
    assert init.collect(z) == 0
    assert isinstance(vq.W.data, gpu.DeviceArray) and vq.W.data.shape == (12, 6)
    with pytest.raises(ValueError, match='channels'):
        init.collect(gpu.to_device(np.zeros((1, 7, 5), np.float32)))
    rep = init.run()
    assert rep['counts'].sum() == 50 and np.isfinite(vq.W.data.get()).all()
    other = V.KMeansCodebookInit(_vq(gpu, 12, 6), rows=50)
    other.collect(z)

    class _NoSuch(object):
        m = v = z
        n_train = 0
        target = V.VQ(3, 2)

        def layout(self):
            return []
    with pytest.raises(ValueError, match='does not hold this codebook'):
        other.run(optimizer=_NoSuch())


# --------------------------------------------------------------------------- #
# inside training
# --------------------------------------------------------------------------- #
def _trainer(data, graph=False, seed=4):
    import vqvae_amd as V
    from vqvae_amd.optimizers import Adam
    _, model = H.build_model(CFG, seed=seed)
    model.to_gpu()
    opt = Adam(2e-4)
    opt.setup(model)
    return model, opt, V.VQVAE_StandardUpdater(_It(data), opt, device=0, graph=graph)


def _state(model, opt):
    return dict(_params(model), m=opt.m.get(), v=opt.v.get())


def test_run_between_steps_touches_the_codebook_slot_only_and_a_recorded_step_replays_it(gpu):
    """Eager and recorded trainers run the same schedule: 4 steps, kmeans_init at the step boundary, 3 steps.  W keeps its
    address; Adam's m and v of the codebook slot are zero and every other word of params / m / v keeps its bits; an attached
    EMACodebook holds N = 1, m = W, a monitor the scaled counts; the recording made before the call is replayed after it
    and ends in the eager run's bits."""
    import vqvae_amd as V
    data = _batches(4)
    out = {}
    for graph in (False, True):
        model, opt, upd = _trainer(data, graph=graph)
        for _ in range(4):
            upd.update()
        recorded = upd._graphed
        assert (recorded is not None) == graph
        off, size = {n: (o, s) for n, o, s in opt.layout()}['/vq/W']
        before = dict(params=opt.params.get(), m=opt.m.get(), v=opt.v.get())
        assert np.abs(before['m'][off:off + size]).max() > 0
        addr = model.vq.W.data.ptr
        rep = V.kmeans_init(model, _It(data), rows=100, iters=2, seed=1, optimizer=opt)
        after = dict(params=opt.params.get(), m=opt.m.get(), v=opt.v.get())
        assert model.vq.W.data.ptr == addr and rep['counts'].sum() == 100 and len(rep['inertia']) == 3
        for key in ('params', 'm', 'v'):
            changed = np.nonzero(_bits(after[key]) != _bits(before[key]))[0]
            assert changed.size and changed.min() >= off and changed.max() < off + size, key
        assert not after['m'][off:off + size].any() and not after['v'][off:off + size].any()
        for _ in range(3):
            upd.update()
        assert upd._graphed is recorded                      # no re-recording: W did not move
        out[graph] = (_state(model, opt), rep)
    _assert_same_bits(out[False][0], out[True][0], 'eager against recorded')
    assert out[False][1]['inertia'] == out[True][1]['inertia']


def test_run_resets_an_attached_ema_and_primes_an_attached_monitor(gpu):
    import vqvae_amd as V
    from vqvae_amd import core
    k, d, B, T = 20, 8, 2, 60
    rs = np.random.RandomState(2)
    vq = _vq(gpu, k, d)
    ema, mon = V.EMACodebook(vq, decay=0.9), V.CodebookMonitor(vq, decay=0.9, seed=1)
    vq.codebook_ema, vq.monitor = ema, mon
    try:
        z = gpu.to_device(rs.standard_normal((B, d, T)).astype(np.float32))
        with core.using_config('train', True):
            vq(core.Variable(z))
        ema.step()
        assert (ema.count_dev.get() != 1).any()
        init = V.KMeansCodebookInit(vq, rows=B * T + 30, iters=2, seed=0)
        init.collect(z)
        init.collect(z)
        rep = init.run()
        W = vq.W.data.get()
        assert (ema.count_dev.get() == 1).all()
        np.testing.assert_array_equal(_bits(ema.sum_dev.get()), _bits(W))
        want = (rep['counts'] * np.float32(float(B * T) / float(B * T + 30))).astype(np.float32)
        np.testing.assert_array_equal(_bits(mon.usage()), _bits(want))
        assert mon.reseed(None, threshold=0.05) == int((rep['counts'] == 0).sum())
    finally:
        vq.codebook_ema = vq.monitor = None


def test_a_model_that_never_calls_the_api_steps_as_before(gpu):
    """Two fresh models take the same steps, one in a process state where an init object exists for ANOTHER codebook."""
    import vqvae_amd as V
    data = _batches(2)
    states = []
    for other in (False, True):
        model, opt, upd = _trainer(data)
        if other:
            init = V.KMeansCodebookInit(_vq(gpu, 16, 8), rows=40)
            init.collect(gpu.to_device(np.ones((1, 8, 40), np.float32)))
            init.run()
        for _ in range(3):
            upd.update()
        states.append(_state(model, opt))
    _assert_same_bits(states[0], states[1], 'without against beside an initialisation')


# --------------------------------------------------------------------------- #
# data parallel, two processes on one GPU
# --------------------------------------------------------------------------- #
def test_two_process_initialisation_ends_with_rank_zeros_codebook(gpu, tmp_path):
    d = str(tmp_path)
    worker = os.path.join(HERE, 'dp_kmeans_worker.py')
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    procs = [subprocess.Popen([sys.executable, worker, 'rank', str(r), '2', d], env=env) for r in range(2)]
    try:
        for p in procs:
            assert p.wait(timeout=600) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert subprocess.call([sys.executable, worker, 'single', '2', d], env=env, timeout=600) == 0
    W = [np.load(os.path.join(d, 'W_rank%d.npy' % r)) for r in range(2)]
    single = np.load(os.path.join(d, 'W_single.npy'))
    np.testing.assert_array_equal(_bits(W[0]), _bits(W[1]))
    np.testing.assert_array_equal(_bits(W[0]), _bits(single))
    c = [np.load(os.path.join(d, 'counts_rank%d.npy' % r)) for r in range(2)]
    assert c[0].sum() == c[1].sum() and (c[0] != c[1]).any()      # the same codebook on two different pools
    assert np.load(os.path.join(d, 'calls_rank0.npy')) == 1       # one float all-reduce, nothing else
