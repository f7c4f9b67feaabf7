"""EMA codebook updates on the device (include/vqvae_vq_ema.h, vqvae_amd/codebook_ema.py): the three entry points against
the NumPy restatement of tests/vq_ema_ref.py, inside red zones (tests/zoned.py), then through the Python object: inside the
training step (eager and recorded), in the data-parallel form, with re-seeding, and across a snapshot."""
import threading

import numpy as np
import pytest

import helpers as H
import vq_ema_ref as R
from test_gpu_codebook import CFG, _PairComm, _assert_same_bits, _batches, _bits, _It, _params
from zoned import In, Out, Ws, run_contract

pytestmark = pytest.mark.gpu


def _lib():
    from vqvae_amd import _lib as L
    return L


def _idx(rs, B, T, k, kind):
    if kind == 'one':                 # a collapsed assignment
        return np.full((B, T), k // 3, np.int32)
    if kind == 'hot':                 # a few hot codes among many empty ones
        alive = rs.choice(k, max(k // 8, 1), replace=False)
        return alive[(rs.standard_exponential(B * T) * alive.size / 6).astype(np.int64) % alive.size].reshape(B, T).astype(np.int32)
    idx = rs.randint(0, k, (B, T)).astype(np.int32)
    if kind == 'outside':             # indices outside [0, k) are ignored
        flat = idx.reshape(-1)
        flat[::7] = -1
        flat[5::11] = k
        flat[3 % flat.size] = 2 ** 31 - 1
    return idx


def _accumulate(gpu, a, B, d, T, k):
    _lib().call('vqvae_vq_ema_accumulate', a.idx.ptr, a.z.ptr, B, d, T, k, a.stats.ptr, a.ws.ptr, a.ws.nbytes, gpu.stream())


def _ulps(a, b):
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b)).max()


ACC_SHAPES = [
    # B, T, k, d, kind
    (2, 960, 512, 64, 'hot'),               # configs[1]: N = 1 920
    (2, 960, 512, 64, 'one'),
    (4, 120, 128, 512, 'uniform'),          # the reference's default model: N = 480
    (4, 120, 128, 512, 'one'),
    (3, 37, 7, 3, 'uniform'),               # N = 111, T = 37: no multiples of 64
    (2, 333, 130, 65, 'outside'),
    (5, 1, 16, 32, 'uniform'),              # T = 1
    (1, 4096, 64, 8, 'hot'),                # the largest N of the one-launch form
    (1, 4097, 64, 8, 'hot'),                # the smallest of the bucketed form; one full chunk and one row
    (3, 3001, 130, 65, 'outside'),          # bucketed, N = 9 003: no multiple of 64, of the piece or of the sort chunk
    (2, 5000, 96, 16, 'one'),               # bucketed, collapsed: 20 pieces of one code, every other code empty
    (1, 20011, 16384 + 64, 4, 'uniform'),   # k above the LDS cursors of the placement kernel
    (9, 1, 16, 32, 'uniform'),
]


@pytest.mark.parametrize('B,T,k,d,kind', ACC_SHAPES)
def test_accumulate_contract(gpu, B, T, k, d, kind):
    """One call inside red zones: writes stay inside stats and an exactly-sized workspace, the result does not depend on
    what those held before or on what surrounds the inputs, two runs agree bit for bit (run_contract compares a plain and
    a zoned run); n is exact, S is the header's ordered float64 sum bit for bit -- the same order in the one-launch and in
    the bucketed form -- and within one float32 ulp of the plain float64 sum."""
    rs = np.random.RandomState(B * 1000 + T + k + d)
    idx = _idx(rs, B, T, k, kind)
    z = (rs.standard_normal((B, d, T)) * rs.choice([1e-3, 1.0, 50.0], (B, d, 1))).astype(np.float32)
    need = _lib().load().vqvae_vq_ema_workspace_bytes(B, d, T, k)
    assert need > 0 and ((B * T <= _lib().VQ_EMA_SMALL_MAX_N) == (need == 256))
    specs = dict(idx=In(idx, index_range=(0, k)), z=In(z), stats=Out((k * (d + 1),)), ws=Ws(need))
    got = run_contract(gpu, lambda a: _accumulate(gpu, a, B, d, T, k), specs)['stats']
    n, S = R.accumulate(idx, z, k)
    valid = (idx >= 0) & (idx < k)
    np.testing.assert_array_equal(got[:k], n)
    assert got[:k].sum() == valid.sum() and (kind != 'outside' or valid.sum() < B * T)
    np.testing.assert_array_equal(_bits(got[k:].reshape(k, d)), _bits(S))
    assert _ulps(got[k:].reshape(k, d), R.accumulate(idx, z, k, ordered=False)[1]) <= 1
    assert (got[k:].reshape(k, d)[n == 0] == 0).all()
    if kind == 'one':
        assert got[k // 3] == B * T and np.count_nonzero(got[:k]) == 1


def test_both_forms_sum_in_the_same_order(gpu):
    """The same rows and indices once as N = 4 096 (one launch) and once with one more, out-of-range row in front and
    behind the batch boundary so that N = 4 098 takes the bucketed form: every code's list is the same, so is every bit."""
    k, d, T = 40, 24, 2048
    rs = np.random.RandomState(5)
    idx = _idx(rs, 2, T, k, 'hot')
    z = rs.standard_normal((2, d, T)).astype(np.float32)
    idx2 = np.concatenate([idx, np.full((2, 1), -1, np.int32)], 1)
    z2 = np.concatenate([z, np.ones((2, d, 1), np.float32)], 2)
    out = []
    for i, zz in ((idx, z), (idx2, z2)):
        B, _, Tt = zz.shape
        need = _lib().load().vqvae_vq_ema_workspace_bytes(B, d, Tt, k)
        a = dict(idx=gpu.to_device(i), z=gpu.to_device(zz), stats=gpu.zeros((k * (d + 1),), np.float32),
                 ws=gpu.DeviceArray((need,), np.uint8))
        _lib().call('vqvae_vq_ema_accumulate', a['idx'].ptr, a['z'].ptr, B, d, Tt, k, a['stats'].ptr, a['ws'].ptr, need,
                    gpu.stream())
        out.append(a['stats'].get())
    assert (4096 <= _lib().VQ_EMA_SMALL_MAX_N) and (4098 > _lib().VQ_EMA_SMALL_MAX_N)
    np.testing.assert_array_equal(_bits(out[0]), _bits(out[1]))
    assert out[0][:k].sum() == 4096


def test_accumulate_full_size_configs3_once(gpu):
    """configs[3]: N = 1 048 560 rows, k = 8 192, d = 128, an eighth of the codes alive; two calls agree bit for bit."""
    B, T, k, d = 16, 65535, 8192, 128
    rs = np.random.RandomState(1)
    idx = _idx(rs, B, T, k, 'hot')
    z = np.random.default_rng(2).standard_normal((B, d, T), dtype=np.float32)
    need = _lib().load().vqvae_vq_ema_workspace_bytes(B, d, T, k)
    di, dz = gpu.to_device(idx), gpu.to_device(z)
    ws = gpu.DeviceArray((need,), np.uint8)
    got = []
    for _ in range(2):
        stats = gpu.DeviceArray((k * (d + 1),), np.float32)
        _lib().call('vqvae_vq_ema_accumulate', di.ptr, dz.ptr, B, d, T, k, stats.ptr, ws.ptr, need, gpu.stream())
        got.append(stats.get())
    np.testing.assert_array_equal(_bits(got[0]), _bits(got[1]))
    n, S = R.accumulate(idx, z, k)
    np.testing.assert_array_equal(got[0][:k], n)
    assert n.sum() == B * T and (n == 0).sum() >= k - k // 8
    np.testing.assert_array_equal(_bits(got[0][k:].reshape(k, d)), _bits(S))
    assert _ulps(got[0][k:].reshape(k, d), R.accumulate(idx, z, k, ordered=False)[1]) <= 1


# --------------------------------------------------------------------------- #
# apply / reset
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('decay,eps', [(0.99, 1e-5), (0.0, 1e-5), (1.0, 1e-5), (0.5, 1e-2), (0.9, 1e-12)])
@pytest.mark.parametrize('k,d', [(512, 64), (7, 3), (2500, 5)])
def test_apply_is_the_rule_bit_for_bit_over_five_steps(gpu, k, d, decay, eps):
    rs = np.random.RandomState(k + d)
    B, T = 2, 300
    W0 = (rs.standard_normal((k, d)) * 0.1).astype(np.float32)
    W, N, m = gpu.to_device(W0), gpu.zeros((k,), np.float32), gpu.zeros((k, d), np.float32)
    _lib().call('vqvae_vq_ema_reset', W.ptr, N.ptr, m.ptr, k, d, None, gpu.stream())
    np.testing.assert_array_equal(N.get(), np.ones(k, np.float32))
    np.testing.assert_array_equal(_bits(m.get()), _bits(W0))
    want = (W0, np.ones(k, np.float32), W0.copy())
    stats = gpu.zeros((k * (d + 1),), np.float32)
    ws = gpu.DeviceArray((256,), np.uint8)
    for step in range(5):
        idx = _idx(rs, B, T, k, ('hot', 'uniform', 'one')[step % 3])
        z = rs.standard_normal((B, d, T)).astype(np.float32)
        _lib().call('vqvae_vq_ema_accumulate', gpu.to_device(idx).ptr, gpu.to_device(z).ptr, B, d, T, k, stats.ptr, ws.ptr, 256,
                    gpu.stream())
        _lib().call('vqvae_vq_ema_apply', W.ptr, N.ptr, m.ptr, stats.ptr, k, d, decay, eps, gpu.stream())
        s = stats.get()                                               # the device's own statistics
        want = R.apply(want[0], want[1], want[2], s[:k], s[k:].reshape(k, d), decay, eps)
        for got, ref, name in zip((W, N, m), want, ('W', 'ema_count', 'ema_sum')):
            np.testing.assert_array_equal(_bits(got.get()), _bits(ref), 'step %d: %s' % (step, name))
    if decay == 1.0:
        np.testing.assert_array_equal(_bits(m.get()), _bits(W0))     # nothing moves the state


def test_apply_leaves_the_codebook_when_nothing_was_ever_counted(gpu):
    k, d = 9, 4
    W0 = np.arange(k * d, dtype=np.float32).reshape(k, d)
    W, N, m = gpu.to_device(W0), gpu.to_device(np.ones(k, np.float32)), gpu.to_device(W0)
    stats = gpu.zeros((k * (d + 1),), np.float32)
    _lib().call('vqvae_vq_ema_apply', W.ptr, N.ptr, m.ptr, stats.ptr, k, d, 0.0, 1e-5, gpu.stream())
    np.testing.assert_array_equal(W.get(), W0)
    assert (N.get() == 0).all() and (m.get() == 0).all()


@pytest.mark.parametrize('k,d', [(512, 64), (7, 3), (130, 65)])
def test_reset_contract(gpu, k, d):
    rs = np.random.RandomState(k)
    W = rs.standard_normal((k, d)).astype(np.float32)
    N0, m0 = rs.uniform(0, 5, k).astype(np.float32), rs.standard_normal((k, d)).astype(np.float32)
    mask = (rs.uniform(size=k) < 0.3).astype(np.int32) * rs.randint(1, 9, k).astype(np.int32)      # any non-zero selects
    sel = mask != 0
    specs = dict(W=In(W), mask=In(mask), N=Out(init=N0, valid=sel), m=Out(init=m0, valid=np.repeat(sel[:, None], d, 1)))
    got = run_contract(gpu, lambda a: _lib().call('vqvae_vq_ema_reset', a.W.ptr, a.N.ptr, a.m.ptr, k, d, a.mask.ptr,
                                                  gpu.stream()), specs)
    np.testing.assert_array_equal(_bits(got['N']), _bits(np.where(sel, np.float32(1), N0)))
    np.testing.assert_array_equal(_bits(got['m']), _bits(np.where(sel[:, None], W, m0)))
    specs = dict(W=In(W), N=Out((k,)), m=Out((k, d)))
    got = run_contract(gpu, lambda a: _lib().call('vqvae_vq_ema_reset', a.W.ptr, a.N.ptr, a.m.ptr, k, d, None, gpu.stream()),
                       specs)
    assert (got['N'] == 1).all()
    np.testing.assert_array_equal(_bits(got['m']), _bits(W))


# --------------------------------------------------------------------------- #
# inside the training step
# --------------------------------------------------------------------------- #
def _trainer(data, graph=False, ema=True, monitor=False, start=0, seed=4, decay=0.9):
    import vqvae_amd as V
    from vqvae_amd.optimizers import Adam
    _, model = H.build_model(CFG, seed=seed)
    model.to_gpu()
    opt = Adam(2e-4)
    opt.setup(model)
    obj = mon = None
    if ema:
        obj = V.EMACodebook(model.vq, decay=decay, eps=1e-5)
        model.vq.codebook_ema = obj
    if monitor:
        mon = V.CodebookMonitor(model.vq, decay=0.9, seed=21)
        model.vq.monitor = mon
    upd = V.VQVAE_StandardUpdater(_It(data, start), opt, device=0, graph=graph)
    return model, opt, obj, mon, upd


def _detach(model):
    model.vq.codebook_ema = None
    model.vq.monitor = None


def _ema_state(ema):
    return dict(count=ema.count_dev.get(), sum=ema.sum_dev.get(), n=ema.counts(), S=ema.sums())


def _w_slot(model, opt):
    named = dict(model.namedparams())
    for name, off, size in opt.layout():
        if named.get(name) is model.vq.W:
            return off, size
    raise AssertionError('the optimizer does not hold the codebook')


def test_one_step_moves_the_codebook_by_the_rule_and_nothing_else_differently(gpu, monkeypatch):
    data = _batches(1)
    L = _lib()
    real_call, seen = L.call, []
    monkeypatch.setattr(L, 'call', lambda name, *a: (seen.append(name), real_call(name, *a))[1])
    out, launches = {}, {}
    for with_ema in (False, True):
        model, opt, ema, _, upd = _trainer(data, ema=with_ema)
        W0 = model.vq.W.data.get()
        caught = []
        if with_ema:
            acc = ema.accumulate
            monkeypatch.setattr(ema, 'accumulate', lambda z, i: (caught.append((z, i)), acc(z, i))[1])
        del seen[:]
        upd.update()
        launches[with_ema] = list(seen)
        out[with_ema] = (_params(model), np.array([l.data.get() for l in upd.last_losses]))
        if with_ema:
            (z, idx), = caught                                        # once per step: the second application is a preset
            z, idx = z.get(), idx.get()                               # (the references kept both buffers from being recycled)
            k, d = W0.shape
            n, S = R.accumulate(idx, z.reshape(z.shape[:3]), k)
            np.testing.assert_array_equal(ema.counts(), n)
            np.testing.assert_array_equal(_bits(ema.sums()), _bits(S))
            W, N, m = R.apply(W0, np.ones(k, np.float32), W0.copy(), n, S, 0.9, 1e-5)
            np.testing.assert_array_equal(_bits(model.vq.W.data.get()), _bits(W))
            np.testing.assert_array_equal(_bits(ema.count_dev.get()), _bits(N))
            np.testing.assert_array_equal(_bits(ema.sum_dev.get()), _bits(m))
            assert n.sum() == idx.size and (W != W0).any()
            off, size = _w_slot(model, opt)
            assert not opt.grads.get()[off:off + size].any()
            assert not opt.m.get()[off:off + size].any() and not opt.v.get()[off:off + size].any()
            with pytest.raises(RuntimeError, match='accumulated'):
                ema.step()
        _detach(model)
    plain, with_ = out[False], out[True]
    np.testing.assert_array_equal(_bits(plain[1]), _bits(with_[1]))   # loss2 is still computed and reported
    assert sorted(plain[0]) == sorted(with_[0])
    for name in plain[0]:
        if name != '/vq/W':
            np.testing.assert_array_equal(_bits(plain[0][name]), _bits(with_[0][name]), name)
    assert (plain[0]['/vq/W'] != with_[0]['/vq/W']).any()
    assert launches[False].count('vqvae_vq_grad_w') == 1 and launches[True].count('vqvae_vq_grad_w') == 0
    new = [n for n in launches[True] if 'vq_ema' in n]
    assert new == ['vqvae_vq_ema_accumulate', 'vqvae_vq_ema_apply'] and not [n for n in launches[False] if 'vq_ema' in n]
    # the codebook loss is still computed (forward) and no longer back-propagated
    assert launches[True].count('vqvae_sqdiff_mean') == launches[False].count('vqvae_sqdiff_mean') == 2
    assert launches[True].count('vqvae_sqdiff_mean_bwd') == launches[False].count('vqvae_sqdiff_mean_bwd') - 1 == 1


def test_recorded_steps_equal_eager_steps_and_changes_record_again(gpu):
    n = 6
    data = _batches(3)
    out = {}
    for graph in (False, True):
        model, opt, ema, _, upd = _trainer(data, graph=graph)
        losses = []
        for _ in range(n):
            upd.update()
            losses.append(np.array([l.data.get() for l in upd.last_losses]))
        assert (upd._graphed is not None) == graph
        out[graph] = (dict(enumerate(losses)), _params(model), _ema_state(ema), dict(m=opt.m.get(), v=opt.v.get()))
        if graph:
            first = upd._graphed
            ema.decay = 0.8                                           # a kernel argument of the recording
            upd.update()
            second = upd._graphed
            assert second is not None and second is not first
            model.vq.codebook_ema = None
            upd.update()
            third = upd._graphed
            assert third is not None and third is not second
            W = model.vq.W.data.get()
            model.vq.codebook_ema = ema
            upd.update()
            assert upd._graphed is not third and (model.vq.W.data.get() != W).any()
        _detach(model)
    for i, what in enumerate(('losses', 'parameters', 'EMA state', 'moments')):
        _assert_same_bits(out[False][i], out[True][i], what)
    assert (out[True][2]['count'] != 1).any()


def test_data_parallel_replicas_stay_identical_with_one_more_all_reduce(gpu):
    """Two replicas, each its own shard: one step of VQVAE_ParallelUpdater through a size-2 communicator.  Both end with
    the same codebook and state, equal to the rule applied to the summed shard statistics; attaching the EMA objects adds
    exactly one all-reduce to the step."""
    import vqvae_amd as V
    from vqvae_amd.optimizers import Adam
    data = _batches(1, B=4)

    def run(with_ema):
        shared = dict(buf=[None, None], barrier=threading.Barrier(2, timeout=300), calls=0)
        reps, errors = [], []
        for r in range(2):
            _, model = H.build_model(CFG, seed=4)
            model.to_gpu()
            opt = Adam(1e-4)
            opt.setup(model)
            ema = None
            if with_ema:
                ema = V.EMACodebook(model.vq, decay=0.9)
                model.vq.codebook_ema = ema
            upd = V.VQVAE_ParallelUpdater(_It(data), opt, comm=_PairComm(r, shared, gpu), device=0, overlap_comm=False)
            reps.append((model, opt, ema, upd))
        W0 = reps[0][0].vq.W.data.get()
        local = [None, None]

        def work(r):
            try:
                model, opt, ema, upd = reps[r]
                if with_ema:
                    step = ema.step
                    ema.step = lambda comm=None: (local.__setitem__(r, (ema.counts(), ema.sums())), step(comm))[1]
                upd.update()
            except Exception as e:          # (a broken barrier on the other side ends that thread too)
                errors.append(e)
                shared['barrier'].abort()
        threads = [threading.Thread(target=work, args=(r,)) for r in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        gpu.synchronize()
        return reps, shared['calls'], W0, local
    _, plain_calls, _, _ = run(False)
    reps, calls, W0, local = run(True)
    assert calls == plain_calls + 1
    (m0, _, e0, _), (m1, _, e1, _) = reps
    _assert_same_bits(_params(m0), _params(m1), 'replicas')
    _assert_same_bits(_ema_state(e0), _ema_state(e1), 'EMA state')
    assert (local[0][1] != local[1][1]).any()                         # the shards differ
    n, S = local[0][0] + local[1][0], local[0][1] + local[1][1]       # float32 sums, as the all-reduce forms them
    np.testing.assert_array_equal(e0.counts(), n)
    np.testing.assert_array_equal(_bits(e0.sums()), _bits(S))
    k = W0.shape[0]
    W, N, m = R.apply(W0, np.ones(k, np.float32), W0.copy(), n, S, 0.9, 1e-5)
    np.testing.assert_array_equal(_bits(m0.vq.W.data.get()), _bits(W))
    np.testing.assert_array_equal(_bits(e0.count_dev.get()), _bits(N))
    np.testing.assert_array_equal(_bits(e0.sum_dev.get()), _bits(m))
    for model, _, _, _ in reps:
        _detach(model)


def test_reseed_restarts_the_state_of_the_replaced_rows_only(gpu):
    data = _batches(4)
    model, opt, ema, mon, upd = _trainer(data, monitor=True)
    for _ in range(3):
        upd.update()
    before = (ema.count_dev.get(), ema.sum_dev.get(), model.vq.W.data.get())
    thr = float(np.sort(mon.usage())[CFG['k'] // 4]) + 0.125
    replaced = mon.reseed(opt, threshold=thr)
    mask = mon.last_mask != 0
    assert replaced == mask.sum() and 0 < replaced < CFG['k']
    W, N, m = model.vq.W.data.get(), ema.count_dev.get(), ema.sum_dev.get()
    assert (N[mask] == 1).all()
    np.testing.assert_array_equal(_bits(m[mask]), _bits(W[mask]))
    np.testing.assert_array_equal(_bits(N[~mask]), _bits(before[0][~mask]))
    np.testing.assert_array_equal(_bits(m[~mask]), _bits(before[1][~mask]))
    assert (W[mask] != before[2][mask]).any(1).all()
    upd.update()
    # the next step is the rule from the restarted state: a replaced row nobody chose stays where it was put (to rounding
    # of the smoothing), and none is pulled back to its old place
    n, S = ema.counts(), ema.sums()
    want = R.apply(W, N, m, n, S, 0.9, 1e-5)
    W2 = model.vq.W.data.get()
    np.testing.assert_array_equal(_bits(W2), _bits(want[0]))
    idle = mask & (n == 0)
    if idle.any():
        np.testing.assert_allclose(W2[idle], W[idle], rtol=1e-3, atol=1e-6)
    moved_back = np.abs(W2[mask] - before[2][mask]).sum(1) < np.abs(W2[mask] - W[mask]).sum(1)
    assert not moved_back.any()
    _detach(model)


def test_resume_from_a_snapshot_continues_bit_for_bit(gpu, tmp_path):
    import vqvae_amd as V
    from vqvae_amd import serializers
    from vqvae_amd.codebook_ema import SNAPSHOT_PREFIX
    data = _batches(5)
    path = str(tmp_path / 'snap.npz')
    model, opt, ema, _, upd = _trainer(data, decay=0.75)
    for _ in range(3):
        upd.update()
    serializers.save_npz(path, upd)
    with np.load(path) as f:
        assert {SNAPSHOT_PREFIX + 'vq/' + key for key in ('decay', 'eps', 'count', 'sum')} <= set(f.files)
        np.testing.assert_array_equal(_bits(f[SNAPSHOT_PREFIX + 'vq/count']), _bits(ema.count_dev.get()))
    for _ in range(2):
        upd.update()
    want = (_params(model), dict(m=opt.m.get(), v=opt.v.get()), _ema_state(ema))
    _detach(model)
    model2, opt2, ema2, _, upd2 = _trainer(data, start=3, seed=99, decay=0.5)     # everything comes from the file
    serializers.load_npz(path, upd2)
    assert (ema2.decay, ema2.eps, upd2.iteration) == (0.75, 1e-5, 3)
    for _ in range(2):
        upd2.update()
    _assert_same_bits(_params(model2), want[0], 'parameters')
    _assert_same_bits(dict(m=opt2.m.get(), v=opt2.v.get()), want[1], 'moments')
    _assert_same_bits(_ema_state(ema2), want[2], 'EMA state')
    _detach(model2)


# --------------------------------------------------------------------------- #
# what it is for: the 300-step run of tests/test_gpu_trained.py
# --------------------------------------------------------------------------- #
MEASURED_EMA_LIVE = 2


def _train_ema(gpu):
    """tests/test_gpu_trained_live.py's _train(gpu, reseed=True), restated with an EMA object beside the monitor (that
    function has no hook for one).  Returns (first losses, last losses, distinct codes at the trained state, codes replaced
    per re-seed, finite everywhere)."""
    import vqvae_amd as V
    import vqvae_oracle as O
    import test_gpu_trained as TT
    import test_gpu_trained_live as TL
    from test_gpu_configs import CFG0
    from test_gpu_model import _Iter
    from vqvae_amd import core
    from vqvae_amd.optimizers import Adam
    cfg = dict(CFG0)
    _, model = H.build_model(cfg, seed=5, ema_decay=0.9999)
    model.to_gpu()
    opt = Adam(TT.TRAIN_LR)
    opt.setup(model)
    batches = [O.synth_batch(1, length=TT.T, n_speaker=cfg['n_speaker'], seed=300 + s) for s in range(4)]
    upd = V.VQVAE_StandardUpdater(_Iter(batches), opt, device=0)
    mon = V.CodebookMonitor(model.vq, decay=0.9, seed=0)
    model.vq.monitor = mon
    ema = V.EMACodebook(model.vq)
    model.vq.codebook_ema = ema
    first = last = None
    replaced = []
    try:
        for step in range(TT.TRAIN_STEPS):
            upd.update()
            if step in (0, TT.TRAIN_STEPS - 1):
                l = [float(v.data.get()) for v in upd.last_losses]
                first, last = (l, last) if step == 0 else (first, l)
            it = step + 1
            if it % TL.RESEED_EVERY == 0 and it < TT.TRAIN_STEPS:
                replaced.append(mon.reseed(opt, threshold=TL.THRESHOLD))
        finite = all(np.isfinite(a).all() for a in list(_params(model).values()) + [ema.count_dev.get(), ema.sum_dev.get()])
    finally:
        _detach(model)
    arrays = V.concat_examples(_Iter([batches[1]]).next(), 0)
    with core.using_config('train', False), core.no_backprop_mode():
        model(*arrays)
    distinct = int(np.unique(model.vq._cache[3][0].get()).size)
    return first, last, distinct, replaced, finite


def test_the_ema_rule_against_the_gradient_rule_after_300_steps(gpu):
    import test_gpu_trained as TT
    import test_gpu_trained_live as TL
    gpu.set_matmul_dtype('float32')
    try:
        plain = TL._train(gpu, reseed=False)
        live = TL._train(gpu, reseed=True)
        ema = _train_ema(gpu)
    finally:
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())
    print('trained state, %d steps: distinct codes %d (gradient rule) / %d (gradient rule, re-seeded) / %d (EMA rule, '
          're-seeded; codes replaced per re-seed: %s); final loss2 %.6g / %.6g / %.6g; final loss1 %.4f / %.4f / %.4f'
          % (TT.TRAIN_STEPS, plain[3], live[3], ema[2], ema[3], plain[2][1][1], live[2][1][1], ema[1][1],
             plain[2][1][0], live[2][1][0], ema[1][0]))
    assert ema[4] and np.isfinite(ema[0]).all() and np.isfinite(ema[1]).all()
    # Measured on an MI355X (one run): 1 / 6 / 2 distinct codes, final loss2 7.14e-4 / 5.62e-5 / 2.61e-4.  On this synthetic
    # data (120 latents a step for 512 codes, 300 steps at decay 0.99) the EMA run does NOT reach that file's LIVE_BAR of 3
    # codes, and its loss2 is NOT below the re-seeded gradient run's: neither is asserted.  What holds, and is asserted: it
    # beats the plain gradient rule on both counts.
    assert ema[2] >= MEASURED_EMA_LIVE > plain[3], (plain[3], live[3], ema[2])
    assert ema[1][1] < plain[2][1][1], (plain[2][1], live[2][1], ema[1])
