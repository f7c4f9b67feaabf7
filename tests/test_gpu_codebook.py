"""Codebook monitor on the device (include/vqvae_codebook.h, vqvae_amd/codebook.py): both entry points against NumPy
restatements written here, inside red zones (tests/zoned.py), then through the Python object: inside the training step
(eager and recorded), across a snapshot, and in the data-parallel form."""
import threading

import numpy as np
import pytest

import helpers as H
import vqvae_oracle as O
from zoned import In, Out, run_contract

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
STATS = 8


# --------------------------------------------------------------------------- #
# NumPy restatements
# --------------------------------------------------------------------------- #
def _rows(seed, step, k, n):
    """The reservoir hash of include/vqvae_codebook.h (uint64 arithmetic wraps)."""
    with np.errstate(over='ignore'):
        ctr = (np.uint64(step & 0xFFFFFFFF) << np.uint64(32)) | np.arange(k, dtype=np.uint64)
        x = np.uint64(seed & M64) + (ctr + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x % np.uint64(n)).astype(np.int64)


def _observe_ref(idx, z, k, decay, seed, usage, steps, stats):
    """One observe call: (counts, usage, reservoir, steps, stats)."""
    B, d, T = z.shape
    n = B * T
    flat = idx.reshape(-1)
    counts = np.bincount(flat[(flat >= 0) & (flat < k)], minlength=k).astype(np.int32)
    cf = counts.astype(np.float32)
    dec = np.float32(decay)
    new_usage = cf if steps == 0 else dec * usage + (np.float32(1) - dec) * cf
    p = counts[counts > 0].astype(np.float64) / float(n)
    perp = float(np.exp(-(p * np.log(p)).sum()))
    used = float((counts > 0).sum())
    st = np.array(stats, np.float64)
    st[0], st[1] = perp, used
    st[2] += perp
    st[3] += used
    st[4] += 1
    reservoir = z.transpose(0, 2, 1).reshape(n, d)[_rows(seed, steps, k, n)]
    return counts, new_usage.astype(np.float32), reservoir, steps + 1, st


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _check_observe(got, want, name):
    counts, usage, reservoir, steps, st = want
    np.testing.assert_array_equal(got['counts'], counts, name + ' counts')
    np.testing.assert_array_equal(_bits(got['usage']), _bits(usage), name + ' usage')
    np.testing.assert_array_equal(_bits(got['reservoir']), _bits(reservoir), name + ' reservoir')
    assert int(got['steps'][0]) == steps, name
    np.testing.assert_allclose(got['stats'][:5], st[:5], rtol=1e-6, atol=0, err_msg=name + ' stats')
    np.testing.assert_array_equal(got['stats'][[1, 3, 4]], st[[1, 3, 4]], name + ' integer stats')
    np.testing.assert_array_equal(got['stats'][5:], st[5:], name + ' reserved stats words')


def _idx(rs, B, T, k, kind):
    if kind == 'equal':
        return np.full((B, T), k // 3, np.int32)
    if kind == 'skewed':             # a few popular codes, many dead ones
        alive = rs.choice(k, max(k // 8, 1), replace=False)
        return alive[(rs.standard_exponential(B * T) * alive.size / 6).astype(np.int64) % alive.size].reshape(B, T).astype(np.int32)
    return rs.randint(0, k, (B, T)).astype(np.int32)


def _lib():
    from vqvae_amd import _lib as L
    return L


def _observe(gpu, a, B, d, T, k, decay, seed):
    _lib().call('vqvae_codebook_observe', a.idx.ptr, a.z.ptr, B, d, T, k, decay, seed, a.counts.ptr, a.usage.ptr,
                a.reservoir.ptr, a.steps.ptr, a.stats.ptr, gpu.stream())


# --------------------------------------------------------------------------- #
# observe
# --------------------------------------------------------------------------- #
OBSERVE_SHAPES = [
    # B, T, k, d, kind
    (2, 960, 512, 64, 'skewed'),            # configs[1]: N = 1 920
    (3, 37, 128, 512, 'uniform'),           # the default model's codebook; N = 111 and T = 37 are no multiples of 64
    (1, 1, 16, 32, 'uniform'),
    (5, 1027, 512, 64, 'equal'),            # every index the same code
    (1, 100003, 8192, 16, 'skewed'),        # many workgroups, 32 KB of bins each
    (2, 25000, 16384 + 64, 8, 'uniform'),   # k above VQVAE_CODEBOOK_LDS_MAX_K: the global-atomic path
    (1, 70001, 16384, 4, 'equal'),          # the largest k whose bins stay in LDS
]


@pytest.mark.parametrize('steps0', [0, 3])
@pytest.mark.parametrize('B,T,k,d,kind', OBSERVE_SHAPES)
def test_observe_contract(gpu, B, T, k, d, kind, steps0):
    """One call inside red zones: writes stay inside counts / usage / reservoir / steps_seen / stats, the result does not
    depend on what those held before (counts, reservoir; usage too at the first step) or on what surrounds the inputs, two
    runs agree bit for bit (run_contract compares a plain and a zoned run), and the values are the restatement's."""
    assert (k > _lib().CODEBOOK_LDS_MAX_K) == (k == 16384 + 64)
    rs = np.random.RandomState(B * 1000 + T + k + d + steps0)
    idx = _idx(rs, B, T, k, kind)
    z = rs.standard_normal((B, d, T)).astype(np.float32)
    decay, seed = 0.9, 0x1234567890ABCDEF + steps0
    usage0 = (rs.uniform(0, 4, k)).astype(np.float32)
    stats0 = np.array([7.5, 3, 100.25, 41, 9, 0, 0, 0], np.float64) if steps0 else np.zeros(STATS, np.float64)
    specs = dict(idx=In(idx, index_range=(0, k)), z=In(z), counts=Out((k,), np.int32), reservoir=Out((k, d)),
                 usage=Out(init=usage0) if steps0 else Out((k,)), steps=Out(init=np.array([steps0], np.int32)),
                 stats=Out(init=stats0))
    got = run_contract(gpu, lambda a: _observe(gpu, a, B, d, T, k, decay, seed), specs)
    _check_observe(got, _observe_ref(idx, z, k, decay, seed, usage0, steps0, stats0), 'B%d T%d k%d d%d' % (B, T, k, d))
    if kind == 'equal':
        assert got['stats'][0] == 1.0 and got['stats'][1] == 1.0 and got['counts'][k // 3] == B * T


def test_observe_ignores_indices_outside_the_codebook(gpu):
    B, T, k, d = 1, 300, 32, 8
    rs = np.random.RandomState(3)
    idx = rs.randint(0, k, (B, T)).astype(np.int32)
    idx[0, ::7] = -1
    idx[0, 5::11] = k
    idx[0, 3] = 2 ** 31 - 1
    z = rs.standard_normal((B, d, T)).astype(np.float32)
    specs = dict(idx=In(idx), z=In(z), counts=Out((k,), np.int32), reservoir=Out((k, d)), usage=Out((k,)),
                 steps=Out(init=np.zeros(1, np.int32)), stats=Out(init=np.zeros(STATS)))
    got = run_contract(gpu, lambda a: _observe(gpu, a, B, d, T, k, 0.5, 1), specs)
    np.testing.assert_array_equal(got['counts'], _observe_ref(idx, z, k, 0.5, 1, None, 0, np.zeros(STATS))[0])
    assert got['counts'].sum() == ((idx >= 0) & (idx < k)).sum() < B * T


class _State(object):
    """Persistent device state of a sequence of direct calls."""

    def __init__(self, gpu, k, d):
        self.counts = gpu.DeviceArray((k,), np.int32)
        self.usage = gpu.DeviceArray((k,), np.float32)
        self.reservoir = gpu.DeviceArray((k, d), np.float32)
        self.steps = gpu.zeros((1,), np.int32)
        self.stats = gpu.zeros((STATS,), np.float64)

    def host(self):
        return dict(counts=self.counts.get(), usage=self.usage.get(), reservoir=self.reservoir.get(), steps=self.steps.get(),
                    stats=self.stats.get())


def test_observe_sequence_usage_and_interval_sums(gpu):
    """Usage after 1, 2 and 5 calls, the interval sums over those calls and after a reset by the host (configs[1])."""
    B, T, k, d, decay, seed = 2, 960, 512, 64, 0.99, 5
    rs = np.random.RandomState(11)
    st = _State(gpu, k, d)
    usage, steps, stats = None, 0, np.zeros(STATS)
    for call in range(1, 8):
        idx = _idx(rs, B, T, k, 'skewed' if call % 2 else 'uniform')
        z = rs.standard_normal((B, d, T)).astype(np.float32)
        st.idx, st.z = gpu.to_device(idx), gpu.to_device(z)
        _observe(gpu, st, B, d, T, k, decay, seed)
        want = _observe_ref(idx, z, k, decay, seed, usage, steps, stats)
        _, usage, _, steps, stats = want
        if call in (1, 2, 5, 7):
            _check_observe(st.host(), want, 'call %d' % call)
        if call == 5:
            assert stats[4] == 5
            st.stats.fill_zero()          # the host closes a reporting interval
            stats = np.zeros(STATS)
    assert stats[4] == 2 and steps == 7


def test_observe_full_size_configs3_twice(gpu):
    """configs[3] at full size: N = 16 x 65 535 = 1 048 560 rows, k = 8 192, d = 128 (512 MB of latents); two runs from the
    same state give the same bits."""
    B, T, k, d, decay, seed = 16, 65535, 8192, 128, 0.99, 77
    rs = np.random.RandomState(12)
    idx = _idx(rs, B, T, k, 'skewed')
    z = np.random.default_rng(13).random((B, d, T), dtype=np.float32)
    dz, di = gpu.to_device(z), gpu.to_device(idx)
    usage0 = rs.uniform(0, 300, k).astype(np.float32)
    runs = []
    for _ in range(2):
        st = _State(gpu, k, d)
        st.idx, st.z = di, dz
        st.usage.set(usage0)
        st.steps.set(np.array([4], np.int32))
        _observe(gpu, st, B, d, T, k, decay, seed)
        runs.append(st.host())
    _check_observe(runs[0], _observe_ref(idx, z, k, decay, seed, usage0, 4, np.zeros(STATS)), 'configs[3]')
    for key in runs[0]:
        np.testing.assert_array_equal(_bits(runs[0][key]), _bits(runs[1][key]), key)
    dead = int((runs[0]['counts'] == 0).sum())
    print('configs[3] synthetic histogram: %d of %d codes unused, perplexity %.1f' % (dead, k, runs[0]['stats'][0]))
    assert dead >= k // 2


# --------------------------------------------------------------------------- #
# reseed
# --------------------------------------------------------------------------- #
def _reseed(gpu, a, k, d, thr, revived, moments=True):
    _lib().call('vqvae_codebook_reseed', a.W.ptr, a.m.ptr if moments else None, a.v.ptr if moments else None, k, d,
                a.usage.ptr, a.reservoir.ptr, thr, revived, a.n.ptr, a.mask.ptr, gpu.stream())


@pytest.mark.parametrize('k,d,thr', [(512, 64, 0.5), (128, 512, 1.0), (8192, 128, 0.25), (7, 3, 0.5), (130, 65, 0.0),
                                     (64, 32, 1e9)])
@pytest.mark.parametrize('moments', [True, False])
def test_reseed_contract(gpu, k, d, thr, moments):
    """Exactly the codes under the threshold change: their rows are the reservoir's, their moments zero, their usage the
    revived value; every other code keeps its bits; count and mask are right; threshold 0 re-seeds nothing; inside red
    zones."""
    rs = np.random.RandomState(k + d)
    W, m, v, res = [rs.standard_normal((k, d)).astype(np.float32) for _ in range(4)]
    usage = rs.uniform(0, 2 * min(max(thr, 0.25), 10), k).astype(np.float32)
    usage[::5] = np.float32(thr)            # at the threshold: alive
    revived = 0.75
    specs = dict(W=Out(init=W), usage=Out(init=usage), reservoir=In(res), n=Out((1,), np.int32), mask=Out((k,), np.int32))
    if moments:
        specs.update(m=Out(init=m), v=Out(init=v))
    got = run_contract(gpu, lambda a: _reseed(gpu, a, k, d, thr, revived, moments), specs)
    dead = usage < np.float32(thr)
    assert int(got['n'][0]) == int(dead.sum())
    np.testing.assert_array_equal(got['mask'], dead.astype(np.int32))
    np.testing.assert_array_equal(_bits(got['W']), _bits(np.where(dead[:, None], res, W)))
    np.testing.assert_array_equal(_bits(got['usage']), _bits(np.where(dead, np.float32(revived), usage)))
    if moments:
        np.testing.assert_array_equal(_bits(got['m']), _bits(np.where(dead[:, None], np.float32(0), m)))
        np.testing.assert_array_equal(_bits(got['v']), _bits(np.where(dead[:, None], np.float32(0), v)))
    if thr == 0.0:
        assert int(got['n'][0]) == 0
    if thr == 1e9:
        assert int(got['n'][0]) == k - len(range(0, k, 5))       # everything but the codes AT the threshold


# --------------------------------------------------------------------------- #
# inside the training step
# --------------------------------------------------------------------------- #
CFG = dict(H.SMALL)
LENGTH = 512


def _batches(n, B=3):
    out = []
    for s in range(n):
        x_enc, x_dec, spk, t = O.synth_batch(B, length=LENGTH, n_speaker=CFG['n_speaker'], seed=900 + s)
        out.append([(x_enc[i][..., None], x_dec[i][..., None], spk[i], t[i][..., None]) for i in range(B)])
    return out


class _It(object):
    def __init__(self, data, start=0):
        self.data, self.i = data, start

    def next(self):
        self.i += 1
        return self.data[(self.i - 1) % len(self.data)]


def _trainer(data, graph=False, monitor=True, start=0, seed=4):
    import vqvae_amd as V
    from vqvae_amd.optimizers import Adam
    _, model = H.build_model(CFG, seed=seed)
    model.to_gpu()
    opt = Adam(2e-4)
    opt.setup(model)
    mon = None
    if monitor:
        mon = V.CodebookMonitor(model.vq, decay=0.9, seed=21)
        model.vq.monitor = mon
    upd = V.VQVAE_StandardUpdater(_It(data, start), opt, device=0, graph=graph)
    return model, opt, mon, upd


def _params(model):
    return {n: p.data.get() for n, p in model.namedparams()}


def _mon_state(mon):
    return dict(counts=mon.counts(), usage=mon.usage(), reservoir=mon.reservoir_dev.get(),
                steps=np.array([mon.steps_seen()]), stats=mon.stats_dev.get())


def _assert_same_bits(a, b, what):
    assert sorted(a) == sorted(b)
    for key in a:
        np.testing.assert_array_equal(_bits(a[key]), _bits(b[key]), '%s: %s' % (what, key))


@pytest.mark.parametrize('graph', [False, True])
def test_step_with_a_monitor_computes_what_the_step_without_one_computes(gpu, graph):
    """Losses, gradients, parameters and Adam moments are bit-identical with and without a monitor; the monitor saw one
    observation per step (the second, preset application of the quantiser is not observed)."""
    n = 6
    data = _batches(3)
    out = {}
    for monitor in (False, True):
        model, opt, mon, upd = _trainer(data, graph=graph, monitor=monitor)
        losses = []
        for _ in range(n):
            upd.update()
            losses.append(np.array([l.data.get() for l in upd.last_losses]))
        if graph:
            assert upd._graphed is not None
        grads = {name: p.grad.get() for name, p in model.namedparams() if p._grad_slot is not None and p.grad is not None} \
            if not graph else {}
        out[monitor] = (dict(enumerate(losses)), grads, _params(model), dict(m=opt.m.get(), v=opt.v.get()))
        if monitor:
            assert mon.steps_seen() == n
            s = mon.summary()
            assert set(s) == {'main/perplexity', 'main/codes_used', 'main/codes_live'}
            counts = mon.counts()
            assert counts.sum() > 0 and counts.sum() % 3 == 0 and 1 <= s['main/codes_used'] <= CFG['k']
            assert 1.0 <= s['main/perplexity'] <= s['main/codes_used'] + 1e-9
        model.vq.monitor = None
    for i, what in enumerate(('losses', 'gradients', 'parameters', 'moments')):
        _assert_same_bits(out[False][i], out[True][i], what)


def test_recorded_steps_leave_the_monitor_where_eager_steps_leave_it(gpu):
    """After n steps through a recording (two eager warm-up steps, the capture, replays) the monitor's whole state equals
    its state after n eager steps, bit for bit: the first-step rule and the hash counter are read from the device word."""
    n = 7
    data = _batches(4)
    states, summaries = {}, {}
    for graph in (False, True):
        model, opt, mon, upd = _trainer(data, graph=graph)
        for i in range(n):
            upd.update()
            if i == 3:
                summaries.setdefault(graph, []).append(mon.summary(reset=True))
        assert (upd._graphed is not None) == graph
        states[graph] = _mon_state(mon)
        summaries[graph].append(mon.summary())
        model.vq.monitor = None
    _assert_same_bits(states[False], states[True], 'monitor state')
    assert summaries[False] == summaries[True]
    assert states[True]['stats'][4] == n - 4 and states[True]['steps'][0] == n


def test_attaching_a_monitor_to_a_recorded_step_records_again(gpu):
    data = _batches(2)
    model, opt, mon, upd = _trainer(data, graph=True, monitor=False)
    for _ in range(4):
        upd.update()
    first = upd._graphed
    assert first is not None
    import vqvae_amd as V
    mon = V.CodebookMonitor(model.vq, decay=0.9, seed=1)
    model.vq.monitor = mon
    for _ in range(3):
        upd.update()
    assert upd._graphed is not None and upd._graphed is not first
    assert mon.steps_seen() == 3
    model.vq.monitor = None


def test_search_cache_is_refreshed_after_reseed(gpu):
    """The quantiser reuses an earlier search while the latents and the codebook are unchanged; reseed changes the codebook
    outside the optimizer, so the next application must search again: its indices are the all-exact search's on the new
    codebook."""
    import vqvae_amd as V
    from vqvae_amd import core
    k, d, B, T = 64, 32, 2, 50
    rs = np.random.RandomState(8)
    vq = V.VQ(k, d)
    vq.W.data = (rs.standard_normal((k, d)) * 0.01).astype(np.float32)
    vq.to_gpu()
    z_host = rs.standard_normal((B, d, T)).astype(np.float32)
    z = core.Variable(gpu.to_device(z_host))
    mon = V.CodebookMonitor(vq, decay=0.5, seed=9)
    vq.monitor = mon
    with core.using_config('train', True):
        vq(z)
        idx_before = vq._cache[3][0].get()
        assert mon.steps_seen() == 1
        vq(z)                                   # a preset application: not observed
        assert mon.steps_seen() == 1
        usage = mon.usage()
        thr = float(np.sort(usage)[k // 2]) + 0.5
        n = mon.reseed(None, threshold=thr)
        assert n == int((usage < np.float32(thr)).sum()) > 0
        assert mon.last_mask.sum() == n and mon.threshold == thr
        W_new = vq.W.data.get()
        rows = z_host.transpose(0, 2, 1).reshape(B * T, d)[_rows(9, 0, k, B * T)]
        np.testing.assert_array_equal(W_new[mon.last_mask == 1], rows[mon.last_mask == 1])
        vq(z)
        idx_after = vq._cache[3][0].get()
    with core.using_config('train', False):
        vq(core.Variable(gpu.to_device(z_host)))      # evaluation: searched, not observed
        assert mon.steps_seen() == 2
    exact = gpu.DeviceArray((B, T), np.int32)
    ws = gpu.workspace(_lib().load().vqvae_vq_workspace_bytes(B, d, T, k))
    _lib().call('vqvae_vq_nearest_fwd', z.data.ptr, vq.W.data.ptr, B, d, T, k, 1, exact.ptr, None, None, ws.ptr, ws.nbytes,
                gpu.stream())
    np.testing.assert_array_equal(idx_after, exact.get())
    assert (idx_after != idx_before).any()
    zr = z_host.transpose(0, 2, 1).reshape(B * T, d).astype(np.float64)
    dist = ((zr[:, None, :] - W_new[None].astype(np.float64)) ** 2).sum(2)
    assert (dist[np.arange(B * T), idx_after.reshape(-1)] <= dist.min(1) + 1e-4).all()
    vq.monitor = None


def test_reseed_through_the_optimizer_resets_the_moments_of_the_replaced_rows_only(gpu):
    data = _batches(3)
    model, opt, mon, upd = _trainer(data)
    for _ in range(3):
        upd.update()
    lay = {name: (off, size) for name, off, size in opt.layout()}
    off, size = lay['/vq/W']
    before = dict(W=model.vq.W.data.get(), m=opt.m.get(), v=opt.v.get(), params=opt.params.get())
    assert np.abs(before['m'][off:off + size]).max() > 0
    usage = mon.usage()
    thr = float(np.sort(usage)[CFG['k'] // 2]) + 0.25
    n = mon.reseed(opt, threshold=thr)
    dead = usage < np.float32(thr)
    assert n == dead.sum() > 0
    after = dict(W=model.vq.W.data.get(), m=opt.m.get(), v=opt.v.get(), params=opt.params.get())
    k, d = before['W'].shape
    for key in ('m', 'v'):
        want = before[key].copy()
        want[off:off + size].reshape(k, d)[dead] = 0
        np.testing.assert_array_equal(_bits(after[key]), _bits(want), key)
    np.testing.assert_array_equal(after['W'][~dead], before['W'][~dead])
    np.testing.assert_array_equal(after['W'][dead], mon.reservoir_dev.get()[dead])
    changed = np.nonzero(_bits(after['params']) != _bits(before['params']))[0]
    assert changed.size and changed.min() >= off and changed.max() < off + size, 'reseed touched another parameter'
    assert mon.summary()['main/codes_live'] == float((mon.usage() >= np.float32(thr)).sum()) == CFG['k']
    upd.update()                              # the step goes on from the re-seeded codebook
    assert np.isfinite([float(l.data.get()) for l in upd.last_losses]).all()
    model.vq.monitor = None


def test_resume_from_a_snapshot_continues_bit_for_bit(gpu, tmp_path):
    """train, snapshot, continue  ==  load, continue: parameters, Adam state and the monitor's state."""
    from vqvae_amd import serializers
    from vqvae_amd.codebook import SNAPSHOT_PREFIX
    data = _batches(5)
    path = str(tmp_path / 'snap.npz')
    model, opt, mon, upd = _trainer(data)
    for _ in range(3):
        upd.update()
    mon.reseed(opt, threshold=float(np.sort(mon.usage())[CFG['k'] // 4]) + 0.125)
    serializers.save_npz(path, upd)
    with np.load(path) as f:
        assert {SNAPSHOT_PREFIX + 'vq/' + key for key in ('usage', 'steps_seen', 'seed', 'decay')} <= set(f.files)
        assert int(f[SNAPSHOT_PREFIX + 'vq/steps_seen']) == 3
    for _ in range(2):
        upd.update()
    want = (_params(model), dict(m=opt.m.get(), v=opt.v.get()), _mon_state(mon))
    model.vq.monitor = None

    import vqvae_amd as V
    model2, opt2, _, upd2 = _trainer(data, monitor=False, start=3, seed=99)      # other initial weights: everything comes from the file
    mon2 = V.CodebookMonitor(model2.vq, decay=0.5, seed=0)                        # decay and seed come from the file too
    model2.vq.monitor = mon2
    serializers.load_npz(path, upd2)
    assert (mon2.decay, mon2.seed, mon2.steps_seen(), upd2.iteration) == (0.9, 21, 3, 3)
    for _ in range(2):
        upd2.update()
    got = (_params(model2), dict(m=opt2.m.get(), v=opt2.v.get()), _mon_state(mon2))
    for key in ('counts', 'usage', 'reservoir', 'steps'):
        np.testing.assert_array_equal(_bits(got[2][key]), _bits(want[2][key]), key)
    _assert_same_bits(got[0], want[0], 'parameters')
    _assert_same_bits(got[1], want[1], 'moments')
    model2.vq.monitor = None


# --------------------------------------------------------------------------- #
# data parallel, one process
# --------------------------------------------------------------------------- #
class _PairComm(object):
    """A communicator of size 2 for two threads of one process: allreduce_grad adds the two ranks' buffers on the device
    (vqvae_elementwise) and leaves the sum in both."""
    size = 2

    def __init__(self, rank, shared, gpu):
        self.rank, self.shared, self.gpu = rank, shared, gpu

    def allreduce_grad(self, flat, stream=None):
        sh = self.shared
        sh['buf'][self.rank] = flat
        sh['barrier'].wait()
        if self.rank == 0:
            a, b = sh['buf']
            assert a.size == b.size
            total = self.gpu.DeviceArray((a.size,), np.float32)
            _lib().call('vqvae_elementwise', _lib().EW_ADD, a.size, a.ptr, b.ptr, total.ptr, 1.0, 1.0, self.gpu.stream())
            a.copy_from(total)
            b.copy_from(total)
            self.gpu.synchronize()
            sh['calls'] += 1
        sh['barrier'].wait()
        return flat


def test_data_parallel_reseed_keeps_the_replicas_identical(gpu):
    """Two replicas of one codebook observe different latents; after reseed through a size-2 communicator both hold the
    same codebook, usage and decisions, and every re-seeded row is a latent of the rank that owns it."""
    import vqvae_amd as V
    from vqvae_amd import core
    from vqvae_amd.codebook import reservoir_owner
    k, d, B, T, steps = 96, 16, 2, 40, 3
    rs = np.random.RandomState(31)
    W0 = (rs.standard_normal((k, d)) * 0.05).astype(np.float32)
    zs = [[(rs.standard_normal((B, d, T)) + 3 * r).astype(np.float32) for _ in range(steps)] for r in range(2)]
    vqs, mons = [], []
    for r in range(2):
        vq = V.VQ(k, d)
        vq.W.data = W0.copy()
        vq.to_gpu()
        mon = V.CodebookMonitor(vq, decay=0.8, seed=17)
        vq.monitor = mon
        with core.using_config('train', True):
            for z in zs[r]:
                vq(core.Variable(gpu.to_device(z)))
        vqs.append(vq)
        mons.append(mon)
    usage = [m.usage() for m in mons]
    assert (usage[0] != usage[1]).any()
    summed = usage[0] + usage[1]
    thr = float(np.sort(summed)[k // 2]) + 0.01
    shared = dict(buf=[None, None], barrier=threading.Barrier(2, timeout=120), calls=0)
    result, errors = [None, None], []

    def work(r):
        try:
            result[r] = mons[r].reseed(None, threshold=thr, comm=_PairComm(r, shared, gpu))
        except Exception as e:              # (a broken barrier on the other side ends that thread too)
            errors.append(e)
            shared['barrier'].abort()
    threads = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    gpu.synchronize()
    assert shared['calls'] == 2              # usage, reservoir: the communicator's float all-reduce, nothing else
    dead = summed < np.float32(thr)
    assert result[0] == result[1] == int(dead.sum()) > 0
    W = [vq.W.data.get() for vq in vqs]
    np.testing.assert_array_equal(_bits(W[0]), _bits(W[1]))
    np.testing.assert_array_equal(_bits(mons[0].usage()), _bits(mons[1].usage()))
    np.testing.assert_array_equal(mons[0].last_mask, mons[1].last_mask)
    np.testing.assert_array_equal(W[0][~dead], W0[~dead])
    owners = reservoir_owner(np.arange(k), steps, 2)
    rows = _rows(17, steps - 1, k, B * T)
    for j in np.nonzero(dead)[0]:
        zr = zs[owners[j]][-1].transpose(0, 2, 1).reshape(B * T, d)
        np.testing.assert_array_equal(W[0][j], zr[rows[j]], 'code %d comes from rank %d' % (j, owners[j]))
    assert set(owners[dead]) == {0, 1}
    for vq in vqs:
        vq.monitor = None
