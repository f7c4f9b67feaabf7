"""Optimizer hooks on the device (include/vqvae_optim.h, vqvae_amd/optimizers.py): the norm pass against its NumPy
restatement bit for bit, the hooked Adam against the plain one on pre-scaled gradients, whole steps against the
oracle, the guard, recorded steps against eager ones, the groups, and data parallelism."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import optim_hooks_ref as R
import vqvae_oracle as O
from helpers import assert_close

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHUNK = R.CHUNK
AWKWARD = [1, 7, CHUNK + 1, 0, CHUNK, 3 * CHUNK + 1, 3, 2 * CHUNK - 2, 5]
CFG0 = dict(d=64, k=512, n_loop=2, n_layer=10, filter_size=2, input_dim=256, residual=256,
            dilated=256, skip=256, out_dim=256, local_dim=64, global_dim=128, n_speaker=109)
CFG = dict(H.SMALL)
LENGTH = 512


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b, what=''):
    np.testing.assert_array_equal(_bits(np.asarray(a)), _bits(np.asarray(b)), what)


# ---- the C ABI, directly -------------------------------------------------------------------------------------------
class _Pass(object):
    """The tables of one layout on the device and a state block: what Adam._prepare_hooks builds, by hand."""

    def __init__(self, gpu, sizes, groups=(), slots=3):
        from vqvae_amd import _lib, optimizers as Op
        self.gpu, self.lib, self.slots = gpu, _lib, slots
        self.sizes = [int(s) for s in sizes]
        items, params = Op.plan_items(self.sizes)
        self.n_items, self.n_params, self.groups = len(items), len(self.sizes), [list(m) for m in groups]
        self.items = gpu.to_device(items.reshape(-1))
        self.params = gpu.to_device(params.reshape(-1))
        goff = np.zeros(len(self.groups) + 1, np.int32)
        goff[1:] = np.cumsum([len(m) for m in self.groups])
        self.goff = gpu.to_device(goff)
        self.gmem = gpu.to_device(np.asarray([i for m in self.groups for i in m] + [0], np.int32))
        nbytes = _lib.load().vqvae_optim_state_bytes(self.n_params, len(self.groups), slots)
        assert nbytes == 64 + 8 * self.n_params + 4 * len(self.groups) + 4 * slots * (2 + len(self.groups))
        self.state = gpu.zeros(((nbytes + 7) // 8,), np.float64)
        self.ws = gpu.empty((self.n_items,), np.float64)
        assert self.ws.nbytes == _lib.load().vqvae_optim_workspace_bytes(self.n_items)

    def run(self, g, threshold=np.inf, flags=0, stream=None):
        self.lib.call('vqvae_optim_sumsq', g.ptr, g.size, self.items.ptr, self.n_items, self.params.ptr, self.n_params,
                      self.goff.ptr, self.gmem.ptr, len(self.groups), self.slots, float(threshold), flags, self.state.ptr, self.ws.ptr,
                      self.ws.nbytes, stream if stream is not None else self.gpu.stream())
        if stream is not None:
            self.lib.call('vqvae_stream_synchronize', stream)
        return self.read()

    def read(self):
        raw = self.state.get().view(np.uint8)
        h, n_p, n_g = 64, self.n_params, len(self.groups)
        return {'S': raw[0:8].view(np.float64)[0], 'norm': raw[8:16].view(np.float64)[0],
                'rate': raw[16:24].view(np.float64)[0], 'scale': raw[24:28].view(np.float32)[0],
                'nonfinite': int(raw[28:32].view(np.int32)[0]), 'skipped': int(raw[32:36].view(np.int32)[0]),
                'norm_f32': raw[40:44].view(np.float32)[0], 'rate_f32': raw[44:48].view(np.float32)[0],
                'sp': raw[h:h + 8 * n_p].view(np.float64).copy(),
                'gn': raw[h + 8 * n_p:h + 8 * n_p + 4 * n_g].view(np.float32).copy(),
                'steps': int(raw[36:40].view(np.int32)[0]),
                'ring': raw[h + 8 * n_p + 4 * n_g:][:4 * self.slots * (2 + n_g)].view(np.float32).reshape(self.slots, 2 + n_g).copy(),
                # everything a launch computes from the arena: the block without the launch count and the ring
                'raw': np.concatenate([raw[:36], raw[40:h + 8 * n_p + 4 * n_g]])}


def _check_against_restatement(got, g_host, sizes, threshold=np.inf, groups=()):
    sp = R.param_sumsq(g_host, sizes)
    want = R.finalise(sp, threshold, groups)
    _same_bits(got['sp'], sp, 'S_p')
    _same_bits(got['S'], want['S'], 'S')
    _same_bits(got['norm'], want['norm'], 'norm')
    _same_bits(got['rate'], want['rate'], 'rate')
    _same_bits(got['scale'], want['scale'], 'scale')
    assert got['nonfinite'] == want['nonfinite']
    with np.errstate(over='ignore', invalid='ignore'):
        _same_bits(got['norm_f32'], np.float32(want['norm']), 'norm as float32')
        _same_bits(got['rate_f32'], np.float32(want['rate']), 'rate as float32')
    _same_bits(got['gn'], want['group_norms'], 'group norms')
    return sp, want


def _random_arena(n, seed):
    rng = np.random.RandomState(seed)
    return (10.0 ** rng.uniform(-8, 1, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def _model_step_parts(cfg, length, B, seed, data_seed, ema_decay=None):
    """A model on the device, its optimizer, and one batch's device arrays."""
    from vqvae_amd.optimizers import Adam
    from vqvae_amd.updaters import concat_examples
    P, model = H.build_model(cfg, seed=seed, ema_decay=ema_decay)
    model.to_gpu()
    opt = Adam(2e-4)
    opt.setup(model)
    batch = O.synth_batch(B, length=length, n_speaker=cfg['n_speaker'], seed=data_seed)
    ex = [(batch[0][i][..., None], batch[1][i][..., None], batch[2][i], batch[3][i][..., None]) for i in range(B)]
    return P, model, opt, batch, concat_examples(ex, 0)


def _backward(model, arrays):
    from vqvae_amd import core
    from vqvae_amd.updaters import three_loss_backward
    with core.force_backprop_mode():
        losses = model(*arrays)
    three_loss_backward(model, losses)
    return losses


def _train_sizes(opt):
    return [size for _, off, size in opt.layout() if off + size <= opt.n_train]


def test_norm_pass_config0_after_a_real_backward(gpu):
    """S_p of every parameter and S, bit for bit, on the configs[0] model's gradient arena after one backward."""
    _, model, opt, _, arrays = _model_step_parts(CFG0, 7680, 1, 0, 71, ema_decay=0.9999)
    _backward(model, arrays)
    sizes = _train_sizes(opt)
    assert sum(sizes) == opt.n_train and len(sizes) > 150
    g = opt.grads.get()
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    ps = _Pass(gpu, sizes, groups=[range(0, 5), range(5, len(sizes))])
    got = ps.run(opt.grads, threshold=0.25)
    sp, want = _check_against_restatement(got, g, sizes, 0.25, ps.groups)
    assert want['nonfinite'] == 0 and want['S'] > 0
    exact = float(np.sum(g.astype(np.float64) ** 2))
    assert abs(float(got['S']) - exact) <= 1e-9 * exact


def test_norm_pass_awkward_layout(gpu):
    """A 1-element parameter, odd offsets, a parameter one element longer than a chunk, an empty one."""
    g = _random_arena(sum(AWKWARD), 3)
    ps = _Pass(gpu, AWKWARD, groups=[[0, 1, 2], [8, 5], []])
    got = ps.run(gpu.to_device(g), threshold=1e-3)
    _check_against_restatement(got, g, AWKWARD, 1e-3, ps.groups)
    assert got['sp'][3] == 0.0 and got['gn'][2] == 0.0
    assert got['scale'] < 1.0
    # embedded in a larger buffer: nothing outside g[0, n) takes part
    pad = np.full(sum(AWKWARD) + 64, np.float32(np.nan))
    pad[32:32 + g.size] = g
    big = gpu.to_device(pad)
    got2 = ps.run(big.flat_view(32, g.size), threshold=1e-3)
    np.testing.assert_array_equal(got2['raw'], got['raw'])


@pytest.mark.parametrize('bad', [np.inf, -np.inf, np.nan])
def test_norm_pass_planted_nonfinite(gpu, bad):
    g = _random_arena(sum(AWKWARD), 4)
    offs = np.concatenate([[0], np.cumsum(AWKWARD)])
    owner = 5
    g[offs[owner] + CHUNK + 17] = bad
    ps = _Pass(gpu, AWKWARD, groups=[[0, 1], [4, 5]])
    got = ps.run(gpu.to_device(g), threshold=1.0, flags=1)
    _check_against_restatement(got, g, AWKWARD, 1.0, ps.groups)
    assert got['nonfinite'] == 1 and got['skipped'] == 1
    finite = np.isfinite(got['sp'])
    assert not finite[owner] and finite[np.arange(len(AWKWARD)) != owner].all()
    assert np.isfinite(got['gn'][0]) and not np.isfinite(got['gn'][1])
    if np.isnan(bad):
        assert np.isnan(got['rate']) and got['scale'] == np.float32(1.0)       # a NaN rate clips nothing
    else:
        assert got['rate'] == 0.0 and got['scale'] == np.float32(0.0)
    assert ps.run(gpu.to_device(g), threshold=1.0, flags=0)['skipped'] == 1     # without the guard flag nothing is counted
    assert ps.run(gpu.to_device(g), threshold=1.0, flags=1)['skipped'] == 2     # the counter runs on


def test_norm_pass_is_deterministic(gpu):
    """The same arena gives bit-identical state blocks over 10 launches, and on a second stream."""
    sizes = [70000, 3, 524288, 1, 65537, 12289]
    g = _random_arena(sum(sizes), 5)
    dev = gpu.to_device(g)
    ps = _Pass(gpu, sizes, groups=[[0, 1], [2, 3, 4, 5]])
    first = ps.run(dev, threshold=0.5)
    _check_against_restatement(first, g, sizes, 0.5, ps.groups)
    for _ in range(9):
        ps.ws.fill_zero()
        np.testing.assert_array_equal(ps.run(dev, threshold=0.5)['raw'], first['raw'])
    gpu.synchronize()
    other = _Pass(gpu, sizes, groups=[[0, 1], [2, 3, 4, 5]])
    np.testing.assert_array_equal(other.run(dev, threshold=0.5, stream=gpu.side_stream())['raw'], first['raw'])


def test_report_ring_keeps_one_row_per_launch(gpu):
    """Launch i writes (norm, rate, group norms) as float32 into row i mod n_slots and advances `steps`; group bounds
    outside the member table are clipped to it."""
    sizes = [5, CHUNK + 3, 64]
    ps = _Pass(gpu, sizes, groups=[[0, 1], [2]], slots=3)
    want = []
    for i in range(5):
        g = _random_arena(sum(sizes), 40 + i)
        got = ps.run(gpu.to_device(g), threshold=0.5 + i)
        f = R.finalise(R.param_sumsq(g, sizes), 0.5 + i, ps.groups)
        want.append(np.concatenate([[np.float32(f['norm']), np.float32(f['rate'])], f['group_norms']]).astype(np.float32))
        assert got['steps'] == i + 1
        for j in range(max(0, i - 2), i + 1):                    # the last three launches are all still there
            _same_bits(got['ring'][j % 3], want[j], 'row of launch %d after launch %d' % (j, i))
    # a group table whose bounds reach outside its members: clipped, nothing else is read
    bad = gpu.to_device(np.array([-7, 1, 2], np.int32))
    ps.goff = bad
    got = ps.run(gpu.to_device(g), threshold=1.0)
    sp = R.param_sumsq(g, sizes)
    _same_bits(got['gn'], np.array([np.sqrt(sp[0]), np.sqrt(sp[1])], np.float32))       # members [0:1] and [1:2]
    wild = gpu.to_device(np.array([0, 1 << 30, 2], np.int32))
    ps.goff = wild
    got = ps.run(gpu.to_device(g), threshold=1.0)
    _same_bits(got['gn'], np.array([np.sqrt(R.total(sp[[0, 1]])), 0.0], np.float32))


def test_sumsq_rejects_bad_arguments(gpu):
    from vqvae_amd import _lib
    g = gpu.to_device(_random_arena(64, 1))
    ps = _Pass(gpu, [64])
    lib = _lib.load()
    st = gpu.stream()
    args = lambda **kw: [kw.get('g', g.ptr), kw.get('n', 64), ps.items.ptr, kw.get('n_items', 1), ps.params.ptr, 1, None,
                         None, kw.get('n_groups', 0), kw.get('n_slots', 3), 1.0, 0, ps.state.ptr, ps.ws.ptr,
                         kw.get('ws_bytes', 8), st]
    assert lib.vqvae_optim_sumsq(*args()) == 0
    assert lib.vqvae_optim_sumsq(*args(g=g.ptr + 4)) != 0            # misaligned arena
    assert lib.vqvae_optim_sumsq(*args(n=0)) != 0
    assert lib.vqvae_optim_sumsq(*args(ws_bytes=4)) != 0
    assert lib.vqvae_optim_sumsq(*args(n_groups=1)) != 0             # groups without their tables
    assert lib.vqvae_optim_sumsq(*args(n_items=0)) != 0
    assert lib.vqvae_optim_sumsq(*args(n_slots=0)) != 0
    gpu.synchronize()


# ---- hooked Adam == plain Adam on pre-scaled gradients, device against device ------------------------------------------
def _arenas(gpu, n, seed):
    rng = np.random.RandomState(seed)
    host = dict(p=rng.standard_normal(n).astype(np.float32), g=_random_arena(n, seed + 1),
                m=(1e-3 * rng.standard_normal(n)).astype(np.float32), v=(1e-6 * rng.rand(n)).astype(np.float32))
    return host, {k: gpu.to_device(a) for k, a in host.items()}


@pytest.mark.parametrize('recorded_form', [False, True])
def test_hooked_adam_equals_plain_adam_on_prescaled_gradients(gpu, recorded_form):
    from vqvae_amd import _lib
    sizes = AWKWARD + [70001]
    n = sum(sizes)
    host, _ = _arenas(gpu, n, 11)
    ps = _Pass(gpu, sizes)
    n0 = float(ps.run(gpu.to_device(host['g']))['norm'])
    lr, b1, b2, eps = 3.1e-4, 0.9, 0.999, 1e-8
    st = gpu.stream()
    lr_table = gpu.to_device(np.array([9.0, np.float32(lr), 7.0], np.float32))

    def plain(a, scale=None):
        if scale is not None:        # a plain elementwise multiply by float32(rate), then today's kernel
            _lib.call('vqvae_elementwise', _lib.EW_SCALE, n, a['g'].ptr, None, a['g'].ptr, float(scale), 0.0, st)
        _lib.call('vqvae_adam_step', a['p'].ptr, a['g'].ptr, a['m'].ptr, a['v'].ptr, n, lr, b1, b2, eps, st)

    def hooked(a, threshold):
        got = ps.run(a['g'], threshold=threshold)
        if recorded_form:
            step = gpu.to_device(np.array([1], np.int32))
            _lib.call('vqvae_optim_adam_step_hooked', a['p'].ptr, a['g'].ptr, a['m'].ptr, a['v'].ptr, n, 0.0,
                      lr_table.ptr, step.ptr, b1, b2, eps, ps.state.ptr, 0, st)
            assert int(step.get()[0]) == 2
        else:
            _lib.call('vqvae_optim_adam_step_hooked', a['p'].ptr, a['g'].ptr, a['m'].ptr, a['v'].ptr, n, lr, None, None,
                      b1, b2, eps, ps.state.ptr, 0, st)
        return got

    # 0.5 * n0: the step clips, by float32 of the float64 rate
    _, a = _arenas(gpu, n, 11)
    _, b = _arenas(gpu, n, 11)
    got = hooked(a, 0.5 * n0)
    want_scale = np.float32(np.float64(0.5 * n0) / np.float64(n0))
    _same_bits(got['scale'], want_scale, 'scale')
    assert got['scale'] < 1.0
    plain(b, scale=want_scale)
    for k in 'pmvg':
        _same_bits(a[k].get(), b[k].get(), 'clipped step: ' + k)
    assert np.any(a['g'].get() != host['g'])                    # the arena holds the clipped gradients
    # 2 * n0: no clipping, the arena is untouched, the step is the un-hooked one
    _, a = _arenas(gpu, n, 11)
    _, b = _arenas(gpu, n, 11)
    got = hooked(a, 2.0 * n0)
    assert got['scale'] == np.float32(1.0) and got['rate'] == 2.0
    plain(b)
    for k in 'pmv':
        _same_bits(a[k].get(), b[k].get(), 'unclipped step: ' + k)
    _same_bits(a['g'].get(), host['g'], 'unclipped step leaves the gradients alone')


def test_hooked_adam_guard_flag(gpu):
    """With the guard flag and a non-finite state the kernel touches nothing, but the device step counter advances."""
    from vqvae_amd import _lib
    n = 4099
    host, a = _arenas(gpu, n, 17)
    host['g'][77] = np.nan
    a['g'].set(host['g'])
    ps = _Pass(gpu, [n])
    assert ps.run(a['g'], threshold=1.0, flags=1)['nonfinite'] == 1
    lr_table = gpu.to_device(np.array([1e-3, 1e-3], np.float32))
    step = gpu.to_device(np.array([0], np.int32))
    _lib.call('vqvae_optim_adam_step_hooked', a['p'].ptr, a['g'].ptr, a['m'].ptr, a['v'].ptr, n, 0.0, lr_table.ptr,
              step.ptr, 0.9, 0.999, 1e-8, ps.state.ptr, 1, gpu.stream())
    for k in 'pmvg':
        _same_bits(a[k].get(), host[k], 'guarded step: ' + k)
    assert int(step.get()[0]) == 1
    _lib.call('vqvae_optim_adam_step_hooked', a['p'].ptr, a['g'].ptr, a['m'].ptr, a['v'].ptr, n, 1e-3, None, None,
              0.9, 0.999, 1e-8, ps.state.ptr, 0, gpu.stream())
    assert np.isnan(a['p'].get()[77]) and np.isfinite(a['p'].get()[:77]).all()      # without the flag: as Chainer


# ---- through the optimizer ------------------------------------------------------------------------------------------
def _batches(n, B=3):
    out = []
    for s in range(n):
        x_enc, x_dec, spk, t = O.synth_batch(B, length=LENGTH, n_speaker=CFG['n_speaker'], seed=900 + s)
        out.append([(x_enc[i][..., None], x_dec[i][..., None], spk[i], t[i][..., None]) for i in range(B)])
    return out


class _It(object):
    def __init__(self, data):
        self.data, self.i = data, 0

    def next(self):
        self.i += 1
        return self.data[(self.i - 1) % len(self.data)]


def _trainer(data, hooks=(), graph=False, parallel=False, seed=4):
    import vqvae_amd as V
    from vqvae_amd.optimizers import Adam
    _, model = H.build_model(CFG, seed=seed)
    model.to_gpu()
    opt = Adam(2e-4)
    opt.setup(model)
    for h in hooks:
        opt.add_hook(h)
    cls = V.VQVAE_ParallelUpdater if parallel else V.VQVAE_StandardUpdater
    return model, opt, cls(_It(data), opt, device=0, graph=graph)


def _arena_state(opt):
    return dict(p=opt.params.get(), m=opt.m.get(), v=opt.v.get())


def _reported():
    from vqvae_amd import core
    from vqvae_amd.reporting import _scalar
    obs = core.get_current_reporter().observation
    return {k: _scalar(v) for k, v in obs.items() if 'grad_norm' in k or 'clip_rate' in k}


def test_whole_step_with_clipping_matches_oracle_config0(gpu):
    """One VQVAE_StandardUpdater step at configs[0] with GradientClipping(0.5 * n0) against the oracle's gradients scaled
    in NumPy as Chainer scales them [chainer-recalled], then the oracle's Adam; test_gpu_configs.py's bars."""
    import vqvae_amd as V
    from test_gpu_model import _Iter
    from test_gpu_configs import _limit_blas
    T = 7680
    batch = O.synth_batch(1, length=T, n_speaker=CFG0['n_speaker'], seed=71)
    # n0: the norm of this very step, measured on a twin
    _, twin, topt, _, arrays = _model_step_parts(CFG0, T, 1, 0, 71, ema_decay=0.9999)
    topt.add_hook(V.GradientNorms())
    _backward(twin, arrays)
    topt.update()
    n0 = topt.grad_norms()['grad_norm']
    assert np.isfinite(n0) and n0 > 0
    threshold = 0.5 * n0
    del twin, topt

    P, model = H.build_model(CFG0, seed=0, ema_decay=0.9999)
    P_ema = copy.deepcopy(P['decoder'])
    model.to_gpu()
    opt = V.optimizers.Adam(2e-4)
    opt.setup(model)
    opt.add_hook(V.GradientClipping(threshold))
    opt.add_hook(V.GradientNorms())
    upd = V.VQVAE_StandardUpdater(_Iter([batch]), opt, device=0)
    sites = H.device_relu_sites(model, batch[0], batch[1], batch[2])
    upd.update()
    got = opt.grad_norms()
    reported = _reported()

    with _limit_blas():
        losses, cache = O.vae_forward(P, batch[0], batch[1], batch[2], batch[3], CFG0['n_loop'], CFG0['n_layer'], 0.25)
        for (_, a), (_, b) in zip(O.flatten_params(P_ema), O.flatten_params(P['decoder'])):
            O.ema_update(a, b, 0.9999)
        H.align_relu_kinks(cache, sites)
        G = O.vae_backward(P, cache, batch[2], batch[3], CFG0['n_loop'], CFG0['n_layer'], 0.25)
    flatP, flatG = dict(O.flatten_params(P)), dict(O.flatten_params(G))
    # chainer.optimizer.GradientClipping.__call__ [chainer-recalled]: norm = sqrt(sum over params of sum(g*g));
    # rate = threshold / norm; if rate < 1: grad *= rate  (a float32 array times a scalar: a float32 product)
    sqnorm = sum(float(np.sum(g.astype(np.float64) ** 2)) for g in flatG.values())
    rate = float(threshold / np.sqrt(sqnorm))          # (a Python scalar: the float32 loop, as under Chainer-era NumPy)
    assert rate < 1
    for g in flatG.values():
        g *= rate
    state = {}
    for name, p in flatP.items():
        if name in flatG:
            m = state.setdefault('m' + name, np.zeros_like(p))
            v = state.setdefault('v' + name, np.zeros_like(p))
            O.adam_update(p, flatG[name], m, v, 1, 2e-4)
    print('configs[0] clip_rate: device %.9g, oracle %.9g, relative difference %.3e'
          % (got['clip_rate'], rate, abs(got['clip_rate'] - rate) / rate))
    assert abs(got['clip_rate'] - rate) <= 1e-6 * rate
    assert abs(reported['main/clip_rate'] - rate) <= 1e-6 * rate
    for i, (a, b) in enumerate(zip([float(l.data.get()) for l in upd.last_losses], losses)):
        assert_close(a, float(b), 1e-4, 'loss%d' % (i + 1))
    named = dict(model.namedparams())
    for name, arr in O.flatten_params(P):
        dn = H._dev_name(name, True)
        assert_close(named[dn].data.get().reshape(arr.shape), arr, 1e-4, 'configs[0] param ' + dn)
    # after update() the arena holds the clipped gradients, as p.grad does after Chainer's hook
    for name, arr in flatG.items():
        dn = H._dev_name(name, True)
        H.assert_close_scaled(named[dn].grad.get().reshape(arr.shape), arr, 1e-4, 'clipped grad ' + dn)


def _manual_step(model, opt, arrays, plant=None):
    _backward(model, arrays)
    if plant is not None:            # between backward and update, through the arena view
        opt.grads.flat_view(plant[0], 1).set(np.array([plant[1]], np.float32))
    opt.update()


def test_guard_skips_a_nonfinite_step(gpu):
    import vqvae_amd as V
    from vqvae_amd.updaters import concat_examples
    data = _batches(2)
    arrays = [concat_examples(b, 0) for b in data]
    model, opt, _ = _trainer(data, hooks=[V.NonFiniteGuard()])
    ref_model, ref_opt, _ = _trainer(data, hooks=[V.NonFiniteGuard()])
    _manual_step(model, opt, arrays[0])
    _manual_step(ref_model, ref_opt, arrays[0])
    before = _arena_state(opt)
    where = opt.n_train // 3
    _manual_step(model, opt, arrays[1], plant=(where, np.nan))
    after = _arena_state(opt)
    for k in 'pmv':
        _same_bits(after[k], before[k], 'skipped step: ' + k)
    assert opt.skipped_steps() == 1 and opt.t == 2
    st = opt.hook_state()
    assert st['nonfinite'] == 1 and np.isnan(opt.grads.get()[where])      # the gradients were not touched either
    # the next clean step updates as if the skipped one had only advanced t
    ref_opt.t += 1
    _manual_step(model, opt, arrays[0])
    _manual_step(ref_model, ref_opt, arrays[0])
    a, b = _arena_state(opt), _arena_state(ref_opt)
    for k in 'pmv':
        _same_bits(a[k], b[k], 'step after the skipped one: ' + k)
    assert opt.skipped_steps() == 1 and ref_opt.skipped_steps() == 0 and opt.t == ref_opt.t == 3
    assert np.any(a['p'] != before['p'])


def test_without_the_guard_a_nan_gradient_poisons_the_parameters(gpu):
    """Pins the "as Chainer" behaviour: clipping does not mask a non-finite gradient."""
    import vqvae_amd as V
    from vqvae_amd.updaters import concat_examples
    data = _batches(1)
    arrays = concat_examples(data[0], 0)
    model, opt, _ = _trainer(data, hooks=[V.GradientClipping(1e-3)])
    where = opt.n_train // 3
    _manual_step(model, opt, arrays, plant=(where, np.nan))
    p = opt.params.get()
    assert np.isnan(p[where]) and np.isfinite(np.delete(p[:opt.n_train], where)).all()    # a NaN rate clips nothing
    assert opt.hook_state()['scale'] == np.float32(1.0) and opt.skipped_steps() == 0
    model, opt, _ = _trainer(data, hooks=[V.GradientClipping(1e-3)])
    _manual_step(model, opt, arrays, plant=(where, np.inf))
    p = opt.params.get()
    assert np.isnan(p[where])                                   # rate 0: 0 * inf = NaN
    assert opt.hook_state()['scale'] == np.float32(0.0)


def _run_steps(upd, opt, n, collect):
    for _ in range(n):
        upd.update()
        collect.append((np.array([l.data.get() for l in upd.last_losses]), _reported(), opt.grad_norms()))


def test_recorded_steps_match_eager_steps_with_all_hooks(gpu):
    """6 steps with graph=True (2 warm-up, the capture, replays) against 6 eager steps from the same state, all three hooks
    attached, the threshold between the smallest and the largest of the six norms; then another threshold."""
    import vqvae_amd as V
    data = _batches(4)
    # the six norms, measured
    _, popt, pupd = _trainer(data, hooks=[V.GradientNorms()])
    probe = []
    _run_steps(pupd, popt, 6, probe)
    norms = [r[2]['grad_norm'] for r in probe]
    threshold = 0.5 * (min(norms) + max(norms))
    assert min(norms) < threshold < max(norms)
    runs = {}
    for graph in (False, True):
        clip = V.GradientClipping(threshold)
        model, opt, upd = _trainer(data, hooks=[clip, V.NonFiniteGuard(), V.GradientNorms()], graph=graph)
        log = []
        _run_steps(upd, opt, 6, log)
        first = upd._graphed
        assert (first is not None) == graph
        mid = _arena_state(opt)
        clip.threshold = 0.75 * min(norms)                 # re-parameterised: every step clips now
        _run_steps(upd, opt, 3, log)
        if graph:
            assert upd._graphed is not None and upd._graphed is not first        # recorded again, not a stale replay
        runs[graph] = (log, mid, _arena_state(opt), opt.skipped_steps(), opt.t)
    rates = [r[2]['clip_rate'] for r in runs[False][0][:6]]
    assert any(r < 1 for r in rates) and any(r >= 1 for r in rates), rates        # both kinds of step occur
    assert all(r[2]['clip_rate'] < 1 for r in runs[False][0][6:])
    for i, (e, g) in enumerate(zip(runs[False][0], runs[True][0])):
        _same_bits(e[0], g[0], 'losses of step %d' % i)
        assert e[1] == g[1] and set(e[1]) == {'main/grad_norm', 'main/clip_rate', 'main/grad_norm/encoder',
                                              'main/grad_norm/vq', 'main/grad_norm/decoder',
                                              'main/grad_norm/condition_embed'}, (i, e[1], g[1])
        assert e[2] == g[2], (i, e[2], g[2])
        assert e[1]['main/grad_norm'] == float(np.float32(e[2]['grad_norm']))
    for which in (1, 2):
        for k in 'pmv':
            _same_bits(runs[False][which][k], runs[True][which][k], 'arena %s after %s' % (k, ('', '6 steps', '9 steps')[which]))
    assert runs[False][3:] == runs[True][3:] == (0, 9)


@pytest.mark.parametrize('graph', [False, True])
def test_logreport_averages_the_steps_of_an_interval(gpu, graph):
    """LogReport(trigger=3) over 6 steps whose norms differ: each entry's grad_norm / group norms / clip_rate is the mean
    of the three steps' own values (read per step on demand), not the last step's repeated."""
    import vqvae_amd as V
    data = _batches(4)
    _, popt, pupd = _trainer(data, hooks=[V.GradientNorms()])
    probe = []
    _run_steps(pupd, popt, 6, probe)
    norms = [r[2]['grad_norm'] for r in probe]
    threshold = 0.5 * (min(norms) + max(norms))
    model, opt, upd = _trainer(data, hooks=[V.GradientClipping(threshold), V.GradientNorms(slots=4)], graph=graph)
    log = V.LogReport(trigger=3)
    per_step, entries = [], []
    for _ in range(6):
        upd.update()
        st = opt.hook_state()
        row = {'main/grad_norm': st['norm_f32'], 'main/clip_rate': st['rate_f32']}
        for g, v in zip(opt._hook_dev['groups'], st['group_norms']):
            row['main/grad_norm/' + g] = v
        per_step.append(row)
        e = log(upd)
        if e is not None:
            entries.append(e)
    assert (upd._graphed is not None) == graph and len(entries) == 2
    assert len({float(r['main/grad_norm']) for r in per_step}) == 6          # the norms do differ
    rates = [float(r['main/clip_rate']) for r in per_step]
    assert any(r < 1 for r in rates) and any(r >= 1 for r in rates)
    for i, e in enumerate(entries):
        for key in per_step[0]:
            want = float(np.mean([float(r[key]) for r in per_step[3 * i:3 * i + 3]]))
            assert e[key] == want, (graph, i, key, e[key], want)
            assert e[key] != float(per_step[3 * i + 2][key])                 # and not the interval's last step
        assert 'main/loss1' in e


def test_a_second_setup_drops_the_previous_hook_state(gpu):
    import vqvae_amd as V
    from vqvae_amd.updaters import concat_examples
    data = _batches(1)
    model, opt, _ = _trainer(data, hooks=[V.NonFiniteGuard()])
    _manual_step(model, opt, concat_examples(data[0], 0), plant=(3, np.nan))
    assert opt.skipped_steps() == 1
    opt.setup(model)
    assert opt.skipped_steps() == 0 and opt._hook_dev is None and not opt._hooks
    with pytest.raises(RuntimeError):
        opt.hook_state()


def test_group_norms(gpu):
    import vqvae_amd as V
    from vqvae_amd.updaters import concat_examples
    data = _batches(1)
    model, opt, _ = _trainer(data, hooks=[V.GradientNorms()])
    _backward(model, concat_examples(data[0], 0))
    g = opt.grads.get()
    opt.update()
    sizes = _train_sizes(opt)
    sp = R.param_sumsq(g, sizes)
    names = [n for n, off, size in opt.layout() if off + size <= opt.n_train]
    got = opt.grad_norms()
    assert set(got) == {'grad_norm', 'grad_norm/encoder', 'grad_norm/vq', 'grad_norm/decoder', 'grad_norm/condition_embed'}
    _same_bits(np.float64(got['grad_norm']), np.sqrt(R.total(sp)))
    sq = 0.0
    for group in ('encoder', 'vq', 'decoder', 'condition_embed'):
        members = [i for i, n in enumerate(names) if n.startswith('/%s/' % group)]
        assert members
        want = np.float32(np.sqrt(R.total(sp[members])))
        _same_bits(np.float32(got['grad_norm/' + group]), want, group)
        sq += float(got['grad_norm/' + group]) ** 2
    assert abs(sq - got['grad_norm'] ** 2) <= 4 * 2.0 ** -24 * got['grad_norm'] ** 2
    # a dict overrides the default
    opt.remove_hook('GradientNorms')
    opt.add_hook(V.GradientNorms({'enc': model.encoder, 'everything': model}))
    _backward(model, concat_examples(data[0], 0))
    opt.update()
    got = opt.grad_norms()
    assert set(got) == {'grad_norm', 'grad_norm/enc', 'grad_norm/everything'}
    assert got['grad_norm/everything'] == float(np.float32(got['grad_norm']))


def test_no_hook_identity(gpu):
    """An optimizer that had a hook added and removed again launches the plain kernel and matches a never-hooked run."""
    import vqvae_amd as V
    from vqvae_amd import _lib
    data = _batches(2)
    out = {}
    for touched in (False, True):
        model, opt, upd = _trainer(data)
        if touched:
            opt.add_hook(V.GradientClipping(1e-6))
            opt.add_hook(V.GradientNorms())
            opt.remove_hook('GradientClipping')
            opt.remove_hook('GradientNorms')
            assert opt.capture_key() == (0.9, 0.999, 1e-8) and opt._hook_dev is None
        calls = []
        real = _lib.call
        _lib.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
        try:
            for _ in range(3):
                upd.update()
        finally:
            _lib.call = real
        assert calls.count('vqvae_adam_step') == 3 and not [c for c in calls if c.startswith('vqvae_optim_')]
        out[touched] = _arena_state(opt)
    for k in 'pmv':
        _same_bits(out[False][k], out[True][k], k)


def test_parallel_updater_single_communicator_equals_standard_updater(gpu):
    import vqvae_amd as V
    data = _batches(3)
    # a threshold that clips some of the steps: from the norms of an un-clipped run
    _, popt, pupd = _trainer(data, hooks=[V.GradientNorms()])
    probe = []
    _run_steps(pupd, popt, 4, probe)
    norms = [r[2]['grad_norm'] for r in probe]
    threshold = 0.5 * (min(norms) + max(norms))
    out = {}
    for parallel in (False, True):
        hooks = [V.GradientClipping(threshold), V.NonFiniteGuard(), V.GradientNorms()]
        model, opt, upd = _trainer(data, hooks=hooks, parallel=parallel)
        log = []
        _run_steps(upd, opt, 4, log)
        out[parallel] = (log, _arena_state(opt))
    for e, g in zip(out[False][0], out[True][0]):
        _same_bits(e[0], g[0], 'losses')
        assert e[1] == g[1] and e[2] == g[2]
    for k in 'pmv':
        _same_bits(out[False][1][k], out[True][1][k], k)


def _run_workers(cmds, env, timeout=600):
    procs = [subprocess.Popen(c, env=env) for c in cmds]
    try:
        for p in procs:
            assert p.wait(timeout=timeout) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()


def test_two_process_parallel_updater_with_hooks(gpu, tmp_path):
    """Two real processes on one GPU, each a VQVAE_ParallelUpdater with the three hooks on its strided shard: bit-identical
    parameters, the same clip_rate on both ranks, and that rate is the one process's that sums the two shards' gradients."""
    d = str(tmp_path)
    worker = os.path.join(HERE, 'dp_hooks_worker.py')
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    _run_workers([[sys.executable, worker, 'single', '2', d, 'inf', 'probe']], env)
    norms = np.load(os.path.join(d, 'norms_probe.npy'))
    assert np.isfinite(norms).all() and (norms > 0).all()
    threshold = repr(float(0.5 * norms.min()))                       # every step clips
    _run_workers([[sys.executable, worker, 'rank', str(r), '2', d, threshold] for r in range(2)], env)
    _run_workers([[sys.executable, worker, 'single', '2', d, threshold, 'single']], env)
    a = np.load(os.path.join(d, 'params_rank0.npy'))
    b = np.load(os.path.join(d, 'params_rank1.npy'))
    s = np.load(os.path.join(d, 'params_single.npy'))
    assert a.size > 100000 and np.isfinite(a).all()
    _same_bits(a, b, 'replicas')
    _same_bits(a, s, 'two ranks against one process summing the shards')
    ra = np.load(os.path.join(d, 'rates_rank0.npy'))
    rb = np.load(os.path.join(d, 'rates_rank1.npy'))
    rs = np.load(os.path.join(d, 'rates_single.npy'))
    assert (ra < 1).all() and len(ra) == 3
    _same_bits(ra, rb, 'clip_rate of the two ranks')
    _same_bits(ra, rs, 'clip_rate against the summed shards')
    assert np.any(np.load(os.path.join(d, 'losses_rank0.npy')) != np.load(os.path.join(d, 'losses_rank1.npy')))
