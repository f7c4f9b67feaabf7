"""GPU checks of lockstep generation with refill (csrc/generate_slots.hip, WaveNet.generate_lockstep(refill=True),
synthesize_many): a sequence may start at any tick in any slot and gets, bit for bit, what lockstep generation without
refill gives it; the device scheduler places every sequence where generation.plan_refill says; writes stay inside the
outputs and the state."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
from helpers import _bits
import vqvae_oracle as O
from helpers import assert_close
from test_gpu_generate import _cond, _decoder, _random_biases
from zoned import In, Out, run_contract

pytestmark = pytest.mark.gpu

LENGTHS11 = np.array([40, 7, 23, 1, 40, 12, 2, 31, 23, 9, 18])


def _both(gpu, dec, cond, u, **kw):
    """(out, logits) without and with refill, same arguments."""
    c = gpu.to_device(cond)
    a = dec.generate_lockstep(c, u, return_logits=True, **kw)
    b = dec.generate_lockstep(c, u, return_logits=True, refill=True, **kw)
    return a, b


def _assert_same(a, b, what=''):
    assert a[0].shape == b[0].shape and a[0].dtype == b[0].dtype and a[1].shape == b[1].shape, what
    np.testing.assert_array_equal(_bits(b[0]), _bits(a[0]), what + ' out')
    np.testing.assert_array_equal(_bits(b[1]), _bits(a[1]), what + ' logits')


def test_refill_equals_no_refill_and_the_oracle(gpu):
    """11 sequences in 5 slots.  One has length 1 and is never queued; five start at tick 0 and five are refills, at
    ticks 22 22 30 33 38, none a multiple of the largest dilation 4 (a stale ring entry under tick % dilation would be
    read if the age predicate were wrong); one tenant (1 step) ends before any ring of its slot wraps; the queue drains
    and the slots go idle one by one."""
    from vqvae_amd.generation import plan_refill
    cfg = dict(H.SMALL)
    p, dec = _decoder(cfg, 127)
    N, T = 11, 40
    cond = _cond(cfg, N, T, 47)
    u = np.random.RandomState(48).random_sample((T, N))
    ticks, where = plan_refill(LENGTHS11 - 1, 5)
    assert sorted(where[where[:, 1] > 0, 1]) == [22, 22, 30, 33, 38] and where[3, 0] == -1 and ticks == 39
    a, b = _both(gpu, dec, cond, u, lengths=LENGTHS11, group=5)
    _assert_same(a, b)
    got, logits = b
    assert got.shape == (N, T) and got.dtype == np.int32 and logits.shape == (39, N, cfg['out_dim'])
    for i, L in enumerate(LENGTHS11):
        assert (got[i, L - 1:] == 0).all() and (logits[L - 1:, i] == 0).all(), i
        if L > 1:
            want, _ = O.wavenet_generate(p, cond[i:i + 1, :, :L], u[:L, i:i + 1], cfg['n_loop'], cfg['n_layer'])
            np.testing.assert_array_equal(got[i, :L], want[0], 'sequence %d of length %d' % (i, L))
    assert len(np.unique(got)) > 10


def test_idle_slots_from_the_first_tick(gpu):
    """3 sequences in 5 slots equal the same three inside a batch of 7 without refill."""
    cfg = dict(H.SMALL)
    p, dec = _decoder(cfg, 128)
    n, T = 7, 19
    cond = _cond(cfg, n, T, 49)
    u = np.random.RandomState(50).random_sample((T, n))
    want, want_l = dec.generate_lockstep(gpu.to_device(cond), u, return_logits=True)
    pick = np.array([5, 0, 3])
    got, got_l = dec.generate_lockstep(gpu.to_device(np.ascontiguousarray(cond[pick])), np.ascontiguousarray(u[:, pick]),
                                       return_logits=True, refill=True, group=5)
    np.testing.assert_array_equal(got, want[pick])
    np.testing.assert_array_equal(_bits(got_l), _bits(want_l[:, pick]))


def test_partial_column_tile_and_odd_channel_counts(gpu):
    cfg = dict(H.SMALL, residual=72, dilated=88, skip=56, out_dim=250)
    p, dec = _decoder(cfg, 123)
    N, T = 50, 13
    rs = np.random.RandomState(301)
    lengths = rs.randint(1, T + 1, N)
    cond = _cond(cfg, N, T, 302)
    u = rs.random_sample((T, N))
    a, b = _both(gpu, dec, cond, u, lengths=lengths, group=21)
    _assert_same(a, b)
    assert len(np.unique(b[0])) > 10


def test_full_width_trace_and_tick(gpu):
    """300 sequences in 128 slots; the scheduler's trace is plan_refill's placement and the device tick its tick count."""
    from vqvae_amd import _lib
    from vqvae_amd.generation import LockstepRefill, plan_lockstep
    cfg = dict(H.SMALL, residual=72, skip=56)
    p, dec = _decoder(cfg, 126)
    N, T = 300, 24
    rs = np.random.RandomState(303)
    lengths = rs.randint(2, T + 1, N)
    cond = _cond(cfg, N, T, 304)
    u = rs.random_sample((T, N))
    a, b = _both(gpu, dec, cond, u, lengths=lengths, group=128)
    _assert_same(a, b)
    r = LockstepRefill(dec, gpu.to_device(cond), lengths - 1, u.reshape(T, N, 1), None, _lib.GEN_SOFTMAX, 128, True)
    try:
        r.run(8)
        np.testing.assert_array_equal(r.started.get(), r.placement)
        assert int(r.state.step.get()[0]) == r.ticks
        assert int(r.live.get()[0]) == 0 and int(r.next.get()[0]) == N and (r.slot_seq.get() == -1).all()
        np.testing.assert_array_equal(r.out.get(), b[0])
        np.testing.assert_array_equal(_bits(r.logits_out.get()), _bits(b[1]))
    finally:
        r.close()
    _, groups = plan_lockstep(N, T, lengths, group=128)
    assert r.ticks < sum(g for _, g in groups)


def test_graph_steps_and_replay_past_the_end(gpu):
    """Eager launches, 3 and 8 ticks per graph give the same bits; the tick count (41) is no multiple of 3 or 8, so the
    last replay's surplus launches are no-ops, and so is a whole further replay."""
    from vqvae_amd import _lib
    from vqvae_amd.generation import LockstepRefill
    cfg = dict(H.SMALL)
    p, dec = _decoder(cfg, 127)
    N, T = 11, 40
    cond = _cond(cfg, N, T, 47)
    u = np.random.RandomState(48).random_sample((T, N))
    c = gpu.to_device(cond)
    lengths = LENGTHS11.copy()
    lengths[10] = 20                                                   # slot 3 takes it at tick 22: 22 + 19 = 41 ticks
    runs = [dec.generate_lockstep(c, u, lengths=lengths, group=5, return_logits=True, refill=True, graph_steps=g)
            for g in (0, 3, 8)]
    _assert_same(runs[0], runs[1], 'graph_steps 3')
    _assert_same(runs[0], runs[2], 'graph_steps 8')
    r = LockstepRefill(dec, c, lengths - 1, u.reshape(T, N, 1), None, _lib.GEN_SOFTMAX, 5, True)
    try:
        r.run(8)
        assert r.ticks == 41
        names = ('out', 'logits_out', 'slot_seq', 'slot_t', 'next', 'live', 'started')
        before = [getattr(r, k).get() for k in names] + [r.state.step.get(), r.state.x_cur.get(), r.state.x_prev.get()]
        assert int(before[-3][0]) == r.ticks
        r.replay()
        gpu.synchronize()
        after = [getattr(r, k).get() for k in names] + [r.state.step.get(), r.state.x_cur.get(), r.state.x_prev.get()]
        for k, x, y in zip(names + ('tick', 'x_cur', 'x_prev'), before, after):
            np.testing.assert_array_equal(_bits(x), _bits(y), k)
        np.testing.assert_array_equal(before[0], runs[0][0])
        assert not before[-1].any() and not before[-2].any()           # every slot was left with a fresh embed queue
    finally:
        r.close()


def test_teacher_forcing_with_logits(gpu):
    cfg = dict(H.SMALL)
    p, dec = _decoder(cfg, 122)
    N, T = 9, 14
    rs = np.random.RandomState(305)
    lengths = np.array([14, 3, 9, 14, 1, 6, 11, 2, 8])
    cond = _cond(cfg, N, T, 306)
    forced = rs.randint(0, cfg['input_dim'], (T, N)).astype(np.int32)
    forced[3, N - 1] = -1                                              # all-zero input vector
    u = rs.random_sample((T, N))
    out, logits = dec.generate_lockstep(gpu.to_device(cond), u, lengths=lengths, forced=forced, return_logits=True,
                                        group=5, refill=True, graph_steps=5)
    assert logits.shape == (T - 1, N, cfg['out_dim'])
    for i, L in enumerate(lengths):
        assert (logits[L - 1:, i] == 0).all() and (out[i, L - 1:] == 0).all(), i
        if L > 1:
            _, want = O.wavenet_generate(p, cond[i:i + 1, :, :L], u[:L, i:i + 1], cfg['n_loop'], cfg['n_layer'],
                                         forced=forced[:L, i:i + 1])
            assert_close(logits[:L - 1, i], want[:, 0], 1e-4, 'teacher-forced logits of sequence %d' % i)


@pytest.mark.parametrize('input_dim', [1, 256])
def test_mixture_of_logistics(gpu, input_dim):
    cfg = dict(H.MOL, input_dim=input_dim)
    p, dec = _decoder(cfg, 125, use_logistic=True)
    N, T = 9, 150
    lengths = np.array([150, 20, 77, 1, 150, 140, 3, 64, 99])
    cond = _cond(cfg, N, T, 43)
    u = np.random.RandomState(44).uniform(0.02, 0.98, (T, N, 10))
    a, b = _both(gpu, dec, cond, u, lengths=lengths, group=5)
    _assert_same(a, b)
    assert b[0].dtype == np.float32 and np.abs(b[0]).max() <= 1.0 and len(np.unique(b[0])) > 100


def test_sampling_controls_mixed_per_sequence(gpu):
    cfg = dict(H.SMALL)
    p, dec = _decoder(cfg, 129)
    N, T = 12, 30
    lengths = np.array([30, 5, 17, 30, 2, 11, 24, 8, 1, 29, 13, 20])
    cond = _cond(cfg, N, T, 307)
    u = np.random.RandomState(308).random_sample((T, N))
    ctl = dict(temperature=[0.0, 1.0, 1.0, 0.7, 1.0, 0.0, 1.0, 0.7, 1.0, 1.0, 1.3, 1.0],
               top_k=[0, 3, 0, 0, 0, 0, 3, 5, 0, 0, 0, 3],
               top_p=[1.0, 1.0, 0.9, 1.0, 1.0, 1.0, 0.9, 1.0, 1.0, 0.5, 1.0, 1.0])
    a, b = _both(gpu, dec, cond, u, lengths=lengths, group=5, **ctl)
    _assert_same(a, b)
    plain = dec.generate_lockstep(gpu.to_device(cond), u, lengths=lengths, group=5, refill=True)
    assert (plain != b[0]).any()                                       # the controls were read
    np.testing.assert_array_equal(plain[4], b[0][4])                   # ... per sequence: 4 and 8 are neutral


def test_gen_step_slots_abi_contract_37_slots(gpu):
    """vqvae_gen_slots_init + four ticks of vqvae_wavenet_gen_step_slots at 37 slots (two full column tiles + 5) through
    ctypes, 44 sequences of 0..4 steps (refills at ticks 1 and 2, slots going idle from tick 2 on): every state buffer, ring, table
    array, `out` and `logits_out` between NaN red zones.  Zones intact, results bit-identical to the run on
    zero-initialised pool buffers, no NaN, unwritten elements untouched."""
    from vqvae_amd import _lib
    from vqvae_amd.generation import LockstepState, plan_refill, refill_queue
    cfg = dict(H.SMALL, residual=72, skip=56, local_dim=31)
    p, dec = _decoder(cfg, 130)
    S, N, T = 37, 44, 6
    steps = (np.arange(N) % 4 + 1).astype(np.int32)
    steps[5] = 0
    queue = refill_queue(steps)
    ticks, where = plan_refill(steps, S)
    assert ticks == 4
    st = LockstepState(dec, S)
    cond_h = _cond(cfg, N, T, 53)
    u_h = np.random.RandomState(54).random_sample((4, N))
    cond, u = gpu.to_device(cond_h), gpu.to_device(u_h)
    f32, i32 = np.float32, np.int32
    half = st.dilated // 2
    ran = np.arange(T)[None, :] < steps[:, None]
    specs = dict(step=Out(init=np.full(1, 99, i32)), x_cur=Out(init=np.zeros((S, st.input_dim), f32)),
                 x_prev=Out(init=np.zeros((S, st.input_dim), f32)), h0=Out((S, st.residual)), h1=Out((S, st.residual)),
                 z=Out((S, half)), skip_acc=Out((S, st.skip)), s1=Out((S, st.skip)), logits=Out((S, st.out_dim)),
                 out=Out(init=np.zeros((N, T), i32), valid=ran),
                 logits_out=Out(init=np.zeros((4, N, st.out_dim), f32),
                                valid=np.array(np.broadcast_to(ran[:, :4].T[:, :, None], (4, N, st.out_dim)))),
                 steps=In(steps, index_range=(1, 2)), queue=In(queue, index_range=(0, N)),
                 slot_seq=Out((S,), i32), slot_t=Out((S,), i32), next=Out((1,), i32), live=Out((1,), i32),
                 started=Out(init=np.full((N, 2), -1, i32), valid=np.array(np.broadcast_to((steps > 0)[:, None], (N, 2)))))
    for i, ring in enumerate(st.rings):
        specs['ring%d' % i] = Out(init=np.zeros(ring.shape, f32))

    def fn(b):
        d = st.desc
        for name in ('step', 'x_cur', 'x_prev', 'h0', 'h1', 'z', 'skip_acc', 's1', 'logits'):
            setattr(d, name, b[name].ptr)
        for i, blk in enumerate(st._blocks):
            blk.ring = b['ring%d' % i].ptr
        d.sample_mode = _lib.GEN_SOFTMAX
        d.cond, d.cond_bstride, d.cond_cstride, d.cond_follows_step = cond.ptr, st.cond_dim * T, T, 1
        d.uniforms, d.n_uniform, d.forced_next = u.ptr, 1, None
        d.out, d.out_bstride, d.logits_out = b['out'].ptr, T, b['logits_out'].ptr
        d.max_steps = 2 ** 31 - 1
        t = _lib.GenSlots()
        t.n_seq, t.n_queue = N, len(queue)
        for name in ('steps', 'queue', 'next', 'slot_seq', 'slot_t', 'live', 'started'):
            setattr(t, name, b[name].ptr)
        _lib.call('vqvae_gen_slots_init', C.byref(d), C.byref(t), gpu.stream())
        for _ in range(ticks + 1):                                     # the last one finds live == 0
            _lib.call('vqvae_wavenet_gen_step_slots', C.byref(d), C.byref(t), None, gpu.stream())

    r = run_contract(gpu, fn, specs)
    assert int(r['step'][0]) == ticks and int(r['live'][0]) == 0 and int(r['next'][0]) == len(queue)
    np.testing.assert_array_equal(r['started'], where)
    assert (r['slot_seq'] == -1).all()
    for i in range(N):
        k = int(steps[i])
        if k:
            want_out, want_logits = O.wavenet_generate(p, cond_h[i:i + 1, :, :k + 1], u_h[:, i:i + 1], cfg['n_loop'],
                                                       cfg['n_layer'], n_steps=k)
            assert_close(r['logits_out'][:k, i], want_logits[:, 0], 1e-4, 'logits of sequence %d through the C ABI' % i)
            np.testing.assert_array_equal(r['out'][i, :k], want_out[0, :k])


class _Column(object):
    """The stand-in for synthesize's RandomState that hands it one column of uniforms drawn for the whole list."""

    def __init__(self, u):
        self.u = u

    def random_sample(self, shape):
        assert shape == (self.u.shape[0], 1), shape
        return self.u.reshape(shape).copy()


def test_synthesize_many(gpu):
    import vqvae_amd as V
    cfg = dict(H.SMALL)
    P, model = H.build_model(cfg, seed=131, tweak=_random_biases(132))
    model.to_gpu()
    sizes = (128, 64, 192)                                             # the encoder's stride is 64: other lengths are cut to these
    speaker = np.array([2, 5, 2], np.int32)
    waves = [O.synth_batch(1, length=L, n_speaker=cfg['n_speaker'], seed=6 + i)[0] for i, L in enumerate(sizes)]
    got = V.synthesize_many(model.encoder, model.vq, model.decoder, model.condition_embed, [w.reshape(-1) for w in waves],
                            speaker, rng=np.random.RandomState(78), group=5, return_output=True)
    Ts = [len(w) for w, _ in got]
    Tmax = max(Ts)
    assert len(got) == 3 and len(set(Ts)) == 3
    u = np.random.RandomState(78).random_sample((Tmax - 1, 3))
    for i, (wave, out) in enumerate(got):
        x = waves[i]
        z, _ = O.encoder_fwd(P['encoder'], x)
        e4, _ = O.vq_forward(O.expand4(z), P['vq'])
        cond, _ = O.cond_embed_fwd(P['condition_embed'], np.ascontiguousarray(O.squeeze4(e4)), speaker[i:i + 1])
        T = cond.shape[2]
        assert T == Ts[i]
        want_out, _ = O.wavenet_generate(P['decoder'], cond, u[:T - 1, i:i + 1], cfg['n_loop'], cfg['n_layer'])
        np.testing.assert_array_equal(out, want_out[0])
        np.testing.assert_allclose(wave, O.MuLaw(256).itransform(want_out)[0], rtol=0, atol=1e-7)
        alone_wave, alone_out = V.synthesize(model.encoder, model.vq, model.decoder, model.condition_embed, x[..., None],
                                             speaker[i:i + 1], rng=_Column(u[:T - 1, i]), lockstep=True)
        np.testing.assert_array_equal(out, alone_out[0])
        np.testing.assert_array_equal(wave, alone_wave[0])
    sorted_groups = V.synthesize_many(model.encoder, model.vq, model.decoder, model.condition_embed,
                                      [w.reshape(-1) for w in waves], speaker, rng=np.random.RandomState(78), refill=False)
    for (wave, _), other in zip(got, sorted_groups):
        np.testing.assert_array_equal(wave, other)


def test_errors(gpu):
    cfg = dict(H.SMALL)
    p, dec = _decoder(cfg, 131)
    N, T = 6, 12
    cond = gpu.to_device(_cond(cfg, N, T, 55))
    u = np.random.RandomState(56).random_sample((T, N))
    lengths = np.array([12, 3, 7, 5, 12, 2])
    for bad in (dict(group=4), dict(group=129), dict(lengths=lengths[:-1]), dict(lengths=lengths.reshape(2, 3)[:, :2]),
                dict(lengths=np.full(N, T + 1)), dict(uniforms=u[:10]), dict(uniforms=u[:, :5]), dict(n_steps=T + 1, lengths=None)):
        kw = dict(uniforms=u, lengths=lengths, refill=True)
        kw.update(bad)
        with pytest.raises(ValueError):
            dec.generate_lockstep(cond, kw.pop('uniforms'), **kw)
    ok = dec.generate_lockstep(cond, u[:11], lengths=lengths, refill=True)       # the longest sequence runs 11 steps
    np.testing.assert_array_equal(ok, dec.generate_lockstep(cond, u, lengths=lengths))
