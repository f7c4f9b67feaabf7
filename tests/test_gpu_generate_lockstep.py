"""GPU parity of lockstep generation (csrc/generate_lockstep.hip): 5..128 sequences per step with the batch in MFMA
columns, through vqvae_wavenet_gen_step / WaveNet.generate_lockstep, against the NumPy oracle, the per-step
matrix-vector kernels, the training forward, and against itself (a sequence's values do not depend on the batch)."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import vqvae_oracle as O
from helpers import assert_close, assert_close_scaled
from test_gpu_generate import _cond, _decoder, _random_biases
from zoned import Out, run_contract

pytestmark = pytest.mark.gpu


def _forced_case(cfg, n, T, seed):
    rs = np.random.RandomState(seed)
    forced = rs.randint(0, cfg['input_dim'], (T, n)).astype(np.int32)
    forced[min(3, T - 1), n - 1] = -1                                  # all-zero input vector
    return _cond(cfg, n, T, seed + 1), forced, rs.random_sample((T, n))


@pytest.mark.parametrize('n', [5, 16, 33, 128])
def test_teacher_forced_logits_small(gpu, n):
    """Every step's logits against the oracle; T > 2 x the largest dilation (4): every ring wraps."""
    cfg = dict(H.SMALL)
    p, dec = _decoder(cfg, 122)
    T = 14
    cond, forced, u = _forced_case(cfg, n, T, 200 + n)
    want_out, want_logits = O.wavenet_generate(p, cond, u, cfg['n_loop'], cfg['n_layer'], forced=forced)
    out, logits = dec.generate_lockstep(gpu.to_device(cond), u, forced=forced, return_logits=True, graph_steps=5)
    assert logits.shape == (T - 1, n, cfg['out_dim']) and out.shape == (n, T) and out.dtype == np.int32
    assert_close(logits, want_logits, 1e-4, 'teacher-forced logits n=%d' % n)
    assert (out[:, -1] == 0).all()
    for i in range(T - 1):
        for b in range(n):
            cdf = O.softmax_axis1(want_logits[i, b:b + 1])[0].astype(np.float64).cumsum()
            cdf /= cdf[-1]
            if np.abs(cdf - u[i, b]).min() > 1e-5:
                assert out[b, i] == want_out[b, i], (i, b)


@pytest.mark.parametrize('shape', [dict(residual=320, skip=288), dict(residual=72, dilated=88, skip=56, out_dim=250),
                                   dict(local_dim=31), dict(local_dim=30, global_dim=31, residual=40)])
def test_teacher_forced_logits_partial_tiles(gpu, shape):
    """Channel counts that are not multiples of the 16-row tile / the 16-wide K chunk / 4 (scalar operand loads),
    a condition width that is not a multiple of 4; n = 21 leaves a partial column tile."""
    cfg = dict(H.SMALL, **shape)
    p, dec = _decoder(cfg, 123)
    n, T = 21, 13
    cond, forced, u = _forced_case(cfg, n, T, 300 + cfg['residual'])
    _, want_logits = O.wavenet_generate(p, cond, u, cfg['n_loop'], cfg['n_layer'], forced=forced)
    _, logits = dec.generate_lockstep(gpu.to_device(cond), u, forced=forced, return_logits=True)
    assert_close(logits, want_logits, 1e-4, 'logits at %s' % (shape,))


def test_free_running_equals_oracle_and_single_sequences(gpu):
    """The autoregressive loop of generate.py:105-145 for 7 sequences: every sampled bin equals the oracle's and what
    the sequence gets alone on the matrix-vector kernels."""
    cfg = dict(H.SMALL)
    p, dec = _decoder(cfg, 124)
    n, T = 7, 64
    cond = _cond(cfg, n, T, 41)
    u = np.random.RandomState(42).random_sample((T, n))
    want_out, _ = O.wavenet_generate(p, cond, u, cfg['n_loop'], cfg['n_layer'])
    got = dec.generate_lockstep(gpu.to_device(cond), u)
    np.testing.assert_array_equal(got, want_out)
    for i in range(n):
        alone = dec.generate_sequence(gpu.to_device(cond[i:i + 1]), u[:, i:i + 1], persistent=False).get()
        np.testing.assert_array_equal(got[i:i + 1], alone)
    assert len(np.unique(got)) > 10


@pytest.mark.parametrize('input_dim', [1, 256])
def test_mol_generation_matches_oracle(gpu, input_dim):
    """Mixture of logistics (generate.py:113-133): scalar feedback into a 1-channel embed, and the same value fed to
    all input_dim channels (generate.py:127)."""
    cfg = dict(H.MOL, input_dim=input_dim)
    p, dec = _decoder(cfg, 125, use_logistic=True)
    n, T = 6, 150
    cond = _cond(cfg, n, T, 43)
    rs = np.random.RandomState(44)
    u = rs.uniform(0.02, 0.98, (T, n, 10))
    forced = rs.uniform(-1, 1, (T, n)).astype(np.float32)
    want_out, want_logits = O.wavenet_generate(p, cond, u, cfg['n_loop'], cfg['n_layer'], loss_kind='mol', forced=forced)
    out, logits = dec.generate_lockstep(gpu.to_device(cond), u, forced=forced, return_logits=True)
    assert_close(logits, want_logits, 1e-4, 'mol logits')
    assert out.dtype == np.float32
    np.testing.assert_allclose(out, want_out, rtol=0, atol=2e-5)
    want_out, _ = O.wavenet_generate(p, cond, u, cfg['n_loop'], cfg['n_layer'], loss_kind='mol', n_steps=40)
    got = dec.generate_lockstep(gpu.to_device(cond), u, n_steps=40)
    np.testing.assert_allclose(got, want_out, rtol=0, atol=1e-3)
    assert np.abs(got).max() <= 1.0 and np.abs(got[:, :40]).max() > 0 and (got[:, 40:] == 0).all()


def test_sequences_are_independent_and_runs_identical(gpu):
    """Bit for bit: a sequence in a batch of 37 == in a batch of 5 == in a batch of 128 (other neighbours, another
    column, another position of its tile); graph replay == eager launches; two runs; group 16 == group 128."""
    cfg = dict(H.SMALL, residual=72, skip=56)
    p, dec = _decoder(cfg, 126)
    N, T = 128, 24
    cond = _cond(cfg, N, T, 45)
    u = np.random.RandomState(46).random_sample((T, N))

    def run(idx, **kw):
        o, l = dec.generate_lockstep(gpu.to_device(np.ascontiguousarray(cond[idx])), np.ascontiguousarray(u[:, idx]),
                                     return_logits=True, **kw)
        return o, l.view(np.uint32)

    all128 = np.arange(N)
    o128, l128 = run(all128)
    pick37 = np.arange(91, 128)                                        # sequence 91 + j sits in column j
    o37, l37 = run(pick37)
    np.testing.assert_array_equal(o37, o128[pick37])
    np.testing.assert_array_equal(l37, l128[:, pick37])
    pick5 = np.array([120, 3, 91, 64, 17])
    o5, l5 = run(pick5)
    np.testing.assert_array_equal(o5, o128[pick5])
    np.testing.assert_array_equal(l5, l128[:, pick5])
    for kw in (dict(graph_steps=0), dict(), dict(group=16), dict(graph_steps=3, group=50)):
        o, l = run(all128, **kw)
        np.testing.assert_array_equal(o, o128, str(kw))
        np.testing.assert_array_equal(l, l128, str(kw))
    assert len(np.unique(o128)) > 10


def test_lengths_mixed_in_one_call(gpu):
    """Sequences of different lengths: each equals the run of its own truncated condition, its tail is 0, and the
    caller's order survives the sort by length (two groups)."""
    cfg = dict(H.SMALL)
    p, dec = _decoder(cfg, 127)
    N, T = 11, 40
    cond = _cond(cfg, N, T, 47)
    u = np.random.RandomState(48).random_sample((T, N))
    lengths = np.array([40, 7, 23, 1, 40, 12, 2, 31, 23, 9, 18])
    got, logits = dec.generate_lockstep(gpu.to_device(cond), u, lengths=lengths, return_logits=True, group=6)
    assert got.shape == (N, T) and logits.shape == (39, N, cfg['out_dim'])
    for i, L in enumerate(lengths):
        assert (got[i, L - 1:] == 0).all() and (logits[L - 1:, i] == 0).all(), i
        if L > 1:
            want, _ = O.wavenet_generate(p, cond[i:i + 1, :, :L], u[:L, i:i + 1], cfg['n_loop'], cfg['n_layer'])
            np.testing.assert_array_equal(got[i, :L], want[0], 'sequence %d of length %d' % (i, L))
    # n_steps caps every sequence
    capped = dec.generate_lockstep(gpu.to_device(cond), u, lengths=lengths, n_steps=10, group=6)
    for i, L in enumerate(lengths):
        k = min(L - 1, 10)
        np.testing.assert_array_equal(capped[i, :k], got[i, :k])
        assert (capped[i, k:] == 0).all()
    with pytest.raises(ValueError):
        dec.generate_lockstep(gpu.to_device(cond), u, lengths=lengths[:-1])
    with pytest.raises(ValueError):
        dec.generate_lockstep(gpu.to_device(cond), u, lengths=np.full(N, T + 1))


def test_partial_steps_and_fresh_state(gpu):
    from vqvae_amd import _lib
    from vqvae_amd.generation import LockstepState
    cfg = dict(H.SMALL)
    p, dec = _decoder(cfg, 128)
    n, T = 6, 30
    cond = _cond(cfg, n, T, 49)
    u = np.random.RandomState(50).random_sample((T, n))
    full = dec.generate_lockstep(gpu.to_device(cond), u)
    part = dec.generate_lockstep(gpu.to_device(cond), u, n_steps=11)
    np.testing.assert_array_equal(part[:, :11], full[:, :11])
    assert (part[:, 11:] == 0).all()
    st = LockstepState(dec, n)
    first = st.run(gpu.to_device(cond), u, _lib.GEN_SOFTMAX, 11, persistent=False).get()
    np.testing.assert_array_equal(first, part)
    with pytest.raises(RuntimeError):                                  # not fresh any more
        st.run(gpu.to_device(cond), u, _lib.GEN_SOFTMAX, 1, persistent=False)
    with pytest.raises(ValueError):
        LockstepState(dec, 129)
    with pytest.raises(ValueError):
        dec.initialize(5)                                              # initialize keeps the persistent kernel's limit
    with pytest.raises(ValueError):
        dec.generate_lockstep(gpu.to_device(cond), u, n_steps=T + 1)
    with pytest.raises(ValueError):
        dec.generate_lockstep(gpu.to_device(cond), u[:, :5])


def test_reference_default_decoder_equals_training_forward(gpu):
    """params.py unedited: 3 x 10 blocks, 512 / 512 / 256, condition 512 + 128; 64 sequences, 1 100 steps (the rings
    of dilation 512 wrap twice): step i equals column i of the training forward (modules.py:148-160)."""
    from vqvae_amd.core import Variable
    cfg = dict(d=64, k=512, n_loop=3, n_layer=10, filter_size=2, input_dim=256, residual=512,
               dilated=512, skip=256, out_dim=256, local_dim=512, global_dim=128, n_speaker=5)
    p, dec = _decoder(cfg, 129)
    n, T = 64, 1101
    cond = _cond(cfg, n, T, 51)
    rs = np.random.RandomState(52)
    forced = rs.randint(0, 256, (T, n)).astype(np.int32)
    u = rs.random_sample((T, n))
    _, logits = dec.generate_lockstep(gpu.to_device(cond), u, forced=forced, return_logits=True)
    x = np.zeros((n, 256, T), np.float32)
    for i in range(T - 1):
        x[np.arange(n), forced[i], i + 1] = 1
    for b0 in range(0, n, 16):
        y = dec(Variable(gpu.to_device(x[b0:b0 + 16, ..., None])),
                Variable(gpu.to_device(cond[b0:b0 + 16, ..., None]))).data.get()
        y = y.reshape(16, 256, T).transpose(2, 0, 1)[:T - 1]
        assert_close_scaled(logits[:, b0:b0 + 16], y, 1e-4, 'lockstep vs training forward, sequences %d..' % b0)


def _desc_on(st, b, cond, u, T, mode):
    d = st.desc
    for name in ('step', 'x_cur', 'x_prev', 'h0', 'h1', 'z', 'skip_acc', 's1', 'logits'):
        setattr(d, name, b[name].ptr)
    for i, blk in enumerate(st._blocks):
        blk.ring = b['ring%d' % i].ptr
    d.sample_mode = mode
    d.cond, d.cond_bstride, d.cond_cstride, d.cond_follows_step = cond.ptr, st.cond_dim * T, T, 1
    d.uniforms, d.n_uniform = u.ptr, 1
    d.forced_next = None
    d.out, d.out_bstride = b['out'].ptr, T
    d.logits_out = b['logits_out'].ptr
    d.max_steps = 2 ** 31 - 1
    return d


def test_gen_step_abi_contract_n37(gpu):
    """vqvae_wavenet_gen_step at n = 37 (two full column tiles + 5 columns) through ctypes, three steps: every state
    buffer, ring, `out` and `logits_out` sized for exactly n between NaN red zones.  Zones intact (a store for a padded
    column >= n would land in one), results bit-identical to the run on zero-initialised pool buffers, no NaN."""
    from vqvae_amd import _lib
    from vqvae_amd.generation import LockstepState
    cfg = dict(H.SMALL, residual=72, skip=56, local_dim=31)
    p, dec = _decoder(cfg, 130)
    n, T, steps = 37, 8, 3
    st = LockstepState(dec, n)
    cond_h = _cond(cfg, n, T, 53)
    u_h = np.random.RandomState(54).random_sample((T, n))
    cond, u = gpu.to_device(cond_h), gpu.to_device(u_h)
    f32 = np.float32
    half = st.dilated // 2
    specs = dict(step=Out(init=np.zeros(1, np.int32)), x_cur=Out(init=np.zeros((n, st.input_dim), f32)),
                 x_prev=Out(init=np.zeros((n, st.input_dim), f32)), h0=Out((n, st.residual)), h1=Out((n, st.residual)),
                 z=Out((n, half)), skip_acc=Out((n, st.skip)), s1=Out((n, st.skip)), logits=Out((n, st.out_dim)),
                 out=Out(init=np.zeros((n, T), np.int32), valid=np.arange(T)[None, :].repeat(n, 0) < steps),
                 logits_out=Out((steps, n, st.out_dim)))
    for i, ring in enumerate(st.rings):
        specs['ring%d' % i] = Out(init=np.zeros(ring.shape, f32))

    def fn(b):
        d = _desc_on(st, b, cond, u, T, _lib.GEN_SOFTMAX)
        for _ in range(steps):
            _lib.call('vqvae_wavenet_gen_step', C.byref(d), gpu.stream())

    r = run_contract(gpu, fn, specs)
    assert int(r['step'][0]) == steps
    want_out, want_logits = O.wavenet_generate(p, cond_h, u_h, cfg['n_loop'], cfg['n_layer'], n_steps=steps)
    assert_close(r['logits_out'], want_logits, 1e-4, 'logits through the C ABI')
    np.testing.assert_array_equal(r['out'], want_out)
    np.testing.assert_array_equal(r['logits'], r['logits_out'][steps - 1])


def test_gen_step_limits(gpu):
    """n = 129 is refused with the library's error string; the persistent kernel stays at n <= 4."""
    from vqvae_amd import _lib
    from vqvae_amd.generation import LockstepState
    cfg = dict(H.SMALL)
    p, dec = _decoder(cfg, 131)
    st = LockstepState(dec, 128)
    d = st.desc
    cond = gpu.zeros((128, st.cond_dim, 4))
    u = gpu.to_device(np.full((4, 128), 0.5))
    out = gpu.zeros((128, 4), np.int32)
    d.sample_mode = _lib.GEN_SOFTMAX
    d.cond, d.cond_bstride, d.cond_cstride, d.cond_follows_step = cond.ptr, st.cond_dim * 4, 4, 1
    d.uniforms, d.n_uniform, d.out, d.out_bstride, d.max_steps = u.ptr, 1, out.ptr, 4, 4
    lib = _lib.load()
    d.n = 129
    with pytest.raises(_lib.HipError) as e:
        _lib.call('vqvae_wavenet_gen_step', C.byref(d), gpu.stream())
    assert '1..128' in str(e.value) and '129' in str(e.value)
    assert '1..128' in lib.vqvae_last_error_string().decode()
    d.n = 5
    assert lib.vqvae_wavenet_gen_run_workspace_bytes(C.byref(d)) == 0
    assert lib.vqvae_wavenet_gen_run_concurrency(C.byref(d)) == 0
    d.n = 4
    assert lib.vqvae_wavenet_gen_run_workspace_bytes(C.byref(d)) > 0
    assert _lib.GEN_MAX_LOCKSTEP == 128 and _lib.GEN_MAX_N == 4


def test_synthesize_lockstep_matches_oracle_pipeline(gpu):
    """generate.py:94-149 end to end for six waveforms converted to two speakers, against the same pipeline composed
    from the oracle's parts."""
    import vqvae_amd as V
    cfg = dict(H.SMALL)
    P, model = H.build_model(cfg, seed=131, tweak=_random_biases(132))
    model.to_gpu()
    n = 6
    x_enc, _, spk, _ = O.synth_batch(n, length=128, n_speaker=cfg['n_speaker'], seed=6)
    speaker = np.array([2, 5, 2, 5, 5, 2], np.int32)
    z, _ = O.encoder_fwd(P['encoder'], x_enc)
    e4, idx = O.vq_forward(O.expand4(z), P['vq'])
    cond, _ = O.cond_embed_fwd(P['condition_embed'], np.ascontiguousarray(O.squeeze4(e4)), speaker)
    T = cond.shape[2]
    u = np.random.RandomState(78).random_sample((T - 1, n))
    want_out, _ = O.wavenet_generate(P['decoder'], cond, u, cfg['n_loop'], cfg['n_layer'])
    want_wave = O.MuLaw(256).itransform(want_out)
    wave, out = V.synthesize(model.encoder, model.vq, model.decoder, model.condition_embed,
                             x_enc[..., None], speaker,
                             rng=np.random.RandomState(78), lockstep=True)
    assert out.shape == (n, T)
    np.testing.assert_array_equal(out, want_out)
    np.testing.assert_allclose(wave, want_wave, rtol=0, atol=1e-7)
    with pytest.raises(ValueError):                                    # the default road keeps its limit of 4
        V.synthesize(model.encoder, model.vq, model.decoder, model.condition_embed, x_enc[..., None], speaker,
                     rng=np.random.RandomState(78))
