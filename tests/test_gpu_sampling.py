"""Sampling controls on the device (include/vqvae_sampling.h, csrc/sampling.hip): the filtered sampler alone and at the end
of a generation step (per-step kernels, lockstep kernels, synthesize) against the NumPy restatement tests/sampling_ref.py.

Two float32 evaluations of the same rule may differ in the last bits of a probability, so a draw is compared only where
the case is not AMBIGUOUS (sampling_ref.ambiguous): the uniform within 1e-5 of an edge of the restated cdf (the margin
test_generate_sequence_teacher_forced uses), or a rank-order cumulative mass within 1e-5 of top_p.  Every test that skips
such cases asserts that they are at most 5 % of its draws; greedy and top_k == 1 rows are never skipped."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import sampling_ref as R
import vqvae_oracle as O
import zoned as Z
from helpers import assert_close

pytestmark = pytest.mark.gpu

MARGIN = 1e-5
MAX_AMBIGUOUS = 0.05


def _random_biases(seed):
    def tweak(P):
        rs = np.random.RandomState(seed)
        dec = P['decoder']
        for name in ('embed', 'proj1', 'proj2'):
            dec[name] = (dec[name][0], (0.1 * rs.standard_normal(dec[name][1].shape)).astype(np.float32))
        for blk in dec['blocks']:
            for name in blk:
                blk[name] = (blk[name][0], (0.1 * rs.standard_normal(blk[name][1].shape)).astype(np.float32))
    return tweak


@pytest.fixture(scope='module')
def small(gpu):
    """(oracle decoder parameters, device decoder, cfg) of helpers.SMALL, shared by the softmax tests (nothing changes it)."""
    cfg = dict(H.SMALL)
    P, model = H.build_model(cfg, seed=61, tweak=_random_biases(62))
    model.to_gpu()
    return P['decoder'], model.decoder, cfg


def _cond(cfg, n, T, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((n, cfg['local_dim'] + cfg['global_dim'], T)).astype(np.float32)


class _Tally(object):
    """Draws compared and draws left out as ambiguous."""

    def __init__(self):
        self.compared = self.skipped = 0

    def draw(self, got, l, u, T, k, tp, where):
        if R.ambiguous(l, u, T, k, tp, MARGIN):
            self.skipped += 1
            return
        self.compared += 1
        assert got == R.sample(l, u, T, k, tp), (where, got, R.sample(l, u, T, k, tp), (T, k, tp))

    def check(self):
        share = self.skipped / float(max(self.compared + self.skipped, 1))
        print('ambiguous: %d of %d draws (%.2f %%)' % (self.skipped, self.compared + self.skipped, 100 * share))
        assert self.compared > 0 and share <= MAX_AMBIGUOUS, (self.skipped, self.compared)


# ---- 1. the sampler alone -------------------------------------------------------------------------------------------
SEVEN = [(1.0, 0, 1.0), (0.7, 0, 1.0), (1.0, 16, 1.0), (1.0, 0, 0.9), (0.8, 32, 0.95), (0.0, 0, 1.0), (1.0, 1, 1.0)]


def _sample_contract(gpu, logits, u, controls):
    """vqvae_sample_logits on red-zoned buffers (and once on plain ones: tests/zoned.py), softmax mode, all three control
    arrays given.  Returns (classes (n,), probs (n, out_dim))."""
    from vqvae_amd import _lib
    n, n_cls = logits.shape
    T = np.array([c[0] for c in controls], np.float32)
    k = np.array([c[1] for c in controls], np.int32)
    tp = np.array([c[2] for c in controls], np.float32)

    def fn(q):
        s = _lib.GenSampling(q.T.ptr, q.k.ptr, q.tp.ptr)
        _lib.call('vqvae_sample_logits', q.logits.ptr, n, n_cls, _lib.GEN_SOFTMAX, -40.0, q.u.ptr, 1, C.byref(s),
                  q.out.ptr, q.probs.ptr, gpu.stream())

    r = Z.run_contract(gpu, fn, dict(logits=Z.In(logits), u=Z.In(u), T=Z.In(T), k=Z.In(k), tp=Z.In(tp),
                                     out=Z.Out((n,), np.int32), probs=Z.Out((n, n_cls))))
    return r['out'], r['probs']


SUBNORMAL_FLOOR = 4 * 2.0 ** -149


def _check_rows(tally, got, probs, logits, u, controls, where):
    """Membership is read from probs_out > 0 and is exact: no class outside the restated kept set has a positive
    probability, and every kept class has one -- down to the floor of the number format.  expf may be off by one unit in
    the last place, which among subnormals is 2^-149 itself: a kept class whose restated probability is a few units of
    2^-149 (logits of scale 80 put classes there: exp(-103.3) = 0.94 * 2^-149) can be 0 in one evaluation and 2^-149 in
    the other.  Such a class is kept in both, cannot be drawn in either, and is not compared; 4 units leave room for
    the division by the sum as well."""
    for b, (T, k, tp) in enumerate(controls):
        l = logits[b]
        want_p = R.probs(l, T, k, tp)
        _, kept, mass = R.filtered(l, T, k, tp)
        nucleus_edge = mass is not None and np.abs(mass - np.float64(np.float32(tp))).min() <= MARGIN
        exact = T == 0 or k == 1
        assert not (exact and nucleus_edge)
        assert 0 <= got[b] < l.size
        if not nucleus_edge:
            err = np.abs(probs[b].astype(np.float64) - want_p).max()
            assert err <= 1e-6, (where, b, 'probs_out differs by %.3e' % err)
            outside = np.flatnonzero((probs[b] > 0) & ~kept)
            assert outside.size == 0, (where, b, 'classes outside the kept set have a probability', outside[:8])
            missing = np.flatnonzero((probs[b] == 0) & kept & (want_p > SUBNORMAL_FLOOR))
            assert missing.size == 0, (where, b, 'kept classes without a probability', missing[:8], want_p[missing[:8]])
        assert probs[b, got[b]] > 0 or nucleus_edge, (where, b, 'drew a class outside the kept set')
        tally.draw(int(got[b]), l, u[b], T, k, tp, (where, b))


def _alone_cases(n_cls):
    """Seven rows per call; over the seven calls of a scale every row position sees every setting."""
    rs = np.random.RandomState(1000 + n_cls)
    for scale in (0.1, 1.5, 3.0, 80.0):
        for trial in range(7):
            logits = (scale * rs.standard_normal((7, n_cls))).astype(np.float32)
            yield logits, rs.random_sample(7), SEVEN[trial:] + SEVEN[:trial], (n_cls, scale, trial)


@pytest.mark.parametrize('n_cls', [3, 64, 65, 256, 1000, 1024])
def test_sampler_alone_against_the_restatement(gpu, n_cls):
    tally = _Tally()
    for logits, u, controls, where in _alone_cases(n_cls):
        got, probs = _sample_contract(gpu, logits, u, controls)
        _check_rows(tally, got, probs, logits, u, controls, where)
    tally.check()


ADVERSARIAL = [(1.0, 5, 1.0), (0.0, 0, 1.0), (1.0, 4, 1.0), (1.0, 0, 0.5), (0.05, 0, 1.0), (1.0, 8, 0.45), (1.0, 3, 1.0)]


def _adversarial_logits(n_cls):
    rs = np.random.RandomState(2000 + n_cls)
    logits = (1.5 * rs.standard_normal((7, n_cls))).astype(np.float32)
    logits[0] = 0.25                                          # all equal, top_k = 5: classes 0..4
    logits[1] = 0.25                                          # all equal, greedy: class 0
    logits[2] = -3.0
    logits[2, 7::9] = 2.0                                     # the same value at 7, 16, 25, ...: top_k = 4 cuts through the tie
    logits[3] = -4.0
    logits[3, n_cls - 2] = 9.0                                # one dominant class, top_p below its mass
    logits[4] *= 80.0 / 1.5                                   # temperature 0.05 on logits of scale 80: |x| up to ~6000
    logits[5] = 0.25                                          # all equal, top_k = 8, nucleus .45: masses .125 .25 .375 .5
    logits[6, :] = np.float32(-0.0)
    logits[6, 5] = 0.0                                        # -0 ties with +0: rank is by index
    return logits, rs


@pytest.mark.parametrize('n_cls', [65, 256, 1024])
def test_sampler_alone_adversarial_rows(gpu, n_cls):
    logits, rs = _adversarial_logits(n_cls)
    tally = _Tally()
    for call in range(8):
        u = rs.random_sample(7)
        if call < 2:
            u[:] = (0.0, np.nextafter(1.0, 0.0))[call]
        got, probs = _sample_contract(gpu, logits, u, ADVERSARIAL)
        assert list(np.flatnonzero(probs[0])) == [0, 1, 2, 3, 4] and got[1] == 0
        assert list(np.flatnonzero(probs[2])) == [7, 16, 25, 34]
        assert list(np.flatnonzero(probs[3])) == [n_cls - 2] and got[3] == n_cls - 2 and probs[3, n_cls - 2] == 1.0
        assert list(np.flatnonzero(probs[5])) == [0, 1, 2, 3] and list(np.flatnonzero(probs[6])) == [0, 1, 2]
        assert np.isfinite(probs).all()
        if call == 0:                                         # u = 0: every cdf entry in front of the first kept class is 0 <= u
            np.testing.assert_array_equal(got, (probs > 0).argmax(axis=1))
        elif call == 1:                                       # the largest u: still a class with a positive probability
            assert (probs[np.arange(7), got] > 0).all()
        _check_rows(_Tally() if call < 2 else tally, got, probs, logits, u, ADVERSARIAL, ('adversarial', n_cls, call))
    tally.check()


def test_sampler_alone_null_controls_and_mixture(gpu):
    """s == NULL and single NULL members are neutral; the Python wrapper; the mixture of logistics with a temperature."""
    from vqvae_amd import _lib
    from vqvae_amd.generation import sample_logits
    rs = np.random.RandomState(5)
    logits = (1.5 * rs.standard_normal((7, 256))).astype(np.float32)
    u = rs.random_sample(7)
    ld = gpu.to_device(logits)
    plain, p_plain = sample_logits(ld, u, return_probs=True)
    neutral, p_neutral = sample_logits(ld, u, temperature=1.0, return_probs=True)
    np.testing.assert_array_equal(plain.get(), neutral.get())
    np.testing.assert_array_equal(p_plain.get().view(np.uint32), p_neutral.get().view(np.uint32))
    tally = _Tally()
    for b in range(7):
        tally.draw(int(plain.get()[b]), logits[b], u[b], 1.0, 0, 1.0, ('null', b))
    only_k = sample_logits(ld, u, top_k=[1, 1, 1, 1, 1, 1, 1]).get()
    np.testing.assert_array_equal(only_k, logits.argmax(axis=1))
    tally.check()
    out = rs.standard_normal((7, 30)).astype(np.float32)
    um = rs.uniform(0.02, 0.98, (7, 10))
    temps = np.array([0.5, 1.0, 2.0, 0.1, 1.0, 0.9, 1.3], np.float32)
    got = sample_logits(gpu.to_device(out), um, mode=_lib.GEN_MOL, temperature=temps).get()
    np.testing.assert_allclose(got, R.mol_sample(out, um, temps), rtol=0, atol=1e-5)
    plain = sample_logits(gpu.to_device(out), um, mode=_lib.GEN_MOL).get()
    np.testing.assert_array_equal(plain[[1, 4]].view(np.uint32), got[[1, 4]].view(np.uint32))
    np.testing.assert_allclose(plain, O.mol_sample_from_uniform(out, um), rtol=0, atol=1e-5)
    with pytest.raises(ValueError):
        sample_logits(gpu.to_device(out), um, mode=_lib.GEN_MOL, top_k=4)


# ---- 2. neutral controls equal the call without them, bit for bit ------------------------------------------------------
def test_explicit_neutral_controls_equal_today(gpu, small):
    """Both calls on the per-step kernels (persistent=False): with controls the persistent kernel is never used, and it
    sums in another order than the per-step kernels do."""
    p, dec, cfg = small
    n, T = 2, 41
    cond = _cond(cfg, n, T, 6)
    u = np.random.RandomState(10).random_sample((T, n))
    out0, lg0 = dec.generate_sequence(gpu.to_device(cond), u, return_logits=True, persistent=False)
    out1, lg1 = dec.generate_sequence(gpu.to_device(cond), u, return_logits=True, persistent=False,
                                      temperature=1.0, top_k=0, top_p=1.0)
    np.testing.assert_array_equal(out0.get(), out1.get())
    np.testing.assert_array_equal(lg0.get().view(np.uint32), lg1.get().view(np.uint32))
    assert len(np.unique(out0.get())) > 5
    N, T = 6, 24
    cond = _cond(cfg, N, T, 7)
    u = np.random.RandomState(11).random_sample((T, N))
    out0, lg0 = dec.generate_lockstep(gpu.to_device(cond), u, return_logits=True)
    out1, lg1 = dec.generate_lockstep(gpu.to_device(cond), u, return_logits=True, temperature=[1.0] * N, top_k=0, top_p=1.0)
    np.testing.assert_array_equal(out0, out1)
    np.testing.assert_array_equal(lg0.view(np.uint32), lg1.view(np.uint32))


# ---- 3. teacher-forced, per-step path -----------------------------------------------------------------------------------
def test_generate_sequence_teacher_forced_with_controls(gpu, small):
    p, dec, cfg = small
    n, T = 2, 41
    cond = _cond(cfg, n, T, 8)
    rs = np.random.RandomState(12)
    forced = rs.randint(0, cfg['input_dim'], (T, n)).astype(np.int32)
    u = rs.random_sample((T, n))
    controls = [(0.7, 16, 1.0), (1.0, 0, 0.9)]
    kw = dict(forced=forced, return_logits=True, temperature=[c[0] for c in controls], top_k=[c[1] for c in controls],
              top_p=[c[2] for c in controls])
    _, want_logits = O.wavenet_generate(p, cond, u, cfg['n_loop'], cfg['n_layer'], forced=forced)
    out, logits = dec.generate_sequence(gpu.to_device(cond), u, graph_steps=8, persistent=False, **kw)
    got, logits = out.get(), logits.get()
    assert_close(logits, want_logits, 1e-4, 'teacher-forced logits with controls')      # the controls do not touch them
    assert got.shape == (n, T) and got.dtype == np.int32 and (got[:, -1] == 0).all()
    tally = _Tally()
    for i in range(T - 1):
        for b, (Tb, k, tp) in enumerate(controls):
            tally.draw(int(got[b, i]), logits[i, b], u[i, b], Tb, k, tp, (i, b))
    tally.check()
    for other in (dict(graph_steps=0, persistent=False), dict(graph_steps=1, persistent=False),
                  dict(graph_steps=8, persistent=True)):                                 # persistent falls back
        o, lg = dec.generate_sequence(gpu.to_device(cond), u, **dict(kw, **other))
        np.testing.assert_array_equal(o.get(), got, err_msg=str(other))
        np.testing.assert_array_equal(lg.get().view(np.uint32), logits.view(np.uint32), err_msg=str(other))


# ---- 4. lockstep ---------------------------------------------------------------------------------------------------------
def test_generate_lockstep_with_mixed_controls_and_permutation(gpu, small):
    p, dec, cfg = small
    N, T = 9, 24
    cond = _cond(cfg, N, T, 9)
    rs = np.random.RandomState(13)
    forced = rs.randint(0, cfg['input_dim'], (T, N)).astype(np.int32)
    u = rs.random_sample((T, N))
    lengths = np.array([24, 7, 19, 24, 12, 3, 16, 9, 21])
    controls = [(1.0, 0, 1.0), (0.7, 16, 1.0), (1.0, 0, 0.9), (0.8, 32, 0.95), (0.0, 0, 1.0), (1.0, 1, 1.0), (1.3, 5, 0.5),
                (0.5, 0, 0.99), (2.0, 200, 0.8)]
    tk = dict(temperature=np.array([c[0] for c in controls]), top_k=np.array([c[1] for c in controls]),
              top_p=np.array([c[2] for c in controls]))
    got, logits = dec.generate_lockstep(gpu.to_device(cond), u, lengths=lengths, forced=forced, return_logits=True, group=5, **tk)
    tally = _Tally()
    for b, (Tb, k, tp) in enumerate(controls):
        assert (got[b, lengths[b] - 1:] == 0).all()
        for i in range(lengths[b] - 1):
            tally.draw(int(got[b, i]), logits[i, b], u[i, b], Tb, k, tp, (i, b))
    tally.check()
    perm = np.array([4, 8, 0, 6, 2, 7, 1, 3, 5])
    got_p, logits_p = dec.generate_lockstep(gpu.to_device(np.ascontiguousarray(cond[perm])), np.ascontiguousarray(u[:, perm]),
                                            lengths=lengths[perm], forced=np.ascontiguousarray(forced[:, perm]),
                                            return_logits=True, group=5, **dict((k, v[perm]) for k, v in tk.items()))
    np.testing.assert_array_equal(got_p, got[perm])
    np.testing.assert_array_equal(logits_p.view(np.uint32), logits[:, perm].view(np.uint32))


# ---- 5. greedy, free running ---------------------------------------------------------------------------------------------
def test_greedy_free_running_is_the_argmax_and_ignores_the_uniforms(gpu, small):
    p, dec, cfg = small
    T = 48
    cond = _cond(cfg, 1, T, 10)
    u1 = np.random.RandomState(14).random_sample((T, 1))
    u2 = np.random.RandomState(15).random_sample((T, 1))
    g1, lg = dec.generate_sequence(gpu.to_device(cond), u1, return_logits=True, temperature=0.0)
    g1, lg = g1.get(), lg.get()
    np.testing.assert_array_equal(g1[0, :T - 1], lg[:, 0].argmax(axis=1))
    np.testing.assert_array_equal(dec.generate_sequence(gpu.to_device(cond), u2, temperature=0.0).get(), g1)
    np.testing.assert_array_equal(dec.generate_sequence(gpu.to_device(cond), u2, top_k=1).get(), g1)
    N, T = 5, 24
    cond = _cond(cfg, N, T, 11)
    u1 = np.random.RandomState(16).random_sample((T, N))
    u2 = np.random.RandomState(17).random_sample((T, N))
    g1, lg = dec.generate_lockstep(gpu.to_device(cond), u1, return_logits=True, temperature=0.0)
    np.testing.assert_array_equal(g1[:, :T - 1], lg.argmax(axis=2).T)
    np.testing.assert_array_equal(dec.generate_lockstep(gpu.to_device(cond), u2, temperature=0.0), g1)
    np.testing.assert_array_equal(dec.generate_lockstep(gpu.to_device(cond), u2, top_k=1), g1)


# ---- 6. mixture of logistics ---------------------------------------------------------------------------------------------
def test_mol_generation_with_a_temperature(gpu):
    cfg = dict(H.MOL)
    P, model = H.build_model(cfg, seed=63, use_logistic=True, tweak=_random_biases(64))
    model.to_gpu()
    dec = model.decoder
    n, T = 2, 20
    cond = _cond(cfg, n, T, 12)
    rs = np.random.RandomState(18)
    u = rs.uniform(0.02, 0.98, (T, n, 10))
    forced = rs.uniform(-1, 1, (T, n)).astype(np.float32)
    temps = np.array([0.5, 1.0], np.float32)
    out, logits = dec.generate_sequence(gpu.to_device(cond), u, forced=forced, return_logits=True, temperature=temps)
    got, logits = out.get(), logits.get()
    for i in range(T - 1):
        np.testing.assert_allclose(got[:, i], R.mol_sample(logits[i], u[i], temps), rtol=0, atol=1e-5)
    plain = dec.generate_sequence(gpu.to_device(cond), u, forced=forced, persistent=False).get()
    np.testing.assert_array_equal(plain[1].view(np.uint32), got[1].view(np.uint32))
    assert np.abs(plain[0] - got[0]).max() > 1e-3                                         # the temperature did something
    for kw in (dict(top_k=4), dict(top_p=0.9), dict(temperature=0.0)):
        with pytest.raises(ValueError):
            dec.generate_sequence(gpu.to_device(cond), u, **kw)


# ---- 7. synthesize --------------------------------------------------------------------------------------------------------
def test_synthesize_passes_the_controls_through(gpu):
    import vqvae_amd as V
    from vqvae_amd import core
    from vqvae_amd.core import Variable
    cfg = dict(H.SMALL)
    P, model = H.build_model(cfg, seed=65, tweak=_random_biases(66))
    model.to_gpu()
    x_enc, _, spk, _ = O.synth_batch(2, length=128, n_speaker=cfg['n_speaker'], seed=5)
    speaker = ((spk + 1) % cfg['n_speaker']).astype(np.int32)
    with core.using_config('train', False), core.no_backprop_mode():                    # synthesize's own first lines
        e = model.vq(model.encoder(Variable(gpu.to_device(np.ascontiguousarray(x_enc[..., None], np.float32)))))
        cond = model.condition_embed(e, Variable(gpu.to_device(speaker))).data
    T = cond.shape[2]
    u = np.random.RandomState(77).random_sample((T - 1, 2))
    kw = dict(temperature=0.8, top_k=32)
    want = model.decoder.generate_sequence(cond, u, **kw).get()
    wave, out = V.synthesize(model.encoder, model.vq, model.decoder, model.condition_embed, x_enc[..., None], speaker,
                             rng=np.random.RandomState(77), **kw)
    np.testing.assert_array_equal(out, want)
    np.testing.assert_allclose(wave, O.MuLaw(256).itransform(want), rtol=0, atol=1e-7)
    free = V.synthesize(model.encoder, model.vq, model.decoder, model.condition_embed, x_enc[..., None], speaker,
                        rng=np.random.RandomState(77))[1]
    assert (free != out).any()
    want = model.decoder.generate_lockstep(cond, u, **kw)
    _, out = V.synthesize(model.encoder, model.vq, model.decoder, model.condition_embed, x_enc[..., None], speaker,
                          rng=np.random.RandomState(77), lockstep=True, **kw)
    np.testing.assert_array_equal(out, want)
