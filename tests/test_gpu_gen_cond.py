"""GPU checks of lockstep generation from the latent-rate condition (csrc/generate_cond.hip,
generation.LatentCondition, WaveNet.generate_lockstep, synthesize / synthesize_many): the column launch alone writes the
bits of the dense up-sampling's column and nothing else, and every generation path gives, bit for bit, what it gives with
the dense tensor."""
import ctypes as C

import numpy as np
import pytest

import gen_cond_ref as R
import helpers as H
from helpers import _bits
import vqvae_oracle as O
from test_gpu_generate import _decoder, _random_biases
from zoned import In, Out, run_contract

pytestmark = pytest.mark.gpu

TL11 = (3, 1, 2, 3, 1, 2, 2, 1, 3, 1, 2)


def _latent(gpu, cfg, tl, seed, upscale=64):
    """(LatentCondition, host latents, host speaker vectors) of random values."""
    from vqvae_amd.generation import LatentCondition
    rs = np.random.RandomState(seed)
    xs = [rs.standard_normal((cfg['local_dim'], int(t))).astype(np.float32) for t in tl]
    g = rs.standard_normal((len(tl), cfg['global_dim'])).astype(np.float32)
    lc = LatentCondition.from_latents([gpu.to_device(x) for x in xs], gpu.to_device(g), upscale)
    return lc, xs, g


def _assert_same(a, b, what=''):
    assert a[0].shape == b[0].shape and a[0].dtype == b[0].dtype and a[1].shape == b[1].shape, what
    np.testing.assert_array_equal(_bits(b[0]), _bits(a[0]), what + ' out')
    np.testing.assert_array_equal(_bits(b[1]), _bits(a[1]), what + ' logits')


def _latent_and_dense(dec, lc, u, **kw):
    dense = lc.dense()
    kw_dense = dict(kw)
    kw_dense.setdefault('lengths', lc.lengths)
    a = dec.generate_lockstep(dense, u, return_logits=True, **kw_dense)
    b = dec.generate_lockstep(lc, u, return_logits=True, **kw)
    return a, b


# ---- 1. the launch alone ----------------------------------------------------------------------------------------------
def test_column_launch_under_red_zones(gpu):
    """tl = 1 2 3 5 2, Cl = 20, G = 13 (Cc = 33 is odd).  Plain form with a permuting col_seq at the first steps, at both
    sides of a latent frame boundary, at every sequence's last step and at the first one past it; slots form with a
    hand-written table that has an idle slot; both done-conditions.  Rows equal column t of the dense expansion
    (vqvae_upsample_linear_fwd + vqvae_embed_broadcast_fwd) and of the NumPy restatement bit for bit; past T_q the local
    channels are 0 and the speaker channels are still the speaker vector."""
    from vqvae_amd import _lib
    cfg = dict(local_dim=20, global_dim=13)
    tl = np.array([1, 2, 3, 5, 2], np.int32)
    Cl, G, Cc, nseq = 20, 13, 33, 5
    lc, xs, g = _latent(gpu, cfg, tl, 401)
    dense = lc.dense().get()
    assert dense.shape == (5, 33, 320)
    Tq = 64 * tl
    for q in range(nseq):                                               # the existing kernels against the restatement, once
        np.testing.assert_array_equal(_bits(dense[q, :, :Tq[q]]), _bits(R.dense(xs[q], g[q], 64)))
        assert not dense[q, :, Tq[q]:].any()
    local = np.concatenate([x.reshape(-1) for x in xs])
    off = lc.local_off

    def want_row(q, t):
        row = R.column(xs[q], g[q], t, 64)
        if t < Tq[q]:
            np.testing.assert_array_equal(_bits(row), _bits(dense[q, :, t]))
        else:
            assert not row[:Cl].any()
        return row

    def launch(b, n, max_steps, slots):
        c = _lib.GenLatentCond()
        c.local, c.local_off, c.tl, c.global_vec = b['local'].ptr, b['local_off'].ptr, b['tl'].ptr, b['global_vec'].ptr
        c.col_seq = b['col_seq'].ptr if 'col_seq' in b else None
        c.column = b['column'].ptr
        c.n_seq, c.Cl, c.G, c.upscale = nseq, Cl, G, 64
        d = _lib.GenDesc()
        d.n, d.cond_dim, d.step, d.max_steps = n, Cc, b['step'].ptr, max_steps
        t = None
        if slots:
            t = _lib.GenSlots()
            t.n_seq = nseq
            t.slot_seq, t.slot_t, t.live = b['slot_seq'].ptr, b['slot_t'].ptr, b['live'].ptr
        _lib.call('vqvae_gen_cond_column', C.byref(c), C.byref(d), None if t is None else C.byref(t), gpu.stream())

    def inputs():
        return dict(local=In(local), local_off=In(off), tl=In(tl, index_range=(1, 2)), global_vec=In(g))

    col_seq = np.array([3, 0, 4, 2, 1], np.int32)
    steps = sorted(set([0, 1, 63, 64, 127] + [int(T) - 1 for T in Tq] + [int(T) for T in Tq]))
    assert steps == [0, 1, 63, 64, 127, 128, 191, 192, 319, 320]
    for t in steps:
        specs = dict(inputs(), col_seq=In(col_seq, index_range=(0, nseq)), step=In(np.array([t], np.int32)),
                     column=Out((nseq, Cc)))
        r = run_contract(gpu, lambda b: launch(b, nseq, 2 ** 31 - 1, False), specs)
        for c, q in enumerate(col_seq):
            np.testing.assert_array_equal(_bits(r['column'][c]), _bits(want_row(q, t)), 'step %d column %d sequence %d' % (t, c, q))
    # the identity (col_seq NULL), fewer columns than the decoder's lockstep minimum
    specs = dict(inputs(), step=In(np.array([70], np.int32)), column=Out((3, Cc)))
    r = run_contract(gpu, lambda b: launch(b, 3, 71, False), specs)
    for q in range(3):
        np.testing.assert_array_equal(_bits(r['column'][q]), _bits(want_row(q, 70)))
    # slots: rows are addressed by the sequence, slot 1 is idle, sequence 1 is in no slot; the tick is not the step
    slot_seq = np.array([2, -1, 4, 0, 3], np.int32)
    slot_t = np.array([5, 99, 127, 63, 319], np.int32)
    live_rows = np.zeros((nseq, Cc), bool)
    live_rows[[2, 4, 0, 3]] = True
    table = dict(slot_seq=In(slot_seq, index_range=(0, nseq)), slot_t=In(slot_t, index_range=(0, 64)))
    specs = dict(inputs(), step=In(np.array([1000], np.int32)), live=In(np.array([4], np.int32)),
                 column=Out(init=np.full((nseq, Cc), 7.0, np.float32), valid=live_rows), **table)
    r = run_contract(gpu, lambda b: launch(b, nseq, 2 ** 31 - 1, True), specs)
    for s, q in enumerate(slot_seq):
        if q >= 0:
            np.testing.assert_array_equal(_bits(r['column'][q]), _bits(want_row(q, int(slot_t[s]))), 'slot %d' % s)
    assert (r['column'][1] == 7.0).all()
    # done: step >= max_steps (both forms), live == 0 (slots): nothing is written
    nothing = np.zeros((nseq, Cc), bool)
    for slots, step, max_steps, live in ((False, 10, 10, 4), (True, 10, 10, 4), (True, 3, 10, 0), (False, 11, 10, 4)):
        specs = dict(inputs(), col_seq=In(col_seq, index_range=(0, nseq)), step=In(np.array([step], np.int32)),
                     live=In(np.array([live], np.int32)),
                     column=Out(init=np.full((nseq, Cc), 7.0, np.float32), valid=nothing), **table)
        r = run_contract(gpu, lambda b: launch(b, nseq, max_steps, slots), specs)
        assert (r['column'] == 7.0).all(), (slots, step, max_steps, live)


# ---- 2..6. generation: latent equals dense ----------------------------------------------------------------------------
def test_plain_path_equals_dense(gpu):
    cfg = dict(H.SMALL)
    p, dec = _decoder(cfg, 127)
    lc, xs, g = _latent(gpu, cfg, [3] * 7, 402)
    N, Cc, T = lc.shape
    assert (N, T) == (7, 192) and lc.nbytes * 30 < lc.dense_nbytes
    u = np.random.RandomState(403).random_sample((T, N))
    a, b = _latent_and_dense(dec, lc, u)
    _assert_same(a, b)
    assert b[0].shape == (N, T) and b[1].shape == (T - 1, N, cfg['out_dim']) and len(np.unique(b[0])) > 10


@pytest.mark.parametrize('refill', [False, True])
def test_ragged_equals_dense(gpu, refill):
    """Without refill the groups are 0 3 8 2 5 | 6 10 1 4 7 | 9 9 9 9 9: a sorted, non-consecutive col_seq, members that
    run past their own end (their column reads as 0 there) and a group filled up with repeats.  With refill the rows of
    the column array are addressed by the sequence and sequences change slots mid-run."""
    from vqvae_amd.generation import plan_lockstep
    cfg = dict(H.SMALL)
    p, dec = _decoder(cfg, 127)
    lc, xs, g = _latent(gpu, cfg, TL11, 404)
    N, Cc, T = lc.shape
    _, groups = plan_lockstep(N, T, lc.lengths, group=5)
    assert [i.tolist() for i, _ in groups] == [[0, 3, 8, 2, 5], [6, 10, 1, 4, 7], [9, 9, 9, 9, 9]]
    u = np.random.RandomState(405).random_sample((T, N))
    a, b = _latent_and_dense(dec, lc, u, group=5, refill=refill)
    _assert_same(a, b)
    for i, L in enumerate(lc.lengths):
        assert (b[0][i, L - 1:] == 0).all() and (b[1][L - 1:, i] == 0).all() and b[1][:L - 1, i].any(), i
    assert len(np.unique(b[0])) > 10


def test_graph_replay_past_the_end(gpu):
    """191 steps and 317 ticks are no multiples of 8: the last replay's surplus column launches are no-ops like the
    step's own kernels, and so is a whole further replay."""
    from vqvae_amd import _lib
    from vqvae_amd.generation import LockstepRefill, plan_refill
    cfg = dict(H.SMALL)
    p, dec = _decoder(cfg, 127)
    lc, xs, g = _latent(gpu, cfg, TL11, 404)
    N, Cc, T = lc.shape
    u = np.random.RandomState(405).random_sample((T, N))
    assert plan_refill(lc.lengths - 1, 5)[0] == 317
    for refill in (False, True):
        runs = [dec.generate_lockstep(lc, u, group=5, return_logits=True, refill=refill, graph_steps=gs) for gs in (0, 8)]
        _assert_same(runs[0], runs[1], 'refill %s' % refill)
    r = LockstepRefill(dec, lc, (lc.lengths - 1).astype(np.int32), u.reshape(T, N, 1), None, _lib.GEN_SOFTMAX, 5, True)
    try:
        r.run(8)
        assert r.ticks == 317 and int(r.state.step.get()[0]) == 317
        before = [r.out.get(), r.logits_out.get(), r.column.get()]
        r.replay()
        gpu.synchronize()
        for x, y in zip(before, [r.out.get(), r.logits_out.get(), r.column.get()]):
            np.testing.assert_array_equal(_bits(x), _bits(y))
        np.testing.assert_array_equal(before[0], runs[0][0])
    finally:
        r.close()


@pytest.mark.parametrize('refill', [False, True])
def test_odd_channel_counts(gpu, refill):
    cfg = dict(H.SMALL, residual=72, dilated=88, skip=56, out_dim=250, local_dim=20, global_dim=13)
    p, dec = _decoder(cfg, 123)
    tl = np.random.RandomState(5).randint(1, 3, 21)
    assert set(tl) == {1, 2}
    lc, xs, g = _latent(gpu, cfg, tl, 406)
    N, Cc, T = lc.shape
    assert (N, Cc, T) == (21, 33, 128)
    u = np.random.RandomState(407).random_sample((T, N))
    a, b = _latent_and_dense(dec, lc, u, group=21, refill=refill)
    _assert_same(a, b)
    assert len(np.unique(b[0])) > 10


def test_mixture_of_logistics(gpu):
    cfg = dict(H.MOL, input_dim=1)
    p, dec = _decoder(cfg, 125, use_logistic=True)
    lc, xs, g = _latent(gpu, cfg, [2] * 6, 408)
    N, Cc, T = lc.shape
    u = np.random.RandomState(409).uniform(0.02, 0.98, (T, N, 10))
    a, b = _latent_and_dense(dec, lc, u)
    _assert_same(a, b)
    assert b[0].dtype == np.float32 and np.abs(b[0]).max() <= 1.0 and len(np.unique(b[0])) > 100


@pytest.mark.parametrize('refill', [False, True])
def test_sampling_controls_mixed_per_sequence(gpu, refill):
    cfg = dict(H.SMALL)
    p, dec = _decoder(cfg, 129)
    lc, xs, g = _latent(gpu, cfg, (2, 1, 2, 1, 1, 2, 1), 410)
    N, Cc, T = lc.shape
    u = np.random.RandomState(411).random_sample((T, N))
    ctl = dict(temperature=[0.0, 1.0, 1.0, 0.7, 1.0, 1.3, 1.0], top_k=[0, 3, 0, 0, 0, 5, 0],
               top_p=[1.0, 1.0, 0.9, 1.0, 1.0, 0.5, 1.0])
    a, b = _latent_and_dense(dec, lc, u, group=5, refill=refill, **ctl)
    _assert_same(a, b)
    plain = dec.generate_lockstep(lc, u, group=5, refill=refill)
    assert (plain != b[0]).any()                                       # the controls were read
    np.testing.assert_array_equal(plain[4], b[0][4])                   # ... per sequence: 4 is neutral


# ---- 7. synthesis -----------------------------------------------------------------------------------------------------
def test_synthesize_many_and_synthesize(gpu, monkeypatch):
    """Utterances of 2, 1 and 3 latent frames.  The latent calls return the dense calls' waves and outputs bit for bit and
    expand no condition of two or more frames to the sample rate (the condition of a single frame is returned dense, 64
    samples, by ConditionEmbed itself; its column 0 is taken)."""
    import vqvae_amd as V
    from vqvae_amd import _lib
    from vqvae_amd.functions import LazyUpsampled
    cfg = dict(H.SMALL)
    P, model = H.build_model(cfg, seed=131, tweak=_random_biases(132))
    model.to_gpu()
    sizes = (128, 64, 192)
    speaker = np.array([2, 5, 2], np.int32)
    waves = [O.synth_batch(1, length=L, n_speaker=cfg['n_speaker'], seed=6 + i)[0] for i, L in enumerate(sizes)]
    expansions = []
    real_call = _lib.call

    def counting(name, *args):
        if name == 'vqvae_upsample_linear_fwd' and args[4] > args[3] >= 2:        # (x, B, C, Tin, Tout, ...)
            expansions.append((args[3], args[4]))
        return real_call(name, *args)

    monkeypatch.setattr(_lib, 'call', counting)
    materialised = []
    real_materialize = LazyUpsampled.materialize
    monkeypatch.setattr(LazyUpsampled, 'materialize', lambda self: materialised.append(self.shape) or real_materialize(self))
    links = (model.encoder, model.vq, model.decoder, model.condition_embed)

    def many(**kw):
        return V.synthesize_many(*links, [w.reshape(-1) for w in waves], speaker, rng=np.random.RandomState(78), group=5,
                                 return_output=True, **kw)

    for refill in (True, False):
        del expansions[:], materialised[:]
        want = many(refill=refill)
        assert len(expansions) == 2 and len(materialised) == 2          # the instruments see the dense path's expansions
        del expansions[:], materialised[:]
        got = many(refill=refill, latent_condition=True)
        assert not expansions and not materialised
        assert len(got) == 3 and len(set(len(w) for w, _ in got)) == 3
        for (w0, o0), (w1, o1) in zip(want, got):
            assert w1.shape == w0.shape and w1.dtype == w0.dtype and o1.dtype == o0.dtype
            np.testing.assert_array_equal(o1, o0)
            np.testing.assert_array_equal(w1, w0)
    for i, x in enumerate(waves):                                       # one waveform: a group of five repeats of sequence 0
        want = V.synthesize(*links, x[..., None], speaker[i:i + 1], rng=np.random.RandomState(79), lockstep=True)
        del expansions[:], materialised[:]
        got = V.synthesize(*links, x[..., None], speaker[i:i + 1], rng=np.random.RandomState(79), lockstep=True,
                           latent_condition=True)
        assert not expansions and not materialised
        np.testing.assert_array_equal(got[1], want[1])
        assert got[0].shape == want[0].shape and (got[0] == want[0]).all()
    with pytest.raises(ValueError, match='lockstep=True'):
        V.synthesize(*links, waves[0][..., None], speaker[:1], latent_condition=True)


def test_from_condition_of_a_batch_splits_local_and_speaker(gpu):
    """ConditionEmbed's lazy tensor for 3 sequences of 3 frames -> LatentCondition without the full-rate tensor; its dense()
    is that tensor, bit for bit."""
    from vqvae_amd import core
    from vqvae_amd.core import Variable
    from vqvae_amd.functions import LazyUpsampled
    from vqvae_amd.generation import LatentCondition
    cfg = dict(H.SMALL)
    P, model = H.build_model(cfg, seed=133)
    model.to_gpu()
    e = np.random.RandomState(412).standard_normal((3, cfg['d'], 3, 1)).astype(np.float32)
    with core.using_config('train', False), core.no_backprop_mode():
        cond = model.condition_embed(Variable(gpu.to_device(e)), Variable(gpu.to_device(np.array([1, 6, 1], np.int32)))).data
    assert isinstance(cond, LazyUpsampled)
    lc = LatentCondition.from_condition(cond)
    assert cond._full is None
    assert lc.shape == (3, 64, 192) and (lc.Cl, lc.G, lc.upscale) == (32, 32, 64) and lc.tl.tolist() == [3, 3, 3]
    np.testing.assert_array_equal(_bits(lc.dense().get()), _bits(cond.get().reshape(3, 64, 192)))
    with pytest.raises(TypeError, match='LazyUpsampled'):
        LatentCondition.from_condition(cond.materialize())


# ---- 8. the dense paths ----------------------------------------------------------------------------------------------
def test_refused_paths(gpu):
    cfg = dict(H.SMALL)
    p, dec = _decoder(cfg, 131)
    lc, xs, g = _latent(gpu, cfg, [2, 2], 413)
    u = np.random.RandomState(414).random_sample((128, 2))
    with pytest.raises(TypeError, match='generate_lockstep'):
        dec.generate_sequence(lc, u)
    with pytest.raises(TypeError, match=r'\.dense\(\)'):
        dec.generate_batch(lc, u)
    assert dec.generate_sequence(lc.dense(), u, n_steps=3).shape == (2, 128)       # what the message names works
    with pytest.raises(ValueError):                                     # a decoder of another condition width
        dec.generate_lockstep(_latent(gpu, dict(local_dim=20, global_dim=13), [2] * 5, 415)[0], np.zeros((128, 5)))
