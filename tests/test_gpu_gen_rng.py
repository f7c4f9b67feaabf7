"""The uniforms of generation drawn on the device (include/vqvae_gen_rng.h, csrc/gen_rng.hip, vqvae_amd.DeviceUniforms)
against the independent restatement tests/gen_rng_ref.py: the fill launch under red zones, and every call that takes a
DeviceUniforms against the same call fed the restatement's array.  The generator is integer arithmetic and the kernels
are the array form's kernels with the load replaced, so every comparison is bit equality; there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import gen_rng_ref as R
import helpers as H
from helpers import _bits, _same
import vqvae_oracle as O
from test_gpu_generate import _cond, _decoder, _random_biases
from zoned import In, Out, run_contract

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE1234567890                    # bits above 32 set
HIGH_IDS = [2 ** 40 + 3, 5, 2 ** 64 - 1]     # ... and in the ids
TL11 = (3, 1, 2, 3, 1, 2, 2, 1, 3, 1, 2)
LENGTHS11 = np.array([48, 17, 33, 48, 9, 40, 25, 1, 48, 2, 31])
IDS11 = np.array([900, 2 ** 33 + 1, 7, 2 ** 63, 4, 3, 2, 1, 0, 2 ** 64 - 1, 12], np.uint64)     # permuted, not arange


def _same_pair(a, b, what=''):
    _same(a[0], b[0], what + ' out')
    _same(a[1], b[1], what + ' logits')


_REF = {}


def _ref(seed, ids, steps, n_uniform=1, t0=0):
    """The restatement's array, computed once per argument set and never changed: (steps, N) or (steps, N, n_uniform)."""
    key = (seed, tuple(int(i) for i in ids), steps, n_uniform, t0)
    if key not in _REF:
        u = R.uniforms(seed, key[1], steps, n_uniform, t0)
        u = u[:, :, 0] if n_uniform == 1 else u
        u.setflags(write=False)
        _REF[key] = u
    return _REF[key]


@pytest.fixture(scope='module')
def softmax_decoder(gpu):
    return dict(H.SMALL), _decoder(dict(H.SMALL), 141)[1]


@pytest.fixture(scope='module')
def mol_decoder(gpu):
    cfg = dict(H.MOL, input_dim=1)
    return cfg, _decoder(cfg, 143, use_logistic=True)[1]


# ---- 1. the fill launch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_uniform', [1, 3, 10])
def test_fill_under_red_zones(gpu, n_uniform):
    """n = 3; steps 0..6 and 5..11; ids NULL and ids with bits above 32; the seed has bits above 32.  n_uniform = 3 leaves
    half of every second block unused, and its rows are 24 bytes, so a store of the unused half would land in the next
    row or, in the last row, in the red zone."""
    from vqvae_amd import _lib
    n, steps = 3, 7
    for t0 in (0, 5):
        for ids in (None, HIGH_IDS):
            def fn(q):
                r = _lib.GenRng()
                r.seed, r.ids = SEED, None if ids is None else q.ids.ptr
                _lib.call('vqvae_gen_rng_fill', C.byref(r), t0, steps, n, n_uniform, q.out.ptr, gpu.stream())
            specs = dict(out=Out((steps, n, n_uniform), np.float64))
            if ids is not None:
                specs['ids'] = In(np.array(ids, np.uint64))
            got = run_contract(gpu, fn, specs)['out']
            want = R.uniforms(SEED, range(n) if ids is None else ids, steps, n_uniform, t0)
            _same(got, want, 'n_uniform %d t0 %d ids %s' % (n_uniform, t0, ids))
            assert (got >= 0).all() and (got < 1).all()


# ---- 2. the sampler alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['softmax', 'mol'])
def test_sampler_alone_equals_the_array_entry_point(gpu, mode):
    from vqvae_amd import _lib
    from vqvae_amd.generation import DeviceUniforms, sample_logits
    n = 6
    rs = np.random.RandomState(31)
    ids = [2 ** 35 + 1, 0, 7, 7, 2 ** 64 - 1, 3]
    if mode == 'softmax':
        logits = (1.5 * rs.standard_normal((n, 256))).astype(np.float32)
        gmode, nu = _lib.GEN_SOFTMAX, 1
        settings = (dict(), dict(temperature=[0.0, 0.8, 1.0, 0.8, 0.0, 0.8], top_k=[0, 5, 5, 0, 5, 0],
                                 top_p=[1.0, 0.9, 1.0, 0.9, 0.9, 1.0]))
    else:
        logits = rs.standard_normal((n, 30)).astype(np.float32)
        gmode, nu = _lib.GEN_MOL, 10
        settings = (dict(), dict(temperature=[1.0, 0.8, 0.8, 1.0, 0.8, 1.3]))
    ld = gpu.to_device(logits)
    draws = []
    for step in (0, 9):
        for g, gids in ((DeviceUniforms(SEED, ids), ids), (DeviceUniforms(SEED), range(n))):
            u = _ref(SEED, gids, 1, nu, step)[0]
            for kw in settings:
                want = sample_logits(ld, u, gmode, **kw).get()
                got = sample_logits(ld, g, gmode, step=step, **kw).get()
                _same(got, want, '%s step %d %s' % (mode, step, sorted(kw)))
                draws.append(got)
        if mode == 'softmax':
            kw = settings[1]
            a = sample_logits(ld, _ref(SEED, ids, 1, 1, step)[0], gmode, return_probs=True, **kw)
            b = sample_logits(ld, DeviceUniforms(SEED, ids), gmode, return_probs=True, step=step, **kw)
            _same(b[0].get(), a[0].get())
            _same(b[1].get(), a[1].get())
    assert any((draws[0] != d).any() for d in draws[1:])                 # the step, the ids and the controls are read


# ---- 3. generate_sequence (n <= 4: the array is filled on the device) ---------------------------------------------------
@pytest.mark.parametrize('n', [1, 3])
def test_generate_sequence_equals_the_array_call(gpu, softmax_decoder, n):
    from vqvae_amd.generation import DeviceUniforms
    cfg, dec = softmax_decoder
    T = 41
    cond = gpu.to_device(_cond(cfg, n, T, 17))
    ids = HIGH_IDS[:n]
    forced = np.random.RandomState(3).randint(0, cfg['input_dim'], (T, n)).astype(np.int32)
    for g, gids in ((DeviceUniforms(SEED), range(n)), (DeviceUniforms(SEED, ids), ids)):
        u = _ref(SEED, gids, T - 1)
        outs = []
        for kw in (dict(persistent=True), dict(persistent=False), dict(persistent=False, graph_steps=0),
                   dict(temperature=0.8, top_k=[5, 0, 7][:n], top_p=0.9), dict(persistent=False, forced=forced)):
            want = dec.generate_sequence(cond, u, return_logits=True, **kw)
            got = dec.generate_sequence(cond, g, return_logits=True, **kw)
            _same_pair([x.get() for x in got], [x.get() for x in want], 'n %d %s' % (n, sorted(kw)))
            outs.append(got[0].get())
        _same(outs[1], outs[0])
        assert (outs[3] != outs[0]).any() and len(np.unique(outs[0])) > 10
    short = dec.generate_sequence(cond, DeviceUniforms(SEED), n_steps=11).get()           # fewer steps: the same first rows
    _same(short[:, :11], dec.generate_sequence(cond, DeviceUniforms(SEED)).get()[:, :11])


# ---- 4. / 5. generate_lockstep: groups and refill -----------------------------------------------------------------------
@pytest.fixture(scope='module')
def eleven(gpu, softmax_decoder):
    """11 sequences of ragged lengths on the softmax decoder, and what the array call gives them in one group of 11."""
    cfg, dec = softmax_decoder
    T = 48
    cond = gpu.to_device(_cond(cfg, 11, T, 19))
    u = _ref(SEED, range(11), T - 1)
    want = dec.generate_lockstep(cond, u, lengths=LENGTHS11, return_logits=True)
    return cond, T, u, want


@pytest.mark.parametrize('group', [128, 5])
def test_lockstep_groups_equal_the_array_call(gpu, softmax_decoder, eleven, group):
    """group = 128: one group of 11 whose shorter members keep running; group = 5: 5 + 5 + 1, the last group four repeats
    of its only member, and members gathered out of order (longest first)."""
    from vqvae_amd.generation import DeviceUniforms, plan_lockstep
    cfg, dec = softmax_decoder
    cond, T, u, want11 = eleven
    groups = plan_lockstep(11, T, LENGTHS11, group=group)[1]
    assert [len(i) for i, _ in groups] == ([11] if group == 128 else [5, 5, 5]) and (group == 128 or len(set(groups[-1][0])) == 1)
    want = dec.generate_lockstep(cond, u, lengths=LENGTHS11, return_logits=True, group=group)
    got = dec.generate_lockstep(cond, DeviceUniforms(SEED), lengths=LENGTHS11, return_logits=True, group=group)
    _same_pair(got, want, 'group %d' % group)
    _same_pair(got, want11, 'group %d against one group of 11' % group)
    for i, L in enumerate(LENGTHS11):
        assert (got[0][i, L - 1:] == 0).all() and (got[1][L - 1:, i] == 0).all()
    assert len(np.unique(got[0])) > 10
    # stream ids of the caller's own, permuted: sequence i draws stream IDS11[i]
    up = _ref(SEED, IDS11, T - 1)
    wantp = dec.generate_lockstep(cond, up, lengths=LENGTHS11, return_logits=True, group=group)
    gotp = dec.generate_lockstep(cond, DeviceUniforms(SEED, IDS11), lengths=LENGTHS11, return_logits=True, group=group)
    _same_pair(gotp, wantp, 'group %d permuted ids' % group)
    assert (gotp[0] != got[0]).any()
    # teacher forcing
    forced = np.random.RandomState(5).randint(0, cfg['input_dim'], (T, 11)).astype(np.int32)
    wantf = dec.generate_lockstep(cond, u, lengths=LENGTHS11, return_logits=True, group=group, forced=forced)
    gotf = dec.generate_lockstep(cond, DeviceUniforms(SEED), lengths=LENGTHS11, return_logits=True, group=group, forced=forced)
    _same_pair(gotf, wantf, 'group %d forced' % group)
    assert (gotf[1] != got[1]).any()


def test_refill_equals_the_array_call_and_the_groups(gpu, softmax_decoder, eleven):
    from vqvae_amd.generation import DeviceUniforms, plan_refill
    cfg, dec = softmax_decoder
    cond, T, u, want11 = eleven
    ticks, placement = plan_refill(LENGTHS11 - 1, 5)
    assert (placement[LENGTHS11 > 1, 1] > 0).sum() >= 5                  # sequences that start in a used slot, mid-run
    for gs in (8, 0):
        want = dec.generate_lockstep(cond, u, lengths=LENGTHS11, return_logits=True, group=5, refill=True, graph_steps=gs)
        got = dec.generate_lockstep(cond, DeviceUniforms(SEED), lengths=LENGTHS11, return_logits=True, group=5, refill=True,
                                    graph_steps=gs)
        _same_pair(got, want, 'refill graph_steps %d' % gs)
        _same_pair(got, want11, 'refill against the groups')
    gotp = dec.generate_lockstep(cond, DeviceUniforms(SEED, IDS11), lengths=LENGTHS11, return_logits=True, group=5, refill=True)
    wantp = dec.generate_lockstep(cond, _ref(SEED, IDS11, T - 1), lengths=LENGTHS11, return_logits=True, group=5, refill=True)
    _same_pair(gotp, wantp, 'refill permuted ids')
    assert (gotp[0] != want11[0]).any()


# ---- 6. the latent-rate condition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('refill', [True, False])
def test_latent_condition_with_mixed_controls(gpu, softmax_decoder, refill):
    from test_gpu_gen_cond import _latent
    from vqvae_amd.generation import DeviceUniforms
    cfg, dec = softmax_decoder
    lc, xs, g = _latent(gpu, cfg, TL11, 412, upscale=16)
    N, Cc, T = lc.shape
    assert (N, T) == (11, 48)
    ctl = dict(temperature=[0.0, 1.0, 1.0, 0.7, 1.0, 1.3, 1.0, 0.8, 0.0, 1.0, 0.8], top_k=[0, 3, 0, 0, 0, 5, 0, 5, 5, 0, 0],
               top_p=[1.0, 1.0, 0.9, 1.0, 1.0, 0.5, 1.0, 0.9, 1.0, 1.0, 0.9])
    want = dec.generate_lockstep(lc, _ref(SEED, IDS11, T - 1), return_logits=True, group=5, refill=refill, **ctl)
    got = dec.generate_lockstep(lc, DeviceUniforms(SEED, IDS11), return_logits=True, group=5, refill=refill, **ctl)
    _same_pair(got, want, 'latent refill %s' % refill)
    plain = dec.generate_lockstep(lc, DeviceUniforms(SEED, IDS11), group=5, refill=refill)
    assert (plain != got[0]).any()                                       # the controls were read
    _same(plain[4], got[0][4])                                           # ... per sequence: 4 is neutral


# ---- 7. the mixture of logistics ----------------------------------------------------------------------------------------
def test_mixture_of_logistics(gpu, mol_decoder):
    from vqvae_amd.generation import DeviceUniforms
    cfg, dec = mol_decoder
    N, T = 6, 24
    cond = gpu.to_device(_cond(cfg, N, T, 23))
    ids = [2 ** 40, 1, 2, 3, 2 ** 64 - 1, 5]
    u = _ref(SEED, ids, T - 1, 10)
    lengths = np.array([24, 10, 24, 17, 3, 24])
    outs = []
    for kw in (dict(), dict(refill=True), dict(refill=True, temperature=[1.0, 0.8, 1.2, 1.0, 0.8, 1.0])):
        want = dec.generate_lockstep(cond, u, lengths=lengths, return_logits=True, **kw)
        got = dec.generate_lockstep(cond, DeviceUniforms(SEED, ids), lengths=lengths, return_logits=True, **kw)
        _same_pair(got, want, 'mol %s' % sorted(kw))
        outs.append(got)
    _same_pair(outs[1], outs[0], 'mol refill against lockstep')
    assert outs[0][0].dtype == np.float32 and np.abs(outs[0][0]).max() <= 1.0 and len(np.unique(outs[0][0])) > 50
    assert (outs[2][0] != outs[0][0]).any()


# ---- 8. the new promise: the same bits in any batch, position and slot --------------------------------------------------
def test_a_sequence_gets_the_same_bits_in_any_batch(gpu, softmax_decoder):
    """The sequence with stream id 7 and its own condition rows: at position 3 of a batch of 11, at position 0 of a batch of
    6, and in a refilled run of 11 in 5 slots where it is the shortest and so a late tenant of a used slot."""
    from vqvae_amd.generation import DeviceUniforms, plan_refill
    cfg, dec = softmax_decoder
    T, L = 48, 20
    mine = _cond(cfg, 1, T, 29)[0]

    def batch(N, pos, seed, lengths):
        c = _cond(cfg, N, T, seed)
        c[pos] = mine
        ids = np.arange(100, 100 + N).astype(np.uint64)
        ids[pos] = 7
        lengths = np.array(lengths)
        lengths[pos] = L
        return gpu.to_device(c), DeviceUniforms(SEED, ids), lengths

    runs = []
    c, g, lengths = batch(11, 3, 31, [48] * 11)
    o, lg = dec.generate_lockstep(c, g, lengths=lengths, return_logits=True)
    runs.append((o[3], lg[:, 3]))
    c, g, lengths = batch(6, 0, 33, [30, 48, 25, 48, 41, 48])
    o, lg = dec.generate_lockstep(c, g, lengths=lengths, return_logits=True)
    runs.append((o[0], lg[:, 0]))
    c, g, lengths = batch(11, 9, 35, [48, 40, 45, 33, 48, 37, 29, 48, 26, 48, 31])
    ticks, placement = plan_refill(lengths - 1, 5)
    assert placement[9, 1] > 20, placement[9]                            # it starts late, in a slot another sequence has used
    o, lg = dec.generate_lockstep(c, g, lengths=lengths, return_logits=True, group=5, refill=True)
    runs.append((o[9], lg[:, 9]))
    for k, (o, lg) in enumerate(runs):
        assert o[:L - 1].any() and not o[L - 1:].any()
        _same(o, runs[0][0], 'run %d out' % k)
        _same(lg[:L - 1], runs[0][1][:L - 1], 'run %d logits' % k)
    assert len(np.unique(runs[0][0])) > 5


# ---- 9. synthesis -------------------------------------------------------------------------------------------------------
class _StandIn(object):
    """A RandomState whose draws are the restatement's array for the given streams."""

    def __init__(self, seed, ids):
        self.seed, self.ids, self.calls = seed, ids, 0

    def random_sample(self, shape):
        self.calls += 1
        assert shape[1] == len(self.ids)
        return np.array(_ref(self.seed, self.ids, shape[0]))

    def uniform(self, lo, hi, shape):
        self.calls += 1
        assert (lo, hi) == (0, 1) and shape[1] == len(self.ids)
        return np.array(_ref(self.seed, self.ids, shape[0], shape[2]))


def test_synthesize_many_depends_on_the_utterance_alone(gpu):
    import vqvae_amd as V
    cfg = dict(H.SMALL)
    P, model = H.build_model(cfg, seed=145, tweak=_random_biases(146))
    model.to_gpu()
    links = (model.encoder, model.vq, model.decoder, model.condition_embed)
    sizes = (128, 64, 192, 320, 256)
    speaker = np.array([2, 5, 2, 0, 6], np.int32)
    ids = [11, 2 ** 40 + 7, 3, 2 ** 64 - 1, 0]
    waves = [O.synth_batch(1, length=L, n_speaker=cfg['n_speaker'], seed=16 + i)[0].reshape(-1) for i, L in enumerate(sizes)]

    def many(ws, spk, rng):
        return V.synthesize_many(*links, ws, spk, rng=rng, group=5, return_output=True, latent_condition=True)

    stand = _StandIn(SEED, ids)
    want = many(waves, speaker, stand)
    got = many(waves, speaker, V.DeviceUniforms(SEED, ids))
    back = many(waves[::-1], speaker[::-1].copy(), V.DeviceUniforms(SEED, ids[::-1]))[::-1]
    assert stand.calls == 1 and len(got) == 5 and sorted(len(w) for w, _ in got) == sorted(sizes)
    for i in range(5):
        for a, b in ((got[i], want[i]), (back[i], got[i])):
            assert a[1].dtype == b[1].dtype == np.int32
            _same(a[1], b[1], 'utterance %d output' % i)
            _same(a[0], b[0], 'utterance %d wave' % i)
        assert len(np.unique(got[i][1])) > 10
    # one waveform through generate_sequence (the array is filled on the device) and through a lockstep group of repeats
    x = waves[1].reshape(1, 1, -1, 1)
    for kw in (dict(), dict(lockstep=True), dict(lockstep=True, latent_condition=True)):
        w0, o0 = V.synthesize(*links, x, speaker[1:2], rng=_StandIn(SEED, ids[1:2]), **kw)
        w1, o1 = V.synthesize(*links, x, speaker[1:2], rng=V.DeviceUniforms(SEED, ids[1:2]), **kw)
        _same(np.asarray(o1), np.asarray(o0), 'synthesize %s' % sorted(kw))
        _same(np.asarray(w1), np.asarray(w0), 'synthesize %s' % sorted(kw))
