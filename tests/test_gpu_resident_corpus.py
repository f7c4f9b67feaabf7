"""The device-resident corpus (include/vqvae_corpus.h, csrc/corpus.hip, vqvae_amd.corpus) against the independent
restatement tests/resident_corpus_ref.py.  The rule is integer arithmetic, the samples are copied and the bins are the
streaming path's thresholds, so every comparison is bit equality; there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
from helpers import _bits, _same
import resident_corpus_ref as R
from zoned import In, Out, run_contract

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 71                          # bits above 32 set
BATCH = 5


def _normalised(w):
    return (w / np.abs(w).max()).astype(np.float32)


def _waves(lengths, seed):
    """Raw waveforms (not normalised: peaks between 0.3 and 3) and speaker ids 0..6."""
    rs = np.random.RandomState(seed)
    waves = [(rs.uniform(-1, 1, size=n) * rs.uniform(0.3, 3.0)).astype(np.float32) for n in lengths]
    for w in waves:
        w[w == 0] = 0.5
    return waves, [(3 * i + 1) % 7 for i in range(len(lengths))]


_CASES = {}


def _case(L1):
    """Seven utterances around the crop length: the pad / crop edge (len <= L1), count 1 and 2, a tail shorter than a
    workgroup's span.  Computed once and never changed."""
    if L1 not in _CASES:
        lengths = [1, L1 - 1, L1, L1 + 1, L1 + 2, 3 * L1 + 7, 4099]
        waves, speakers = _waves(lengths, 500 + L1)
        norm = [_normalised(w) for w in waves]
        for w in norm:
            w.setflags(write=False)
        _CASES[L1] = (lengths, waves, speakers, norm)
    return _CASES[L1]


_REF = {}


def _ref(L1, shuffle, iteration, rows=None, batch=BATCH):
    """The restatement's (x_enc, x_dec, speaker, t, utt, start) of one batch of _case(L1), computed once."""
    key = (L1, shuffle, iteration, None if rows is None else tuple(rows), batch)
    if key not in _REF:
        lengths, _, speakers, norm = _case(L1)
        plan = R.plan(SEED, iteration, batch, lengths, L1, shuffle, rows=rows)
        out = R.batch(norm, speakers, plan, L1) + (np.array([u for u, _ in plan], np.int32), np.array([s for _, s in plan], np.int64))
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _check_arrays(arrays, ref, what=''):
    """A Batch's .arrays against the restatement's first four arrays."""
    from vqvae_amd.inputs import IndexInput
    x_enc, x_dec, spk, t = arrays
    rows, L1 = ref[0].shape
    assert isinstance(x_dec, IndexInput) and x_dec.quantize == 256
    _same(x_enc.get(), ref[0].reshape(rows, 1, L1, 1), what + ' x_enc')
    _same(x_dec.get(), ref[1], what + ' x_dec')
    _same(spk.get(), ref[2], what + ' speaker')
    _same(t.get(), ref[3].reshape(rows, L1 - 1, 1), what + ' t')


_CORPORA = {}


def _corpus(L1):
    from vqvae_amd.corpus import ResidentCorpus
    if L1 not in _CORPORA:
        _, waves, speakers, _ = _case(L1)
        _CORPORA[L1] = ResidentCorpus(waves, speakers)
    return _CORPORA[L1]


# ---- 1. the draw ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shuffle', [True, False])
@pytest.mark.parametrize('L1', [2, 65, 130, 513])
def test_draw_is_the_restatement(gpu, L1, shuffle):
    """Batch 5 over 7 utterances, four consecutive iterations: 20 draws over three epochs."""
    from vqvae_amd.corpus import ResidentCorpusIterator
    corpus = _corpus(L1)
    assert corpus.samples.size == sum(_case(L1)[0])
    _same(corpus.samples.get(), np.concatenate(_case(L1)[3]), 'the uploaded corpus is the normalised waves end to end')
    it = ResidentCorpusIterator(corpus, BATCH, L1 - 1, SEED, shuffle=shuffle)
    seen = []
    for i in range(4):
        ref = _ref(L1, shuffle, i)
        arrays, utt, start = it.draw(i, record=True)
        _check_arrays(arrays, ref, 'iteration %d' % i)
        _same(utt.get(), ref[4], 'utt_out')
        _same(start.get(), ref[5], 'start_out')
        assert [tuple(r) for r in it.plan(i).tolist()] == list(zip(ref[4].tolist(), ref[5].tolist()))
        seen += ref[4].tolist()
    assert sorted(seen[:7]) == sorted(seen[7:14]) == list(range(7))


def test_upload_in_chunks_smaller_than_a_wave(gpu, monkeypatch):
    """The staging buffer cut to 1 000 floats: the corpus of L1 = 513 (7 700 samples) takes eight copies, waves span them."""
    from vqvae_amd import corpus as K
    monkeypatch.setattr(K, 'UPLOAD_CHUNK_BYTES', 4000)
    _, waves, speakers, norm = _case(513)
    c = K.ResidentCorpus(waves, speakers)
    _same(c.samples.get(), np.concatenate(norm))
    assert c.nbytes == 4 * sum(len(w) for w in waves) + 16 * 7 and len(c) == 7


# ---- 2. under red zones ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [0, 4])
@pytest.mark.parametrize('L1', [65, 130])
def test_draw_under_red_zones(gpu, L1, shift):
    """Every output between poisoned zones; the samples buffer ends with the last utterance's last element; `shift`
    moves the samples and the outputs by 4 bytes (odd dword addresses: no wider access can be assumed)."""
    from vqvae_amd import _lib
    from vqvae_amd.inputs import mulaw_thresholds
    lengths, _, speakers, norm = _case(L1)
    offsets = np.concatenate(([0], np.cumsum(lengths[:-1]))).astype(np.int64)
    view = np.array([6, 5, 4, 3, 2, 1, 0], np.int32)
    L = L1 - 1
    for shuffle, use_view, it_no in ((True, False, 1), (False, False, 2), (True, True, 3)):
        def fn(q):
            d = _lib.Corpus()
            d.samples, d.offset, d.length, d.speaker = q.samples.ptr, q.offset.ptr, q.length.ptr, q.speaker.ptr
            d.view, d.n_view = (q.view.ptr if use_view else None), 7
            _lib.call('vqvae_corpus_draw', C.byref(d), SEED, int(shuffle), it_no, BATCH, 0, 1, BATCH, L1, q.thr.ptr, 255,
                      q.x_enc.ptr, q.x_dec.ptr, q.t.ptr, q.spk.ptr, q.utt.ptr, q.start.ptr, gpu.stream())
        specs = dict(samples=In(np.concatenate(norm), shift=shift), offset=In(offsets), length=In(np.array(lengths, np.int32)),
                     speaker=In(np.array(speakers, np.int32)), thr=In(mulaw_thresholds(256)),
                     x_enc=Out((BATCH, L1), np.float32, shift=shift), x_dec=Out((BATCH, L), np.int32, shift=shift),
                     t=Out((BATCH, L), np.int32, shift=shift), spk=Out((BATCH,), np.int32, shift=shift),
                     utt=Out((BATCH,), np.int32, shift=shift), start=Out((BATCH,), np.int64))
        if use_view:
            specs['view'] = In(view, index_range=(0, 7))
        got = run_contract(gpu, fn, specs)
        if use_view:
            plan = R.plan(SEED, it_no, BATCH, lengths, L1, shuffle, view)
            ref = R.batch(norm, speakers, plan, L1) + (np.array([u for u, _ in plan], np.int32), np.array([s for _, s in plan], np.int64))
        else:
            ref = _ref(L1, shuffle, it_no)
        for name, want in zip(('x_enc', 'x_dec', 'spk', 't', 'utt', 'start'), ref):
            _same(got[name], want, '%s (shuffle %s, view %s)' % (name, shuffle, use_view))


# ---- 3. the streaming path's arrays ------------------------------------------------------------------------------------------
def test_arrays_are_the_device_input_pipelines(gpu):
    from vqvae_amd.corpus import ResidentCorpusIterator
    from vqvae_amd.inputs import DeviceInputPipeline
    L1 = 130
    it = ResidentCorpusIterator(_corpus(L1), BATCH, L1 - 1, SEED)
    pipe = DeviceInputPipeline(256)
    for i in range(2):
        ref = _ref(L1, True, i)
        want = pipe(ref[0], ref[2])
        got = it.next().arrays
        assert len(got) == len(want) == 4
        for g, w in zip(got, want):
            assert type(g) is type(w)
            _same(g.get(), w.get())
    assert it.iteration == 2


# ---- 4. training ---------------------------------------------------------------------------------------------------------
def test_training_from_the_corpus_equals_training_from_the_restated_minibatches(gpu):
    """H.SMALL, B = 3, L = 512, graph=True: two eager steps, the recording, two replays.  Losses of every step and every
    parameter, bit for bit."""
    import vqvae_amd as V
    from vqvae_amd.corpus import ResidentCorpus, ResidentCorpusIterator
    from vqvae_amd.inputs import DeviceInputPipeline
    from vqvae_amd.optimizers import Adam
    cfg = dict(H.SMALL)
    B, L, steps = 3, 512, 5
    lengths = [400, 513, 514, 700, 2000, 4099]
    waves, speakers = _waves(lengths, 77)
    norm = [_normalised(w) for w in waves]
    host = [R.batch(norm, speakers, R.plan(SEED, i, B, lengths, L + 1), L + 1) for i in range(steps)]

    class _Resident(object):
        def __init__(self):
            pipe = DeviceInputPipeline(256)
            self.batches = [pipe(x, spk) for x, _, spk, _ in host]
            self.i = 0

        def next(self):
            self.i += 1
            return self.batches[self.i - 1]

    def run(make_it, conv):
        _, model = H.build_model(cfg, seed=3)
        model.to_gpu()
        opt = Adam(2e-4)
        opt.setup(model)
        upd = V.VQVAE_StandardUpdater(make_it(), opt, converter=conv, device=0, graph=True)
        losses = []
        for _ in range(steps):
            upd.update()
            losses.append([l.data.get().copy() for l in upd.last_losses])
        assert upd._graphed is not None
        return losses, {n: p.data.get().copy() for n, p in model.namedparams()}

    la, pa = run(lambda: ResidentCorpusIterator(ResidentCorpus(waves, speakers), B, L, SEED), lambda b, d: b.arrays)
    lb, pb = run(_Resident, lambda b, d: b)
    for a, b in zip(la, lb):
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)
    assert set(pa) == set(pb)
    for n in pa:
        np.testing.assert_array_equal(pa[n], pb[n], err_msg=n)


# ---- 5. shards -----------------------------------------------------------------------------------------------------------
def test_rank_shards_are_strided_rows_of_the_global_batch(gpu):
    from vqvae_amd.corpus import ResidentCorpusIterator
    L1 = 130
    whole = ResidentCorpusIterator(_corpus(L1), BATCH, L1 - 1, SEED)
    parts = [ResidentCorpusIterator(_corpus(L1), BATCH, L1 - 1, SEED, rank=r, size=2) for r in (0, 1)]
    for i in range(3):
        full = [a.get() for a in whole.next().arrays]
        _check_arrays(whole.draw(i), _ref(L1, True, i))
        for r, it in enumerate(parts):
            got = [a.get() for a in it.next().arrays]
            assert got[0].shape[0] == (3, 2)[r]
            for g, f in zip(got, full):
                _same(g, np.ascontiguousarray(f[r::2]), 'rank %d iteration %d' % (r, i))


# ---- 6. one pass, the evaluator ------------------------------------------------------------------------------------------
def test_one_pass_in_order_and_the_evaluator(gpu):
    from vqvae_amd.corpus import ResidentCorpus, ResidentCorpusIterator
    from vqvae_amd.evaluator import Evaluator
    L = 512
    lengths = [300, 513, 514, 600, 1000, 2000, 4099]
    waves, _ = _waves(lengths, 78)
    speakers = list(range(7))
    norm = [_normalised(w) for w in waves]
    it = ResidentCorpusIterator(ResidentCorpus(waves, speakers), 3, L, SEED, shuffle=False, repeat=False)
    for i, utts in enumerate(([0, 1, 2], [3, 4, 5], [6])):
        plan = R.plan(SEED, i, 3, lengths, L + 1, shuffle=False, rows=range(len(utts)))
        assert [u for u, _ in plan] == utts
        _check_arrays(it.next().arrays, R.batch(norm, speakers, plan, L + 1), 'batch %d' % i)
        assert (it.epoch, it.is_new_epoch) == ((0, False), (0, False), (1, True))[i]
    assert it.epoch_detail == 1.0
    with pytest.raises(StopIteration):
        it.next()
    with pytest.raises(StopIteration):
        it.next()
    it.reset()
    _, model = H.build_model(dict(H.SMALL), seed=3)
    model.to_gpu()
    rep = Evaluator(it, model, converter=lambda b, d: b.arrays, device=0).evaluate()
    assert it.iteration == 3
    assert set(rep) == {'validation/main/loss', 'validation/main/loss1', 'validation/main/loss2', 'validation/main/loss3'}
    assert all(np.isfinite(v) for v in rep.values()), rep


# ---- 7. resume -----------------------------------------------------------------------------------------------------------
def test_resume_from_a_state_dict(gpu):
    from vqvae_amd.corpus import ResidentCorpusIterator
    L1 = 65
    fresh = ResidentCorpusIterator(_corpus(L1), BATCH, L1 - 1, SEED)
    for _ in range(3):
        fresh.next()
    state = fresh.state_dict()
    fourth = [a.get() for a in fresh.next().arrays]
    resumed = ResidentCorpusIterator(_corpus(L1), BATCH, L1 - 1, SEED)
    resumed.load_state_dict(state)
    assert resumed.iteration == 3 and resumed.epoch == fresh.epoch_of(3)
    got = resumed.next().arrays
    _check_arrays(got, _ref(L1, True, 3))
    for g, f in zip(got, fourth):
        _same(g.get(), f)


# ---- 8. addresses beyond 2^31 elements -----------------------------------------------------------------------------------
def test_utterance_beyond_2_to_31_elements(gpu):
    """One allocation of 2^31 + 8192 floats (8.6 GB, never initialised); only the last utterance, which starts beyond
    element 2^31 and ends with the allocation, is written and drawn (the view names it alone)."""
    from vqvae_amd import _lib
    from vqvae_amd.inputs import mulaw_thresholds
    total, off, L1, rows = 2 ** 31 + 8192, 2 ** 31 + 101, 513, 4
    lengths = [4096, total - off]
    try:
        samples = gpu.DeviceArray((total,), np.float32)
    except _lib.HipError as e:
        pytest.skip('the allocator refused %d bytes: %s' % (4 * total, e))
    try:
        wave = _normalised(_waves([lengths[1]], 79)[0][0])
        _lib.call('vqvae_memcpy_h2d', samples.ptr + 4 * off, wave.ctypes.data, wave.nbytes, gpu.stream())
        offset = gpu.to_device(np.array([0, off], np.int64))
        length = gpu.to_device(np.array(lengths, np.int32))
        speaker = gpu.to_device(np.array([2, 5], np.int32))
        view = gpu.to_device(np.array([1], np.int32))
        thr = gpu.to_device(mulaw_thresholds(256))
        x_enc, x_dec = gpu.DeviceArray((rows, L1), np.float32), gpu.DeviceArray((rows, L1 - 1), np.int32)
        t, spk = gpu.DeviceArray((rows, L1 - 1), np.int32), gpu.DeviceArray((rows,), np.int32)
        utt, start = gpu.DeviceArray((rows,), np.int32), gpu.DeviceArray((rows,), np.int64)
        d = _lib.Corpus()
        d.samples, d.offset, d.length, d.speaker, d.view, d.n_view = samples.ptr, offset.ptr, length.ptr, speaker.ptr, view.ptr, 1
        _lib.call('vqvae_corpus_draw', C.byref(d), SEED, 1, 6, rows, 0, 1, rows, L1, thr.ptr, 255, x_enc.ptr, x_dec.ptr, t.ptr,
                  spk.ptr, utt.ptr, start.ptr, gpu.stream())
        plan = R.plan(SEED, 6, rows, lengths, L1, True, [1])
        assert [u for u, _ in plan] == [1] * rows and len(set(s for _, s in plan)) > 1
        ref = R.batch([np.zeros(1, np.float32), wave], [2, 5], plan, L1)
        for g, w in zip((x_enc, x_dec, spk, t), ref):
            _same(g.get(), w)
        assert utt.get().tolist() == [1] * rows and start.get().tolist() == [s for _, s in plan]
    finally:
        gpu.synchronize()
        del samples
        gpu.free_all_blocks()                # the 8.6 GB go back to the driver, not into the pool
