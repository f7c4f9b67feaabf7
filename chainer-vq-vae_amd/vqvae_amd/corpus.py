"""The training corpus on the device, minibatches drawn there (include/vqvae_corpus.h, csrc/corpus.hip).

The reference decodes, trims, normalises and crops one file per example on the host, every epoch (train.py:55-61,
utils.py:54-110).  The preprocessed corpus is small next to the device's memory (float32 at 16 kHz: 230.4 MB per hour),
so ``ResidentCorpus`` keeps it there, and ``ResidentCorpusIterator.next()`` is one small launch that chooses the
utterances (a new shuffled order per epoch), the crop offsets, pads short utterances with zeros, bins the samples and
gathers the speaker ids: no host work that grows with the batch and no host-to-device copy per step.  Row r of batch i is
a pure function of (seed, i, r) -- the rule is in the header, ``plan_rows`` replays it on the host -- so the data order
resumes exactly, does not depend on the number of ranks, and a rank draws batch[rank::size] without communication.
"""
import ctypes as C
import operator

import numpy as np

from . import _lib, backend, ragged
from .backend import DeviceArray
from .generation import philox4x32_10
from .inputs import IndexInput, StreamingInputIterator, _Pinned, mulaw_thresholds, peak_normalise

_TAG_PERM, _TAG_CROP = 0x50455231, 0x43524F31      # the fourth counter word of the permutation's and the crop's blocks
_M32 = 0xFFFFFFFF
UPLOAD_CHUNK_BYTES = 16 << 20                      # the page-locked staging buffer of ResidentCorpus's upload


# --------------------------------------------------------------------------- #
# the rule on the host
# --------------------------------------------------------------------------- #
def _word0(counters, seed):
    """First word of one Philox block per row of ``counters`` (R, 4), as Python-sized uint64."""
    key = np.array([seed & _M32, seed >> 32], np.uint64)
    return philox4x32_10(np.asarray(counters, np.uint64), key)[..., 0].astype(np.uint64)


def shuffled_positions(seed, e, p, n):
    """pi(seed, e[i], p[i]) for arrays of epochs and positions: the cycle-walking Feistel bijection of [0, n) of
    include/vqvae_corpus.h, all rows walked together until each has landed below n."""
    e = np.asarray(e, np.uint64).reshape(-1)
    p = np.asarray(p, np.uint64).reshape(-1)
    if n == 1:
        return np.zeros(p.shape, np.int64)
    w = max(2, int(n - 1).bit_length())
    w += w & 1
    h = np.uint64(w // 2)
    mask = np.uint64((1 << (w // 2)) - 1)
    x = p.copy()
    todo = np.ones(x.shape, bool)
    for _ in range(1 << w):
        idx = np.nonzero(todo)[0]
        if not idx.size:
            break
        left, right = x[idx] >> h, x[idx] & mask
        for i in range(4):
            ctr = np.stack([right, np.full_like(right, i), e[idx], np.full_like(right, _TAG_PERM)], axis=-1)
            left, right = right, left ^ (_word0(ctr, seed) & mask)
        x[idx] = (left << h) | right
        todo[idx] = x[idx] >= np.uint64(n)
    return x.astype(np.int64)


def crop_start(seed, d, count):
    """The crop offset of draw ``d`` in an utterance of ``count`` + L1 samples: 0 on the padding branch, else the high
    64 bits of (a 64-bit Philox number) * count, an integer in [0, count - 1] (utils.py:78's range)."""
    d, count = int(d), int(count)
    if count <= 0:
        return 0
    key = np.array([seed & _M32, seed >> 32], np.uint64)
    b = philox4x32_10(np.array([d & _M32, d >> 32, 0, _TAG_CROP], np.uint64), key)
    return (((int(b[0]) << 32) | int(b[1])) * count) >> 64


def plan_rows(seed, iteration, global_batch, lengths, L1, shuffle=True, view=None, rows=None):
    """Host replay of vqvae_corpus_draw: int64 (R, 2) of (utterance, start) for the global rows ``rows`` (default: all
    of them) of global batch ``iteration``.  ``lengths``: samples per utterance of the whole corpus; ``view``: the
    utterance numbers drawn from (None: all)."""
    lengths = np.asarray(lengths, np.int64)
    n = len(lengths) if view is None else len(view)
    rows = np.arange(global_batch) if rows is None else np.asarray(rows, np.int64)
    d = [int(iteration) * int(global_batch) + int(r) for r in rows]
    e, p = [x // n for x in d], [x % n for x in d]
    if max(e, default=0) > _M32:
        raise ValueError('plan_rows: epoch %d does not fit 32 bits' % max(e))
    q = shuffled_positions(seed, e, p, n) if shuffle else np.asarray(p, np.int64)
    u = q if view is None else np.asarray(view, np.int64)[q]
    out = np.empty((len(d), 2), np.int64)
    out[:, 0] = u
    out[:, 1] = [crop_start(seed, di, lengths[ui] - L1) for di, ui in zip(d, u)]
    return out


# --------------------------------------------------------------------------- #
# the corpus
# --------------------------------------------------------------------------- #
class _Utterances(object):
    """What a corpus and a view of it share: the utterance numbers drawn from and the ways to narrow them."""

    def __len__(self):
        return len(self.lengths)

    def subset(self, indices):
        """The view that draws from utterances ``indices`` of this one (in that order; repeats allowed)."""
        idx = np.asarray(indices)
        if idx.ndim != 1 or idx.size == 0 or idx.dtype.kind not in 'iu':
            raise ValueError('subset: indices must be a non-empty (n,) integer array, got %r' % (indices,))
        if idx.min() < 0 or idx.max() >= len(self):
            raise ValueError('subset: indices must be in [0, %d)' % len(self))
        return CorpusView(self.corpus, self.utterances[idx])

    def split(self, first_size, seed=None):
        """Two views: utterances ``numpy.random.RandomState(seed).permutation(len)[:first_size]`` and the rest, the
        order chainer.datasets.split_dataset_random(dataset, first_size, seed) gives (train.py:61)."""
        n = len(self)
        if not 0 < int(first_size) < n:
            raise ValueError('split: first_size must be in (0, %d), got %r' % (n, first_size))
        order = np.random.RandomState(seed).permutation(n)
        return self.subset(order[:int(first_size)]), self.subset(order[int(first_size):])

    def hours(self, sr=16000):
        return float(np.sum(self.lengths, dtype=np.int64)) / float(sr) / 3600.0

    def encode(self, encoder, vq, chunk_bytes=1 << 30):
        """The discrete codes of these utterances, whole (frontend.LatentCodes): the encoder's ragged convs read every
        utterance in place from the corpus buffer through its offsets and lengths, nothing is copied or sliced."""
        from .frontend import encode_corpus
        return encode_corpus(self, encoder, vq, chunk_bytes)

    def segment(self, encoder, vq, penalties, chunk_bytes=1 << 30):
        """The duration-penalised codes of these utterances under every penalty (segmental.SegmentalCodes), read in place
        like ``encode``; see segmental.segment_many."""
        from .segmental import segment_corpus
        return segment_corpus(self, encoder, vq, penalties, chunk_bytes)

    def abx(self, encoder, vq, items, **kwargs):
        """The ABX error of ``items`` (abx.Items, in latent frames of these utterances) over the encoder's latents or the
        codes (abx.ABXScores), read in place like ``encode``; see abx.abx_many for the keywords."""
        from .abx import abx_corpus
        return abx_corpus(self, encoder, vq, items, **kwargs)

    def score(self, wavenet, condition, chunk_bytes=1 << 30, per_sample=False, return_logits=False):
        """The likelihood of these utterances under ``wavenet`` given ``condition`` (scoring.Scores): the samples are
        binned in place from the corpus buffer; see scoring.score_many."""
        from .scoring import score_many
        return score_many(wavenet, condition, self, chunk_bytes, per_sample, return_logits)

    def score_mol(self, wavenet, condition, chunk_bytes=1 << 30, per_sample=False, return_params=False):
        """``score`` for a mixture-of-logistics decoder (scoring_mol.MolScores): inputs and targets are the samples, read in
        place from the corpus buffer; see scoring_mol.score_many_mol."""
        from .scoring_mol import score_many_mol
        return score_many_mol(wavenet, condition, self, chunk_bytes, per_sample, return_params)

    def code_stats(self, codes, **kw):
        """Usage, speaker leakage and durations of these utterances' codes (``encode``'s result) with these utterances'
        speaker ids as the groups (codestats.CodeStats); see codestats.code_stats for the keywords."""
        from .codestats import code_stats
        return code_stats(codes, speakers=self.speakers, **kw)

    def fit_speakers(self, cfg, chunk_bytes=1 << 30, **kw):
        """One Gaussian per speaker over these utterances' mel-cepstra, read in place, with these utterances' speaker ids
        (speakerid.SpeakerModels); see speakerid.fit_speakers for the keywords."""
        from . import speakerid
        from .metrics import features_many
        speakerid.feature_dim(cfg, kw.get('deltas', True), 'fit_speakers')
        speakerid._speaker_ids(self.speakers, kw.get('n_speakers'), len(self), 'fit_speakers')
        return speakerid.fit_speakers(features_many(self, cfg, chunk_bytes=chunk_bytes), self.speakers, **kw)


class ResidentCorpus(_Utterances):
    """``waves``: loaded, silence-trimmed waveforms (what inputs.crop_or_pad takes); ``speakers``: one int id each.
    Every wave is peak-normalised on the host (inputs.peak_normalise, crop_or_pad's expression) and the corpus is
    uploaded in chunks of UPLOAD_CHUNK_BYTES through one page-locked buffer into one ragged float32 device buffer."""

    def __init__(self, waves, speakers):
        waves = list(waves)
        lengths, spk = _check_description([np.shape(w)[0] if np.ndim(w) == 1 else -1 for w in waves], speakers)
        norm = []
        for i, w in enumerate(waves):
            w = np.asarray(w, np.float32)
            peak = np.abs(w).max()
            if not np.isfinite(peak) or not np.isfinite(w).all():
                raise ValueError('ResidentCorpus: wave %d holds a non-finite sample' % i)
            if peak == 0:
                raise ValueError('ResidentCorpus: wave %d is all zeros (no peak to normalise by)' % i)
            norm.append(w)
        self._describe(lengths, spk)
        self.samples = DeviceArray((int(self.offsets[-1] + lengths[-1]),), np.float32)
        self._upload(norm)
        self._offset_dev = backend.to_device(self.offsets)
        self._length_dev = backend.to_device(self.lengths)
        self._speaker_dev = backend.to_device(self.speakers)

    @classmethod
    def describe(cls, lengths, speakers):
        """The description alone -- lengths and speaker ids, nothing on the device: enough to split, to subset and to
        ``plan`` a data order; drawing from it raises."""
        self = cls.__new__(cls)
        self._describe(*_check_description(lengths, speakers))
        self.samples = None
        return self

    @classmethod
    def from_arrays(cls, raws, srs, speakers, sr=16000, res_type='kaiser_fast', top_db=20, batch_bytes=64 << 20,
                    skip_bad=False):
        """The corpus from raw audio, preprocessed on the device (vqvae_amd.ingest, include/vqvae_ingest.h): ``raws`` are
        arrays (frames,) or (frames, channels), int16 or floating, at the sample rates ``srs`` (or one for all).  They are
        decoded to mono, resampled to ``sr``, silence-trimmed at ``top_db`` and peak-normalised there, in batches of at most
        ``batch_bytes`` of raw audio; utterance order is input order.  A wave that is all zeros, holds a non-finite sample,
        is empty or too short to trim is a ValueError naming its index, or with ``skip_bad`` is left out and listed in
        ``corpus.skipped`` as (index, reason)."""
        from . import ingest
        raws = list(raws)
        srs = [srs] * len(raws) if np.ndim(srs) == 0 else list(srs)
        if len(srs) != len(raws):
            raise ValueError('ResidentCorpus: %d sample rates for %d waves' % (len(srs), len(raws)))
        items = [ingest._Array(raw, s, 'wave %d' % i) for i, (raw, s) in enumerate(zip(raws, srs))]
        return cls._from_items(items, speakers, ingest.DeviceIngest(sr, res_type, top_db), batch_bytes, skip_bad,
                               lambda i: i)

    @classmethod
    def from_files(cls, files, speakers, sr=16000, res_type='kaiser_fast', top_db=20, batch_bytes=64 << 20, skip_bad=False):
        """``from_arrays`` for WAV files (ingest.read_wav; ingest.corpus_files lists a VCTK, ARCTIC or 'vs' tree): the
        headers are read first, the samples batch by batch.  Errors and ``corpus.skipped`` name the file."""
        from . import ingest
        files = [str(f) for f in files]
        items = [ingest._File(f) for f in files]
        return cls._from_items(items, speakers, ingest.DeviceIngest(sr, res_type, top_db), batch_bytes, skip_bad,
                               lambda i: files[i])

    @classmethod
    def _from_items(cls, items, speakers, front, batch_bytes, skip_bad, label):
        speakers = list(speakers)
        if not items:
            raise ValueError('ResidentCorpus: no waves')
        if len(speakers) != len(items):
            raise ValueError('ResidentCorpus: %d speakers for %d waves' % (len(speakers), len(items)))
        _check_description([1] * len(items), speakers)
        samples, lengths, keep, skipped = front.ingest(items, batch_bytes, skip_bad, 'ResidentCorpus')
        self = cls.__new__(cls)
        self._describe(*_check_description(lengths.tolist(), [speakers[i] for i in keep]))
        self.samples = samples
        self.skipped = [(label(i), reason) for i, reason in skipped]
        self._offset_dev = backend.to_device(self.offsets)
        self._length_dev = backend.to_device(self.lengths)
        self._speaker_dev = backend.to_device(self.speakers)
        return self

    def _describe(self, lengths, speakers):
        self.corpus = self
        self.lengths, self.speakers = lengths, speakers
        self.offsets = ragged.offsets(lengths)
        self.utterances = np.arange(len(lengths), dtype=np.int32)
        self._view_dev = None

    def _upload(self, waves):
        chunk = UPLOAD_CHUNK_BYTES // 4
        stage = _Pinned((chunk,), np.float32)
        st = backend.stream()
        fill, at = 0, 0                                    # floats staged, floats of the device buffer already sent

        def flush():
            _lib.call('vqvae_memcpy_h2d_async', self.samples.ptr + 4 * at, stage.ptr, 4 * fill, st)
            _lib.call('vqvae_stream_synchronize', st)      # the one staging buffer is refilled next

        for w in waves:
            w = peak_normalise(w)
            done = 0
            while done < len(w):
                take = min(chunk - fill, len(w) - done)
                stage.array[fill:fill + take] = w[done:done + take]
                fill, done = fill + take, done + take
                if fill == chunk:
                    flush()
                    at, fill = at + fill, 0
        if fill:
            flush()

    @property
    def nbytes(self):
        """Bytes of the corpus on the device: the samples and the three per-utterance arrays."""
        return 4 * int(np.sum(self.lengths, dtype=np.int64)) + 16 * len(self.lengths)

    def _view_ptr(self):
        return None


class CorpusView(_Utterances):
    """A list of utterance numbers of a ResidentCorpus (a train or validation subset): ``corpus.split`` and ``subset``
    make them; on the device it is one int32 array, uploaded when an iterator first draws from it."""

    def __init__(self, corpus, utterances):
        self.corpus = corpus
        self.utterances = np.ascontiguousarray(utterances, np.int32)
        self.lengths = corpus.lengths[self.utterances]
        self.speakers = corpus.speakers[self.utterances]
        self._view_dev = None

    @property
    def nbytes(self):
        return 4 * len(self.utterances)

    def _view_ptr(self):
        if self._view_dev is None:
            self._view_dev = backend.to_device(self.utterances)
        return self._view_dev.ptr


def _check_description(lengths, speakers):
    lengths, speakers = list(lengths), list(speakers)
    if not lengths:
        raise ValueError('ResidentCorpus: no waves')
    if len(speakers) != len(lengths):
        raise ValueError('ResidentCorpus: %d speakers for %d waves' % (len(speakers), len(lengths)))
    for i, n in enumerate(lengths):
        if n < 0:
            raise ValueError('ResidentCorpus: wave %d is not a one-dimensional array' % i)
        if n == 0:
            raise ValueError('ResidentCorpus: wave %d is empty' % i)
        if n > 2 ** 31 - 1:
            raise ValueError('ResidentCorpus: wave %d has more than 2**31 - 1 samples' % i)
    try:
        spk = [operator.index(s) for s in speakers]
    except TypeError:
        raise ValueError('ResidentCorpus: speakers must be integers, got %r' % (speakers,))
    if min(spk) < 0 or max(spk) > 2 ** 31 - 1:
        raise ValueError('ResidentCorpus: speaker ids must be in [0, 2**31), got %r' % (speakers,))
    return np.asarray(lengths, np.int32), np.asarray(spk, np.int32)


# --------------------------------------------------------------------------- #
# the iterator
# --------------------------------------------------------------------------- #
class ResidentCorpusIterator(object):
    """Minibatches of ``batch_size`` crops of ``length`` + 1 samples drawn on the device from a ResidentCorpus or a view
    of one.  ``next()`` enqueues one launch on backend.stream() and returns a ``Batch`` whose ``.arrays`` is
    (x_enc (rows, 1, L+1, 1), IndexInput (rows, L), speaker (rows,), t (rows, L, 1)): StreamingInputIterator's tuple, so
    ``converter=lambda b, d: b.arrays`` and both updaters work unchanged.  ``rank`` / ``size``: this iterator yields
    rows rank::size of every global batch (rows = len(range(rank, batch_size, size))).

    ``shuffle``: a new order of the utterances per epoch, else their order in the view.  ``repeat=False``: one pass --
    the last batch holds the rows that are left, the call after it raises StopIteration, ``reset()`` starts over.
    ``iteration`` counts the batches drawn; ``epoch``, ``epoch_detail`` and ``is_new_epoch`` follow Chainer's
    SerialIterator.  ``state_dict()`` / ``load_state_dict()`` resume the order exactly."""

    yields_rank_shard = True
    Batch = StreamingInputIterator.Batch

    def __init__(self, corpus, batch_size, length, seed, shuffle=True, repeat=True, quantize=256, rank=0, size=1):
        if not isinstance(corpus, _Utterances):
            raise TypeError('ResidentCorpusIterator: expected a ResidentCorpus or a view of one, got %r' % type(corpus))
        try:
            seed = operator.index(seed)
        except TypeError:
            raise TypeError('ResidentCorpusIterator: seed must be an integer, got %r' % (seed,))
        if not 0 <= seed < 2 ** 64:
            raise ValueError('ResidentCorpusIterator: seed must be in [0, 2**64), got %r' % (seed,))
        if int(batch_size) < 1 or int(length) < 1:
            raise ValueError('ResidentCorpusIterator: batch_size and length must be at least 1')
        if not 0 <= int(rank) < int(size) or int(size) > int(batch_size):
            raise ValueError('ResidentCorpusIterator: needs 0 <= rank < size <= batch_size, got rank %r, size %r' % (rank, size))
        self.view, self.corpus = corpus, corpus.corpus
        self.batch_size, self.L1, self.seed = int(batch_size), int(length) + 1, seed
        self.shuffle, self.repeat, self.quantize = bool(shuffle), bool(repeat), int(quantize)
        self.rank, self.size = int(rank), int(size)
        self.n_view = len(corpus)
        self.iteration = 0
        self.is_new_epoch = False
        self._thr_host = mulaw_thresholds(self.quantize)
        self._thr = None
        self._desc = None

    # ---- bookkeeping ----
    def _consumed(self, iteration):
        d = iteration * self.batch_size
        return d if self.repeat else min(d, self.n_view)

    def epoch_of(self, iteration):
        """Completed epochs after ``iteration`` batches (LogReport(epoch_of=it.epoch_of))."""
        return self._consumed(int(iteration)) // self.n_view

    @property
    def epoch(self):
        return self.epoch_of(self.iteration)

    @property
    def epoch_detail(self):
        return self._consumed(self.iteration) / float(self.n_view)

    def reset(self):
        self.iteration = 0
        self.is_new_epoch = False

    def state_dict(self):
        return {'seed': self.seed, 'iteration': self.iteration, 'batch_size': self.batch_size, 'n_view': self.n_view}

    def load_state_dict(self, state):
        for k in ('seed', 'batch_size', 'n_view'):
            if int(state[k]) != getattr(self, k):
                raise ValueError('ResidentCorpusIterator.load_state_dict: %s is %r here and %r in the state: another '
                                 'data order' % (k, getattr(self, k), state[k]))
        if int(state['iteration']) < 0:
            raise ValueError('ResidentCorpusIterator.load_state_dict: iteration %r' % (state['iteration'],))
        self.iteration = int(state['iteration'])
        self.is_new_epoch = self.iteration > 0 and self.epoch_of(self.iteration) > self.epoch_of(self.iteration - 1)

    # ---- rows ----
    def _global_rows(self, iteration):
        """Global rows of batch ``iteration`` owned by this rank (empty: the pass is over)."""
        left = self.batch_size if self.repeat else min(self.batch_size, self.n_view - iteration * self.batch_size)
        return range(self.rank, max(left, 0), self.size), max(left, 0)

    def plan(self, iteration=None):
        """Host replay of the rule: int64 (rows, 2) of (utterance, start) per local row of batch ``iteration`` (default:
        the batch the next ``next()`` draws).  Utterance numbers are the corpus's, also through a view."""
        it = self.iteration if iteration is None else int(iteration)
        mine, _ = self._global_rows(it)
        view = None if self.view is self.corpus else self.view.utterances
        return plan_rows(self.seed, it, self.batch_size, self.corpus.lengths, self.L1, self.shuffle, view, list(mine))

    # ---- device ----
    def _descriptor(self):
        if self._desc is None:
            c = self.corpus
            if c.samples is None:
                raise RuntimeError('ResidentCorpusIterator: this corpus is a description only (ResidentCorpus.describe): '
                                   'nothing to draw from')
            d = _lib.Corpus()
            d.samples, d.offset, d.length, d.speaker = c.samples.ptr, c._offset_dev.ptr, c._length_dev.ptr, c._speaker_dev.ptr
            d.view, d.n_view = self.view._view_ptr(), self.n_view
            self._desc = d
            self._thr = backend.to_device(self._thr_host)
        return self._desc

    def draw(self, iteration, record=False):
        """The arrays of batch ``iteration`` (this rank's rows) without moving the iterator.  ``record=True`` also
        returns the device's own (utterance int32 (rows,), start int64 (rows,)), what ``plan`` predicts."""
        mine, left = self._global_rows(int(iteration))
        if left == 0:
            raise StopIteration
        rows = len(mine)
        if rows == 0:
            raise ValueError('ResidentCorpusIterator: the last batch has %d rows, none for rank %d of %d' % (left, self.rank, self.size))
        desc = self._descriptor()
        L1, L = self.L1, self.L1 - 1
        x_enc = DeviceArray((rows, 1, L1, 1), np.float32)
        x_dec = IndexInput((rows, L), self.quantize)
        spk = DeviceArray((rows,), np.int32)
        t = DeviceArray((rows, L, 1), np.int32)
        utt = DeviceArray((rows,), np.int32) if record else None
        start = DeviceArray((rows,), np.int64) if record else None
        _lib.call('vqvae_corpus_draw', C.byref(desc), self.seed, int(self.shuffle), int(iteration), self.batch_size,
                  self.rank, self.size, rows, L1, self._thr.ptr, self._thr.size, x_enc.ptr, x_dec.ptr, t.ptr, spk.ptr,
                  utt.ptr if record else None, start.ptr if record else None, backend.stream())
        arrays = (x_enc, x_dec, spk, t)
        return (arrays, utt, start) if record else arrays

    def next(self):
        arrays = self.draw(self.iteration)           # fresh arrays: the step's Variables may outlive the call
        before = self.epoch_of(self.iteration)
        self.iteration += 1
        self.is_new_epoch = self.epoch_of(self.iteration) > before
        return self.Batch(arrays)

    __next__ = next

    def __iter__(self):
        return self
