"""Speaker identity on the device: one full-covariance Gaussian per enrolled speaker over mel-cepstra and their deltas, for
a ragged list of utterances (csrc/speaker_id.h states the rule, csrc/speaker_id.hip runs it).

    models = fit_speakers(features_many(enrol, cfg), enrol_speakers)     # SpeakerModels: mu, cov, linv, logdet, count
    sc = score_speakers(models, features_many(converted, cfg))           # SpeakerScores: q, ll, identified, count
    sc.llr(targets, sources)                                             # nats per frame: target against source
    sc.accuracy(targets), sc.confusion(targets), sc.rank(targets)
    sc = identify_many(enrol, enrol_speakers, converted, cfg)            # all of it from waves; sc.models
    models = corpus.fit_speakers(cfg)                                    # the corpus's (or the view's) own speakers
    models.divergence()                                                  # (G, G) symmetric KL: how separable the voices are

Whose voice does an utterance sound like?  The classical text-independent answer without a neural model: fit a Gaussian
per speaker over the frames' features and ask under which speaker's Gaussian an utterance's frames are most likely.

What this is and is not.  It is CLOSED-SET identification among the enrolled speakers: ``identified`` is always one of
them, so enrol the corpus's speakers and not just the two a conversion involves.  One Gaussian per speaker: no mixture, no
universal background model, no cepstral mean normalisation, no verification threshold.  NO parity with any toolkit is
claimed or tested.  ``divergence()`` is the scale a log-likelihood ratio is read against.

The device makes the features, the per-utterance sums of x and x x^T, and the mean squared Mahalanobis distance of every
utterance to every model; all of it float64 ``+ - *`` in one written order, so an utterance's results are the same bits
alone, in any list, at any position and for any number of models, and tests/speakerid_ref.py restates them in NumPy.
Everything after the per-utterance sums (the per-speaker sums, mean, covariance, Cholesky factor and its inverse, the
log-likelihoods) is float64 NumPy on the host.

The gate: ``gate_db`` keeps the frames whose summed log-mel energy is within ``gate_db`` decibels (of mean band power) of
the utterance's loudest frame; params.py's ``top_db = 20`` is the value the reference trims silence with.  ``None`` keeps
every frame.

The entry points are declared in csrc/speaker_id.h, which is not under include/, so they are bound here (table,
Structure, revision check) on first use and not in _lib.HEADERS.
"""
import ctypes as C

import numpy as np

from . import _lib, backend, ragged
from .backend import DeviceArray
from .metrics import MelConfig, RaggedFeatures, features_many, tables

_S = backend.stream
MAX_DIM = 48                       # VQVAE_SPK_MAX_DIM
MAX_MELS = 128                     # VQVAE_SPK_MAX_MELS
LANES = 256                        # VQVAE_SPK_LANES
ACC_TILE = 8                       # VQVAE_SPK_ACC_TILE
MODEL_TILE = 8                     # VQVAE_SPK_MODEL_TILE
MAX_MODELS = 524280                # VQVAE_SPK_MAX_MODELS

HEADER = 'speaker_id.h'            # under csrc/
REVISION = 1
P = _lib.P


class SpkDesc(C.Structure):
    _c_name_ = 'vqvae_spk_desc'
    _fields_ = [(n, C.c_int32) for n in ('n', 'n_mels', 'n_mcep', 'deltas', 'dim', 'n_models', 'use_gate', 'reserved')] + \
               [('ftot', C.c_int64), ('stride', C.c_int64), ('thr', C.c_double)]


_D = C.POINTER(SpkDesc)
# the table IS the list of symbols csrc/speaker_id.h declares (tests/test_host_speakerid.py)
PROTOTYPES = {
    'vqvae_spk_revision': (C.c_int, []),
    'vqvae_spk_features': (C.c_int, [_D, P, P, P, P, P, P]),
    'vqvae_spk_stats': (C.c_int, [_D, P, P, P, P, P, P, P]),
    'vqvae_spk_score': (C.c_int, [_D, P, P, P, P, P, P, P, P]),
}
STRUCTS = (SpkDesc,)

_bound = None


def load():
    """libvqvae_hip.so with this header's entry points bound (once); another revision of the header is an ImportError."""
    global _bound
    if _bound is not None:
        return _bound
    lib = _lib.load()
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)               # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    has = lib.vqvae_spk_revision()
    if has != REVISION:
        raise ImportError('libvqvae_hip.so at %s has speaker-identity revision %d, this package binds %d: rebuild it '
                          '(__graft_entry__.build())' % (_lib.LIB_PATH, has, REVISION))
    _bound = lib
    return lib


def call(name, *args):
    """Calls an int-returning entry point of the header and raises _lib.HipError on failure."""
    _lib.check(getattr(load(), name)(*args), name)


# --------------------------------------------------------------------------- #
# the host side of the rule
# --------------------------------------------------------------------------- #
def feature_dim(cfg, deltas=True, who='speaker_features'):
    """D = n_mcep * (1 + deltas); above MAX_DIM is a ValueError."""
    D = cfg.n_mcep * (2 if deltas else 1)
    if D > MAX_DIM:
        raise ValueError('%s: D = %d features a frame (n_mcep = %d%s); at most MAX_DIM = %d (a lane of the score kernel '
                         'keeps a frame in registers)' % (who, D, cfg.n_mcep, ' with deltas' if deltas else '', MAX_DIM))
    return D


def gate_threshold(cfg, gate_db):
    """thr = n_mels * gate_db / 10 * ln 10: ``gate_db`` decibels of every band's power, in the units of the summed natural
    log-mel.  None: no gate."""
    if gate_db is None:
        return None
    g = float(gate_db)
    if not (g >= 0 and np.isfinite(g)):
        raise ValueError('gate_db must be a finite, non-negative number of decibels or None, got %r' % (gate_db,))
    return np.float64(cfg.n_mels) * np.float64(g) / np.float64(10.0) * np.log(np.float64(10.0))


def tri_index(D):
    """(p, q) of every element of the row-major upper triangle, p <= q."""
    return np.triu_indices(int(D))


def pack_lower(linv):
    """(G, D, D) lower-triangular -> (G, D (D + 1) / 2), row-major: [r (r + 1) / 2 + c]."""
    linv = np.asarray(linv, np.float64)
    r, c = np.tril_indices(linv.shape[-1])
    return np.ascontiguousarray(linv[:, r, c])


def _speaker_ids(speakers, n_speakers, N, who):
    """(ids (N,) int64, G); the refusals name the utterance."""
    spk = np.asarray(speakers.get() if backend.is_device(speakers) else speakers)
    if spk.dtype.kind not in 'iu' or spk.ndim != 1 or spk.size != N:
        raise ValueError('%s: one integer speaker id per utterance (%d), got %s %s' % (who, N, spk.dtype, spk.shape))
    spk = spk.astype(np.int64)
    G = int(spk.max()) + 1 if n_speakers is None else int(n_speakers)
    bad = np.nonzero((spk < 0) | (spk >= G))[0]
    if bad.size or G < 1:
        u = int(bad[0]) if bad.size else 0
        raise ValueError('%s: utterance %d has speaker %d; speaker ids must be in [0, %d)' % (who, u, spk[u], G))
    if G > MAX_MODELS:
        raise ValueError('%s: %d speakers; at most %d' % (who, G, MAX_MODELS))
    return spk, G


class RaggedSpeakerFeatures(object):
    """The features of N utterances laid end to end along the frame axis, on the device: ``x`` (Ftot, D) float64, frame f's
    cepstra 1 .. n_mcep and, with ``deltas``, their deltas behind them; ``keep`` (Ftot,) uint8, 1 for a frame the gate
    kept.  ``frames`` (N,), ``frame_off`` (N + 1,), ``cfg``, ``D``, ``deltas`` and ``gate_db`` describe them.  With x None
    it is a description only."""

    def __init__(self, cfg, frames, deltas=True, gate_db=None, x=None, keep=None):
        self.cfg, self.deltas, self.gate_db = cfg, bool(deltas), None if gate_db is None else float(gate_db)
        self.D = cfg.n_mcep * (2 if deltas else 1)
        self.frames = np.asarray(frames, np.int64)
        self.frame_off = ragged.offsets(self.frames, total=True)
        self.x, self.keep = x, keep
        self._host = None
        self._off_dev = None

    def __len__(self):
        return len(self.frames)

    def utterance(self, i):
        """Host copies of utterance i's blocks: (x (F_i, D) float64, keep (F_i,) bool).  The first call copies the whole
        arrays back once."""
        i = int(i)
        if not 0 <= i < len(self.frames):
            raise IndexError('RaggedSpeakerFeatures.utterance: utterance %d of %d' % (i, len(self.frames)))
        if self.x is None:
            raise ValueError('RaggedSpeakerFeatures.utterance: the features are a description only (nothing on the device)')
        if self._host is None:
            self._host = (self.x.get(), self.keep.get())
        a, b = int(self.frame_off[i]), int(self.frame_off[i + 1])
        return self._host[0][a:b].copy(), self._host[1][a:b].astype(bool)

    def _offsets(self):
        if self._off_dev is None:
            self._off_dev = backend.to_device(self.frame_off)
        return self._off_dev

    def _desc(self, n_models=0):
        thr = gate_threshold(self.cfg, self.gate_db)
        ftot = int(self.frame_off[-1])
        return SpkDesc(len(self.frames), self.cfg.n_mels, self.cfg.n_mcep, int(self.deltas), self.D, int(n_models),
                       int(thr is not None), 0, ftot, ftot, 0.0 if thr is None else float(thr))


def _check_feats(feats, who, name='feats'):
    if not isinstance(feats, RaggedFeatures):
        raise TypeError('%s: %s must be a metrics.RaggedFeatures (features_many), got %r' % (who, name, type(feats)))
    if feats.cfg.n_mels > MAX_MELS:
        raise ValueError('%s: n_mels must be at most %d, got %d' % (who, MAX_MELS, feats.cfg.n_mels))


def speaker_features(feats, deltas=True, gate_db=None):
    """Cepstra, deltas and the energy gate of every frame of ``feats`` (metrics.RaggedFeatures from features_many), read in
    place: a RaggedSpeakerFeatures.  One launch.  ``deltas``: append 0.5 (c[f + 1] - c[f - 1]), the edges of an utterance
    replicated (D = 2 n_mcep, else n_mcep).  ``gate_db``: keep the frames within that many decibels of the utterance's
    loudest (see the module docstring; None keeps every frame).  D above MAX_DIM, or features that are a description
    only, are a ValueError raised before any device call."""
    who = 'speaker_features'
    _check_feats(feats, who)
    cfg = feats.cfg
    feature_dim(cfg, deltas, who)
    gate_threshold(cfg, gate_db)
    if feats.log_mel is None:
        raise ValueError('%s: the features are a description only (nothing on the device)' % who)
    sf = RaggedSpeakerFeatures(cfg, feats.frames, deltas, gate_db)
    ftot = int(sf.frame_off[-1])
    dct = backend.to_device(tables(cfg)[2])
    sf.x, sf.keep = DeviceArray((ftot, sf.D), np.float64), DeviceArray((ftot,), np.uint8)
    d = sf._desc()
    call('vqvae_spk_features', C.byref(d), feats.log_mel.ptr, dct.ptr, sf._offsets().ptr, sf.x.ptr, sf.keep.ptr, _S())
    del dct
    return sf


def _as_speaker_features(feats_or_sf, deltas, gate_db, who):
    if isinstance(feats_or_sf, RaggedSpeakerFeatures):
        if feats_or_sf.x is None:
            raise ValueError('%s: the features are a description only (nothing on the device)' % who)
        return feats_or_sf
    _check_feats(feats_or_sf, who, 'feats_or_sf')
    return speaker_features(feats_or_sf, deltas, gate_db)


def speaker_stats(sf):
    """The per-utterance statistics of a RaggedSpeakerFeatures, from the device (one launch), as host arrays:
    (cnt (N,) int64, s1 (N, D), s2 (N, D (D + 1) / 2): the sums of x and of the upper triangle of x x^T over the kept
    frames, in the rule's lane order)."""
    who = 'speaker_stats'
    if not isinstance(sf, RaggedSpeakerFeatures):
        raise TypeError('%s: sf must be a RaggedSpeakerFeatures (speaker_features), got %r' % (who, type(sf)))
    if sf.x is None:
        raise ValueError('%s: the features are a description only (nothing on the device)' % who)
    N, D = len(sf), sf.D
    T = D * (D + 1) // 2
    s1, s2, cnt = DeviceArray((N, D), np.float64), DeviceArray((N, T), np.float64), DeviceArray((N,), np.int64)
    d = sf._desc()
    call('vqvae_spk_stats', C.byref(d), sf.x.ptr, sf.keep.ptr, sf._offsets().ptr, s1.ptr, s2.ptr, cnt.ptr, _S())
    return cnt.get(), s1.get(), s2.get()


# --------------------------------------------------------------------------- #
# models
# --------------------------------------------------------------------------- #
class SpeakerModels(object):
    """G Gaussians.  The raw sums -- ``count`` (G,) int64 kept frames, ``S1`` (G, D), ``S2`` (G, D (D + 1) / 2) upper
    triangle -- and what the host derives from them in float64: ``mu`` (G, D), ``cov`` (G, D, D) = S2 / n - mu mu^T
    (+ ridge * trace(cov) / D * I), ``L`` = cholesky(cov), ``linv`` = inv(L) (lower), ``logdet`` (G,) = log det cov.
    ``cfg_key``, ``deltas``, ``gate_db``, ``D`` and ``ridge`` say what they were fitted on.  One Gaussian per speaker: no
    mixture, no background model; closed-set by construction."""

    def __init__(self, cfg_key, deltas, gate_db, ridge, count, S1, S2):
        self.cfg_key, self.deltas = tuple(cfg_key), bool(deltas)
        self.gate_db, self.ridge = None if gate_db is None else float(gate_db), float(ridge)
        self.count = np.asarray(count, np.int64)
        self.S1, self.S2 = np.asarray(S1, np.float64), np.asarray(S2, np.float64)
        self.G, self.D = self.S1.shape
        self._derive()

    def __len__(self):
        return self.G

    def _derive(self):
        G, D = self.G, self.D
        few = np.nonzero(self.count <= D)[0]
        if few.size:
            g = int(few[0])
            raise ValueError('fit_speakers: speaker %d has %d kept frames; a %d-dimensional covariance needs more than %d '
                             '(enrol more speech of that speaker, or fewer coefficients)' % (g, self.count[g], D, D))
        p, q = tri_index(D)
        n = self.count.astype(np.float64)
        self.mu = self.S1 / n[:, None]
        full = np.zeros((G, D, D), np.float64)
        full[:, p, q] = self.S2
        full[:, q, p] = self.S2
        self.cov = full / n[:, None, None] - self.mu[:, :, None] * self.mu[:, None, :]
        if self.ridge:
            scale = self.ridge * np.trace(self.cov, axis1=1, axis2=2) / D
            self.cov = self.cov + scale[:, None, None] * np.eye(D)[None]
        self.L = np.zeros((G, D, D), np.float64)
        self.linv = np.zeros((G, D, D), np.float64)
        for g in range(G):
            try:
                if not np.isfinite(self.cov[g]).all():
                    raise np.linalg.LinAlgError('not finite')
                self.L[g] = np.linalg.cholesky(self.cov[g])
                self.linv[g] = np.tril(np.linalg.inv(self.L[g]))
            except np.linalg.LinAlgError:
                raise ValueError('fit_speakers: the covariance of speaker %d (%d kept frames, D = %d) is not positive '
                                 'definite: ask for ridge=1e-6 or more, or enrol more speech' % (g, self.count[g], D))
        self.logdet = 2.0 * np.log(np.diagonal(self.L, axis1=1, axis2=2)).sum(axis=1)

    def divergence(self):
        """(G, G) symmetric Kullback-Leibler divergence between the Gaussians in nats, closed form on the host:
        J(a, b) = KL(a || b) + KL(b || a) = 0.5 (tr(Sb^-1 Sa) + tr(Sa^-1 Sb)) - D + 0.5 (ma - mb)^T (Sa^-1 + Sb^-1) (ma - mb).
        0 on the diagonal.  It tells how separable two voices are at all."""
        G, D = self.G, self.D
        prec = np.einsum('gkr,gkc->grc', self.linv, self.linv)          # Sigma^-1 = linv^T linv
        out = np.zeros((G, G), np.float64)
        for a in range(G):
            for b in range(a + 1, G):
                dm = self.mu[a] - self.mu[b]
                j = 0.5 * (np.trace(prec[b].dot(self.cov[a])) + np.trace(prec[a].dot(self.cov[b]))) - D \
                    + 0.5 * dm.dot((prec[a] + prec[b]).dot(dm))
                out[a, b] = out[b, a] = j
        return out

    def save(self, path):
        """Everything, derived arrays included (another LAPACK need not give linv the same bits), as one .npz."""
        np.savez(path, cfg_key=np.array(self.cfg_key, np.float64), deltas=self.deltas, ridge=self.ridge,
                 gate_db=np.nan if self.gate_db is None else self.gate_db, count=self.count, S1=self.S1, S2=self.S2,
                 mu=self.mu, cov=self.cov, L=self.L, linv=self.linv, logdet=self.logdet)

    @classmethod
    def load(cls, path):
        with np.load(path if str(path).endswith('.npz') else str(path) + '.npz') as z:
            key = z['cfg_key']
            cfg_key = tuple(int(v) if i in (0, 1, 2, 3, 6) else float(v) for i, v in enumerate(key))
            gate = float(z['gate_db'])
            m = cls(cfg_key, bool(z['deltas']), None if np.isnan(gate) else gate, float(z['ridge']), z['count'], z['S1'], z['S2'])
            for name in ('mu', 'cov', 'L', 'linv', 'logdet'):           # the saved bits, not this machine's LAPACK's
                setattr(m, name, z[name].copy())
        return m


def models_from_stats(cfg, cnt, s1, s2, speakers, n_speakers=None, deltas=True, gate_db=None, ridge=0.0, accumulate=None):
    """The host half of fit_speakers: per-utterance statistics (speaker_stats' result, or the restatement's) to
    SpeakerModels.  The per-speaker sums are taken in list order, each started from 0.0 or from ``accumulate``'s."""
    who = 'fit_speakers'
    cnt, s1, s2 = np.asarray(cnt, np.int64), np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    N, D = s1.shape
    spk, G = _speaker_ids(speakers, n_speakers if accumulate is None or n_speakers is not None else accumulate.G, N, who)
    if not (float(ridge) >= 0 and np.isfinite(float(ridge))):
        raise ValueError('%s: ridge must be finite and not negative, got %r' % (who, ridge))
    if D != feature_dim(cfg, deltas, who) or s2.shape != (N, D * (D + 1) // 2) or cnt.shape != (N,):
        raise ValueError('%s: statistics of shapes %s, %s, %s are not those of D = %d' % (who, cnt.shape, s1.shape, s2.shape,
                                                                                           cfg.n_mcep * (2 if deltas else 1)))
    if accumulate is not None:
        if not isinstance(accumulate, SpeakerModels):
            raise TypeError('%s: accumulate must be a SpeakerModels, got %r' % (who, type(accumulate)))
        _same_analysis(who, accumulate, cfg, deltas, D, gate_db)
        if accumulate.G != G:
            raise ValueError('%s: accumulate has %d speakers, this call %d' % (who, accumulate.G, G))
        C0, S1, S2 = accumulate.count.copy(), accumulate.S1.copy(), accumulate.S2.copy()
    else:
        C0, S1, S2 = np.zeros(G, np.int64), np.zeros((G, D), np.float64), np.zeros((G, D * (D + 1) // 2), np.float64)
    for i in range(N):                                          # list order: one addition per utterance and accumulator
        g = spk[i]
        C0[g] += cnt[i]
        S1[g] = S1[g] + s1[i]
        S2[g] = S2[g] + s2[i]
    return SpeakerModels(cfg.key(), deltas, gate_db, ridge, C0, S1, S2)


def _same_analysis(who, models, cfg, deltas, D, gate_db=Ellipsis):
    if tuple(models.cfg_key) != tuple(cfg.key()):
        raise ValueError('%s: the models were fitted on another analysis: MelConfig key %r against %r'
                         % (who, tuple(models.cfg_key), tuple(cfg.key())))
    if models.deltas != bool(deltas) or models.D != D:
        raise ValueError('%s: the models have deltas = %r and D = %d, the features deltas = %r and D = %d'
                         % (who, models.deltas, models.D, bool(deltas), D))
    if gate_db is not Ellipsis and models.gate_db != (None if gate_db is None else float(gate_db)):
        raise ValueError('%s: the models were fitted with gate_db = %r, this call has %r' % (who, models.gate_db, gate_db))


def fit_speakers(feats_or_sf, speakers, n_speakers=None, deltas=True, gate_db=None, ridge=0.0, accumulate=None):
    """One full-covariance Gaussian per speaker over the kept frames of the utterances: a SpeakerModels.
    ``feats_or_sf``: metrics.RaggedFeatures (then ``deltas`` and ``gate_db`` make the features) or a RaggedSpeakerFeatures
    (its own hold).  ``speakers``: one int per utterance in [0, n_speakers) (default: the largest id + 1).  The
    per-utterance sums come from the device; everything after them is host float64.  ``ridge``: adds
    ridge * trace(cov) / D to the diagonal.  ``accumulate``: an earlier SpeakerModels whose raw sums this call continues,
    so a corpus can be fitted in parts.  A speaker with no more than D kept frames, or a covariance that is not positive
    definite, is a ValueError naming the speaker.  Closed-set: enrol every speaker of the corpus."""
    who = 'fit_speakers'
    if isinstance(feats_or_sf, RaggedSpeakerFeatures):
        deltas, gate_db = feats_or_sf.deltas, feats_or_sf.gate_db
    elif not isinstance(feats_or_sf, RaggedFeatures):
        raise TypeError('%s: feats_or_sf must be a metrics.RaggedFeatures or a RaggedSpeakerFeatures, got %r' % (who, type(feats_or_sf)))
    cfg = feats_or_sf.cfg
    D = feature_dim(cfg, deltas, who)
    _, G = _speaker_ids(speakers, n_speakers if accumulate is None or n_speakers is not None else accumulate.G,
                        len(feats_or_sf), who)
    if not (float(ridge) >= 0 and np.isfinite(float(ridge))):
        raise ValueError('%s: ridge must be finite and not negative, got %r' % (who, ridge))
    if accumulate is not None:
        if not isinstance(accumulate, SpeakerModels):
            raise TypeError('%s: accumulate must be a SpeakerModels, got %r' % (who, type(accumulate)))
        _same_analysis(who, accumulate, cfg, deltas, D, gate_db)
        if accumulate.G != G:
            raise ValueError('%s: accumulate has %d speakers, this call %d' % (who, accumulate.G, G))
    sf = _as_speaker_features(feats_or_sf, deltas, gate_db, who)
    cnt, s1, s2 = speaker_stats(sf)
    return models_from_stats(cfg, cnt, s1, s2, speakers, G, deltas, gate_db, ridge, accumulate)


# --------------------------------------------------------------------------- #
# scores
# --------------------------------------------------------------------------- #
class SpeakerScores(object):
    """Per utterance, in the caller's order: ``q`` (N, G) float64, the mean squared Mahalanobis distance of the kept
    frames to every model (from the device); ``count`` (N,) int64 kept frames; ``ll`` (N, G) =
    -0.5 (q + logdet + D ln 2 pi), the mean log-likelihood of a frame in nats; ``identified`` (N,), the arg-max of ll,
    ties to the lowest id.  Closed-set: ``identified`` is always an enrolled speaker."""

    def __init__(self, q, count, logdet, D, models=None):
        self.q, self.count = np.asarray(q, np.float64), np.asarray(count, np.int64)
        self.logdet, self.D, self.models = np.asarray(logdet, np.float64), int(D), models
        self.N, self.G = self.q.shape
        self.ll = -0.5 * (self.q + self.logdet[None, :] + self.D * np.log(2.0 * np.pi))
        self.identified = np.argmax(self.ll, axis=1).astype(np.int64)       # the first of equal maxima

    def __len__(self):
        return self.N

    def _ids(self, ids, name):
        v = np.asarray(ids)
        if v.dtype.kind not in 'iu' or v.shape != (self.N,):
            raise ValueError('SpeakerScores: %s must be one integer speaker id per utterance (%d), got %s %s'
                             % (name, self.N, v.dtype, v.shape))
        v = v.astype(np.int64)
        bad = np.nonzero((v < 0) | (v >= self.G))[0]
        if bad.size:
            raise ValueError('SpeakerScores: utterance %d has %s %d; speaker ids must be in [0, %d)'
                             % (bad[0], name, v[bad[0]], self.G))
        return v

    def rank(self, targets):
        """(N,) int64: how many models score strictly higher than the target's, plus those of a lower id that tie: 0 when
        the target is identified."""
        t = self._ids(targets, 'targets')
        own = self.ll[np.arange(self.N), t][:, None]
        ids = np.arange(self.G)[None, :]
        return ((self.ll > own) | ((self.ll == own) & (ids < t[:, None]))).sum(axis=1).astype(np.int64)

    def llr(self, targets, sources=None):
        """(N,) float64, nats per frame: ll under the target's model minus ll under the source's; ``sources=None``: minus
        the best of the OTHER models (the runner-up when the target is identified; NaN with a single model)."""
        t = self._ids(targets, 'targets')
        own = self.ll[np.arange(self.N), t]
        if sources is not None:
            return own - self.ll[np.arange(self.N), self._ids(sources, 'sources')]
        if self.G < 2:
            return np.full(self.N, np.nan)
        rest = self.ll.copy()
        rest[np.arange(self.N), t] = -np.inf
        return own - rest.max(axis=1)

    def accuracy(self, targets):
        return float(np.mean(self.identified == self._ids(targets, 'targets')))

    def confusion(self, targets):
        """(G, G) int64: [t, g] utterances of target t identified as g."""
        t = self._ids(targets, 'targets')
        out = np.zeros((self.G, self.G), np.int64)
        np.add.at(out, (t, self.identified), 1)
        return out


def score_speakers(models, feats_or_sf, gate_db=None):
    """Every utterance against every model, one launch: a SpeakerScores.  ``feats_or_sf``: metrics.RaggedFeatures (the
    features are made as the models' were: their ``deltas``, and ``gate_db`` -- None: the models' own gate) or a
    RaggedSpeakerFeatures.  Models and features of another MelConfig, ``deltas`` or D are a ValueError raised before any
    device call, as are features that are a description only."""
    who = 'score_speakers'
    if not isinstance(models, SpeakerModels):
        raise TypeError('%s: models must be a SpeakerModels (fit_speakers), got %r' % (who, type(models)))
    if isinstance(feats_or_sf, RaggedSpeakerFeatures):
        deltas, D = feats_or_sf.deltas, feats_or_sf.D
    elif isinstance(feats_or_sf, RaggedFeatures):
        deltas, D = models.deltas, feats_or_sf.cfg.n_mcep * (2 if models.deltas else 1)
        gate_db = models.gate_db if gate_db is None else gate_db
    else:
        raise TypeError('%s: feats_or_sf must be a metrics.RaggedFeatures or a RaggedSpeakerFeatures, got %r' % (who, type(feats_or_sf)))
    _same_analysis(who, models, feats_or_sf.cfg, deltas, D)
    feature_dim(feats_or_sf.cfg, deltas, who)
    if models.G > MAX_MODELS:
        raise ValueError('%s: %d models; at most %d' % (who, models.G, MAX_MODELS))
    sf = _as_speaker_features(feats_or_sf, deltas, gate_db, who)
    q, cnt = score_raw(sf, models.mu, pack_lower(models.linv))
    return SpeakerScores(q, cnt, models.logdet, models.D, models)


def score_raw(sf, mu, linv_packed):
    """The device call of score_speakers: host (q (N, G), cnt (N,)) for host ``mu`` (G, D) and packed ``linv``
    (G, D (D + 1) / 2)."""
    N, D = len(sf), sf.D
    mu, lp = np.ascontiguousarray(mu, np.float64), np.ascontiguousarray(linv_packed, np.float64)
    G = mu.shape[0]
    if mu.shape != (G, D) or lp.shape != (G, D * (D + 1) // 2) or G < 1:
        raise ValueError('score_speakers: mu %s and packed linv %s are not those of G models of D = %d' % (mu.shape, lp.shape, D))
    mu_d, lp_d = backend.to_device(mu), backend.to_device(lp)
    q, cnt = DeviceArray((N, G), np.float64), DeviceArray((N,), np.int64)
    d = sf._desc(G)
    call('vqvae_spk_score', C.byref(d), sf.x.ptr, sf.keep.ptr, sf._offsets().ptr, mu_d.ptr, lp_d.ptr, q.ptr, cnt.ptr, _S())
    out = q.get(), cnt.get()
    del mu_d, lp_d
    return out


def identify_many(enrol_waves, enrol_speakers, test_waves, cfg, n_speakers=None, deltas=True, gate_db=None, ridge=0.0,
                  chunk_bytes=1 << 30):
    """``features_many`` on both sides, ``fit_speakers`` on the enrolment, ``score_speakers`` on the test utterances: a
    SpeakerScores whose ``models`` are the fitted ones.  Both wave arguments take what ``features_many`` takes -- host or
    device lists, a ResidentCorpus / CorpusView read in place.  Closed-set: enrol every speaker of the corpus."""
    who = 'identify_many'
    if not isinstance(cfg, MelConfig):
        raise TypeError('%s: cfg must be a MelConfig, got %r' % (who, type(cfg)))
    feature_dim(cfg, deltas, who)
    gate_threshold(cfg, gate_db)
    lengths, _ = ragged.wave_source(enrol_waves, who)
    _speaker_ids(enrol_speakers, n_speakers, len(lengths), who)
    ragged.wave_source(test_waves, who)
    models = fit_speakers(features_many(enrol_waves, cfg, chunk_bytes=chunk_bytes), enrol_speakers, n_speakers, deltas,
                          gate_db, ridge)
    return score_speakers(models, features_many(test_waves, cfg, chunk_bytes=chunk_bytes))
