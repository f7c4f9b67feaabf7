"""ABX discriminability on the device: DTW distances between many short items -- phones or words cut out of utterances --
over arbitrary frame features, and the ABX error they give (csrc/abx.h states the rule, csrc/abx.hip runs it).

    fr = Frames.from_latents(latents)               # list of (D, tl_i) float32, host or device
    fr = Frames.from_features(feats)                # metrics.RaggedFeatures: its log_mel read in place
    fr = Frames.from_codes(codes, vq)               # frontend.LatentCodes (also seg.codes[p]) + the codebook
    items = Items(utterance, start, stop, label, speaker=None, context=None)    # frames [start, stop) of an utterance
    pd = pair_distances(fr, items, ia, ib)          # PairDistances: distance, cost, path_len of the ORDERED pairs
    plan = plan_abx(items)                          # ABXPlan: unique ordered pairs, triples, groups
    sc = abx(fr, items)                             # ABXScores
    sc = abx_many(encoder, vq, waves, items, what='codes')      # front end + abx, nothing to the host in between
    sc = corpus.abx(encoder, vq, items)             # a ResidentCorpus / CorpusView read in place
    table = code_table(vq, 'cosine')                # (k, k) float64 on the device: the local cost of codebook rows

For items A and X of one category and B of another, ABX asks how often X lies nearer to B than to A.  The distance is a
DTW distance over frame features: the summed local cost along the best monotone path divided by the path's length.  The
local cost is ``cosine`` -- 1 - dot / sqrt(|a|^2 |b|^2), clamped at 0, and 1.0 against a zero frame -- or ``euclidean``.
The angular form speech toolkits use needs acos, which has no bit-exact counterpart here, so it is left out.  With
segmental.segment_many trading rate away, this measures what the trade costs: the same items over the encoder's latents,
over the codes of every penalty, and over log-mel as the baseline.

The codes form keeps the int32 codes and a (k, k) float64 table; the local cost of two frames is table[ca, cb].
``code_table`` applies the dense rule to the codebook's rows, so the codes form gives the same bits as the dense form over
the gathered rows W[codes]; a caller may pass a table of its own.

Pairs are ORDERED: the recurrence breaks exact ties by a fixed candidate order, so swapping the sides of a pair can change
the path length on a tie, and the plan never swaps them.  All arithmetic is float64 in one written order, so a pair's
distance, cost and path length are the same bits alone, in any list, at any position and for any ``chunk_bytes``;
tests/abx_ref.py restates them in NumPy.  The triples, their scores and the means are host work in float64 and integers.

What this is not: no parity with any toolkit is claimed (task definitions, the handling of ties and the averaging differ
between them); no angular distance, no KL; no band or slope constraint in the DTW.  The reference has no counterpart.

The entry points are declared in csrc/abx.h, which is not under include/, so they are bound here (table, Structures,
revision check) on first use and not in _lib.HEADERS.
"""
import ctypes as C

import numpy as np

from . import _lib, backend, ragged
from .backend import DeviceArray

_S = backend.stream
MAX_D = 4096                       # VQVAE_ABX_MAX_D
MAX_K = 8192                       # VQVAE_ABX_MAX_K
WAVE_SHORT = 64                    # VQVAE_ABX_WAVE_SHORT
MAX_SHORT = 1024                   # VQVAE_ABX_MAX_SHORT
LANES = 256                        # VQVAE_ABX_LANES
TILE = 16                          # VQVAE_ABX_TILE
MAX_CELLS = 1 << 31                # the local-cost table of ONE pair
METRICS = {'cosine': 0, 'euclidean': 1}      # VQVAE_ABX_COSINE, VQVAE_ABX_EUCLIDEAN
DENSE, CODES = 0, 1                # VQVAE_ABX_DENSE, VQVAE_ABX_CODES

HEADER = 'abx.h'                   # under csrc/
REVISION = 1
P = _lib.P


class AbxDesc(C.Structure):
    _c_name_ = 'vqvae_abx_desc'
    _fields_ = [(n, C.c_int32) for n in ('n', 'd', 'metric', 'form', 'k', 'max_short')] + \
               [(n, C.c_int64) for n in ('ftot_a', 'ftot_b', 'stride_a', 'stride_b', 'cells')]


class AbxTables(C.Structure):
    _c_name_ = 'vqvae_abx_tables'
    _fields_ = [(n, P) for n in ('a_start', 'b_start', 'a_len', 'b_len', 'cell_off')]


_D = C.POINTER(AbxDesc)
_T = C.POINTER(AbxTables)
# the table IS the list of symbols csrc/abx.h declares (tests/test_host_abx.py)
PROTOTYPES = {
    'vqvae_abx_revision': (C.c_int, []),
    'vqvae_abx_workspace_bytes': (C.c_size_t, [_D]),
    'vqvae_abx_norms': (C.c_int, [_D, C.c_int, P, P, P]),
    'vqvae_abx_local': (C.c_int, [_D, _T, P, P, P, P, P, P, C.c_size_t, P]),
    'vqvae_abx_dtw': (C.c_int, [_D, _T, P, C.c_size_t, P, P, P, P]),
    'vqvae_abx_table_workspace_bytes': (C.c_size_t, [C.c_int32]),
    'vqvae_abx_table': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, P, P, P, C.c_size_t, P]),
}
STRUCTS = (AbxDesc, AbxTables)

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
    has = lib.vqvae_abx_revision()
    if has != REVISION:
        raise ImportError('libvqvae_hip.so at %s has abx revision %d, this package binds %d: rebuild it '
                          '(__graft_entry__.build())' % (_lib.LIB_PATH, has, REVISION))
    _bound = lib
    return lib


def call(name, *args):
    """Calls an int-returning entry point of the header and raises _lib.HipError on failure."""
    _lib.check(getattr(load(), name)(*args), name)


# --------------------------------------------------------------------------- #
# argument checks and the planner of the device calls
# --------------------------------------------------------------------------- #
def check_metric(metric, who='pair_distances'):
    if metric not in METRICS:
        raise ValueError('%s: unknown metric %r; one of %s (the angular form needs acos, which has no bit-exact '
                         'counterpart here)' % (who, metric, ', '.join(sorted(METRICS))))
    return METRICS[metric]


def _ints(x, name, who):
    a = np.asarray(x)
    if a.dtype.kind not in 'iu' or a.ndim != 1:
        raise TypeError('%s: %s must be a flat integer array, got %s %s' % (who, name, a.dtype, a.shape))
    return a.astype(np.int64)


def check_pairs(frames_a, frames_b, who='pair_distances'):
    """(Fa, Fb) as int64 (n,) arrays; the refusals, each a ValueError naming the pair: another count on the two sides, an
    empty side, a shorter side above MAX_SHORT, more than 2^31 cells."""
    fa = np.asarray(frames_a, np.int64).reshape(-1)
    fb = np.asarray(frames_b, np.int64).reshape(-1)
    if fa.size != fb.size:
        raise ValueError('%s: %d items on side a and %d on side b' % (who, fa.size, fb.size))
    if fa.size == 0:
        raise ValueError('%s: no pairs' % who)
    empty = np.nonzero((fa < 1) | (fb < 1))[0]
    if empty.size:
        u = int(empty[0])
        raise ValueError('%s: pair %d has %d and %d frames: every side needs one' % (who, u, fa[u], fb[u]))
    long_ = np.nonzero(np.minimum(fa, fb) > MAX_SHORT)[0]
    if long_.size:
        u = int(long_[0])
        raise ValueError('%s: pair %d has %d and %d frames; the shorter side may have at most MAX_SHORT = %d: align whole '
                         'utterances with align_many' % (who, u, fa[u], fb[u], MAX_SHORT))
    big = np.nonzero(fa * fb > MAX_CELLS)[0]
    if big.size:
        u = int(big[0])
        raise ValueError('%s: pair %d has %d x %d = %d cells; one pair may have at most 2^31' % (who, u, fa[u], fb[u], fa[u] * fb[u]))
    return fa, fb


def plan_chunks(cells, chunk_bytes, who='pair_distances'):
    """Runs [(start, stop), ...] of consecutive pairs whose local-cost tables -- 8 bytes per cell -- stay within
    ``chunk_bytes`` together; a pair over the budget stands alone."""
    if int(chunk_bytes) < 1:
        raise ValueError('%s: chunk_bytes must be positive, got %r' % (who, chunk_bytes))
    cum = np.cumsum(8 * np.asarray(cells, np.int64).reshape(-1), dtype=np.int64)
    runs, start, base = [], 0, 0
    while start < cum.size:
        stop = max(int(np.searchsorted(cum, base + int(chunk_bytes), side='right')), start + 1)
        runs.append((start, stop))
        start, base = stop, int(cum[stop - 1])
    return runs


# --------------------------------------------------------------------------- #
# the features and the items
# --------------------------------------------------------------------------- #
class Frames(object):
    """The frame features of N utterances laid end to end.  Dense form: ``x`` one channel-major (d, stride) float32 device
    buffer, ``d`` in [1, MAX_D].  Codes form: ``codes`` a LatentCodes and a (k, k) float64 table per metric.  ``tl`` (N,)
    frames per utterance, ``offsets`` (N + 1,) int64, ``total`` their sum."""

    def __init__(self, tl, x=None, d=0, stride=0, codes=None, W=None, table=None):
        self.tl = ragged.check_lengths(np.asarray(tl).astype(np.int64), 'Frames')
        self.offsets = ragged.offsets(self.tl, total=True)
        self.total = int(self.offsets[-1])
        self.form = DENSE if codes is None else CODES
        self.x, self.d, self.stride = x, int(d), int(stride)
        self.codes, self.W, self._own_table = codes, W, table
        self.k = 0 if codes is None else codes.k
        self._norms, self._tables = None, {}

    def __len__(self):
        return len(self.tl)

    @classmethod
    def from_latents(cls, latents):
        """From a list of (D, tl_i) float32 arrays, host or device: what ``encode_many(return_latents=True)`` hands back
        and ``segment_latents`` takes.  They are laid end to end in one (D, total) device buffer."""
        from .segmental import _gather
        who = 'Frames.from_latents'
        latents = list(latents)
        if not latents:
            raise ValueError('%s: no utterances' % who)
        d = None
        for i, z in enumerate(latents):
            if not backend.is_device(z):
                z = latents[i] = np.asarray(z)
            if z.dtype != np.float32:
                raise ValueError('%s: the features of utterance %d are %s, float32 needed' % (who, i, z.dtype))
            if len(z.shape) != 2 or z.shape[1] < 1:
                raise ValueError('%s: the features of utterance %d have shape %s; (D, frames) with a frame needed'
                                 % (who, i, tuple(z.shape)))
            d = z.shape[0] if d is None else d
            if z.shape[0] != d:
                raise ValueError('%s: utterance %d has D = %d, utterance 0 has D = %d' % (who, i, z.shape[0], d))
        if not 1 <= d <= MAX_D:
            raise ValueError('%s: D = %d; it must be in [1, MAX_D = %d]' % (who, d, MAX_D))
        tl = np.array([z.shape[1] for z in latents], np.int64)
        T = int(tl.sum())
        return cls(tl, x=_gather(latents, d, T), d=d, stride=T)

    @classmethod
    def from_features(cls, feats):
        """From a metrics.RaggedFeatures: its log_mel (n_mels, stride) is read in place."""
        from .metrics import RaggedFeatures
        who = 'Frames.from_features'
        if not isinstance(feats, RaggedFeatures):
            raise TypeError('%s: a metrics.RaggedFeatures is needed, got %r' % (who, type(feats)))
        x = feats.log_mel
        if not backend.is_device(x) or x.dtype != np.float32 or x.ndim != 2:
            raise ValueError('%s: log_mel must be a (n_mels, frames) float32 device array' % who)
        if not 1 <= x.shape[0] <= MAX_D:
            raise ValueError('%s: D = %d; it must be in [1, MAX_D = %d]' % (who, x.shape[0], MAX_D))
        if int(feats.frame_off[-1]) > x.shape[1]:
            raise ValueError('%s: %d frames in a buffer of %d' % (who, int(feats.frame_off[-1]), x.shape[1]))
        return cls(feats.frames, x=x, d=x.shape[0], stride=x.shape[1])

    @classmethod
    def from_codes(cls, codes, vq=None, table=None):
        """From a LatentCodes and the codebook (``code_table`` of the call's metric is the table, computed on first use),
        or a ``table`` of the caller's own: (k, k) float64, host or device, finite and not negative."""
        from .frontend import LatentCodes
        who = 'Frames.from_codes'
        if not isinstance(codes, LatentCodes):
            raise TypeError('%s: codes must be a LatentCodes, got %r' % (who, type(codes)))
        if not 1 <= codes.k <= MAX_K:
            raise ValueError('%s: k = %d codes; at most MAX_K = %d' % (who, codes.k, MAX_K))
        if table is not None:
            host = table.get() if backend.is_device(table) else np.asarray(table)
            if host.dtype != np.float64 or host.shape != (codes.k, codes.k):
                raise ValueError('%s: the table must be (k, k) = (%d, %d) float64, got %s %s'
                                 % (who, codes.k, codes.k, host.dtype, host.shape))
            bad = np.argwhere(~(np.isfinite(host) & (host >= 0)))
            if bad.size:
                r, c = int(bad[0][0]), int(bad[0][1])
                raise ValueError('%s: table[%d, %d] is %r; every entry must be finite and not negative' % (who, r, c, float(host[r, c])))
            if not backend.is_device(table):
                table = backend.to_device(np.ascontiguousarray(host))
            return cls(codes.tl, codes=codes, table=table)
        if vq is None:
            raise ValueError('%s: the codebook or a table is needed' % who)
        W = _codebook(vq, who)
        if W.shape[0] != codes.k:
            raise ValueError('%s: the codes were taken from a codebook of k = %d, this one has k = %d' % (who, codes.k, W.shape[0]))
        return cls(codes.tl, codes=codes, W=W)

    def norms(self):
        """(total,) float64 on the device: step 1 of the rule over the whole buffer, computed once."""
        if self._norms is None:
            d = AbxDesc()
            d.n, d.d, d.metric, d.form, d.max_short = 1, self.d, 0, DENSE, 1
            d.ftot_a = d.ftot_b = d.cells = self.total
            d.stride_a = d.stride_b = self.stride
            out = DeviceArray((self.total,), np.float64)
            call('vqvae_abx_norms', C.byref(d), 0, self.x.ptr, out.ptr, _S())
            self._norms = out
        return self._norms

    def table(self, metric):
        """The (k, k) float64 device table of the codes form: the caller's own, or ``code_table`` of the metric."""
        if self._own_table is not None:
            return self._own_table
        if metric not in self._tables:
            self._tables[metric] = _table_of(self.W, metric)
        return self._tables[metric]

    def pointer(self):
        return self.x.ptr if self.form == DENSE else self.codes.indices.ptr


def _codebook(vq, who):
    from .frontend import _codebook as device_codebook
    W = device_codebook(vq, who)
    if W.dtype != np.float32 or W.ndim != 2:
        raise ValueError('%s: the codebook must be (k, d) float32, got %s %s' % (who, W.dtype, W.shape))
    if not 1 <= W.shape[0] <= MAX_K:
        raise ValueError('%s: k = %d codes; at most MAX_K = %d' % (who, W.shape[0], MAX_K))
    if not 1 <= W.shape[1] <= MAX_D:
        raise ValueError('%s: D = %d; it must be in [1, MAX_D = %d]' % (who, W.shape[1], MAX_D))
    return W


def _table_of(W, metric):
    k, d = W.shape
    lib = load()
    need = lib.vqvae_abx_table_workspace_bytes(k)
    ws = backend.workspace(need)
    table = DeviceArray((k, k), np.float64)
    call('vqvae_abx_table', k, d, METRICS[metric], W.ptr, table.ptr, ws.ptr, need, _S())
    return table


def code_table(vq, metric='cosine'):
    """The (k, k) float64 table of the codes form, on the device: the dense rule's local cost of codebook row against
    codebook row (steps 1 and 2 of the rule alone)."""
    check_metric(metric, 'code_table')
    return _table_of(_codebook(vq, 'code_table'), metric)


class Items(object):
    """M items: item m is the frames [start[m], stop[m]) of utterance ``utterance[m]``, with a ``label`` (the category) and,
    where the task needs them, a ``speaker`` and a ``context``; all (M,) integer arrays.  Items may overlap and repeat."""

    def __init__(self, utterance, start, stop, label, speaker=None, context=None):
        who = 'Items'
        self.utterance, self.start = _ints(utterance, 'utterance', who), _ints(start, 'start', who)
        self.stop, self.label = _ints(stop, 'stop', who), _ints(label, 'label', who)
        self.speaker = None if speaker is None else _ints(speaker, 'speaker', who)
        self.context = None if context is None else _ints(context, 'context', who)
        M = self.utterance.size
        if M == 0:
            raise ValueError('%s: no items' % who)
        for name in ('start', 'stop', 'label', 'speaker', 'context'):
            a = getattr(self, name)
            if a is not None and a.size != M:
                raise ValueError('%s: %s has %d entries, utterance has %d' % (who, name, a.size, M))

    def __len__(self):
        return self.utterance.size

    def resolve(self, tl, who='pair_distances'):
        """(first frame (M,) int64 in the buffer of utterances of ``tl`` frames laid end to end, frames (M,) int64); an item
        outside its utterance or without a frame is a ValueError naming it."""
        tl = np.asarray(tl, np.int64).reshape(-1)
        bad = np.nonzero((self.utterance < 0) | (self.utterance >= tl.size))[0]
        if bad.size:
            m = int(bad[0])
            raise ValueError('%s: item %d names utterance %d of %d' % (who, m, self.utterance[m], tl.size))
        empty = np.nonzero(self.stop <= self.start)[0]
        if empty.size:
            m = int(empty[0])
            raise ValueError('%s: item %d is empty: frames [%d, %d)' % (who, m, self.start[m], self.stop[m]))
        out = np.nonzero((self.start < 0) | (self.stop > tl[self.utterance]))[0]
        if out.size:
            m = int(out[0])
            raise ValueError('%s: item %d, frames [%d, %d), is outside utterance %d of %d frames'
                             % (who, m, self.start[m], self.stop[m], self.utterance[m], tl[self.utterance[m]]))
        return ragged.offsets(tl)[self.utterance] + self.start, self.stop - self.start


# --------------------------------------------------------------------------- #
# the distances
# --------------------------------------------------------------------------- #
class PairDistances(object):
    """Per ordered pair, in the caller's order, on the host: ``distance`` = cost / path_len and ``cost`` float64 (n,),
    ``path_len`` int32 (n,); ``ia``, ``ib`` the items of the two sides, ``frames_a``, ``frames_b`` their lengths."""

    def __init__(self, ia, ib, frames_a, frames_b, distance, cost, path_len, metric):
        self.ia, self.ib, self.frames_a, self.frames_b = ia, ib, frames_a, frames_b
        self.distance, self.cost, self.path_len, self.metric = distance, cost, path_len, metric

    def __len__(self):
        return self.ia.size


class _Tables(object):
    """The five device tables of one call, uploaded in one copy."""

    def __init__(self, a_start, b_start, fa, fb):
        n = a_start.size
        self.cell_off = ragged.offsets(fa * fb, total=True)
        i64 = np.concatenate([a_start, b_start, self.cell_off[:-1]]).astype(np.int64)
        i32 = np.concatenate([fa, fb]).astype(np.int32)
        self.dev = backend.to_device(np.concatenate([i64.view(np.uint8), i32.view(np.uint8)]))
        t, p = AbxTables(), self.dev.ptr
        t.a_start, t.b_start, t.cell_off, t.a_len, t.b_len = p, p + 8 * n, p + 16 * n, p + 24 * n, p + 28 * n
        self.c, self.cells = t, int(self.cell_off[-1])


def _two(x, cls, name, who):
    pair = tuple(x) if isinstance(x, (tuple, list)) else (x, x)
    if len(pair) != 2 or not all(isinstance(v, cls) for v in pair):
        raise TypeError('%s: %s must be a %s or a pair of them, got %r' % (who, name, cls.__name__, x))
    return pair


def _sides(fr, metric, who):
    """(the two Frames, the metric's number) after the refusals that concern both sides."""
    m = check_metric(metric, who)
    fa, fb = _two(fr, Frames, 'fr', who)
    if fa.form != fb.form:
        raise ValueError('%s: side a is the %s form and side b the %s form' % ((who,) + tuple(('dense', 'codes')[f.form] for f in (fa, fb))))
    if fa.form == DENSE and fa.d != fb.d:
        raise ValueError('%s: side a has D = %d and side b has D = %d' % (who, fa.d, fb.d))
    if fa.form == CODES and fa is not fb and (fa.k != fb.k or fa.W is not fb.W or fa._own_table is not fb._own_table):
        raise ValueError('%s: the two sides of the codes form must share k and the codebook or table' % who)
    return fa, fb, m


def pair_distances(fr, items, ia, ib, metric='cosine', chunk_bytes=1 << 30):
    """The DTW distance of every ORDERED pair (items[ia[p]], items[ib[p]]): a PairDistances.  ``fr`` and ``items`` may each
    be a pair (side a's, side b's) when the two sides live in different buffers; they must agree in form and D.
    ``metric``: 'cosine' or 'euclidean' (the angular form needs acos and is left out); the codes form with a table of the
    caller's own ignores it.  Pairs are cut into device calls whose local-cost tables, 8 bytes per cell, fit
    ``chunk_bytes``; pairs whose shorter side has at most WAVE_SHORT frames and the others go to different calls.  The
    result does not depend on ``chunk_bytes``.  A pair whose shorter side is above MAX_SHORT is refused: align_many aligns
    whole utterances."""
    who = 'pair_distances'
    fa, fb, m = _sides(fr, metric, who)
    ita, itb = _two(items, Items, 'items', who)
    ia, ib = _ints(ia, 'ia', who), _ints(ib, 'ib', who)
    if ia.size != ib.size:
        raise ValueError('%s: %d items on side a and %d on side b' % (who, ia.size, ib.size))
    if ia.size == 0:
        raise ValueError('%s: no pairs' % who)
    for name, idx, it in (('ia', ia, ita), ('ib', ib, itb)):
        bad = np.nonzero((idx < 0) | (idx >= len(it)))[0]
        if bad.size:
            raise ValueError('%s: %s[%d] = %d names no item of %d' % (who, name, bad[0], idx[bad[0]], len(it)))
    sa, la = ita.resolve(fa.tl, who)
    sb, lb = itb.resolve(fb.tl, who)
    a_start, b_start = sa[ia], sb[ib]
    Fa, Fb = check_pairs(la[ia], lb[ib], who)
    if int(chunk_bytes) < 1:
        raise ValueError('%s: chunk_bytes must be positive, got %r' % (who, chunk_bytes))
    n = ia.size
    short = np.minimum(Fa, Fb)
    order = np.concatenate([np.nonzero(short <= WAVE_SHORT)[0], np.nonzero(short > WAVE_SHORT)[0]])
    n_wave = int(np.count_nonzero(short <= WAVE_SHORT))

    lib = load()
    dense = fa.form == DENSE
    na = nb = table = None
    if dense and metric == 'cosine':
        na, nb = fa.norms().ptr, fb.norms().ptr
    if not dense:
        table = fa.table(metric).ptr
    cost, dist = DeviceArray((n,), np.float64), DeviceArray((n,), np.float64)
    plen = DeviceArray((n,), np.int32)
    for lo, hi in ((0, n_wave), (n_wave, n)):
        if hi == lo:
            continue
        sel = order[lo:hi]
        for a, b in plan_chunks(Fa[sel] * Fb[sel], chunk_bytes, who):
            part = sel[a:b]
            tb = _Tables(a_start[part], b_start[part], Fa[part], Fb[part])
            d = AbxDesc()
            d.n, d.d, d.metric, d.form, d.k = b - a, fa.d, m, fa.form, fa.k
            d.max_short = int(short[part].max())
            d.ftot_a, d.ftot_b, d.stride_a, d.stride_b, d.cells = fa.total, fb.total, fa.stride, fb.stride, tb.cells
            need = lib.vqvae_abx_workspace_bytes(C.byref(d))
            if need == C.c_size_t(-1).value:
                raise ValueError('%s: the library refuses this description' % who)
            ws = backend.workspace(need)
            call('vqvae_abx_local', C.byref(d), C.byref(tb.c), fa.pointer(), fb.pointer(), na, nb, table, ws.ptr, need, _S())
            at = lo + a
            call('vqvae_abx_dtw', C.byref(d), C.byref(tb.c), ws.ptr, need, cost.ptr + 8 * at, plen.ptr + 4 * at,
                 dist.ptr + 8 * at, _S())
            del tb
    out = []
    for dev in (dist, cost, plen):
        host = np.empty(n, dev.dtype)
        host[order] = dev.get()
        out.append(host)
    return PairDistances(ia, ib, Fa, Fb, out[0], out[1], out[2], metric)


def local_costs(fr, items, ia, ib, metric='cosine'):
    """Step 2 of the rule alone, for analysis and tests: the (Fa, Fb) float64 local-cost table of every pair, a list of host
    arrays, from one call."""
    who = 'local_costs'
    fa, fb, m = _sides(fr, metric, who)
    ita, itb = _two(items, Items, 'items', who)
    ia, ib = _ints(ia, 'ia', who), _ints(ib, 'ib', who)
    sa, la = ita.resolve(fa.tl, who)
    sb, lb = itb.resolve(fb.tl, who)
    Fa, Fb = check_pairs(la[ia], lb[ib], who)
    dense = fa.form == DENSE
    tb = _Tables(sa[ia], sb[ib], Fa, Fb)
    d = AbxDesc()
    d.n, d.d, d.metric, d.form, d.k = ia.size, fa.d, m, fa.form, fa.k
    d.max_short = int(np.minimum(Fa, Fb).max())
    d.ftot_a, d.ftot_b, d.stride_a, d.stride_b, d.cells = fa.total, fb.total, fa.stride, fb.stride, tb.cells
    need = load().vqvae_abx_workspace_bytes(C.byref(d))
    if need == C.c_size_t(-1).value:
        raise ValueError('%s: the library refuses this description' % who)
    ws = DeviceArray((need // 8,), np.float64)
    cosine = dense and metric == 'cosine'
    call('vqvae_abx_local', C.byref(d), C.byref(tb.c), fa.pointer(), fb.pointer(), fa.norms().ptr if cosine else None,
         fb.norms().ptr if cosine else None, None if dense else fa.table(metric).ptr, ws.ptr, need, _S())
    flat = ws.get()
    return [flat[int(o):int(o) + int(x * y)].reshape(int(x), int(y)).copy() for o, x, y in zip(tb.cell_off[:-1], Fa, Fb)]


# --------------------------------------------------------------------------- #
# the triples (host)
# --------------------------------------------------------------------------- #
class ABXPlan(object):
    """The triples of a task.  ``pairs_a``, ``pairs_b`` (P,): the unique ORDERED item pairs -- side a is A or B, side b is X,
    never swapped.  Triple t is (``tri_a``, ``tri_b``, ``tri_x``)[t] in items, its distances are pairs ``tri_ax[t]`` and
    ``tri_bx[t]``, its group ``tri_group[t]``.  ``groups`` (G, 5) int64, sorted rows
    (label_x, label_b, context, speaker_ab, speaker_x); a missing context or speaker column is 0."""

    def __init__(self, across, pairs_a, pairs_b, tri_a, tri_b, tri_x, tri_ax, tri_bx, tri_group, groups):
        self.across_speakers = across
        self.pairs_a, self.pairs_b = pairs_a, pairs_b
        self.tri_a, self.tri_b, self.tri_x = tri_a, tri_b, tri_x
        self.tri_ax, self.tri_bx, self.tri_group, self.groups = tri_ax, tri_bx, tri_group, groups


def plan_abx(items, across_speakers=False, max_per_group=None, seed=0, within_context=None):
    """The triples (A, B, X) of a task over ``items`` and the unique ordered pairs they need: an ABXPlan.

    Within speakers (the default): X, A and B share a speaker (without ``items.speaker`` everyone is one speaker), A is not
    X, label[A] == label[X], label[B] != label[X].  Across speakers: A and B share a speaker and X has another;
    ``items.speaker`` is needed.  ``within_context``: None uses ``items.context`` when it is given, True demands it, False
    ignores it; with contexts X, A and B share one.  A group is (label_x, label_b, context, speaker_ab, speaker_x).
    Triples are enumerated group by group in sorted key order and inside a group with X, then A, then B ascending by item.
    ``max_per_group`` = m keeps, of a group of more than m triples, those at
    ``numpy.random.RandomState(seed).permutation(len(group))[:m]`` of that enumeration (a fresh generator per group), in
    enumeration order.  No parity with any toolkit is claimed."""
    who = 'plan_abx'
    if not isinstance(items, Items):
        raise TypeError('%s: items must be an Items, got %r' % (who, type(items)))
    if across_speakers and items.speaker is None:
        raise ValueError('%s: the across-speaker task needs items.speaker' % who)
    if within_context and items.context is None:
        raise ValueError('%s: within_context needs items.context' % who)
    if max_per_group is not None and int(max_per_group) < 1:
        raise ValueError('%s: max_per_group must be at least 1, got %r' % (who, max_per_group))
    M = len(items)
    spk = items.speaker if items.speaker is not None else np.zeros(M, np.int64)
    use_ctx = items.context is not None and within_context is not False
    ctx = items.context if use_ctx else np.zeros(M, np.int64)
    cells = {}                                                # (speaker, context) -> label -> items, ascending
    for m in range(M):
        cells.setdefault((int(spk[m]), int(ctx[m])), {}).setdefault(int(items.label[m]), []).append(m)
    cells = dict((key, dict((lab, np.array(v, np.int64)) for lab, v in by.items())) for key, by in cells.items())
    cap = None if max_per_group is None else int(max_per_group)
    found = []
    for (s_ab, c), by_label in cells.items():
        others = [s_ab] if not across_speakers else [s for (s, cc) in cells if cc == c and s != s_ab]
        for s_x in others:
            same = s_x == s_ab                                # X is drawn from A's own list: A != X leaves one out
            for lx, xs in cells[(s_x, c)].items():
                if lx not in by_label:
                    continue
                As = by_label[lx]
                nA = As.size - 1 if same else As.size
                if nA < 1:
                    continue
                for lb, bs in by_label.items():
                    if lb == lx:
                        continue
                    # the enumeration: X, then A (without X), then B, each ascending by item; triple t of the group is
                    # X = t // (nA nB), A's rank = t // nB % nA, B = t % nB
                    total = xs.size * nA * bs.size
                    t = np.arange(total) if cap is None or total <= cap else np.sort(np.random.RandomState(seed).permutation(total)[:cap])
                    xi, rank, bi = t // (nA * bs.size), t // bs.size % nA, t % bs.size
                    ai = rank + (rank >= xi) if same else rank
                    found.append(((lx, lb, c, s_ab, s_x), As[ai], bs[bi], xs[xi]))
    if not found:
        raise ValueError('%s: no triple exists: the %s task needs an A and an X of one label and a B of another %s'
                         % (who, 'across-speaker' if across_speakers else 'within-speaker',
                            'with A and B of one speaker and X of another' if across_speakers else 'inside one speaker'
                            + (' and context' if use_ctx else '')))
    found.sort(key=lambda g: g[0])
    tri_a, tri_b, tri_x, tri_g = [], [], [], []
    for gi, (key, A, B, X) in enumerate(found):
        tri_a.append(A), tri_b.append(B), tri_x.append(X), tri_g.append(np.full(A.size, gi, np.int64))
    tri_a, tri_b, tri_x, tri_g = [np.concatenate(v).astype(np.int64) for v in (tri_a, tri_b, tri_x, tri_g)]
    keys, inverse = np.unique(np.concatenate([tri_a * M + tri_x, tri_b * M + tri_x]), return_inverse=True)
    inverse = inverse.reshape(-1)
    return ABXPlan(bool(across_speakers), keys // M, keys % M, tri_a, tri_b, tri_x, inverse[:tri_a.size], inverse[tri_a.size:],
                   tri_g, np.array([g[0] for g in found], np.int64).reshape(-1, 5))


class ABXScores(object):
    """``error``: the mean over ordered label pairs of ``by_label_pair`` {(label_x, label_b): mean of its groups' rates}.
    Per group, rows of ``groups`` (G, 5): int64 ``triples``, ``errors`` (distance(A, X) > distance(B, X)) and ``ties``
    (equal), and ``rates`` = (2 * errors + ties) / (2 * triples).  ``pairs``: the PairDistances; ``plan``: the ABXPlan."""

    def __init__(self, error, by_label_pair, groups, triples, errors, ties, rates, pairs, plan):
        self.error, self.by_label_pair, self.groups = error, by_label_pair, groups
        self.triples, self.errors, self.ties, self.rates, self.pairs, self.plan = triples, errors, ties, rates, pairs, plan


def score_abx(plan, pairs):
    """The ABXScores of a plan and the distances of its pairs (a PairDistances or a (P,) float64 array).  A triple scores 2
    when distance(A, X) > distance(B, X), 1 when they are equal and 0 otherwise; a group's rate is its score sum over twice
    its triples; a label pair's the plain mean of its groups' rates in sorted key order, added up from 0.0; ``error`` the
    plain mean of the label pairs' in sorted order."""
    dist = np.asarray(pairs.distance if isinstance(pairs, PairDistances) else pairs, np.float64)
    if dist.shape != plan.pairs_a.shape:
        raise ValueError('score_abx: %d distances for %d pairs' % (dist.size, plan.pairs_a.size))
    dax, dbx = dist[plan.tri_ax], dist[plan.tri_bx]
    G = len(plan.groups)
    triples = np.bincount(plan.tri_group, minlength=G).astype(np.int64)
    errors = np.bincount(plan.tri_group, weights=(dax > dbx), minlength=G).astype(np.int64)
    ties = np.bincount(plan.tri_group, weights=(dax == dbx), minlength=G).astype(np.int64)
    rates = (2 * errors + ties).astype(np.float64) / (2 * triples).astype(np.float64)
    sums, counts = {}, {}
    for g in range(G):                                        # the groups are in sorted key order
        key = (int(plan.groups[g, 0]), int(plan.groups[g, 1]))
        sums[key] = sums.get(key, 0.0) + float(rates[g])
        counts[key] = counts.get(key, 0) + 1
    by_label_pair = dict((key, sums[key] / float(counts[key])) for key in sorted(sums))
    total = 0.0
    for key in sorted(by_label_pair):
        total = total + by_label_pair[key]
    return ABXScores(total / float(len(by_label_pair)), by_label_pair, plan.groups, triples, errors, ties, rates, pairs, plan)


# --------------------------------------------------------------------------- #
# the public calls
# --------------------------------------------------------------------------- #
def abx(fr, items, across_speakers=False, metric='cosine', max_per_group=None, seed=0, within_context=None,
        chunk_bytes=1 << 30, plan=None):
    """The ABX error of ``items`` over the features ``fr``: ``plan_abx``, ``pair_distances`` over the plan's unique ordered
    pairs, ``score_abx``.  ``plan``: an ABXPlan of ``plan_abx`` over these items to use instead of planning again (the same
    items over several snapshots or penalties); the task's keywords are then not read.  Every refusal comes before the
    first device call."""
    who = 'abx'
    check_metric(metric, who)
    if not isinstance(fr, Frames):
        raise TypeError('%s: fr must be a Frames, got %r' % (who, type(fr)))
    if not isinstance(items, Items):
        raise TypeError('%s: items must be an Items, got %r' % (who, type(items)))
    items.resolve(fr.tl, who)
    plan = _plan(who, plan, items, across_speakers, max_per_group, seed, within_context)
    return score_abx(plan, pair_distances(fr, items, plan.pairs_a, plan.pairs_b, metric, chunk_bytes))


def _plan(who, plan, items, across_speakers, max_per_group, seed, within_context):
    if plan is None:
        return plan_abx(items, across_speakers, max_per_group, seed, within_context)
    if not isinstance(plan, ABXPlan):
        raise TypeError('%s: plan must be an ABXPlan, got %r' % (who, type(plan)))
    if max(int(plan.pairs_a.max()), int(plan.pairs_b.max())) >= len(items):
        raise ValueError('%s: the plan names item %d, there are %d' % (who, max(int(plan.pairs_a.max()), int(plan.pairs_b.max())), len(items)))
    return plan


def _check_task(who, metric, what, items):
    check_metric(metric, who)
    if what not in ('latents', 'codes'):
        raise ValueError("%s: what must be 'latents' or 'codes', got %r" % (who, what))
    if not isinstance(items, Items):
        raise TypeError('%s: items must be an Items, got %r' % (who, type(items)))


def _from_waves(who, encoder, vq, lengths, source, items, what, across_speakers, metric, max_per_group, seed, within_context,
                chunk_bytes, feature_bytes, plan):
    from . import frontend
    _check_task(who, metric, what, items)
    W = _codebook(vq, who)
    k, D = W.shape
    enc = frontend._encoder_params(encoder, who)
    if enc[-1][0].shape[0] != D:
        raise ValueError('%s: the encoder writes %d channels, the codebook has d = %d' % (who, enc[-1][0].shape[0], D))
    lengths, tl = frontend._wave_lengths(lengths, len(enc), who)
    items.resolve(tl, who)
    off = ragged.offsets(tl, total=True)
    total = int(off[-1])
    need = 4 * total * (D if what == 'latents' else 1)
    if need > int(feature_bytes):
        raise ValueError('%s: the %s of %d frames take %d bytes, feature_bytes allows %d' % (who, what, total, need, int(feature_bytes)))
    plan = _plan(who, plan, items, across_speakers, max_per_group, seed, within_context)
    if what == 'codes':
        codes = frontend._run(who, encoder, vq, None, lengths, source, None, chunk_bytes)[0]
        fr = Frames.from_codes(codes, vq)
    else:
        buf = DeviceArray((D, total), np.float32)

        def keep(z_ptr, stride, tb, first):                   # the chunk's z (D, stride) into its columns of buf
            T = int(off[first + tb.n] - off[first])
            dst = (C.c_void_p * D)(*[buf.ptr + 4 * (ch * total + int(off[first])) for ch in range(D)])
            src = (C.c_void_p * D)(*[z_ptr + 4 * ch * int(stride) for ch in range(D)])
            cnt = (C.c_size_t * D)(*([T] * D))
            _lib.call('vqvae_copy_list', D, dst, src, cnt, _S())

        frontend._run(who, encoder, vq, None, lengths, source, None, chunk_bytes, hook=keep)
        fr = Frames(tl, x=buf, d=D, stride=total)
    return score_abx(plan, pair_distances(fr, items, plan.pairs_a, plan.pairs_b, metric, chunk_bytes))


def abx_many(encoder, vq, waves, items, what='latents', across_speakers=False, metric='cosine', max_per_group=None, seed=0,
             within_context=None, chunk_bytes=1 << 30, feature_bytes=8 << 30, plan=None):
    """``abx`` from waveforms: the ragged encoder of ``encode_many`` (same arguments, same chunks) and the distances over
    its output while that is on the device.  ``what`` = 'latents': every chunk's z is copied device-to-device into one
    (D, total) buffer; 'codes': the indices are kept and the local cost is ``code_table``'s.  ``items`` are in latent
    frames.  A buffer above ``feature_bytes`` is a ValueError that names its size."""
    _check_task('abx_many', metric, what, items)
    sizes, source = ragged.wave_source(waves, 'abx_many')
    return _from_waves('abx_many', encoder, vq, sizes, source, items, what, across_speakers, metric, max_per_group, seed,
                       within_context, chunk_bytes, feature_bytes, plan)


def abx_corpus(corpus, encoder, vq, items, what='latents', across_speakers=False, metric='cosine', max_per_group=None, seed=0,
               within_context=None, chunk_bytes=1 << 30, feature_bytes=8 << 30, plan=None):
    """``ResidentCorpus.abx`` / ``CorpusView.abx``: the utterances are read in place from the corpus buffer."""
    _check_task('abx', metric, what, items)
    lengths, source = ragged.wave_source(corpus, 'abx')
    return _from_waves('abx', encoder, vq, lengths, source, items, what, across_speakers, metric, max_per_group, seed,
                       within_context, chunk_bytes, feature_bytes, plan)
