"""Statistics of the discrete codes on the device: speaker leakage, usage, durations and the edit distance of two code
strings for a ragged list of utterances (include/vqvae_codes.h states the rule, csrc/code_stats.hip runs it).

    codes = corpus.encode(encoder, vq)                         # frontend.LatentCodes
    st = code_stats(codes, speakers, n_speakers)               # CodeStats: mi_bits, perplexity, js_bits, run_hist, ...
    st = corpus.code_stats(codes)                              # ... with the corpus's (or the view's) own speakers
    runs = collapse_many(codes)                                # CodeRuns: every run of equal codes as (code, duration)
    cmp = compare_codes_many(codes_a, codes_b)                 # CodeComparison: distance, subs, ins, dels, agreement, ...

How much a code tells about the speaker is ``mi_bits``, the mutual information of code and speaker (near 0 for codes that
carry the sentence and not the voice); ``permutations=P`` gives the same figure for P random relabelings of the utterances,
the finite-sample floor a measured value has to be read against.  Whether two speakers saying one sentence get one code
string -- or a converted utterance, encoded again, the codes it was made from -- is the edit distance of
``compare_codes_many``, by default over the strings with their repetitions collapsed.

The device counts; everything it does is integer arithmetic, so the tables and distances are the same bits for any list
order and launch shape, and tests/codestats_ref.py restates them in NumPy.  The derived figures are float64 NumPy over the
count tables, on the host (``figures``).
"""
import ctypes as C

import numpy as np

from . import _lib, backend
from .backend import DeviceArray
from .frontend import LatentCodes

_S = backend.stream
MAX_SHORT = _lib.CODES_MAX_SHORT   # min(La, Lb) of a pair
THREADS = _lib.CODES_THREADS
MAX_BIGRAM_K = _lib.CODES_MAX_BIGRAM_K


# --------------------------------------------------------------------------- #
# the host side of the rule
# --------------------------------------------------------------------------- #
def _xlog2(p, q=1.0):
    """p * log2(p / q) summed along the last axis over the elements with p > 0, float64."""
    p = np.asarray(p, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(p > 0, p * np.log2(p / q), 0.0).sum(axis=-1)


def mutual_information_bits(uni):
    """sum over u > 0 of (u / n) log2(u n / (n_g n_c)) for a count table (G, k).  u n / (n_g n_c) is exactly 1 wherever
    every speaker has the same histogram, so the figure is exactly 0 then."""
    u = np.asarray(uni, np.int64).astype(np.float64)
    n_g, n_c, n = u.sum(axis=1), u.sum(axis=0), u.sum()
    if n == 0:
        return np.nan
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.where(u > 0, (u / n) * np.log2((u * n) / (n_g[:, None] * n_c[None, :])), 0.0).sum())


def _js_bits(u, n_g):
    """(G, G) Jensen-Shannon divergences between the rows of the count table, nan for a row without a count: the upper
    triangle is computed and mirrored."""
    G = u.shape[0]
    with np.errstate(invalid='ignore', divide='ignore'):
        p = u / n_g[:, None]
    js = np.full((G, G), np.nan)
    for g in range(G):
        mid = 0.5 * (p[g][None, :] + p[g:])
        js[g, g:] = 0.5 * (_xlog2(np.broadcast_to(p[g], mid.shape), mid) + _xlog2(p[g:], mid))
        js[g:, g] = js[g, g:]
    js[n_g == 0, :] = np.nan
    js[:, n_g == 0] = np.nan
    return js


def figures(uni, big=None):
    """The derived figures of a count table ``uni`` (G, k) and, when given, ``big`` (k, k), as a dict of float64 NumPy:
    ``positions``, ``used``, ``used_per_speaker`` (G,), ``entropy_bits``, ``perplexity``, ``mi_bits``,
    ``mi_normalised``, ``js_bits`` (G, G; nan for a speaker without a position); from ``big``: ``transitions``,
    ``self_share``, ``next_entropy_bits`` (nan without a transition)."""
    uni = np.asarray(uni, np.int64)
    G, k = uni.shape
    u = uni.astype(np.float64)
    n_g, n_c, n = u.sum(axis=1), u.sum(axis=0), float(uni.sum())
    out = dict(positions=int(uni.sum()), used=int((uni.sum(axis=0) > 0).sum()), used_per_speaker=(uni > 0).sum(axis=1))
    if n == 0:
        out.update(entropy_bits=np.nan, perplexity=np.nan, mi_bits=np.nan, mi_normalised=np.nan, js_bits=np.full((G, G), np.nan))
    else:
        H, HS, mi = -float(_xlog2(n_c / n)), -float(_xlog2(n_g / n)), mutual_information_bits(uni)
        out.update(entropy_bits=H, perplexity=float(2.0 ** H), mi_bits=mi, mi_normalised=mi / HS if HS > 0 else 0.0,
                   js_bits=_js_bits(u, n_g))
    if big is not None:
        b = np.asarray(big, np.int64).astype(np.float64)
        T = float(b.sum())
        out['transitions'] = int(np.asarray(big, np.int64).sum())
        if T == 0:
            out.update(self_share=np.nan, next_entropy_bits=np.nan)
        else:
            rows = np.broadcast_to(b.sum(axis=1)[:, None], b.shape)
            out.update(self_share=float(np.trace(b)) / T, next_entropy_bits=-float(np.sum((b / T)[b > 0] * np.log2(b[b > 0] / rows[b > 0]))))
    return out


def _codes_arg(codes, name, who):
    if not isinstance(codes, LatentCodes):
        raise TypeError('%s: %s must be a frontend.LatentCodes, got %r' % (who, name, type(codes)))
    return codes


def _groups(speakers, n_speakers, N, who):
    """(group (N,) int32, G); the refusals name the utterance."""
    if speakers is None:
        if n_speakers not in (None, 1):
            raise ValueError('%s: n_speakers = %r without speakers' % (who, n_speakers))
        return np.zeros(N, np.int32), 1
    spk = np.asarray(speakers.get() if backend.is_device(speakers) else speakers)
    if spk.dtype.kind not in 'iu' or spk.ndim != 1 or spk.size != N:
        raise ValueError('%s: one integer speaker id per utterance (%d), got %s %s' % (who, N, spk.dtype, spk.shape))
    spk = spk.astype(np.int64)
    G = int(spk.max()) + 1 if n_speakers is None else int(n_speakers)
    bad = np.nonzero((spk < 0) | (spk >= G))[0]
    if bad.size or G < 1:
        u = int(bad[0]) if bad.size else 0
        raise ValueError('%s: utterance %d has speaker %d; speaker ids must be in [0, %d)' % (who, u, spk[u], G))
    return spk.astype(np.int32), G


def _upload(*arrays):
    """Host tables laid end to end in one device buffer (one copy): (the buffer, the pointer of every table).  The widest
    dtype goes first, so every table is aligned."""
    raw = [np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in arrays]
    dev = backend.to_device(np.concatenate(raw))
    at = np.concatenate([[0], np.cumsum([r.size for r in raw])])
    return dev, [dev.ptr + int(o) for o in at[:-1]]


# --------------------------------------------------------------------------- #
# runs
# --------------------------------------------------------------------------- #
class CodeRuns(object):
    """The runs of equal codes of N utterances, on the device: ``u`` and ``dur``, int32 buffers of the size of the input
    in which utterance i's run codes and durations occupy [offsets[i], offsets[i] + m[i]) (the slots behind them are not
    written); ``m`` (N,) int32, the number of runs; ``run_hist`` (max_run,) int64 on the device, a run of length L
    counted in bucket min(L, max_run) - 1 (None when the runs were taken with max_run=None).  ``tl``, ``offsets`` and ``k`` are the input's.  ``lengths`` (host int64 m),
    ``histogram`` (host run_hist) and ``to_host`` copy back, once."""

    def __init__(self, tl, offsets, k, u, dur, m, run_hist, tables):
        self.tl, self.offsets, self.k = tl, offsets, k
        self.u, self.dur, self.m, self.run_hist = u, dur, m, run_hist
        self._tables = tables                  # (buffer, [start pointer, len pointer]) of the input's layout
        self._lengths = self._hist = self._host = None

    def __len__(self):
        return len(self.tl)

    @property
    def lengths(self):
        if self._lengths is None:
            self._lengths = self.m.get().astype(np.int64)
        return self._lengths

    @property
    def histogram(self):
        if self.run_hist is None:
            raise ValueError('CodeRuns.histogram: the runs were taken with max_run=None')
        if self._hist is None:
            self._hist = self.run_hist.get()
        return self._hist

    @property
    def mean_run(self):
        """Positions per run over the whole list."""
        return float(np.sum(self.tl, dtype=np.int64)) / float(self.lengths.sum())

    def to_host(self):
        """List of N pairs (codes, durations) of host int32 arrays of length m[i]."""
        if self._host is None:
            self._host = (self.u.get(), self.dur.get())
        return [(self._host[0][int(o):int(o) + int(m)].copy(), self._host[1][int(o):int(o) + int(m)].copy())
                for o, m in zip(self.offsets[:-1], self.lengths)]


def collapse_many(codes, max_run=64):
    """Every utterance's codes with their repetitions collapsed: a CodeRuns.  One launch, one workgroup per utterance; a
    run never continues across an utterance boundary.  ``max_run=None``: no histogram of the durations is kept."""
    who = 'collapse_many'
    _codes_arg(codes, 'codes', who)
    if max_run is not None and int(max_run) < 1:
        raise ValueError('%s: max_run must be at least 1, got %r' % (who, max_run))
    N, total = len(codes), int(codes.offsets[-1])
    tables = _upload(codes.offsets[:-1].astype(np.int64), codes.tl.astype(np.int32))
    start, length = tables[1]
    u, dur = DeviceArray((total,), np.int32), DeviceArray((total,), np.int32)
    m, hist = DeviceArray((N,), np.int32), None if max_run is None else DeviceArray((int(max_run),), np.int64)
    d = _lib.CodesRunsDesc(N, 1 if max_run is None else int(max_run), total)
    ws, need = backend.described_workspace('vqvae_codes_runs_workspace_bytes', d, who)
    _lib.call('vqvae_codes_runs', C.byref(d), codes.indices.ptr, start, length, u.ptr, dur.ptr, m.ptr,
              None if hist is None else hist.ptr, ws, need, _S())
    return CodeRuns(codes.tl, codes.offsets, codes.k, u, dur, m, hist, tables)


# --------------------------------------------------------------------------- #
# counts
# --------------------------------------------------------------------------- #
class CodeStats(object):
    """The count tables on the host -- ``uni`` (G, k), ``big`` (k, k) or None, ``invalid``, ``run_hist`` (max_run,), all
    int64 -- and the figures derived from them (``figures``): ``positions``, ``used``, ``used_per_speaker``,
    ``entropy_bits``, ``perplexity``, ``mi_bits``, ``mi_normalised``, ``js_bits``, with bigrams ``transitions``,
    ``self_share`` and ``next_entropy_bits``; from the runs ``runs`` (their number) and ``mean_run``; ``mi_permuted``
    (P,), the mutual information under P random relabelings of the utterances' speakers."""

    def __init__(self, uni, big, invalid, run_hist, runs, mean_run, mi_permuted, n_speakers, collapsed):
        self.uni, self.big, self.invalid, self.run_hist = uni, big, int(invalid), run_hist
        self.runs, self.mean_run, self.mi_permuted = int(runs), float(mean_run), mi_permuted
        self.n_speakers, self.collapsed, self.k = int(n_speakers), bool(collapsed), uni.shape[1]
        for name, value in figures(uni, big).items():
            setattr(self, name, value)


def _count(who, buf, total, start, length, group, N, k, G, uni, big, invalid, accumulate=False):
    d = _lib.CodesHistDesc(N, k, G, int(big is not None), int(bool(accumulate)), 0, total)
    ws, need = backend.described_workspace('vqvae_codes_hist_workspace_bytes', d, who)
    _lib.call('vqvae_codes_hist', C.byref(d), buf.ptr, start, length, group, uni.ptr, None if big is None else big.ptr,
              invalid.ptr, ws, need, _S())


def code_stats(codes, speakers=None, n_speakers=None, bigrams=True, collapsed=False, max_run=64, permutations=0, seed=0):
    """Counts over the codes of a list of utterances (frontend.LatentCodes, on the device or the host) and the figures
    derived from them: a CodeStats.  ``speakers``: one id per utterance in [0, n_speakers) (n_speakers defaults to the
    largest id + 1); without them everything is one group.  ``bigrams``: also the (k, k) table of transitions inside the
    utterances (k of at most 4096).  ``collapsed``: count runs instead of positions, so a long code weighs as much as a
    short one and the transition table has a zero diagonal.  ``permutations=P``: the unigram count is run P more times
    with the speakers of the utterances relabeled by ``RandomState(seed).permutation``, for ``mi_permuted``."""
    who = 'code_stats'
    _codes_arg(codes, 'codes', who)
    N, k, total = len(codes), codes.k, int(codes.offsets[-1])
    if max_run is None or int(max_run) < 1:
        raise ValueError('%s: max_run must be at least 1, got %r' % (who, max_run))
    if int(permutations) < 0:
        raise ValueError('%s: permutations must not be negative, got %r' % (who, permutations))
    if int(permutations) and speakers is None:
        raise ValueError('%s: permutations = %d without speakers: there is nothing to relabel' % (who, permutations))
    if bigrams and k > MAX_BIGRAM_K:
        raise ValueError('%s: k = %d: the bigram table would have %d bytes; k may be at most %d, ask for bigrams=False'
                         % (who, k, 8 * k * k, MAX_BIGRAM_K))
    group, G = _groups(speakers, n_speakers, N, who)
    runs = collapse_many(codes, max_run)
    buf, (start, length) = codes.indices, runs._tables[1]
    if collapsed:
        buf, length = runs.u, runs.m.ptr                     # the runs are read in place, their number from the device
    uni, invalid = DeviceArray((G, k), np.int64), DeviceArray((1,), np.int64)
    big = DeviceArray((k, k), np.int64) if bigrams else None
    gdev = backend.to_device(group)
    _count(who, buf, total, start, length, gdev.ptr, N, k, G, uni, big, invalid)
    uni_h, big_h, inv_h = uni.get(), None if big is None else big.get(), int(invalid.get()[0])
    rs = np.random.RandomState(seed)
    permuted = np.zeros(int(permutations), np.float64)
    for p in range(int(permutations)):
        gdev = backend.to_device(np.ascontiguousarray(group[rs.permutation(N)]))
        _count(who, buf, total, start, length, gdev.ptr, N, k, G, uni, None, invalid)
        permuted[p] = mutual_information_bits(uni.get())
    return CodeStats(uni_h, big_h, inv_h, runs.histogram, runs.lengths.sum(), runs.mean_run, permuted, G, collapsed)


# --------------------------------------------------------------------------- #
# pairs
# --------------------------------------------------------------------------- #
class CodeComparison(object):
    """Per pair, in the caller's order, int64 (N,): ``distance`` (the edit distance), ``subs``, ``ins``, ``dels``,
    ``matches`` (distance = subs + ins + dels, len_a = matches + subs + dels), ``len_a`` and ``len_b`` (the lengths the
    distance was taken over: after the collapse when there was one), ``agree`` and ``overlap`` (raw frames: positions
    below min(tl_a, tl_b) and how many of them hold the same code); float64 (N,): ``error_rate`` = distance / len_a,
    ``normalised`` = distance / max(len_a, len_b), ``agreement`` = agree / overlap."""

    def __init__(self, distance, subs, len_a, len_b, agree, overlap, collapse):
        self.distance, self.subs, self.len_a, self.len_b, self.agree, self.overlap = distance, subs, len_a, len_b, agree, overlap
        self.collapse = bool(collapse)
        self.dels = (distance - subs + len_a - len_b) // 2
        self.ins = (distance - subs - len_a + len_b) // 2
        self.matches = len_a - self.dels - subs
        self.error_rate = distance / len_a.astype(np.float64)
        self.normalised = distance / np.maximum(len_a, len_b).astype(np.float64)
        self.agreement = agree / overlap.astype(np.float64)

    def __len__(self):
        return len(self.distance)


def check_pairs(tl_a, tl_b, who='compare_codes_many'):
    """(tl_a, tl_b) as int64 (N,) arrays; a ValueError naming the pair for another count on the two sides or a shorter
    side above MAX_SHORT."""
    la, lb = np.asarray(tl_a, np.int64).reshape(-1), np.asarray(tl_b, np.int64).reshape(-1)
    if la.size != lb.size:
        raise ValueError('%s: %d utterances on side a and %d on side b' % (who, la.size, lb.size))
    long_ = np.nonzero(np.minimum(la, lb) > MAX_SHORT)[0]
    if long_.size:
        u = int(long_[0])
        raise ValueError('%s: pair %d has %d and %d codes; the shorter side may have at most %d (three anti-diagonals of '
                         'the pair are kept in the 160 KB of LDS of a compute unit)' % (who, u, la[u], lb[u], MAX_SHORT))
    return la, lb


def compare_codes_many(codes_a, codes_b, collapse=True):
    """Utterance i of ``codes_a`` against utterance i of ``codes_b`` (LatentCodes of the same N and k): the unit-cost edit
    distance of the two code strings with its substitutions, insertions and deletions -- over the strings with their
    repetitions collapsed when ``collapse``, else over the raw ones -- and the frame agreement of the raw codes: a
    CodeComparison.  One launch per step for all pairs; the shorter side of a pair may have at most MAX_SHORT codes
    (judged by the raw lengths), a ValueError naming the pair otherwise, raised before any device call."""
    who = 'compare_codes_many'
    _codes_arg(codes_a, 'codes_a', who)
    _codes_arg(codes_b, 'codes_b', who)
    if codes_a.k != codes_b.k:
        raise ValueError('%s: side a has k = %d and side b k = %d: not codes of one codebook' % (who, codes_a.k, codes_b.k))
    la, lb = check_pairs(codes_a.tl, codes_b.tl, who)
    N = len(la)
    d = _lib.CodesPairDesc(N, int(np.minimum(la, lb).max()), int(codes_a.offsets[-1]), int(codes_b.offsets[-1]))
    keep, (sa, sb, na, nb) = _upload(codes_a.offsets[:-1].astype(np.int64), codes_b.offsets[:-1].astype(np.int64),
                                     codes_a.tl.astype(np.int32), codes_b.tl.astype(np.int32))
    out = DeviceArray((3, N), np.int32)                      # agree, dist, subs
    raw = _lib.CodesPairTables(sa, na, sb, nb)
    ws, need = backend.described_workspace('vqvae_codes_agree_workspace_bytes', d, who)
    _lib.call('vqvae_codes_agree', C.byref(d), C.byref(raw), codes_a.indices.ptr, codes_b.indices.ptr, out.ptr, ws, need, _S())
    if collapse:
        ra, rb = collapse_many(codes_a, None), collapse_many(codes_b, None)
        t, a, b = _lib.CodesPairTables(sa, ra.m.ptr, sb, rb.m.ptr), ra.u, rb.u
    else:
        t, a, b = raw, codes_a.indices, codes_b.indices
    ws, need = backend.described_workspace('vqvae_codes_edit_workspace_bytes', d, who)
    _lib.call('vqvae_codes_edit', C.byref(d), C.byref(t), a.ptr, b.ptr, out.ptr + 4 * N, out.ptr + 8 * N, ws, need, _S())
    got = out.get().astype(np.int64)
    len_a, len_b = (ra.lengths, rb.lengths) if collapse else (la.copy(), lb.copy())
    del keep
    return CodeComparison(got[1], got[2], len_a, len_b, got[0], np.minimum(la, lb), collapse)
