"""Held-out likelihood of a mixture-of-logistics decoder on the device: scoring.py's teacher-forced ragged pass with the
raw-sample input and the mixture likelihood (csrc/ragged_mol.h states the rule, csrc/ragged_mol.hip runs the two kernels
that are new; the condition, the blocks, the head's GEMMs and the reduce are include/vqvae_ragged_decoder.h's).

    cond = frontend_many(encoder, vq, condition_embed, waves, speakers)
    s = score_many_mol(model.decoder.ema, cond, waves)             # MolScores: nll, count, bits_per_sample, total()
    s = evaluate_many_mol(encoder, vq, condition_embed, wavenet, waves, speakers)
    s = corpus.score_mol(wavenet, cond)                            # a ResidentCorpus / CorpusView read in place

These are siblings of score_many / evaluate_many / corpus.score, which keep refusing a ``use_logistic`` decoder: the two
passes take different inputs (samples, not classes, are the target), return different things (no arg-max, no hits) and
their figures are not comparable, so a keyword would have hidden a different call.

Utterance i with L_i samples and tl_i latent frames contributes n_i = min(upscale * tl_i, L_i - 1) positions: the input at
j is the sample w[j] (or its mu-law class, for a decoder whose embed reads classes), the target the sample w[j + 1].  A
position's NLL is the same bits alone, in any list, at any position, for any ``chunk_bytes`` and read in place from a
corpus.  The per-utterance sums are float64 in one written order.  Everything runs with dropout off under
no_backprop_mode.

The entry points are declared in csrc/ragged_mol.h, which is not under include/, so they are bound here (table, revision
check) on first use and not in _lib.HEADERS; the structures are _lib's RdecDesc and RdecTables.
"""
import ctypes as C
import math

import numpy as np

from . import _lib, backend, core, ragged, scoring
from .backend import DeviceArray
from .scoring import latent_lengths, positions, reduce_order  # noqa: F401  (the host side of the rule is scoring's)

_S = backend.stream
MAX_MIX = 16                       # VQVAE_RDMOL_MAX_MIX

HEADER = 'ragged_mol.h'            # under csrc/
REVISION = 1
P = _lib.P
_D, _T = C.POINTER(_lib.RdecDesc), C.POINTER(_lib.RdecTables)
# the table IS the list of symbols csrc/ragged_mol.h declares (tests/test_host_scoring_mol.py)
PROTOTYPES = {
    'vqvae_rdmol_revision': (C.c_int, []),
    'vqvae_rdmol_embed': (C.c_int, [_D, _T, P, P, P, P, P, P]),
    'vqvae_rdmol_nll': (C.c_int, [_D, _T, P, P, P, C.c_int, C.c_int, C.c_float, P, P]),
}

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
    has = lib.vqvae_rdmol_revision()
    if has != REVISION:
        raise ImportError('libvqvae_hip.so at %s has mixture-of-logistics scoring revision %d, this package binds %d: rebuild '
                          'it (__graft_entry__.build())' % (_lib.LIB_PATH, has, REVISION))
    _bound = lib
    return lib


def call(name, *args):
    """Calls an int-returning entry point of the header and raises _lib.HipError on failure."""
    _lib.check(getattr(load(), name)(*args), name)


# --------------------------------------------------------------------------- #
# the host side
# --------------------------------------------------------------------------- #
def chunk_elements(n, tl, lengths, dims):
    """(stages, N) int64: scoring.chunk_elements' rows with the (3 M, n_i) output, which this pass always writes, and the
    class buffer only when the embed reads classes."""
    per = scoring.chunk_elements(n, tl, lengths, dims, logits=True)
    return per if dims['Qin'] > 1 else np.delete(per, 6, axis=0)


def plan_chunks(n, tl, lengths, dims, chunk_bytes, who='score_many_mol'):
    """scoring.plan_chunks over chunk_elements above."""
    return scoring.plan_elements(chunk_elements(n, tl, lengths, dims), n, chunk_bytes, who)


class MolScores(object):
    """Per utterance, in the caller's order: ``nll`` float64 (N,) summed negative log-likelihood in nats, ``count`` int64
    (N,) scored positions.  ``per_sample``: the ragged float32 NLL on the device with ``offsets`` (N + 1,), when asked for;
    ``params``: list of N host arrays (3 M, n_i) -- M logits, M means, M log-scales per position -- when asked for.

    What the figure is: the log-probability the mixture gives the bin of width 2 / (quantize - 1) round the target sample
    on a LINEAR amplitude grid (the open tails beyond +-0.999 included).  It is comparable between mixture-of-logistics
    snapshots of one ``quantize``.  It is NOT comparable with the bits of a mu-law softmax decoder (scoring.Scores), whose
    bins are of unequal width in amplitude.  There is no ``hits`` or ``accuracy``: the mixture has no arg-max class."""

    def __init__(self, nll, count, per_sample=None, offsets=None, params=None):
        self.nll, self.count = nll, count
        self.per_sample, self.offsets, self.params = per_sample, offsets, params

    def __len__(self):
        return len(self.nll)

    @property
    def bits_per_sample(self):
        return self.nll / self.count / math.log(2.0)

    def total(self):
        """The corpus-level bits per sample: sum(nll) / sum(count) / ln 2."""
        return float(self.nll.sum() / self.count.sum() / math.log(2.0))

    def sample_nll(self, i):
        """Utterance i's per-sample NLL as a host array (n_i,) (needs per_sample=True)."""
        if self.per_sample is None:
            raise ValueError('MolScores.sample_nll: the scores were computed without per_sample=True')
        return self.per_sample.flat_view(int(self.offsets[i]), int(self.count[i])).get()


def _check_decoder(wavenet, who):
    """The refusals that need no parameter's data; (blocks, dims) with dims = scoring's and Qin, M."""
    if not getattr(wavenet, 'use_logistic', False):
        raise ValueError('%s: the decoder has a softmax output (use_logistic is off): score_many / evaluate_many / '
                         'corpus.score are the calls for it' % who)
    rows = scoring._shape(wavenet.proj2.W, 'proj2.W', who)[0]
    if rows % 3 or not 1 <= rows // 3 <= MAX_MIX:
        raise ValueError('%s: the decoder writes %d rows; a mixture of M logistics has 3 M (logits, means, log-scales) with '
                         '1 <= M <= %d' % (who, rows, MAX_MIX))
    blocks = scoring._check_blocks(wavenet, who)
    We = scoring._shape(wavenet.embed.W, 'embed.W', who)
    b0 = blocks[0]
    Wd, Wc, Ws = (scoring._shape(p, 'resnet.0.' + n, who) for n, p in (('conv.W', b0.conv.W), ('condition_proj.W', b0.condition_proj.W),
                                                                        ('skip.W', b0.skip.W)))
    if tuple(We[2:]) not in ((2,), (2, 1)):
        raise ValueError('%s: the embed conv must have two taps, got W %s' % (who, We))
    if We[1] > scoring.MAX_CLASSES:
        raise ValueError('%s: the embed reads %d classes; at most %d' % (who, We[1], scoring.MAX_CLASSES))
    if int(wavenet.quantize) < 2:
        raise ValueError('%s: quantize must be at least 2, got %r' % (who, wavenet.quantize))
    return blocks, dict(R=We[0], D=Wd[0], S=Ws[0], Q=rows, Qin=We[1], M=rows // 3, Cc=Wc[1], n_blocks=len(blocks))


class _Tables(object):
    """off (n + 1), qoff (n), latoff (n + 1), woff (n) as int64 and tl (n) as int32 on the device, uploaded in one copy."""

    def __init__(self, n_pos, qoff, woff, tl):
        n = len(n_pos)
        off = ragged.offsets(n_pos, total=True)
        latoff = ragged.offsets(tl, total=True)
        i64 = np.concatenate([off, np.asarray(qoff, np.int64), latoff, np.asarray(woff, np.int64)])
        raw = np.concatenate([i64.view(np.uint8), np.ascontiguousarray(tl, np.int32).view(np.uint8)])
        self.dev = backend.to_device(raw)
        p = self.dev.ptr
        self.c = _lib.RdecTables(p, p + 8 * (n + 1), p + 8 * (2 * n + 1), p + 8 * (4 * n + 2))
        self.woff = p + 8 * (3 * n + 2)
        self.ttot, self.tltot, self.off = int(off[-1]), int(latoff[-1]), off


def _run_chunk(d, d_in, tb, m, cp, cond, lat0, u0, w_ptr, q, link, bufs, nll_ptr, sum_ptr, y):
    """Every launch of one chunk, on backend.stream().  d: the descriptor with Q = 3 M; d_in: the class-form embed's, with
    Q = Qin, or None for the sample form; q: the classes (class form) or zeros (sample form: the head wants a target)."""
    T, db, tc = d.ttot, C.byref(d), C.byref(tb.c)
    x = bufs.get('x', d.R * T)
    z = bufs.get('z', (d.D // 2) * T)
    skip = bufs.get('skip', d.S * T)
    hit = bufs.get('hit', T, np.int32)
    Pl = bufs.get('P', d.n_blocks * d.D * d.tltot)
    g = bufs.get('g', d.n * d.n_blocks * d.D)
    hits = bufs.get('hits', d.n, np.int64)
    be = None if m['be'] is None else m['be'].ptr
    if d_in is None:
        call('vqvae_rdmol_embed', db, tc, w_ptr, tb.woff, m['We'].ptr, be, x.ptr, _S())
    else:
        _lib.call('vqvae_rdec_embed', C.byref(d_in), tc, q.ptr, m['We'].ptr, be, x.ptr, _S())
    _lib.call('vqvae_rdec_cond_project', db, tc, cond.local.ptr + 4 * cond.Cl * lat0, cp.Wc_all.ptr, Pl.ptr, _S())
    _lib.call('vqvae_rdec_cond_global', db, None if cond.G == 0 else cond.global_vec.ptr + 4 * cond.G * u0, cp.Wc_all.ptr,
              cp.bc_all.ptr, g.ptr, _S())
    nb = d.n_blocks
    for b, (prm, dil) in enumerate(zip(m['blocks'], m['dils'])):
        Wd, _, _, _, Wr, br, Ws, bs = prm
        _lib.call('vqvae_rdec_gate', db, tc, b, dil, x.ptr, Wd.ptr, Pl.ptr, g.ptr, z.ptr, _S())
        last = b == nb - 1                       # the last block's residual output is not computed
        _lib.call('vqvae_rdec_res_skip', db, z.ptr, None if last else Wr.ptr, None if last else br.ptr, Ws.ptr, bs.ptr,
                  None if last else x.ptr, None if last else x.ptr, skip.ptr, 1 if b else 0, _S())
    need = _lib.load().vqvae_rdec_workspace_bytes(db)
    ws = backend.workspace(need)
    # the head's two GEMMs leave y in its `logits`; its softmax nll (overwritten next) and hit mean nothing here
    _lib.call('vqvae_rdec_head', db, tc, q.ptr, skip.ptr, m['W1'].ptr, m['b1'].ptr, m['W2'].ptr, m['b2'].ptr, nll_ptr, hit.ptr,
              y.ptr, ws.ptr, need, _S())
    call('vqvae_rdmol_nll', db, tc, y.ptr, w_ptr, tb.woff, d.Q // 3, int(link.quantize), float(link.log_scale_min), nll_ptr, _S())
    _lib.call('vqvae_rdec_reduce', db, tc, nll_ptr, hit.ptr, sum_ptr, hits.ptr, _S())


# --------------------------------------------------------------------------- #
# the public calls
# --------------------------------------------------------------------------- #
def score_many_mol(wavenet, condition, waves, chunk_bytes=1 << 30, per_sample=False, return_params=False):
    """The likelihood of ``waves`` under ``wavenet``, a ``use_logistic`` WaveNet link on the device, given ``condition`` (a
    generation.LatentCondition from frontend_many / condition_many).

    ``waves``: what ragged.wave_source accepts -- host or device float32 arrays, or a ResidentCorpus / CorpusView read in
    place.  The samples are the targets, so a list of int32 class arrays is a TypeError.  A decoder whose embed reads
    classes (input_dim > 1) gets them from vqvae_mulaw_bins with the streaming path's thresholds.  Returns MolScores.
    ``per_sample``: also the ragged per-sample NLL as a device array with offsets.  ``return_params``: also the mixture
    parameters of every position as host arrays (a test and inspection facility: at most scoring.MAX_LOGIT_COLUMNS
    positions in all).  The result does not depend on ``chunk_bytes``."""
    who = 'score_many_mol'
    from .generation import LatentCondition
    from . import wavenet as wn
    blocks, dims = _check_decoder(wavenet, who)
    if not isinstance(condition, LatentCondition):
        raise TypeError('%s: condition must be a generation.LatentCondition (frontend_many, condition_many), got %r'
                        % (who, type(condition)))
    if condition.Cl + condition.G != dims['Cc']:
        raise ValueError('%s: the condition has %d + %d channels, the decoder projects %d' % (who, condition.Cl, condition.G, dims['Cc']))
    if condition.Cl < 1:
        raise ValueError('%s: the condition has no local channels' % who)
    if scoring._is_classes(waves):
        raise TypeError('%s: waves are int32 class arrays, but the target of a mixture of logistics is the sample itself: '
                        'pass the float32 waves' % who)
    lengths, source = ragged.wave_source(waves, who)
    N = len(lengths)
    if N == 0:
        raise ValueError('%s: no utterances' % who)
    tl = condition.tl.astype(np.int64)
    if len(tl) != N:
        raise ValueError('%s: %d utterances against a condition of %d' % (who, N, len(tl)))
    want = latent_lengths(lengths, condition.upscale)
    if (want != tl).any():
        u = int(np.nonzero(want != tl)[0][0])
        raise ValueError('%s: utterance %d has %d samples, that is %d latent frames, but the condition holds %d for it: '
                         'the condition was made from other waves' % (who, u, lengths[u], want[u], tl[u]))
    n_pos = positions(lengths, tl, condition.upscale, who)
    off_all = ragged.offsets(n_pos, total=True)
    if return_params and int(off_all[-1]) > scoring.MAX_LOGIT_COLUMNS:
        raise ValueError('%s: return_params is an inspection facility for at most %d positions, got %d'
                         % (who, scoring.MAX_LOGIT_COLUMNS, int(off_all[-1])))
    chunks = plan_chunks(n_pos, tl, lengths, dims, chunk_bytes, who)
    lat_off = ragged.offsets(tl, total=True)
    Q, Qin = dims['Q'], dims['Qin']
    m = scoring._params(wavenet, blocks, who)
    if condition.local is None or (condition.G and condition.global_vec is None):
        raise ValueError('%s: the condition is a description only (nothing on the device)' % who)
    with core.using_config('train', False), core.no_backprop_mode():
        cp = wn._build_cproj([wn.BlockParams(*p) for p in m['blocks']], _S())          # Wc of all blocks stacked; bc_all holds bc + bd
        nll_sum = DeviceArray((N,), np.float64)
        nll_all = DeviceArray((int(off_all[-1]),), np.float32) if per_sample else None
        bufs = scoring._Buffers()
        zeros = backend.zeros((int(n_pos.max()) + 1,), np.int32) if Qin == 1 else None   # the head's targets, sample form
        params_out = [] if return_params else None
        for start, stop in chunks:
            n, L = stop - start, lengths[start:stop]
            w_ptr, woff, keep = source(start, stop)
            if Qin == 1:
                q, qoff, d_in = zeros, np.zeros(n, np.int64), None
            else:
                q, qoff = bufs.get('q', int(L.sum()), np.int32), ragged.offsets(L)
                scoring._bin_runs(w_ptr, woff, L, Qin, q)
            tb = _Tables(n_pos[start:stop], qoff, woff, tl[start:stop])
            d = _lib.RdecDesc(n, dims['R'], dims['D'], dims['S'], Q, condition.Cl, condition.G, dims['n_blocks'], condition.upscale,
                              0, tb.ttot, tb.tltot)
            if Qin > 1:
                d_in = _lib.RdecDesc(n, dims['R'], dims['D'], dims['S'], Qin, condition.Cl, condition.G, dims['n_blocks'],
                                     condition.upscale, 0, tb.ttot, tb.tltot)
            nll_ptr = (nll_all.ptr + 4 * int(off_all[start])) if per_sample else bufs.get('nll', tb.ttot).ptr
            y = bufs.get('y', Q * tb.ttot)
            _run_chunk(d, d_in, tb, m, cp, condition, int(lat_off[start]), start, w_ptr, q, wavenet, bufs, nll_ptr,
                       nll_sum.ptr + 8 * start, y)
            if return_params:
                host = y.flat_view(0, Q * tb.ttot, (Q, tb.ttot)).get()
                params_out += ragged.split(host, tb.off)
            del keep
        out = MolScores(nll_sum.get(), n_pos.astype(np.int64), nll_all, off_all if per_sample else None, params_out)
    return out


def evaluate_many_mol(encoder, vq, condition_embed, wavenet, waves, speakers, chunk_bytes=1 << 30, per_sample=False,
                      return_params=False):
    """``frontend_many`` followed by ``score_many_mol`` on the same waves: host waves are uploaded once and both passes
    read them on the device.  ``speakers``: the input's own speaker ids, or any other (the likelihood under another voice)."""
    from .frontend import frontend_many
    _check_decoder(wavenet, 'evaluate_many_mol')
    waves = scoring._device_waves(waves)
    cond = frontend_many(encoder, vq, condition_embed, waves, speakers, chunk_bytes)
    return score_many_mol(wavenet, cond, waves, chunk_bytes, per_sample, return_params)
