"""Held-out likelihood on the device: the teacher-forced decoder pass over a ragged list of utterances
(include/vqvae_ragged_decoder.h states the rule, csrc/ragged_decoder.hip runs it).

    cond = frontend_many(encoder, vq, condition_embed, waves, speakers)
    s = score_many(model.decoder.ema, cond, waves)                 # Scores: nll, count, hits, bits_per_sample, total()
    s = evaluate_many(encoder, vq, condition_embed, wavenet, waves, speakers)
    s = corpus.score(wavenet, cond)                                # a ResidentCorpus / CorpusView read in place

Utterance i with L_i samples and tl_i latent frames contributes n_i = min(upscale * tl_i, L_i - 1) positions: the input at
j is class q[j], the target q[j + 1], the condition column j of the dense tensor.  The utterances' columns lie end to end
with no padding and every tap stays inside its own utterance, so a position's NLL is the same bits alone, in any list,
at any position and for any ``chunk_bytes``.  The per-utterance sums are float64 in one written order.

Everything runs with dropout off under no_backprop_mode.
"""
import ctypes as C
import math

import numpy as np

from . import _lib, backend, core, ragged
from .backend import DeviceArray

_S = backend.stream
_CAP = 1 << 31                     # elements of one ragged activation stay below this
MAX_LOGIT_COLUMNS = 1 << 16        # return_logits: at most this many positions in one call (Q floats each, copied to the host)
REDUCE_LANES = _lib.RAGGED_DECODER_REDUCE_LANES       # the lanes of the per-utterance reduce
MAX_CLASSES = _lib.RAGGED_DECODER_MAX_CLASSES
MAX_DILATION = _lib.RAGGED_DECODER_MAX_DILATION


# --------------------------------------------------------------------------- #
# the host side of the rule
# --------------------------------------------------------------------------- #
def latent_lengths(lengths, upscale):
    """The latent frames of utterances of ``lengths`` samples: the encoder's length rule (log2(upscale) stride-2 stages of
    frontend.conv_out_len) when upscale is a power of two, else lengths // upscale."""
    from .frontend import stage_lengths
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    depth = int(round(math.log2(upscale))) if upscale >= 1 else 0
    if upscale >= 1 and (1 << depth) == int(upscale):
        return stage_lengths(lengths, depth)[-1]
    return lengths // int(upscale)


def positions(lengths, tl, upscale, who='score_many'):
    """n_i = min(upscale * tl_i, L_i - 1), (N,) int64; an utterance with n_i < 1 is a ValueError naming its index."""
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    tl = np.asarray(tl, np.int64).reshape(-1)
    if lengths.shape != tl.shape:
        raise ValueError('%s: %d utterances against %d latent lengths' % (who, lengths.size, tl.size))
    n = np.minimum(int(upscale) * tl, lengths - 1)
    if (n < 1).any():
        u = int(np.nonzero(n < 1)[0][0])
        raise ValueError('%s: utterance %d (%d samples, %d latent frames) has no position to score: an input and a target '
                         'sample are needed' % (who, u, lengths[u], tl[u]))
    return n


def chunk_elements(n, tl, lengths, dims, logits=False):
    """(stages, N) int64: the float32 elements every utterance takes in each buffer of a chunk -- x, z, skip, the head's
    workspace, nll, the latent-rate projection P, the classes, and the logits when they are asked for."""
    n, tl, lengths = (np.asarray(a, np.int64).reshape(-1) for a in (n, tl, lengths))
    rows = [dims['R'] * n, (dims['D'] // 2) * n, dims['S'] * n, dims['S'] * n, n, dims['n_blocks'] * dims['D'] * tl, lengths]
    if logits:
        rows.append(dims['Q'] * n)
    return np.stack(rows)


def plan_chunks(n, tl, lengths, dims, chunk_bytes, logits=False, who='score_many'):
    """Runs [(start, stop), ...] of consecutive utterances whose largest buffer stays within ``chunk_bytes``
    (ragged.plan_runs over chunk_elements).  An utterance that does not fit one chunk alone is a ValueError naming it:
    an utterance is never split across chunks."""
    return plan_elements(chunk_elements(n, tl, lengths, dims, logits), n, chunk_bytes, who)


def plan_elements(per, n, chunk_bytes, who):
    """plan_chunks over a given (stages, N) table of elements."""
    if int(chunk_bytes) < 1:
        raise ValueError('%s: chunk_bytes must be positive, got %r' % (who, chunk_bytes))
    worst = per.max(axis=0)
    bad = np.nonzero((4 * worst > int(chunk_bytes)) | (worst >= _CAP))[0]
    if bad.size:
        u = int(bad[0])
        raise ValueError('%s: utterance %d (%d positions) needs %d bytes in one buffer and does not fit a chunk of %d bytes '
                         '(below 2^31 elements): an utterance is not split across chunks -- raise chunk_bytes or cut it'
                         % (who, u, int(np.asarray(n).reshape(-1)[u]), 4 * int(worst[u]), int(chunk_bytes)))
    return ragged.plan_runs(per, chunk_bytes, cap=_CAP)


def reduce_order(values, lanes=REDUCE_LANES):
    """The reduce's written order on the host, for float64 or integer ``values`` of one utterance: lane t adds elements t,
    t + lanes, ... in ascending order, then s[k] += s[k + h] for h = lanes / 2 .. 1."""
    v = np.asarray(values).reshape(-1)
    acc_t = np.float64 if v.dtype.kind == 'f' else np.int64
    pad = (-v.size) % lanes
    rows = np.concatenate([v.astype(acc_t), np.zeros(pad, acc_t)]).reshape(-1, lanes)
    s = np.zeros(lanes, acc_t)
    for row in rows:
        s = s + row
    h = lanes // 2
    while h >= 1:
        s[:h] = s[:h] + s[h:2 * h]
        h //= 2
    return s[0]


class Scores(object):
    """Per utterance, in the caller's order: ``nll`` float64 (N,) summed negative log-likelihood in nats, ``count`` int64
    (N,) scored positions, ``hits`` int64 (N,) positions whose most likely class is the target.  ``per_sample``: the
    ragged float32 NLL on the device with ``offsets`` (N + 1,), when asked for; ``logits``: list of N host arrays
    (Q, n_i), when asked for."""

    def __init__(self, nll, count, hits, per_sample=None, offsets=None, logits=None):
        self.nll, self.count, self.hits = nll, count, hits
        self.per_sample, self.offsets, self.logits = per_sample, offsets, logits

    def __len__(self):
        return len(self.nll)

    @property
    def bits_per_sample(self):
        return self.nll / self.count / math.log(2.0)

    @property
    def accuracy(self):
        return self.hits / self.count.astype(np.float64)

    def total(self):
        """The corpus-level bits per sample: sum(nll) / sum(count) / ln 2."""
        return float(self.nll.sum() / self.count.sum() / math.log(2.0))

    def sample_nll(self, i):
        """Utterance i's per-sample NLL as a host array (n_i,) (needs per_sample=True)."""
        if self.per_sample is None:
            raise ValueError('Scores.sample_nll: the scores were computed without per_sample=True')
        return self.per_sample.flat_view(int(self.offsets[i]), int(self.count[i])).get()


# --------------------------------------------------------------------------- #
# argument checks
# --------------------------------------------------------------------------- #
def _dev(p, name, who):
    if p is None or p.data is None:
        raise ValueError('%s: parameter %s has not been created yet (call the link once, or load a snapshot)' % (who, name))
    if not backend.is_device(p.data):
        raise ValueError('%s: parameter %s is not on the device: call to_gpu() first' % (who, name))
    return p.data


def _check_decoder(wavenet, who):
    """The refusals that need no parameter: the blocks of a WaveNet link whose pass this is."""
    if getattr(wavenet, 'use_logistic', False):
        raise NotImplementedError('%s: a mixture-of-logistics decoder (use_logistic) is out of scope here: the pass scores '
                                  'the softmax output only' % who)
    return _check_blocks(wavenet, who)


def _check_blocks(wavenet, who):
    """What the ragged decoder asks of the blocks and of the matmul mode, whatever the output (scoring_mol shares it)."""
    blocks = list(wavenet.resnet.children())
    if not blocks:
        raise ValueError('%s: the decoder has no residual blocks' % who)
    for i, b in enumerate(blocks):
        if b.filter_size != 2:
            raise ValueError('%s: block %d has filter_size %d; the ragged decoder runs two-tap dilated convs (filter_size 2) '
                             'only' % (who, i, b.filter_size))
        if not 1 <= b.dilation <= MAX_DILATION:
            raise ValueError('%s: block %d has dilation %d, outside 1 .. %d' % (who, i, b.dilation, MAX_DILATION))
    if _lib.load().vqvae_get_matmul_dtype() == 1:
        raise ValueError("%s: matmul mode 1 ('bfloat16') is not supported by the ragged decoder: an utterance's result must "
                         "not depend on operand rounding; use 'float32', 'float32x3' or 'float32x2'" % who)
    return blocks


def _shape(p, name, who):
    if p is None or p.data is None:
        raise ValueError('%s: parameter %s has not been created yet (call the link once, or load a snapshot)' % (who, name))
    return tuple(p.data.shape)


def _dims(wavenet, blocks, who):
    """dict(R, D, S, Q, Cc, n_blocks) from the parameters' shapes (host or device)."""
    We = _shape(wavenet.embed.W, 'embed.W', who)
    b0 = blocks[0]
    Wd, Wc, Ws = (_shape(p, 'resnet.0.' + n, who) for n, p in (('conv.W', b0.conv.W), ('condition_proj.W', b0.condition_proj.W),
                                                                 ('skip.W', b0.skip.W)))
    W2 = _shape(wavenet.proj2.W, 'proj2.W', who)
    R, Q = We[0], We[1]
    if tuple(We[2:]) not in ((2,), (2, 1)):
        raise ValueError('%s: the embed conv must have two taps, got W %s' % (who, We))
    if W2[0] != Q:
        raise ValueError('%s: the decoder reads %d classes and writes %d: the target is the next input class' % (who, Q, W2[0]))
    if Q > MAX_CLASSES:
        raise ValueError('%s: %d classes; the head keeps a column tile of logits in LDS and takes at most %d' % (who, Q, MAX_CLASSES))
    return dict(R=R, D=Wd[0], S=Ws[0], Q=Q, Cc=Wc[1], n_blocks=len(blocks))


def _params(wavenet, blocks, who):
    """The parameters as device arrays (a ValueError names the first that is not there)."""
    prm = [[_dev(p, 'resnet.%d.%s' % (i, n), who) for n, p in zip(('Wd', 'bd', 'Wc', 'bc', 'Wr', 'br', 'Ws', 'bs'), b.param_list())]
           for i, b in enumerate(blocks)]
    return dict(We=_dev(wavenet.embed.W, 'embed.W', who), be=None if wavenet.embed.b is None else _dev(wavenet.embed.b, 'embed.b', who),
                blocks=prm, dils=[b.dilation for b in blocks],
                W1=_dev(wavenet.proj1.W, 'proj1.W', who), b1=_dev(wavenet.proj1.b, 'proj1.b', who),
                W2=_dev(wavenet.proj2.W, 'proj2.W', who), b2=_dev(wavenet.proj2.b, 'proj2.b', who))


def _is_classes(waves):
    if isinstance(waves, (list, tuple)) and len(waves):
        return all((isinstance(w, np.ndarray) or backend.is_device(w)) and np.dtype(w.dtype) == np.int32 for w in waves)
    return False


_THR = {}


def _thresholds(Q):
    """The streaming path's mu-law thresholds on the device (inputs.mulaw_thresholds), kept per class count."""
    if Q not in _THR:
        from .inputs import mulaw_thresholds
        _THR[Q] = backend.to_device(mulaw_thresholds(Q))
    return _THR[Q]


def _class_source(waves, Q, who):
    """(lengths, fill): fill(start, stop, q) writes the classes of utterances [start, stop) end to end into the int32
    device buffer q and returns what must stay alive until the chunk's launches are enqueued."""
    if _is_classes(waves):
        waves = list(waves)
        for i, w in enumerate(waves):
            if not backend.is_device(w):
                w = waves[i] = np.ascontiguousarray(w).reshape(-1)
                if w.size and (w.min() < 0 or w.max() >= Q):
                    raise ValueError('%s: utterance %d holds class %d, outside [0, %d)' % (who, i, int(w.min() if w.min() < 0 else w.max()), Q))
        sizes = np.array([w.size for w in waves], np.int64)

        def fill(start, stop, q):
            offs = ragged.offsets(sizes[start:stop])
            part = waves[start:stop]
            host = [w for w in part if not backend.is_device(w)]
            if len(host) == len(part):
                flat = np.ascontiguousarray(np.concatenate(part), np.int32)          # named: it must outlive the copy
                _lib.call('vqvae_memcpy_h2d', q.ptr, flat.ctypes.data, flat.nbytes, _S())
                return flat
            for w, o in zip(part, offs):
                if backend.is_device(w):
                    _lib.call('vqvae_memcpy_d2d', q.ptr + 4 * int(o), w.ptr, 4 * w.size, _S())
                else:
                    _lib.call('vqvae_memcpy_h2d', q.ptr + 4 * int(o), w.ctypes.data, 4 * w.size, _S())
            return part

        return sizes, fill
    sizes, source = ragged.wave_source(waves, who)

    def fill(start, stop, q):
        x_ptr, in_off, keep = source(start, stop)
        _bin_runs(x_ptr, in_off, sizes[start:stop], Q, q)
        return keep

    return sizes, fill


def _bin_runs(x_ptr, in_off, L, Q, q):
    """The classes of utterances of ``L`` samples that start at elements ``in_off`` of the float32 buffer at ``x_ptr``,
    end to end into the int32 device buffer q."""
    thr = _thresholds(Q)
    in_off = np.asarray(in_off, np.int64)
    out = ragged.offsets(L)
    u = 0
    while u < len(L):                      # one call per run of utterances that lie end to end in the source
        v = u + 1
        while v < len(L) and in_off[v] == in_off[v - 1] + L[v - 1]:
            v += 1
        _lib.call('vqvae_mulaw_bins', x_ptr + 4 * int(in_off[u]), int(L[u:v].sum()), thr.ptr, thr.size, q.ptr + 4 * int(out[u]), _S())
        u = v


class _Buffers(object):
    """The working set of a chunk, grown to the largest chunk and reused (as frontend._Buffers)."""

    def __init__(self):
        self.bufs = {}

    def get(self, name, n, dtype=np.float32):
        b = self.bufs.get(name)
        if b is None or b.size < n:
            self.bufs[name] = None
            b = self.bufs[name] = DeviceArray((max(int(n), 1),), dtype)
        return b


class _Tables(object):
    """off (n + 1), qoff (n), latoff (n + 1) as int64 and tl (n) as int32 on the device, uploaded in one copy."""

    def __init__(self, n_pos, lengths, tl):
        n = len(n_pos)
        off = ragged.offsets(n_pos, total=True)
        qoff = ragged.offsets(lengths)
        latoff = ragged.offsets(tl, total=True)
        i64 = np.concatenate([off, qoff, latoff])
        raw = np.concatenate([i64.view(np.uint8), np.ascontiguousarray(tl, np.int32).view(np.uint8)])
        self.dev = backend.to_device(raw)
        p = self.dev.ptr
        self.c = _lib.RdecTables(p, p + 8 * (n + 1), p + 8 * (2 * n + 1), p + 8 * (3 * n + 2))
        self.ttot, self.tltot, self.off = int(off[-1]), int(latoff[-1]), off


def _desc(dims, cond, n, ttot, tltot):
    return _lib.RdecDesc(n, dims['R'], dims['D'], dims['S'], dims['Q'], cond.Cl, cond.G, dims['n_blocks'], cond.upscale, 0, ttot, tltot)


def _run_chunk(d, tb, m, cp, cond, lat0, u0, q, bufs, nll_ptr, sum_ptr, hits_ptr, logits):
    """Every launch of one chunk, on backend.stream()."""
    T, db, tc = d.ttot, C.byref(d), C.byref(tb.c)
    x = bufs.get('x', d.R * T)
    z = bufs.get('z', (d.D // 2) * T)
    skip = bufs.get('skip', d.S * T)
    hit = bufs.get('hit', T, np.int32)
    Pl = bufs.get('P', d.n_blocks * d.D * d.tltot)
    g = bufs.get('g', d.n * d.n_blocks * d.D)
    _lib.call('vqvae_rdec_embed', db, tc, q.ptr, m['We'].ptr, None if m['be'] is None else m['be'].ptr, x.ptr, _S())
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
    _lib.call('vqvae_rdec_head', db, tc, q.ptr, skip.ptr, m['W1'].ptr, m['b1'].ptr, m['W2'].ptr, m['b2'].ptr, nll_ptr, hit.ptr,
              None if logits is None else logits.ptr, ws.ptr, need, _S())
    _lib.call('vqvae_rdec_reduce', db, tc, nll_ptr, hit.ptr, sum_ptr, hits_ptr, _S())


# --------------------------------------------------------------------------- #
# the public calls
# --------------------------------------------------------------------------- #
def score_many(wavenet, condition, waves, chunk_bytes=1 << 30, per_sample=False, return_logits=False):
    """The likelihood of ``waves`` under ``wavenet`` (a WaveNet link on the device: ``model.decoder.ema`` or ``.target``)
    given ``condition`` (a generation.LatentCondition from frontend_many / condition_many).

    ``waves``: what ragged.wave_source accepts -- host or device float32 arrays, or a ResidentCorpus / CorpusView read in
    place -- binned on the device with the streaming path's mu-law thresholds (vqvae_mulaw_bins); or a list of int32
    class arrays, taken as already binned.  Returns Scores.  ``per_sample``: also the ragged per-sample NLL as a device
    array with offsets.  ``return_logits``: also the logits of every position as host arrays (a test and inspection
    facility: at most MAX_LOGIT_COLUMNS positions in all).  The result does not depend on ``chunk_bytes``."""
    who = 'score_many'
    from .generation import LatentCondition
    from . import wavenet as wn
    if not isinstance(condition, LatentCondition):
        raise TypeError('%s: condition must be a generation.LatentCondition (frontend_many, condition_many), got %r'
                        % (who, type(condition)))
    blocks = _check_decoder(wavenet, who)
    dims = _dims(wavenet, blocks, who)
    if condition.Cl + condition.G != dims['Cc']:
        raise ValueError('%s: the condition has %d + %d channels, the decoder projects %d' % (who, condition.Cl, condition.G, dims['Cc']))
    if condition.Cl < 1:
        raise ValueError('%s: the condition has no local channels' % who)
    lengths, fill = _class_source(waves, dims['Q'], who)
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
    if return_logits and int(off_all[-1]) > MAX_LOGIT_COLUMNS:
        raise ValueError('%s: return_logits is an inspection facility for at most %d positions, got %d'
                         % (who, MAX_LOGIT_COLUMNS, int(off_all[-1])))
    chunks = plan_chunks(n_pos, tl, lengths, dims, chunk_bytes, bool(return_logits), who)
    lat_off = ragged.offsets(tl, total=True)
    Q = dims['Q']
    m = _params(wavenet, blocks, who)
    if condition.local is None or (condition.G and condition.global_vec is None):
        raise ValueError('%s: the condition is a description only (nothing on the device)' % who)
    with core.using_config('train', False), core.no_backprop_mode():
        cp = wn._build_cproj([wn.BlockParams(*p) for p in m['blocks']], _S())          # Wc of all blocks stacked; bc_all holds bc + bd
        nll_sum = DeviceArray((N,), np.float64)
        hits = DeviceArray((N,), np.int64)
        nll_all = DeviceArray((int(off_all[-1]),), np.float32) if per_sample else None
        bufs = _Buffers()
        logits_out = [] if return_logits else None
        for start, stop in chunks:
            tb = _Tables(n_pos[start:stop], lengths[start:stop], tl[start:stop])
            q = bufs.get('q', int(lengths[start:stop].sum()), np.int32)
            keep = fill(start, stop, q)
            d = _desc(dims, condition, stop - start, tb.ttot, tb.tltot)
            nll_ptr = (nll_all.ptr + 4 * int(off_all[start])) if per_sample else bufs.get('nll', tb.ttot).ptr
            lg = bufs.get('logits', Q * tb.ttot) if return_logits else None
            _run_chunk(d, tb, m, cp, condition, int(lat_off[start]), start, q, bufs, nll_ptr, nll_sum.ptr + 8 * start,
                       hits.ptr + 8 * start, lg)
            if return_logits:
                host = lg.flat_view(0, Q * tb.ttot, (Q, tb.ttot)).get()
                logits_out += ragged.split(host, tb.off)
            del keep
        out = Scores(nll_sum.get(), n_pos.astype(np.int64), hits.get(), nll_all, off_all if per_sample else None, logits_out)
    return out


def evaluate_many(encoder, vq, condition_embed, wavenet, waves, speakers, chunk_bytes=1 << 30, per_sample=False,
                  return_logits=False):
    """``frontend_many`` followed by ``score_many`` on the same waves: host waves are uploaded once and both passes read
    them on the device.  ``speakers``: the input's own speaker ids, or any other (the likelihood under another voice)."""
    from .frontend import frontend_many
    waves = _device_waves(waves)
    cond = frontend_many(encoder, vq, condition_embed, waves, speakers, chunk_bytes)
    return score_many(wavenet, cond, waves, chunk_bytes, per_sample, return_logits)


def _device_waves(waves):
    """``waves`` with every host wave of a list uploaded (one batched copy); a ResidentCorpus / CorpusView as it is."""
    from .corpus import _Utterances
    if isinstance(waves, _Utterances):
        return waves
    waves = list(waves)
    host = [i for i, w in enumerate(waves) if not backend.is_device(w)]
    if host:
        up = backend.to_device_many([np.ascontiguousarray(waves[i], np.float32).reshape(-1) for i in host])
        for i, a in zip(host, up):
            waves[i] = a
    return waves
