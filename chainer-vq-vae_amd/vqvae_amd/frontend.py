"""The front half of generation for MANY utterances per launch: encoder, quantiser and ConditionEmbed's conv stack over
a ragged batch (include/vqvae_ragged.h, csrc/ragged_front.hip), and the discrete codes as a product of their own.

The utterances of a chunk lie end to end along time with no padding; every conv stage is ONE launch over all of them,
and a tap reads only inside its own utterance.  The arithmetic is composition-independent (see the header), so an
utterance's codes and condition are the same bits alone, in any list, at any position and for any ``chunk_bytes``.

    codes = encode_many(encoder, vq, waves)                       # LatentCodes: the tokens of a corpus
    codes = corpus.encode(encoder, vq)                            # ... read in place from a ResidentCorpus / CorpusView
    cond = condition_many(vq, condition_embed, codes, speakers)   # LatentCondition for WaveNet.generate_lockstep
    cond = frontend_many(encoder, vq, condition_embed, waves, speakers)     # both halves in one pass

Everything runs under no_backprop_mode: there is no backward through the ragged front end.
"""
import ctypes as C

import numpy as np

from . import _lib, backend, core, ragged
from .backend import DeviceArray

_S = backend.stream
_CAP = 1 << 31            # elements of one ragged activation stay below this (the planner's promise to the kernels)
_KSP = (4, 2, 1)          # the encoder's (K, stride, pad); dilation 1


def conv_out_len(t):
    """Output length of one encoder stage (K = 4, stride 2, pad 1): (t - 2) // 2 + 1, 0 for t < 2."""
    t = np.asarray(t, np.int64)
    return np.where(t >= 2, (t - 2) // 2 + 1, 0)


def stage_lengths(lengths, depth=6):
    """(depth + 1, N) int64: row s holds the lengths after s encoder stages."""
    rows = [np.asarray(lengths, np.int64).reshape(-1)]
    for _ in range(depth):
        rows.append(conv_out_len(rows[-1]))
    return np.stack(rows)


def plan_chunks(lengths, widths, chunk_bytes):
    """Cuts utterances 0 .. N - 1 greedily, in input order, into runs [(start, stop), ...] of consecutive utterances.

    lengths: (N,) input lengths.  widths: channels of stage 0, 1, ... (stage s has the lengths after s encoder stages).
    A run is closed when adding the next utterance would make some stage larger than ``chunk_bytes`` (4 * width * sum
    of lengths) or reach 2^31 elements.  An utterance that exceeds the byte budget alone forms a run of its own; one
    that reaches 2^31 elements alone is a ValueError."""
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    widths = [int(w) for w in widths]
    if not widths or min(widths) < 1:
        raise ValueError('plan_chunks: widths must be positive channel counts, got %r' % (widths,))
    if int(chunk_bytes) < 1:
        raise ValueError('plan_chunks: chunk_bytes must be positive, got %r' % (chunk_bytes,))
    per = stage_lengths(lengths, len(widths) - 1) * np.asarray(widths, np.int64)[:, None]     # elements per (stage, utterance)
    if (per >= _CAP).any():
        u = int(np.nonzero((per >= _CAP).any(axis=0))[0][0])
        raise ValueError('plan_chunks: utterance %d (%d samples) alone reaches 2^31 elements in one stage' % (u, lengths[u]))
    return ragged.plan_runs(per, chunk_bytes, cap=_CAP)


class LatentCodes(object):
    """The discrete codes of N utterances: ``tl`` (N,) latent lengths, ``offsets`` (N + 1,) int64 with utterance i's codes at
    indices[offsets[i] : offsets[i + 1]], ``indices`` one ragged int32 device buffer, ``k`` the codebook size.

    ``indices`` may be handed over as a host int32 array (what ``load`` does): it is checked against k on the host and
    uploaded when the device buffer is first asked for."""

    def __init__(self, tl, indices, k):
        self.tl = ragged.check_lengths(tl, 'LatentCodes').astype(np.int32)
        self.offsets = ragged.offsets(self.tl, total=True)
        self.k = int(k)
        if self.k < 1:
            raise ValueError('LatentCodes: k must be at least 1, got %r' % (k,))
        total = int(self.offsets[-1])
        self._host = self._dev = None
        if backend.is_device(indices):
            if indices.dtype != np.int32 or indices.size != total:
                raise ValueError('LatentCodes: indices must be int32 with sum(tl) = %d codes, got %r' % (total, indices))
            self._dev = indices
        else:
            idx = np.asarray(indices).reshape(-1)
            if idx.dtype.kind not in 'iu' or idx.size != total:
                raise ValueError('LatentCodes: indices must be integers with sum(tl) = %d codes, got %s of %d'
                                 % (total, idx.dtype, idx.size))
            _check_codes(idx, self.k, 'LatentCodes')
            self._host = idx.astype(np.int32)

    @property
    def indices(self):
        if self._dev is None:
            self._dev = backend.to_device(self._host)
        return self._dev

    def __len__(self):
        return len(self.tl)

    def codes(self, i):
        """Utterance i's codes, a device view (tl[i],) int32."""
        i = int(i)
        if not 0 <= i < len(self.tl):
            raise IndexError('LatentCodes.codes: utterance %d of %d' % (i, len(self.tl)))
        return self.indices.flat_view(int(self.offsets[i]), int(self.tl[i]))

    def _flat(self):
        if self._host is None:
            self._host = self._dev.get().reshape(-1)
        return self._host

    def to_host(self):
        """List of N int32 host arrays (one device-to-host copy, kept)."""
        return ragged.split(self._flat(), self.offsets)

    @staticmethod
    def _path(path):
        path = str(path)
        return path if path.endswith('.npz') else path + '.npz'

    def save(self, path):
        """``tl``, ``indices`` and ``k`` as an .npz file."""
        np.savez(self._path(path), tl=self.tl, indices=self._flat(), k=np.int64(self.k))

    @classmethod
    def load(cls, path):
        """The codes of ``save``; every code is checked against k on the host, the upload waits for the first use."""
        with np.load(cls._path(path)) as f:
            missing = [n for n in ('tl', 'indices', 'k') if n not in f.files]
            if missing:
                raise ValueError('LatentCodes.load: %s lacks %s' % (path, ', '.join(missing)))
            tl, idx, k = f['tl'], np.asarray(f['indices']).reshape(-1), int(f['k'])
        return cls(tl, idx, k)


def _check_codes(idx, k, who):
    if idx.size and (idx.min() < 0 or idx.max() >= k):
        bad = int(np.nonzero((idx < 0) | (idx >= k))[0][0])
        raise ValueError('%s: code %d at position %d is outside the codebook (k = %d)' % (who, int(idx[bad]), bad, k))


# --------------------------------------------------------------------------- #
# argument checks
# --------------------------------------------------------------------------- #
def _device_param(p, name, who):
    if p is None or p.data is None:
        raise ValueError('%s: parameter %s has not been created yet (a lazily shaped link: call it once, or load a snapshot)'
                         % (who, name))
    if not backend.is_device(p.data):
        raise ValueError('%s: parameter %s is not on the device: call to_gpu() first' % (who, name))
    return p.data


def _encoder_params(encoder, who):
    out, cin = [], 1
    for s in range(1, encoder.depth + 1):
        conv = getattr(encoder, 'conv%d' % s)
        W = _device_param(conv.W, 'encoder.conv%d.W' % s, who)
        b = None if conv.b is None else _device_param(conv.b, 'encoder.conv%d.b' % s, who)
        if (conv.ksize[0], conv.stride[0], conv.pad[0], conv.dilate[0]) != _KSP + (1,) or W.shape[1] != cin:
            raise ValueError('%s: encoder.conv%d is not a (4, 1) stride-2 pad-1 conv over %d channels' % (who, s, cin))
        out.append((W, b))
        cin = W.shape[0]
    return out


def _cond_params(condition_embed, d, who):
    from .net import _COND_DILATIONS
    out, cin = [], d
    for i, dil in enumerate(_COND_DILATIONS, start=1):
        conv = getattr(condition_embed, 'local_embed%d' % i)
        W = _device_param(conv.W, 'condition_embed.local_embed%d.W' % i, who)
        b = None if conv.b is None else _device_param(conv.b, 'condition_embed.local_embed%d.b' % i, who)
        if (conv.ksize[0], conv.stride[0], conv.pad[0], conv.dilate[0]) != (3, 1, dil, dil) or W.shape[1] != cin:
            raise ValueError('%s: condition_embed.local_embed%d is not a 3-tap conv of dilation %d over %d channels'
                             % (who, i, dil, cin))
        out.append((W, b, dil))
        cin = W.shape[0]
    E = _device_param(condition_embed.global_embed.W, 'condition_embed.global_embed.W', who)
    return out, E


def _codebook(vq, who):
    return _device_param(vq.W, 'vq.W', who)


def _speakers(speakers, N, n_speaker, who):
    spk = np.asarray(speakers.get() if backend.is_device(speakers) else speakers)
    if spk.dtype.kind not in 'iu' or spk.reshape(-1).shape != (N,):
        raise ValueError('%s: one integer speaker id per utterance (%d), got %s %s' % (who, N, spk.dtype, spk.shape))
    spk = spk.reshape(-1).astype(np.int32)
    if spk.min() < 0 or spk.max() >= n_speaker:
        raise ValueError('%s: speaker ids must be in [0, %d), got %d .. %d' % (who, n_speaker, spk.min(), spk.max()))
    return spk


def _wave_lengths(lengths, depth, who):
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    if lengths.size == 0:
        raise ValueError('%s: no utterances' % who)
    tl = stage_lengths(lengths, depth)[-1]
    if (tl < 1).any():
        u = int(np.nonzero(tl < 1)[0][0])
        raise ValueError('%s: utterance %d has %d samples, too short for one latent frame (%d needed)'
                         % (who, u, lengths[u], 1 << depth))
    return lengths, tl


# --------------------------------------------------------------------------- #
# the device side of one chunk
# --------------------------------------------------------------------------- #
class _Tables(object):
    """The segment tables of one chunk on the device, uploaded in one copy: off_in of stage 0 (n) and, per stage, the
    int64 prefix off (n + 1) and the int32 lengths (n)."""

    def __init__(self, in_off, per_stage_lengths):
        L = np.asarray(per_stage_lengths, np.int64)
        S, n = L.shape
        self.n, self.lengths = n, L
        self.off = np.stack([ragged.offsets(row, total=True) for row in L])
        in_off = np.ascontiguousarray(in_off, np.int64).reshape(-1)
        i64 = np.concatenate([in_off, self.off.reshape(-1)])
        raw = np.concatenate([i64.view(np.uint8), np.ascontiguousarray(L, np.int32).reshape(-1).view(np.uint8)])
        self.dev = backend.to_device(raw)
        self._off0, self._len0 = 8 * in_off.size, 8 * i64.size

    def in_off(self):
        return self.dev.ptr

    def off_ptr(self, s):
        return self.dev.ptr + self._off0 + 8 * s * (self.n + 1)

    def len_ptr(self, s):
        return self.dev.ptr + self._len0 + 4 * s * self.n

    def ttot(self, s):
        return int(self.off[s, -1])


def _conv(tb, x_ptr, x_cstride, off_in_ptr, s_in, s_out, W, b, y_ptr, window, relu, blocked=False):
    K, stride, pad, dil = window
    d = _lib.RaggedConvDesc()
    d.n, d.cin, d.cout = tb.n, W.shape[1], W.shape[0]
    d.K, d.stride, d.pad, d.dil = K, stride, pad, dil
    d.relu, d.blocked_out = int(relu), int(blocked)
    d.ttot_out, d.x_cstride = tb.ttot(s_out), int(x_cstride)
    need = _lib.load().vqvae_ragged_conv_workspace_bytes(C.byref(d))
    ws = backend.workspace(need) if need else None
    _lib.call('vqvae_ragged_conv_fwd', C.byref(d), x_ptr, off_in_ptr, tb.len_ptr(s_in), tb.off_ptr(s_out), W.ptr,
              None if b is None else b.ptr, y_ptr, None if ws is None else ws.ptr, need, _S())


class _Buffers(object):
    """Two ping-pong activation buffers and the gathered e, grown to the largest chunk and reused."""

    def __init__(self):
        self.bufs = [None, None, None]

    def get(self, i, n):
        if self.bufs[i] is None or self.bufs[i].size < n:
            self.bufs[i] = None
            self.bufs[i] = DeviceArray((max(int(n), 1),), np.float32)
        return self.bufs[i]


def _encode_chunk(enc, W, tb, x_ptr, bufs, idx_ptr, want_e, latents=None, hook=None, first=0):
    """Stages 1..6 and the nearest-code search of one chunk.  Returns e (d, Ttot) when ``want_e``; the chunk's z is
    appended to ``latents`` utterance by utterance as host arrays (d, tl_i) when that is a list.  ``hook``: a callable
    handed the chunk's z while it is on the device -- hook(z pointer, elements between its d channel rows, the chunk's
    tables, the index of its first utterance); with None nothing more is launched."""
    from .utils import StraightThrough
    depth = len(enc)
    d, k = W.shape[1], W.shape[0]
    src, cs = x_ptr, 0
    for s in range(1, depth + 1):
        Ws, bs = enc[s - 1]
        y = bufs.get(s & 1, Ws.shape[0] * tb.ttot(s))
        _conv(tb, src, cs, tb.in_off() if s == 1 else tb.off_ptr(s - 1), s - 1, s, Ws, bs, y.ptr, _KSP + (1,), s < depth)
        src, cs = y.ptr, tb.ttot(s)
    T = tb.ttot(depth)
    e = bufs.get(2, d * T) if want_e else None
    lib = _lib.load()
    ws = backend.workspace(lib.vqvae_vq_workspace_bytes(1, d, T, k))
    _lib.call('vqvae_vq_nearest_fwd', src, W.ptr, 1, d, T, k, StraightThrough.mode, idx_ptr, None if e is None else e.ptr,
              None, ws.ptr, ws.nbytes, _S())
    if latents is not None:
        z = DeviceArray((d, T), np.float32, _block=y._block, _ptr=y.ptr).get()
        latents += ragged.split(z, tb.off[depth])
    if hook is not None:
        hook(src, T, tb, first)
    return e


def _condition_chunk(cond, tb, s, e_ptr, bufs, local_ptr):
    """The five condition convs of one chunk at stage ``s`` of its tables; the last writes LatentCondition.local's blocks."""
    T = tb.ttot(s)
    src, which = e_ptr, 1
    for i, (Wc, bc, dil) in enumerate(cond):
        last = i == len(cond) - 1
        y_ptr = local_ptr if last else bufs.get(which, Wc.shape[0] * T).ptr
        _conv(tb, src, T, tb.off_ptr(s), s, s, Wc, bc, y_ptr, (3, 1, dil, dil), True, blocked=last)
        src, which = y_ptr, which ^ 1


def _run(who, encoder, vq, condition_embed, lengths, source, speakers, chunk_bytes, codes_in=None, latents=None, hook=None):
    """The shared driver.  ``source(start, stop)`` -> (device pointer of x, off_in (n,)) for a run of utterances (encode);
    ``codes_in``: LatentCodes instead of an encoder (condition_many); ``hook``: see _encode_chunk (segmental.segment_many).
    Returns (LatentCodes or None, LatentCondition or None)."""
    from .generation import LatentCondition
    W = _codebook(vq, who)
    k, d = W.shape
    enc = None if encoder is None else _encoder_params(encoder, who)
    if enc is not None and enc[-1][0].shape[0] != d:
        raise ValueError('%s: the encoder writes %d channels, the codebook has d = %d' % (who, enc[-1][0].shape[0], d))
    cond = E = None
    if condition_embed is not None:
        cond, E = _cond_params(condition_embed, d, who)
    depth = 0 if enc is None else len(enc)
    if codes_in is not None:
        if not isinstance(codes_in, LatentCodes):
            raise TypeError('%s: codes must be a LatentCodes, got %r' % (who, type(codes_in)))
        if codes_in.k != k:
            raise ValueError('%s: the codes were taken from a codebook of k = %d, this one has k = %d: a code may be >= k'
                             % (who, codes_in.k, k))
        lengths = tl = codes_in.tl.astype(np.int64)
    else:
        lengths, tl = _wave_lengths(lengths, depth, who)
    N = len(tl)
    spk = None
    if cond is not None:
        spk = _speakers(speakers, N, E.shape[0], who)
    Cl = cond[-1][0].shape[0] if cond is not None else 0
    lat_off = ragged.offsets(tl, total=True)
    if enc is not None:
        widths = [1] + [Wb[0].shape[0] for Wb in enc]
        widths[-1] = max(widths[-1], Cl)
    else:
        widths = [max(d, Cl)]
    chunks = plan_chunks(lengths, widths, chunk_bytes)
    with core.using_config('train', False), core.no_backprop_mode():
        indices = DeviceArray((int(lat_off[-1]),), np.int32) if codes_in is None else codes_in.indices
        local = DeviceArray((max(Cl * int(lat_off[-1]), 1),), np.float32) if cond is not None else None
        bufs = _Buffers()
        for start, stop in chunks:
            if enc is not None:
                x_ptr, in_off, keep = source(start, stop)
                tb = _Tables(in_off, stage_lengths(lengths[start:stop], depth))
                e = _encode_chunk(enc, W, tb, x_ptr, bufs, indices.ptr + 4 * int(lat_off[start]), cond is not None, latents, hook, start)
                del keep
            else:
                tb = _Tables(np.zeros(0, np.int64), tl[None, start:stop])
                T = tb.ttot(0)
                e = bufs.get(2, d * T)
                _lib.call('vqvae_ragged_code_gather', indices.ptr + 4 * int(lat_off[start]), W.ptr, T, d, k, e.ptr, _S())
            if cond is not None:
                _condition_chunk(cond, tb, depth, e.ptr, bufs, local.ptr + 4 * Cl * int(lat_off[start]))
        out_cond = None
        if cond is not None:
            G = E.shape[1]
            gv = DeviceArray((N, G), np.float32)
            _lib.call('vqvae_ragged_speaker_gather', backend.to_device(spk).ptr, E.ptr, N, G, E.shape[0], gv.ptr, _S())
            out_cond = LatentCondition(tl.astype(np.int32), Cl, G, condition_embed.upscale_factor, local=local, global_vec=gv)
    out_codes = LatentCodes(tl.astype(np.int32), indices, k) if codes_in is None else codes_in
    return out_codes, out_cond


# --------------------------------------------------------------------------- #
# the public calls
# --------------------------------------------------------------------------- #
def encode_many(encoder, vq, waves, chunk_bytes=1 << 30, return_latents=False):
    """The codes of a list of waveforms: host or device float32 arrays of any shape, each fed whole (as synthesize_many
    feeds them).  One launch per encoder stage and one nearest-code search per chunk of at most ``chunk_bytes`` per stage;
    host waves are uploaded with one copy per chunk.  The result does not depend on ``chunk_bytes``.
    ``return_latents``: also the encoder's output z of every utterance, a list of host arrays (d, tl_i) (one copy back
    per chunk: for analysis and tests), returned as (codes, latents)."""
    sizes, source = ragged.wave_source(waves, 'encode_many')
    latents = [] if return_latents else None
    codes = _run('encode_many', encoder, vq, None, sizes, source, None, chunk_bytes, latents=latents)[0]
    return (codes, latents) if return_latents else codes


def encode_corpus(corpus, encoder, vq, chunk_bytes=1 << 30):
    """``ResidentCorpus.encode`` / ``CorpusView.encode``: the utterances are read in place from the corpus buffer through
    its offsets and lengths; nothing is copied."""
    lengths, source = ragged.wave_source(corpus, 'encode')
    return _run('encode', encoder, vq, None, lengths, source, None, chunk_bytes)[0]


def condition_many(vq, condition_embed, codes, speakers, chunk_bytes=1 << 30):
    """Stored codes -> the latent-rate condition of lockstep generation: the gathered e, ConditionEmbed's conv stack over
    the ragged batch (its last conv writes ``LatentCondition.local`` directly) and the speaker rows as ``global_vec``.
    Re-synthesis with other speakers needs no second encoding."""
    return _run('condition_many', None, vq, condition_embed, None, None, speakers, chunk_bytes, codes_in=codes)[1]


def frontend_many(encoder, vq, condition_embed, waves, speakers, chunk_bytes=1 << 30, return_codes=False):
    """``encode_many`` and ``condition_many`` in one pass over the chunks, the condition stack reading the e the
    nearest-code search already wrote.  Returns the LatentCondition, with ``return_codes`` (condition, codes)."""
    sizes, source = ragged.wave_source(waves, 'frontend_many')
    codes, cond = _run('frontend_many', encoder, vq, condition_embed, sizes, source, speakers, chunk_bytes)
    return (cond, codes) if return_codes else cond
