"""Incremental WaveNet generation -- the queue machinery of WaveNet/modules.py:58-74, 98-110,
232-255 and the sampling loop of generate.py:101-145, on the device.

``WaveNet.initialize(n)`` / ``WaveNet.generate(x, condition)`` keep the reference's step-by-step
call surface (the host supplies the input vector and the condition column, gets the logits).
``WaveNet.generate_sequence`` is the MI355X-native form of generate.py's ``for i in range(...)``:
the whole loop -- network step, sampler, feedback of the sample, step counter -- lives in device
memory, one step's ~45 kernel launches are captured once into a hipGraph and the graph is
replayed, so the host does nothing per sample.
"""
import ctypes as C

import numpy as np

from . import _lib, backend, core, ragged
from .backend import DeviceArray

_S = backend.stream
_INT_MAX = 2 ** 31 - 1


def sampling_controls(n, temperature=None, top_k=None, top_p=None, use_logistic=False, who='generate_sequence'):
    """The sampling controls of include/vqvae_sampling.h as host arrays, validated: each of ``temperature`` (>= 0 and
    finite; 0 = greedy), ``top_k`` (integers >= 0; 0 or >= out_dim = off) and ``top_p`` (in (0, 1]; 1 = off) is None, a
    scalar or a sequence of ``n`` values, one per sequence.  Returns None when all three are None (the caller then takes
    the path it took before the controls existed), else the tuple (float32 (n,), int32 (n,), float32 (n,)) with None in
    the place of a control that was not given.  The mixture-of-logistics output takes a temperature > 0 only.
    Everything else is a ValueError: the device cannot refuse a value, it reads a bad one as neutral."""
    if temperature is None and top_k is None and top_p is None:
        return None

    def per_sequence(v, name, dtype):
        if v is None:
            return None
        a = np.asarray(v)
        if a.dtype.kind not in 'iuf' or (dtype == np.int32 and a.dtype.kind == 'f' and not (a == np.floor(a)).all()):
            raise ValueError('%s: %s must be %s, got %r' % (who, name, 'integers' if dtype == np.int32 else 'numbers', v))
        if a.ndim == 0:
            a = np.full((n,), a)
        if a.shape != (n,):
            raise ValueError('%s: %s must be a scalar or one value per sequence (%d), got shape %s' % (who, name, n, a.shape))
        return a

    t = per_sequence(temperature, 'temperature', np.float32)
    k = per_sequence(top_k, 'top_k', np.int32)
    p = per_sequence(top_p, 'top_p', np.float32)
    if t is not None and not (np.isfinite(t).all() and (t >= 0).all()):
        raise ValueError('%s: temperature must be finite and >= 0, got %r' % (who, temperature))
    if k is not None and not ((k >= 0).all() and (k <= _INT_MAX).all()):
        raise ValueError('%s: top_k must be >= 0 (0 = off), got %r' % (who, top_k))
    if p is not None and not ((p > 0).all() and (p <= 1).all()):          # a NaN fails both comparisons
        raise ValueError('%s: top_p must be in (0, 1] (1 = off), got %r' % (who, top_p))
    if use_logistic:
        if k is not None or p is not None:
            raise ValueError('%s: top_k and top_p truncate a categorical output; the mixture of logistics '
                             '(use_logistic) takes a temperature only' % who)
        if (t == 0).any():
            raise ValueError('%s: temperature 0 (greedy) needs the softmax output; the mixture of logistics '
                             '(use_logistic) takes a temperature > 0' % who)
    return (None if t is None else t.astype(np.float32), None if k is None else k.astype(np.int32),
            None if p is None else p.astype(np.float32))


def _upload_controls(sampling):
    """(GenSampling, the device arrays it points to) for the tuple sampling_controls returns."""
    arrays = [None if a is None else backend.to_device(np.ascontiguousarray(a)) for a in sampling]
    s = _lib.GenSampling()
    s.temperature, s.top_k, s.top_p = [None if a is None else a.ptr for a in arrays]
    return s, arrays


def sampling_layout(mode, out_dim):
    """(uniforms a step draws per sequence, dtype of a sample): one and an int32 class for the softmax output, nr_mix =
    out_dim // 3 and a float32 value for the mixture of logistics."""
    return (1, np.int32) if mode == _lib.GEN_SOFTMAX else (out_dim // 3, np.float32)


# ---- the uniforms drawn on the device (include/vqvae_gen_rng.h, csrc/gen_rng.hip) -------------------------------------
_U32 = np.uint64(0xFFFFFFFF)
_SH32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 on arrays: ``counter`` (..., 4) and ``key`` (..., 2) 32-bit words (broadcast against each other)
    -> the block's four words, uint32 (..., 4).  The definition is in include/vqvae_gen_rng.h."""
    c = np.asarray(counter, np.uint64)
    k = np.asarray(key, np.uint64)
    c0, c1, c2, c3 = (c[..., i] & _U32 for i in range(4))
    k0, k1 = k[..., 0] & _U32, k[..., 1] & _U32
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                      # 32 x 32 bits: the product fits 64
        c0, c1, c2, c3 = (p1 >> _SH32) ^ c1 ^ k0, p1 & _U32, (p0 >> _SH32) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + w0) & _U32, (k1 + w1) & _U32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def words_to_double(a, b):
    """Two 32-bit words -> the double in [0, 1) with 53 random bits (RandomState.random_sample's construction)."""
    a = np.asarray(a, np.uint64) >> np.uint64(5)
    b = np.asarray(b, np.uint64) >> np.uint64(6)
    return (a.astype(np.float64) * 67108864.0 + b.astype(np.float64)) / 9007199254740992.0


def _u64(values, name, who):
    """``values`` as uint64, every one an integer in [0, 2**64)."""
    # a list goes through Python integers: NumPy would make [0, 2**64 - 1] an array of doubles
    a = values if isinstance(values, np.ndarray) else np.asarray(values, dtype=object)
    if a.dtype.kind in 'iu':
        if a.size and int(a.min()) < 0:
            raise ValueError('%s: %s must be in [0, 2**64), got %r' % (who, name, values))
        return a.astype(np.uint64)
    if a.dtype.kind != 'O':
        raise TypeError('%s: %s must be integers, got %r' % (who, name, values))
    import operator
    try:
        flat = [operator.index(v) for v in a.reshape(-1)]
    except TypeError:
        raise TypeError('%s: %s must be integers, got %r' % (who, name, values))
    if any(not 0 <= v < 2 ** 64 for v in flat):
        raise ValueError('%s: %s must be in [0, 2**64), got %r' % (who, name, values))
    return np.array(flat, np.uint64).reshape(a.shape)


class DeviceUniforms(object):
    """The uniforms of generation as a counter-based generator instead of an array (include/vqvae_gen_rng.h): pass it
    where generate_sequence, generate_lockstep and sample_logits take ``uniforms``.  Uniform (sequence, step, j) is
    Philox4x32-10 keyed by ``seed`` and counted by (step, j // 2, the sequence's stream id): it is computed by the kernel
    that consumes it, nothing is drawn, stored or uploaded, and a sequence's draw is the same in any batch, group, slot
    or list position.

    seed: an integer in [0, 2**64).  stream_ids: (N,) integers in [0, 2**64), one per sequence, or None for
    arange(N), resolved when the call knows N.  Two sequences with one id share a stream (a padded group's repeated
    member already does).  ``host`` gives the same numbers as a NumPy array."""

    def __init__(self, seed, stream_ids=None):
        if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)):
            raise TypeError('DeviceUniforms: seed must be an integer, got %r' % (seed,))
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError('DeviceUniforms: seed must be in [0, 2**64), got %r' % (seed,))
        self.seed = int(seed)
        self.stream_ids = None
        if stream_ids is not None:
            ids = _u64(stream_ids, 'stream_ids', 'DeviceUniforms')
            if ids.ndim != 1:
                raise ValueError('DeviceUniforms: stream_ids must be (N,), one id per sequence, got shape %s' % (ids.shape,))
            self.stream_ids = ids

    def ids_for(self, n, who):
        """The (n,) uint64 ids of a call with ``n`` sequences; a ValueError naming ``who`` when the count differs."""
        if self.stream_ids is None:
            return np.arange(n, dtype=np.uint64)
        if len(self.stream_ids) != n:
            raise ValueError('%s: the DeviceUniforms has %d stream_ids for %d sequences' % (who, len(self.stream_ids), n))
        return self.stream_ids

    def resolved(self, n, who):
        """The same generator with its ids spelled out for ``n`` sequences."""
        return DeviceUniforms(self.seed, self.ids_for(n, who))

    def gather(self, idx):
        """The generator of the sequences ``idx`` of a resolved one, repeats included (a group of run_lockstep)."""
        return DeviceUniforms(self.seed, self.stream_ids[np.asarray(idx, np.int64)])

    def host(self, steps, n_uniform=1, ids=None, t0=0):
        """The numbers the device draws, as the float64 array (steps, N, n_uniform) the array form of the calls takes:
        steps t0 .. t0 + steps - 1 of the streams ``ids`` (default: this object's stream_ids)."""
        ids = self.stream_ids if ids is None else _u64(ids, 'ids', 'DeviceUniforms.host')
        if ids is None:
            raise ValueError('DeviceUniforms.host: no stream_ids were given, so N is not known: pass ids')
        if ids.ndim != 1:
            raise ValueError('DeviceUniforms.host: ids must be (N,), got shape %s' % (ids.shape,))
        steps, n_uniform, t0 = int(steps), int(n_uniform), int(t0)
        if steps < 0 or n_uniform < 1 or t0 < 0 or t0 + steps > _INT_MAX:
            raise ValueError('DeviceUniforms.host: needs steps >= 0, n_uniform >= 1 and steps inside 0..2**31 - 1, got %d, %d, t0 %d'
                             % (steps, n_uniform, t0))
        pairs = (n_uniform + 1) // 2
        t = np.arange(t0, t0 + steps, dtype=np.uint64)[:, None, None]
        jb = np.arange(pairs, dtype=np.uint64)[None, None, :]
        lo, hi = (ids & _U32)[None, :, None], (ids >> _SH32)[None, :, None]
        counter = np.stack(np.broadcast_arrays(t, jb, lo, hi), axis=-1)
        w = philox4x32_10(counter, np.array([self.seed & 0xFFFFFFFF, self.seed >> 32], np.uint64))
        u = words_to_double(w[..., 0::2], w[..., 1::2])                  # (steps, N, pairs, 2): uniforms 2 jb, 2 jb + 1
        return np.ascontiguousarray(u.reshape(steps, len(ids), 2 * pairs)[:, :, :n_uniform])

    def upload(self, n, who):
        """(GenRng, what it points to) for a call with ``n`` sequences: the ids go to the device as (n,) uint64, or stay
        NULL (the identity) when none were given."""
        ids = self.ids_for(n, who)
        dev = None if self.stream_ids is None else backend.to_device(np.ascontiguousarray(ids, dtype=np.uint64))
        r = _lib.GenRng()
        r.seed, r.ids = self.seed, None if dev is None else dev.ptr
        return r, dev


def sample_logits(logits, uniforms, mode=_lib.GEN_SOFTMAX, temperature=None, top_k=None, top_p=None, log_scale_min=-40.0,
                  return_probs=False, step=0):
    """The sampler of a generation step on logits of the caller's own (vqvae_sample_logits): device float32 (n, out_dim),
    host doubles ``uniforms`` (n,) for the softmax output or (n, nr_mix) for the mixture of logistics, the controls as in
    sampling_controls.  Returns the device array (n,) of int32 classes or float32 values (and, with ``return_probs``, the
    filtered probabilities (n, out_dim) the draw used; softmax output only).
    ``uniforms`` may be a DeviceUniforms: sequence q then draws the uniforms of its stream at step ``step``
    (vqvae_sample_logits_rng); with an array ``step`` is not read."""
    backend.require_device(logits)
    n, out_dim = logits.shape
    n_uniform, dtype = sampling_layout(mode, out_dim)
    sampling = sampling_controls(n, temperature, top_k, top_p, mode != _lib.GEN_SOFTMAX, 'sample_logits')
    rng = None
    if isinstance(uniforms, DeviceUniforms):
        if not 0 <= int(step) <= _INT_MAX:
            raise ValueError('sample_logits: step must be in [0, 2**31), got %r' % (step,))
        rng, keep_ids = uniforms.upload(n, 'sample_logits')
    else:
        u = np.ascontiguousarray(uniforms, dtype=np.float64).reshape(n, -1)
        u_dev = backend.to_device(u.reshape(-1))
    out = backend.zeros((n,), dtype)
    probs = DeviceArray((n, out_dim), np.float32) if return_probs else None
    s, keep = (None, None) if sampling is None else _upload_controls(sampling)
    tail = (None if s is None else C.byref(s), out.ptr, None if probs is None else probs.ptr, _S())
    if rng is not None:
        _lib.call('vqvae_sample_logits_rng', logits.ptr, n, out_dim, mode, float(log_scale_min), C.byref(rng), int(step),
                  max(n_uniform, 1), *tail)
    else:
        _lib.call('vqvae_sample_logits', logits.ptr, n, out_dim, mode, float(log_scale_min), u_dev.ptr, u.shape[1], *tail)
    backend.synchronize()                  # the uniforms or the stream ids, and the control arrays, go out of scope here
    return (out, probs) if return_probs else out


class LatentCondition(object):
    """The condition of N sequences at the latent rate, for WaveNet.generate_lockstep (include/vqvae_gen_cond.h).

    The full-rate condition (N, Cc, T) of net.py:54-63 is the x``upscale`` align-corners linear up-sampling of a local
    tensor (Cl, Tl_i) per sequence plus a speaker vector (G,) that is constant in time, Cc = Cl + G.  This object holds
    those two and nothing at the sample rate: ``local`` one ragged float32 device buffer, sequence i a row-major
    (Cl, tl[i]) block at ``local_off[i]`` with no padding to the longest, ``global_vec`` (N, G).  Lockstep generation
    computes the one condition column a step reads from them, at the head of the step
    (csrc/generate_cond.hip), with the bits the dense tensor would hold.
      dense   4 Cc N Tmax bytes (``dense_nbytes``; Tmax = upscale max(tl)): 2 560 bytes per sample for the default model
      latent  4 Cl sum(tl) + 4 G N bytes (``nbytes``): 32 bytes per sample
    generate_sequence, generate_batch and generate run persistent or host-stepped forms that read the dense tensor:
    they refuse this object; ``dense()`` gives them (and tests) the tensor."""
    ndim = 3

    def __init__(self, tl, Cl, G, upscale, local=None, global_vec=None):
        """The description alone (``local`` and ``global_vec`` None) is enough to plan a run; from_latents and
        from_condition fill the device buffers in."""
        tl = ragged.check_lengths(tl, 'LatentCondition')
        if int(Cl) < 0 or int(G) < 0 or int(Cl) + int(G) < 1 or int(upscale) < 1:
            raise ValueError('LatentCondition: needs Cl >= 0, G >= 0, Cl + G >= 1 and upscale >= 1, got %r, %r, %r' % (Cl, G, upscale))
        if int(upscale) * int(tl.max()) > _INT_MAX:
            raise ValueError('LatentCondition: upscale * max(tl) must fit a 32-bit step counter')
        self.tl = tl.astype(np.int32)
        self.Cl, self.G, self.upscale = int(Cl), int(G), int(upscale)
        sizes = self.Cl * self.tl.astype(np.int64)
        self.local_off = ragged.offsets(sizes)
        self.local_size = int(sizes.sum())
        self.local, self.global_vec = local, global_vec
        self._tables = None

    # ---- what a dense array of the same condition would answer ----
    @property
    def shape(self):
        return (len(self.tl), self.Cl + self.G, self.upscale * int(self.tl.max()))

    @property
    def lengths(self):
        """Samples of every sequence, (N,) int64: upscale * tl."""
        return self.upscale * self.tl.astype(np.int64)

    @property
    def nbytes(self):
        return 4 * self.local_size + 4 * self.G * len(self.tl)

    @property
    def dense_nbytes(self):
        N, Cc, Tmax = self.shape
        return 4 * Cc * N * Tmax

    # ---- constructors ----
    @classmethod
    def from_latents(cls, latents, global_vec, upscale):
        """latents: list of N float32 device arrays (Cl, Tl_i[, 1]), Tl_i >= 1; global_vec: float32 device array (N, G), the
        speaker embedding row of every sequence.  The latents are copied into one ragged buffer (N copies, batched)."""
        latents = list(latents)
        if not latents:
            raise ValueError('LatentCondition.from_latents: no sequences')
        shapes = [tuple(a.shape[:2]) if len(a.shape) in (2, 3) and tuple(a.shape[2:]) in ((), (1,)) else None for a in latents]
        if any(sh is None for sh in shapes):
            raise ValueError('LatentCondition.from_latents: every latent must be (Cl, Tl[, 1]), got %s' % [tuple(a.shape) for a in latents])
        Cl = shapes[0][0]
        if any(sh[0] != Cl for sh in shapes):
            raise ValueError('LatentCondition.from_latents: the latents have different channel counts: %s' % sorted(set(sh[0] for sh in shapes)))
        if any(sh[1] < 1 for sh in shapes):
            raise ValueError('LatentCondition.from_latents: a latent of 0 frames (shapes %s)' % shapes)
        N = len(latents)
        if len(global_vec.shape) != 2 or global_vec.shape[0] != N:
            raise ValueError('LatentCondition.from_latents: global_vec must be (N, G) = (%d, G), got %s' % (N, tuple(global_vec.shape)))
        self = cls([sh[1] for sh in shapes], Cl, global_vec.shape[1], upscale)
        backend.require_device(global_vec, *latents)
        self.local = DeviceArray((max(self.local_size, 1),), np.float32)
        backend.copy_many([(self.local.flat_view(int(o), a.size), a.reshape(-1)) for o, a in zip(self.local_off, latents)])
        self.global_vec = global_vec
        return self

    @classmethod
    def from_condition(cls, cond, local_dim=None, upscale=None):
        """From what ConditionEmbed returns for B sequences of equal length, without the full-rate tensor being made: a
        functions.LazyUpsampled, whose ``latent`` (B, Cl + G, Tl) = [local | speaker broadcast] is split into the local
        blocks and column 0 of the speaker rows (``local_dim`` = Cl defaults to what the tensor's producer recorded); or
        the dense (B, Cl + G, upscale[, 1]) tensor ConditionEmbed returns for ONE latent frame, whose column 0 is that
        frame (``local_dim`` and ``upscale`` are needed then).  Any other dense tensor is a TypeError: the latent
        tensor cannot be recovered from its up-sampling."""
        from .functions import LazyUpsampled
        if isinstance(cond, LazyUpsampled):
            src, up, Tl = cond.latent, cond.upscale, cond.latent.shape[2]
            local_dim = cond.local_dim if local_dim is None else local_dim
        else:
            backend.require_device(cond)
            if upscale is None or len(cond.shape) < 3 or cond.shape[2] != int(upscale):
                raise TypeError('LatentCondition.from_condition takes a LazyUpsampled condition (or the dense condition of one '
                                'latent frame, (B, Cc, upscale), with local_dim and upscale), got %r' % (cond,))
            src, up, Tl = cond, int(upscale), 1       # only column 0 of its `upscale` columns is taken
        if local_dim is None:
            raise ValueError('LatentCondition.from_condition: local_dim (Cl) is not known for this tensor, pass it')
        B, Cc, Ts = src.shape[:3]
        Cl = int(local_dim)
        if not 0 <= Cl <= Cc:
            raise ValueError('LatentCondition.from_condition: local_dim %d outside 0..%d' % (Cl, Cc))
        self = cls([Tl] * B, Cl, Cc - Cl, up)
        self.local = DeviceArray((max(self.local_size, 1),), np.float32)
        self.global_vec = DeviceArray((B, max(self.G, 1)), np.float32).flat_view(0, B * self.G, (B, self.G))
        for b in range(B):
            if Cl:                                        # rows 0..Cl-1 of the sequence, the first Tl of their Ts columns
                _lib.call('vqvae_memcpy2d_d2d', self.local.ptr + 4 * b * Cl * Tl, 4 * Tl, src.ptr + 4 * b * Cc * Ts, 4 * Ts,
                          4 * Tl, Cl, _S())
            if self.G:                                    # column 0 of rows Cl..Cc-1
                _lib.call('vqvae_memcpy2d_d2d', self.global_vec.ptr + 4 * b * self.G, 4, src.ptr + 4 * (b * Cc + Cl) * Ts,
                          4 * Ts, 4, self.G, _S())
        return self

    @classmethod
    def concatenate(cls, parts):
        """The sequences of several LatentConditions (same Cl, G and upscale) as one, in order: two batched copies per part."""
        parts = list(parts)
        if not parts or any((p.Cl, p.G, p.upscale) != (parts[0].Cl, parts[0].G, parts[0].upscale) for p in parts):
            raise ValueError('LatentCondition.concatenate: needs parts of one Cl, G and upscale')
        self = cls(np.concatenate([p.tl for p in parts]), parts[0].Cl, parts[0].G, parts[0].upscale)
        N, G = len(self.tl), self.G
        self.local = DeviceArray((max(self.local_size, 1),), np.float32)
        self.global_vec = DeviceArray((N, max(G, 1)), np.float32).flat_view(0, N * G, (N, G))
        pairs, off, row = [], 0, 0
        for p in parts:
            n = len(p.tl)
            pairs.append((self.local.flat_view(off, p.local_size), p.local.flat_view(0, p.local_size)))
            pairs.append((self.global_vec.flat_view(row * G, n * G), p.global_vec.flat_view(0, n * G)))
            off, row = off + p.local_size, row + n
        backend.copy_many(pairs)
        return self

    # ---- the device side ----
    def tables(self):
        """(local_off, tl) on the device, uploaded once."""
        if self._tables is None:
            self._tables = (backend.to_device(self.local_off), backend.to_device(self.tl))
        return self._tables

    def struct(self, column, col_seq=None):
        """The vqvae_gen_latent_cond of this condition writing to ``column``."""
        if self.local is None or self.global_vec is None:
            raise RuntimeError('LatentCondition: no device data (built from its description alone)')
        off, tl = self.tables()
        c = _lib.GenLatentCond()
        c.local, c.local_off, c.tl, c.global_vec = self.local.ptr, off.ptr, tl.ptr, self.global_vec.ptr
        c.col_seq = None if col_seq is None else col_seq.ptr
        c.column = column.ptr
        c.n_seq, c.Cl, c.G, c.upscale = len(self.tl), self.Cl, self.G, self.upscale
        return c

    def dense(self):
        """The condition as the other paths take it: the float32 device array (N, Cc, Tmax), sequence i expanded to its
        upscale * tl[i] samples by vqvae_upsample_linear_fwd and vqvae_embed_broadcast_fwd (the kernels ConditionEmbed's
        full-rate form runs) and zero-padded to the longest."""
        from .functions import resize_tables
        if self.local is None or self.global_vec is None:
            raise RuntimeError('LatentCondition: no device data (built from its description alone)')
        N, Cc, Tmax = self.shape
        Cl, G = self.Cl, self.G
        ids = backend.to_device(np.arange(N, dtype=np.int32))

        def expand(y, q, B, Tl, T):
            tb = resize_tables(Tl, T)
            if Cl:
                _lib.call('vqvae_upsample_linear_fwd', self.local.ptr + 4 * int(self.local_off[q]), B, Cl, Tl, T, tb['v0'].ptr,
                          tb['v1'].ptr, tb['w0'].ptr, tb['w1'].ptr, y.ptr, Cc * T, _S())
            if G:
                _lib.call('vqvae_embed_broadcast_fwd', self.global_vec.ptr, ids.ptr + 4 * q, B, G, T, y.ptr + 4 * Cl * T, Cc * T, _S())

        if (self.tl == self.tl[0]).all():                 # equal lengths: the blocks are one (N, Cl, Tl) tensor
            out = DeviceArray((N, Cc, Tmax), np.float32)
            expand(out, 0, N, int(self.tl[0]), Tmax)
            return out
        keep = []

        def alone(q):                                      # sequence q expanded on its own, (Cc, T_q), kept until the copies are done
            Tl = int(self.tl[q])
            keep.append(DeviceArray((Cc, self.upscale * Tl), np.float32))
            expand(keep[-1], q, 1, Tl, self.upscale * Tl)
            return keep[-1]

        out = ragged.pack_padded(map(alone, range(N)), self.lengths, Cc, Tmax)     # zeroes the output, then walks the map
        backend.synchronize()                              # the per-sequence buffers go out of scope here
        return out


def refuse_latent(condition, who):
    """The paths that read the dense condition say so instead of failing on an attribute."""
    if isinstance(condition, LatentCondition):
        raise TypeError('%s reads the full-rate condition tensor (a persistent launch runs thousands of steps and cannot '
                        'take a per-step column): pass condition.dense(), or use generate_lockstep, which takes a '
                        'LatentCondition as it is' % who)


def refuse_device_uniforms(uniforms, who):
    if isinstance(uniforms, DeviceUniforms):
        raise TypeError('%s runs persistent launches only, which read an array of uniforms: use generate_lockstep (any number '
                        'of sequences) or generate_sequence (n <= 4), which take a DeviceUniforms, or pass its .host(...) array'
                        % who)


def _uniform_source(uniforms, n, columns, steps, n_uniform):
    """The uniforms of ``n`` sequences that run ``steps`` steps in a state of ``columns`` columns, a host array or a
    DeviceUniforms -> (the device array the descriptor points at or None, the GenRng the step draws from or None, what
    the GenRng points to).  Up to 4 columns run the matrix-vector kernels or the persistent kernel, which read an array:
    a DeviceUniforms fills it on the device (at most steps * 4 * n_uniform doubles) and the generator is dropped.  More
    columns draw inside the step's finishing launch and have no array."""
    count = steps * n * n_uniform
    if isinstance(uniforms, DeviceUniforms):
        rng, ids = uniforms.upload(n, 'generate_sequence' if columns <= _lib.GEN_MAX_N else 'generate_lockstep')
        if columns > _lib.GEN_MAX_N:
            return None, rng, ids
        u_dev = DeviceArray((max(1, count),), np.float64)
        _lib.call('vqvae_gen_rng_fill', C.byref(rng), 0, steps, n, n_uniform, u_dev.ptr, _S())
        return u_dev, None, ids
    u = np.ascontiguousarray(uniforms, dtype=np.float64).reshape(-1)
    if u.size < count:
        raise ValueError('generate_sequence: need %d uniform doubles (steps, n, %d), got %d' % (count, n_uniform, u.size))
    return backend.to_device(u[:max(1, count)]), None, None


def step_launcher(d, smp=None, rng=None, table=None, lat=None):
    """The callable that issues one step of the descriptor ``d`` on the main stream: the entry point that goes with the
    sampling controls ``smp`` (GenSampling), the generator ``rng`` (GenRng) and the slot table ``table`` (GenSlots), each
    None when absent, and, for a latent condition, the launch that computes the step's condition column (``lat``, a
    GenLatentCond) in front of it.  The structs are read at every call."""
    dp, sp, rp, tp = [None if s is None else C.byref(s) for s in (d, smp, rng, table)]
    if table is not None and rng is not None:
        name, args = 'vqvae_wavenet_gen_step_slots_rng', (dp, tp, sp, rp)
    elif table is not None:
        name, args = 'vqvae_wavenet_gen_step_slots', (dp, tp, sp)
    elif rng is not None:
        name, args = 'vqvae_wavenet_gen_step_rng', (dp, sp, rp)
    elif smp is not None:
        name, args = 'vqvae_wavenet_gen_step_sampled', (dp, sp)
    else:
        name, args = 'vqvae_wavenet_gen_step', (dp,)

    def step():
        if lat is not None:               # with a table: reads what vqvae_gen_slots_init or the previous tick's scheduler left
            _lib.call('vqvae_gen_cond_column', C.byref(lat), dp, tp, _S())
        _lib.call(name, *(args + (_S(),)))
    return step


class Replay(object):
    """``steps`` calls of ``step`` on the main stream.  run(0) issues them eagerly (profilers, debugging); run(graph_steps)
    captures per = min(graph_steps, steps) of them as a hipGraph and launches it ceil(steps / per) times, the surplus
    steps being device no-ops; both synchronise.  launch() is one more launch of the graph, past the end a device
    no-op; close() synchronises and destroys the graph, whatever happened before."""

    def __init__(self, step, steps):
        self.step, self.steps, self.graph = step, steps, None

    def run(self, graph_steps=8):
        if not graph_steps:
            for _ in range(self.steps):
                self.step()
        elif self.steps:
            per = max(1, min(int(graph_steps), self.steps))
            graph = C.c_void_p()
            _lib.call('vqvae_graph_capture_begin', _S())
            try:
                for _ in range(per):
                    self.step()
            finally:
                _lib.call('vqvae_graph_capture_end', _S(), C.byref(graph))
            self.graph = graph
            for _ in range((self.steps + per - 1) // per):
                self.launch()
        backend.synchronize()

    def launch(self):
        _lib.call('vqvae_graph_launch', self.graph, _S())

    def close(self):
        graph, self.graph = self.graph, None
        if graph is not None:
            try:
                backend.synchronize()
            finally:
                _lib.call('vqvae_graph_destroy', graph)


def _check_persistent(ws, hint=''):
    """The status word at the head of a persistent launch's workspace: non-zero when a bounded spin ran out."""
    status = int(ws.flat_view(0, 1).get()[0])
    if status:
        raise RuntimeError('persistent generation kernel gave up waiting (status %d)%s' % (status, hint))


class GenerationState(object):
    """Device state behind WaveNet.initialize(n): zero queues (modules.py:58-67, 232-244) as
    per-block rings of ``dilation`` slots, the 2-sample embed queue, the step counter."""
    max_n = _lib.GEN_MAX_N

    def __init__(self, wavenet, n):
        if not 1 <= n <= self.max_n:
            raise ValueError('generation runs 1..%d sequences in lockstep (generate.py:42 runs 1), got %d'
                             % (self.max_n, n))
        blocks = list(wavenet.resnet.children())
        for p in wavenet.params():
            if p.data is None:
                raise RuntimeError('WaveNet.initialize: parameters are not initialised')
            backend.require_device(p.data)
        b0 = blocks[0]
        if b0.filter_size != 2:
            raise NotImplementedError('incremental generation supports filter_size == 2 (params.py:31)')
        self.n = n
        # the state holds raw device pointers of the weights: keep their buffers alive and
        # remember which parameter layout / contents they belong to
        self._weights = [p.data for p in wavenet.params()]
        self._epochs = (core.param_epoch('layout'), core.param_epoch('load'))
        self.input_dim = wavenet.embed.W.shape[1]
        self.residual = wavenet.embed.W.shape[0]
        self.dilated = b0.conv.W.shape[0]
        self.skip = b0.skip.W.shape[0]
        self.cond_dim = b0.condition_proj.W.shape[1]
        self.out_dim = wavenet.proj2.W.shape[0]
        f32 = np.float32
        self.step = backend.zeros((1,), np.int32)
        self.x_cur = backend.zeros((n, self.input_dim), f32)
        self.x_prev = backend.zeros((n, self.input_dim), f32)
        self.h0 = backend.zeros((n, self.residual), f32)
        self.h1 = backend.zeros((n, self.residual), f32)
        self.z = backend.zeros((n, self.dilated // 2), f32)
        self.skip_acc = backend.zeros((n, self.skip), f32)
        self.s1 = backend.zeros((n, self.skip), f32)
        self.logits = backend.zeros((n, self.out_dim), f32)
        self.rings = [backend.zeros((b.dilation, n, self.residual), f32) for b in blocks]
        self._blocks = (_lib.GenBlock * len(blocks))()
        for gb, b, ring in zip(self._blocks, blocks, self.rings):
            gb.conv_W, gb.conv_b = b.conv.W.data.ptr, b.conv.b.data.ptr
            gb.cond_W, gb.cond_b = b.condition_proj.W.data.ptr, b.condition_proj.b.data.ptr
            gb.res_W, gb.res_b = b.res.W.data.ptr, b.res.b.data.ptr
            gb.skip_W, gb.skip_b = b.skip.W.data.ptr, b.skip.b.data.ptr
            gb.ring, gb.dilation = ring.ptr, b.dilation
        d = _lib.GenDesc()
        d.n, d.n_blocks = n, len(blocks)
        d.input_dim, d.residual, d.dilated, d.skip = self.input_dim, self.residual, self.dilated, self.skip
        d.cond_dim, d.out_dim = self.cond_dim, self.out_dim
        d.log_scale_min = float(wavenet.log_scale_min)
        d.embed_W, d.embed_b = wavenet.embed.W.data.ptr, wavenet.embed.b.data.ptr
        d.proj1_W, d.proj1_b = wavenet.proj1.W.data.ptr, wavenet.proj1.b.data.ptr
        d.proj2_W, d.proj2_b = wavenet.proj2.W.data.ptr, wavenet.proj2.b.data.ptr
        d.blocks = self._blocks
        for name in ('step', 'x_cur', 'x_prev', 'h0', 'h1', 'z', 'skip_acc', 's1', 'logits'):
            setattr(d, name, getattr(self, name).ptr)
        d.sample_mode = _lib.GEN_NONE
        d.max_steps = _INT_MAX
        self.desc = d
        self._bound = []

    def bind(self, cond, uniforms, n_uniform, forced, out, logits_out, sample_mode, max_steps, keep=()):
        """The per-run fields of the descriptor, written here and nowhere else; returns the descriptor.
        ``cond``: the dense condition (rows, condition_dim, T), read at the sequence's step, or a column buffer
        (rows, condition_dim) that a launch in front of the step fills.  ``uniforms``, ``forced``, ``out`` (rows, T) and
        ``logits_out`` are device arrays or None.  The descriptor holds raw pointers: every array given, and whatever
        ``keep`` lists besides (what the structs next to the descriptor point to), stays alive until the next bind."""
        d = self.desc
        if cond.ndim == 3:
            Cc, T = cond.shape[1:]
            d.cond, d.cond_bstride, d.cond_cstride, d.cond_follows_step = cond.ptr, Cc * T, T, 1
        else:
            d.cond, d.cond_bstride, d.cond_cstride, d.cond_follows_step = cond.ptr, cond.shape[1], 1, 0
        d.uniforms, d.n_uniform = None if uniforms is None else uniforms.ptr, n_uniform
        d.forced_next = None if forced is None else forced.ptr
        d.out, d.out_bstride = (None, 0) if out is None else (out.ptr, out.shape[1])
        d.logits_out = None if logits_out is None else logits_out.ptr
        d.sample_mode, d.max_steps = sample_mode, max_steps
        self._bound = [cond, uniforms, forced, out, logits_out] + list(keep)
        return d

    # ---- reference-shaped single step: WaveNet.generate(x, condition) (modules.py:246-255) ----
    def step_logits(self, x, condition):
        n = self.n
        if x.size != n * self.input_dim:
            raise ValueError('generate: x must hold (n, input_dim, 1, 1) = (%d, %d, 1, 1) values, got %s'
                             % (n, self.input_dim, x.shape))
        if condition.size != n * self.cond_dim:
            raise ValueError('generate: condition must hold (n, condition_dim, 1, 1) = (%d, %d, 1, 1) '
                             'values, got %s' % (n, self.cond_dim, condition.shape))
        self.x_cur.copy_from(x)
        d = self.bind(condition.reshape(n, self.cond_dim), None, 1, None, None, None, _lib.GEN_NONE, _INT_MAX, keep=(x,))
        step_launcher(d)()
        return self.logits.copy().reshape(n, self.out_dim, 1, 1)

    # ---- the whole loop of generate.py:105-145 on the device ----------------------------------
    def run(self, condition, uniforms, mode, n_steps=None, forced=None, return_logits=False,
            graph_steps=8, persistent=False, chunk=4096, sampling=None, col_seq=None):
        """``sampling``: None or the tuple of sampling_controls(n, ...).  With controls every step ends in the filtered
        sampler of csrc/sampling.hip and ``persistent`` is not honoured: the persistent kernel has no filtered form, the
        run is a replayed hipGraph of per-step launches (step_launcher picks the entry point).
        ``condition`` may be a LatentCondition (per-step launches only): every step then starts with the launch that
        computes its condition column, and ``col_seq`` (n,) int32 on the device, or None for the identity, says which
        of the object's sequences sits in which column.
        ``uniforms`` may be a DeviceUniforms with one stream id per column: n <= 4 fills the array on the device and runs
        as with an array, more columns draw in the finishing launch (_uniform_source)."""
        n = self.n
        latent = isinstance(condition, LatentCondition)
        if latent:
            if persistent:
                refuse_latent(condition, 'the persistent kernel')
            if condition.shape[1] != self.cond_dim or (col_seq is None and condition.shape[0] != n):
                raise ValueError('generate_lockstep: the latent condition must be (n, condition_dim, T) = (%d, %d, T), got %s'
                                 % (n, self.cond_dim, condition.shape))
        elif condition.ndim == 4:
            condition = condition.reshape(condition.shape[:3])
        if not latent and condition.shape[:2] != (n, self.cond_dim):
            raise ValueError('generate_sequence: condition must be (n, condition_dim, T[, 1]) = (%d, %d, T), got %s'
                             % (n, self.cond_dim, condition.shape))
        T = condition.shape[2]
        steps = T - 1 if n_steps is None else int(n_steps)          # generate.py:105
        if not 0 <= steps <= T:
            raise ValueError('generate_sequence: n_steps must be in [0, %d]' % T)
        n_uniform, dtype = sampling_layout(mode, self.out_dim)
        u_dev, rng, ids = _uniform_source(uniforms, n, n, steps, n_uniform)
        out = backend.zeros((n, T), dtype)                                   # generate.py:103
        forced_dev = None if forced is None else backend.to_device(
            np.ascontiguousarray(forced, dtype=dtype).reshape(-1)[:steps * n])
        logits_out = DeviceArray((max(steps, 1), n, self.out_dim), np.float32) if return_logits else None
        cond, lat = condition, None
        if latent:
            # the step reads the compact column its first launch wrote: (n, cond_dim), unit stride, no time axis
            cond = backend.zeros((n, self.cond_dim), np.float32)
            lat = condition.struct(cond, col_seq)
        if int(self.step.get()[0]) != 0:
            raise RuntimeError('generate_sequence starts from fresh queues: call initialize(n) first')
        smp, controls = (None, None) if sampling is None else _upload_controls(sampling)
        d = self.bind(cond, u_dev, n_uniform, forced_dev, out, logits_out, mode, steps, keep=(condition, col_seq, ids, controls))
        if smp is not None or rng is not None:
            persistent = False
        step = step_launcher(d, smp, rng, lat=lat)
        nbytes = 0
        if steps and persistent:
            # the library picks the width class (<= 256 or <= 512 channels per vector); shapes outside
            # both (or a device too small to hold a launch) get 0 bytes and run on the per-step
            # kernels below -- same results, more launches
            nbytes = _lib.load().vqvae_wavenet_gen_run_workspace_bytes(C.byref(d))
        if steps and persistent and nbytes:
            # one persistent launch per `chunk` steps; queues + mailboxes live in its workspace
            ws = DeviceArray((nbytes // 4 + 1,), np.int32)
            for t0 in range(0, steps, chunk):
                _lib.call('vqvae_wavenet_gen_run', C.byref(d), t0, min(chunk, steps - t0), ws.ptr,
                          ws.nbytes, _S())
            backend.synchronize()
            self._last_ws = ws
            _check_persistent(ws, ': are all its workgroups resident?')
            self.step.set(np.array([steps], np.int32))
        elif steps:
            replay = Replay(step, steps)
            try:
                replay.run(graph_steps)
            finally:
                replay.close()
        d.max_steps = _INT_MAX
        return (out, logits_out) if return_logits else out


def run_many(wavenet, condition, uniforms, mode, n_steps=None, group=_lib.GEN_MAX_N, max_streams=8,
             chunk=4096):
    """Batched serving form of the loop: N sequences = ceil(N / group) independent persistent
    launches of <= ``group`` lockstep sequences each, spread over ``max_streams`` HIP streams so
    they run concurrently (a launch occupies 128 or 256 two-wave workgroups: a fraction of the GPU).
    condition (N, condition_dim, T) on the device, uniforms (T, N[, nr_mix]) on the host.
    Returns the host array (N, T) of sampled bins / values."""
    refuse_latent(condition, 'generate_batch')
    refuse_device_uniforms(uniforms, 'generate_batch')
    if condition.ndim == 4:
        condition = condition.reshape(condition.shape[:3])
    N, Cc, T = condition.shape
    steps = T - 1 if n_steps is None else int(n_steps)
    u = np.asarray(uniforms, np.float64)
    u = u.reshape(u.shape[0], N, -1)
    lib = _lib.load()
    jobs = []
    for g0 in range(0, N, group):
        n = min(group, N - g0)
        st = GenerationState(wavenet, n)                       # holds the descriptor and, after bind, what it points to
        n_uniform, dtype = sampling_layout(mode, st.out_dim)
        if u.shape[0] < steps or u.shape[2] < n_uniform:
            raise ValueError('generate_batch: need (steps, N, %d) uniform doubles, got %s' % (n_uniform, u.shape))
        u_dev = backend.to_device(np.ascontiguousarray(u[:max(steps, 1), g0:g0 + n, :n_uniform]).reshape(-1))
        out = backend.zeros((n, T), dtype)
        d = st.bind(condition.flat_view(g0 * Cc * T, n * Cc * T, (n, Cc, T)), u_dev, n_uniform, None, out, None, mode, steps)
        nbytes = lib.vqvae_wavenet_gen_run_workspace_bytes(C.byref(d))
        if not nbytes:
            raise ValueError('persistent generation: ' + lib.vqvae_last_error_string().decode())
        jobs.append((st, out, DeviceArray((nbytes // 4 + 1,), np.int32)))
    backend.synchronize()                  # buffers above were prepared on the main stream
    # every workgroup of a launch must be resident at once (its waves wait for each other): the
    # library knows the width class's workgroup count and the kernel's occupancy on this device
    resident = min(lib.vqvae_wavenet_gen_run_concurrency(C.byref(st.desc)) for st, _, _ in jobs)
    max_streams = max(1, min(max_streams, resident))
    for t0 in range(0, steps, chunk):
        for i, (st, out, ws) in enumerate(jobs):
            _lib.call('vqvae_wavenet_gen_run', C.byref(st.desc), t0, min(chunk, steps - t0), ws.ptr, ws.nbytes,
                      backend.pool_stream(i % max_streams))
    backend.synchronize()
    res = []
    for st, out, ws in jobs:
        _check_persistent(ws)
        res.append(out.get())
    return np.concatenate(res, axis=0)


class LockstepState(GenerationState):
    """The same descriptor and buffers for 1..128 sequences: the step entry points run n > 4 on the lockstep
    kernels (csrc/generate_lockstep.hip, the batch in MFMA columns).  The persistent kernel stays at n <= 4, so
    ``run`` is used with ``persistent=False``."""
    max_n = _lib.GEN_MAX_LOCKSTEP


def _check_group(group):
    if not _lib.GEN_MAX_N < group <= _lib.GEN_MAX_LOCKSTEP:
        raise ValueError('generate_lockstep: group must be %d..%d, got %d' % (_lib.GEN_MAX_N + 1, _lib.GEN_MAX_LOCKSTEP, group))


def plan_lockstep(N, T, lengths=None, n_steps=None, group=_lib.GEN_MAX_LOCKSTEP):
    """Who runs with whom, and for how long.  Returns (steps, groups): steps[i] = steps sequence i runs
    (lengths[i] - 1 as generate.py:105 would for a condition of that length, capped by ``n_steps``), groups = list of
    (indices, group_steps) in running order.  With ``lengths`` the sequences are sorted by length (longest first,
    ties in the caller's order) before they are cut into groups of <= ``group``, so that a group stops at its
    longest member; without, groups are consecutive slices.  A group of fewer than 5 is filled up to 5 with
    repeats of its last member."""
    _check_group(group)
    if lengths is None:
        full = T - 1 if n_steps is None else int(n_steps)
        if not 0 <= full <= T:
            raise ValueError('generate_lockstep: n_steps must be in [0, %d]' % T)
        steps = np.full((N,), full, np.int64)
        order = np.arange(N)
    else:
        lengths = np.asarray(lengths).astype(np.int64).reshape(-1)
        if lengths.shape != (N,) or (lengths < 1).any() or (lengths > T).any():
            raise ValueError('generate_lockstep: lengths must be (N,) = (%d,) integers in [1, %d]' % (N, T))
        steps = lengths - 1
        if n_steps is not None:
            if int(n_steps) < 0:
                raise ValueError('generate_lockstep: n_steps must not be negative')
            steps = np.minimum(steps, int(n_steps))
        order = np.argsort(-steps, kind='stable')
    groups = []
    for g0 in range(0, N, group):
        idx = order[g0:g0 + group]
        if len(idx) <= _lib.GEN_MAX_N:
            # n <= 4 would run the matrix-vector kernels, which sum in another order: repeat the last member so
            # that every sequence of every call goes through the same arithmetic
            idx = np.concatenate([idx, np.repeat(idx[-1:], _lib.GEN_MAX_N + 1 - len(idx))])
        groups.append((idx, int(steps[idx].max())))
    return steps, groups


def _group_runner(wavenet, condition, mode, graph_steps, return_logits):
    """One group of run_lockstep on the device: fresh LockstepState, a replayed hipGraph of per-step launches on the main
    stream.  The group's rows of a dense condition are gathered into one array (a view when they are consecutive).  From
    a LatentCondition no rows are gathered: the group's indices (repeats of the last member included) go to the device
    as ``col_seq`` and every step computes its (n, condition_dim) column."""
    N, Cc, T = condition.shape

    def run_group(idx, u, forced, steps, sampling=None):
        n = len(idx)
        cond, col_seq = condition, None
        if isinstance(condition, LatentCondition):
            col_seq = backend.to_device(np.ascontiguousarray(idx, dtype=np.int32))
        elif (np.diff(idx) == 1).all():
            cond = condition.flat_view(int(idx[0]) * Cc * T, n * Cc * T, (n, Cc, T))
        else:
            cond = DeviceArray((n, Cc, T), np.float32)
            backend.copy_many([(cond.flat_view(j * Cc * T, Cc * T), condition.flat_view(int(i) * Cc * T, Cc * T))
                               for j, i in enumerate(idx)])
        res = LockstepState(wavenet, n).run(cond, u, mode, steps, forced, return_logits, graph_steps, persistent=False,
                                            sampling=sampling, col_seq=col_seq)
        if return_logits:
            return res[0].get(), res[1].get()[:steps]
        return res.get(), None
    return run_group


def _lockstep_uniforms(uniforms, N, T, max_steps, n_uniform):
    """The uniforms of a lockstep call, checked: the host array as (T', N, n_uniform'), or the DeviceUniforms with its
    ids spelled out for the N sequences."""
    if isinstance(uniforms, DeviceUniforms):
        return uniforms.resolved(N, 'generate_lockstep')
    u = np.asarray(uniforms, np.float64)
    if u.ndim < 2 or u.shape[1] != N:
        raise ValueError('generate_lockstep: uniforms must be (T, N[, %d]) = (%d, %d, ...), got %s'
                         % (n_uniform, T, N, u.shape))
    u = u.reshape(u.shape[0], N, -1)
    if u.shape[0] < max_steps or u.shape[2] < n_uniform:
        raise ValueError('generate_lockstep: need (%d, %d, %d) uniform doubles, got %s' % (max_steps, N, n_uniform, u.shape))
    return u


def _lockstep_args(wavenet, condition, uniforms, mode, n_steps, lengths, forced, return_logits, group):
    """The argument work of run_lockstep and run_lockstep_refill -> (condition (N, Cc, T), N, T, steps (N,), groups,
    n_uniform, max_steps, the checked uniforms, the checked forced values (steps', N) or None, zeroed host ``out``
    (N, T), zeroed host ``logits`` (max_steps, N, out_dim) or None)."""
    if isinstance(condition, LatentCondition) and lengths is None:
        lengths = condition.lengths
    if condition.ndim == 4:
        condition = condition.reshape(condition.shape[:3])
    N, Cc, T = condition.shape
    steps, groups = plan_lockstep(N, T, lengths, n_steps, group)
    out_dim = wavenet.proj2.W.shape[0]
    n_uniform, dtype = sampling_layout(mode, out_dim)
    max_steps = int(steps.max()) if N else 0
    u = _lockstep_uniforms(uniforms, N, T, max_steps, n_uniform)
    if forced is not None:
        forced = np.asarray(forced).reshape(-1, N)
        if forced.shape[0] < max_steps:
            raise ValueError('generate_lockstep: forced must be (steps, N) = (%d, %d), got %s' % (max_steps, N, forced.shape))
    out = np.zeros((N, T), dtype)                                                # generate.py:103
    logits = np.zeros((max_steps, N, out_dim), np.float32) if return_logits else None
    return condition, N, T, steps, groups, n_uniform, max_steps, u, forced, out, logits


def _scatter(out, logits, steps, idx, o, lg):
    """Row j of a run's result ``o`` (and column j of its logits ``lg``) is sequence idx[j]: its own steps go to its row of
    ``out``; what a sequence that kept running (or a stub) wrote past them is discarded."""
    for j, i in enumerate(idx):
        out[i, :steps[i]] = o[j, :steps[i]]
        if logits is not None:
            logits[:steps[i], i] = lg[:steps[i], j]


def run_lockstep(wavenet, condition, uniforms, mode, n_steps=None, lengths=None, forced=None, return_logits=False,
                 graph_steps=8, group=_lib.GEN_MAX_LOCKSTEP, _run_group=None, sampling=None):
    """Many sequences at once (converting a validation set or a corpus): N sequences of any count as groups of
    <= ``group`` (<= 128) lockstep sequences, each group a replayed hipGraph of ``graph_steps`` per-step launches
    (0 = eager launches), the groups one after another on the main stream.  The weights are streamed once per
    step for the whole group.

    condition (N, condition_dim, T) on the device, uniforms (T, N[, nr_mix]) host doubles, forced (T, N) or None.
    ``lengths`` (N,) integers: sequence i runs lengths[i] - 1 steps, as generate.py:105 would for a condition of
    that length, and its output columns from lengths[i] - 1 on are 0.
    Returns the host array (N, T) in the caller's order (and, with ``return_logits``, the host array
    (max steps, N, out_dim), rows past a sequence's own steps 0).  Every sequence gets the values it gets in any
    other batch of 5..128 and in any other position of it, bit for bit.
    ``sampling``: None or the tuple of sampling_controls(N, ...); every group gets its members' values, gathered with the
    group's indices like the uniforms (repeats of the last member included), and the promise above holds with them.
    ``condition`` may be a LatentCondition: T is its longest sequence, ``lengths`` defaults to its own, and the values are
    those of the call with ``condition.dense()``, bit for bit, without that tensor.
    ``uniforms`` may be a DeviceUniforms: a group then gets the generator with its members' stream ids (gathered with the
    group's indices, repeats included) in place of an array, and the values are those of the call with
    ``uniforms.host(steps, n_uniform)``."""
    condition, N, T, steps, groups, n_uniform, max_steps, u, forced, out, logits = _lockstep_args(
        wavenet, condition, uniforms, mode, n_steps, lengths, forced, return_logits, group)
    run_group = _run_group or _group_runner(wavenet, condition, mode, graph_steps, return_logits)
    for idx, gsteps in groups:
        # a DeviceUniforms has no (steps, n) array on either side: the group gets its members' stream ids
        ug = u.gather(idx) if isinstance(u, DeviceUniforms) else np.ascontiguousarray(u[:max(gsteps, 1), idx, :n_uniform])
        fg = None if forced is None else np.ascontiguousarray(forced[:gsteps, idx])
        if sampling is None:
            o, lg = run_group(idx, ug, fg, gsteps)
        else:
            o, lg = run_group(idx, ug, fg, gsteps, tuple(None if a is None else a[idx] for a in sampling))
        _scatter(out, logits, steps, idx, o, lg)          # a shorter sequence kept running: its tail is discarded
    return (out, logits) if return_logits else out


# ---- lockstep generation with refill (include/vqvae_gen_slots.h, csrc/generate_slots.hip) -----------------------------
def refill_queue(steps):
    """The serving order of run_lockstep_refill: longest first, ties in the caller's order, sequences with 0 steps left
    out (their output rows stay 0)."""
    steps = np.asarray(steps, np.int64).reshape(-1)
    order = np.argsort(-steps, kind='stable')
    return order[steps[order] > 0].astype(np.int32)


def refill_slots(n_queue, group=_lib.GEN_MAX_LOCKSTEP):
    """S = clamp(min(sequences to run, group), 5, 128): the slot count of a refilled run."""
    _check_group(group)
    return max(_lib.GEN_MAX_N + 1, min(int(n_queue), int(group)))


def plan_refill(steps, slots):
    """The device scheduler's rule (csrc/generate_slots.hip) replayed on the host.  ``steps`` (N,) steps per sequence,
    ``slots`` = S.  Slot s starts with queue[s]; at the end of every tick the slots whose sequence has run all its
    steps are freed and take, in slot order, the next waiting sequences of refill_queue(steps).
    Returns (ticks, placement): the number of ticks until every slot is idle, and the int64 array (N, 2) of every
    sequence's (slot, first tick), (-1, -1) for a sequence with 0 steps, which is never queued.  The host issues
    ``ticks`` steps and never asks the device how far it is."""
    import heapq
    steps = np.asarray(steps, np.int64).reshape(-1)
    if (steps < 0).any() or slots < 1:
        raise ValueError('plan_refill: steps must be >= 0 and slots >= 1')
    queue = refill_queue(steps)
    placement = np.full((len(steps), 2), -1, np.int64)
    head = queue[:slots]
    placement[head, 0] = np.arange(len(head))
    placement[head, 1] = 0
    ends = [(int(steps[q]), s) for s, q in enumerate(head)]           # (tick at which the slot is free again, slot)
    heapq.heapify(ends)
    nxt, ticks = len(head), 0
    while ends:
        tick, slot = heapq.heappop(ends)                              # equal ticks come out in slot order
        ticks = max(ticks, tick)
        if nxt < len(queue):
            q = queue[nxt]
            nxt += 1
            placement[q] = (slot, tick)
            heapq.heappush(ends, (tick + int(steps[q]), slot))
    return ticks, placement


class LockstepRefill(object):
    """One refilled run on the device: the slot table, the queue and every sequence's inputs uploaded once, one
    LockstepState of S slots, ``graph_steps`` ticks captured as a hipGraph (0 = eager) and replayed
    ceil(ticks / graph_steps) times; surplus ticks are device no-ops.

    Device memory besides the decoder state of S slots: the condition as the caller holds it (the (N, condition_dim, T)
    floats, 2 560 bytes per sample for the default model, or a LatentCondition: 4 Cl sum(tl) + 4 G N bytes, 32 bytes per
    sample, plus the (N, condition_dim) column that every tick's first launch, vqvae_gen_cond_column, fills for the live
    slots), the uniforms (an array: max_steps x N x n_uniform doubles, dense; a DeviceUniforms: the N stream ids, 8 N bytes,
    the numbers being computed in the finishing launch), the dense forced values max_steps x N, ``out`` N x T, with
    ``return_logits`` max_steps x N x out_dim floats (a test and inspection facility: 25 MB per 100 steps of 256
    sequences and classes), and 3 N + 2 S + 2 integers of table.  For a corpus of N = 300 utterances of up to 10 s at
    16 kHz the dense condition would be 123 GB and the latent one is at most 1.5 GB; an array of uniforms is 384 MB (3.8 GB
    for a mixture of 10 logistics), its rows dense because ragged storage would make a sequence's addresses depend on its
    neighbours' lengths; a DeviceUniforms is 2 400 bytes.  ``out`` and the forced values stay dense."""

    def __init__(self, wavenet, condition, steps, u, forced, mode, group, return_logits=False, sampling=None):
        N, Cc, T = condition.shape
        steps = np.ascontiguousarray(steps, dtype=np.int32)
        queue = refill_queue(steps)
        self.n_slots = S = refill_slots(len(queue), group)
        self.ticks, self.placement = plan_refill(steps, S)
        max_steps = int(steps.max())
        st = self.state = LockstepState(wavenet, S)
        n_uniform, dtype = sampling_layout(mode, st.out_dim)
        if not isinstance(u, DeviceUniforms):
            n_uniform = u.shape[2]
        u_dev, rng, ids = _uniform_source(u, N, S, max_steps, n_uniform)     # S > 4: a generator is kept, nothing is filled
        steps_dev, queue_dev = backend.to_device(steps), backend.to_device(queue)
        self.out = backend.zeros((N, T), dtype)
        self.logits_out = backend.zeros((max_steps, N, st.out_dim), np.float32) if return_logits else None
        self.slot_seq, self.slot_t = backend.zeros((S,), np.int32), backend.zeros((S,), np.int32)
        self.next, self.live = backend.zeros((1,), np.int32), backend.zeros((1,), np.int32)
        self.started = backend.to_device(np.full((N, 2), -1, np.int32))
        cond, lat = condition, None
        if isinstance(condition, LatentCondition):
            # rows are addressed by the sequence: (N, condition_dim); a tick's first launch writes the live slots' rows
            cond = self.column = backend.zeros((N, Cc), np.float32)
            lat = condition.struct(self.column)
        forced_dev = None if forced is None else backend.to_device(
            np.ascontiguousarray(forced[:max_steps], dtype=dtype).reshape(-1))
        smp, controls = (None, None) if sampling is None else _upload_controls(sampling)
        d = self.desc = st.bind(cond, u_dev, n_uniform, forced_dev, self.out, self.logits_out, mode, self.ticks,
                                keep=(condition, steps_dev, queue_dev, ids, controls))
        t = self.table = _lib.GenSlots()
        t.n_seq, t.steps, t.queue, t.n_queue = N, steps_dev.ptr, queue_dev.ptr, len(queue)
        t.next, t.slot_seq, t.slot_t, t.live = self.next.ptr, self.slot_seq.ptr, self.slot_t.ptr, self.live.ptr
        t.started = self.started.ptr
        self.tick = step_launcher(d, smp, rng, t, lat)
        self._replay = Replay(self.tick, self.ticks)
        _lib.call('vqvae_gen_slots_init', C.byref(d), C.byref(t), _S())

    def replay(self):
        """One more launch of the captured graph (``graph_steps`` ticks); past the end a device no-op."""
        self._replay.launch()

    def run(self, graph_steps=8):
        self._replay.run(graph_steps)
        return self

    def close(self):
        self._replay.close()


def _device_refill_runner(wavenet, condition, mode, graph_steps, group, return_logits):
    def run(steps, u, forced, sampling):
        r = LockstepRefill(wavenet, condition, steps, u, forced, mode, group, return_logits, sampling)
        try:
            r.run(graph_steps)
            return r.out.get(), None if r.logits_out is None else r.logits_out.get()
        finally:
            r.close()
    return run


def run_lockstep_refill(wavenet, condition, uniforms, mode, n_steps=None, lengths=None, forced=None, return_logits=False,
                        graph_steps=8, group=_lib.GEN_MAX_LOCKSTEP, _run=None, sampling=None):
    """run_lockstep with the columns refilled on the device: ``group`` is the number of slots, a slot whose sequence
    has finished takes the next waiting one (longest first) at the next step, and the whole call is one replayed
    hipGraph with no host read-back until the end (csrc/generate_slots.hip; memory: see LockstepRefill).  Arguments
    and return value as run_lockstep; every sequence gets the values run_lockstep gives it, bit for bit.
    ``_run(steps, u, forced, sampling)`` -> (out (N, T), logits (max steps, N, out_dim) or None), both in the caller's
    order, stands in for the device in host tests; ``u`` is the (max steps, N, n_uniform) array or, when ``uniforms`` is a
    DeviceUniforms, that object with its (N,) stream ids spelled out."""
    # the same step counts and argument errors as run_lockstep; its groups are not used
    condition, N, T, steps, _, n_uniform, max_steps, u, forced, out, logits = _lockstep_args(
        wavenet, condition, uniforms, mode, n_steps, lengths, forced, return_logits, group)
    if max_steps:
        run = _run or _device_refill_runner(wavenet, condition, mode, graph_steps, group, return_logits)
        o, lg = run(steps, u if isinstance(u, DeviceUniforms) else u[:max_steps, :, :n_uniform], forced, sampling)
        _scatter(out, logits, steps, range(N), o, lg)   # the device wrote nothing past a sequence's own steps; a stub may have
    return (out, logits) if return_logits else out
