"""CodebookMonitor -- codebook health for the VQ layer: usage statistics gathered on the device inside the training
step, and re-seeding of codes that have gone unused (include/vqvae_codebook.h, csrc/vq_codebook.hip).

The reference has neither: its step reports loss1..3 only, and with the plain codebook loss (net.py:85) a code that is
never selected receives a zero gradient for ever.  Opt-in and additive: a VQ link without a monitor runs exactly the
launches it ran before.

    mon = CodebookMonitor(model.vq, decay=0.99, seed=0)
    model.vq.monitor = mon
    ...
    updater.update()                                   # observe() rides inside the step, recorded or eager
    if updater.iteration % 100 == 0:
        log.report(mon.summary(reset=True))            # main/perplexity, main/codes_used, main/codes_live
    if updater.iteration % 500 == 0:
        mon.reseed(updater.get_optimizer('main'), threshold=1e-3, comm=getattr(updater, 'comm', None))

Device state (all persistent, allocated once, never from a recorded step's arena): ``counts_dev`` int32 (k),
``usage_dev`` float32 (k), ``reservoir_dev`` float32 (k, d), ``steps_seen_dev`` int32 (1), ``stats_dev`` float64 (8).
Nothing is read back per step: ``summary()`` copies the interval sums (64 bytes) and the usage vector once per
reporting interval.
"""
import numpy as np

from . import _lib, backend, core
from .backend import DeviceArray

SNAPSHOT_PREFIX = 'updater/codebook:main/'
_MASK64 = (1 << 64) - 1


def reservoir_rows(seed, step, k, n_rows):
    """Row n_j of the latents that ``observe`` number ``step`` (0-based) draws for code j, j = 0..k-1: the counter-based
    hash of include/vqvae_codebook.h, restated on the host (uint64 arithmetic wraps)."""
    with np.errstate(over='ignore'):
        ctr = (np.uint64(int(step) & 0xFFFFFFFF) << np.uint64(32)) | np.arange(k, dtype=np.uint64)
        x = np.uint64(int(seed) & _MASK64) + (ctr + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x % np.uint64(n_rows)).astype(np.int64)


def reservoir_owner(j, steps_seen, size):
    """The rank whose reservoir row re-seeds code j in a data-parallel ``reseed`` after ``steps_seen`` observations."""
    return (np.asarray(j, np.int64) + int(steps_seen)) % int(size)


def attached_monitors(link):
    """[(link path without slashes at the ends, monitor)] of every VQ link under ``link`` that has a monitor."""
    owners = [l for l in link.links() if getattr(l, 'monitor', None) is not None]
    out = []
    for name, p in link.namedparams():
        for l in owners:
            if l.W is p:
                out.append((name[:-len('/W')].strip('/'), l.monitor))
    return out


class CodebookMonitor(object):
    """Watches one VQ link.  ``decay``: weight of the past in the running usage; ``seed``: of the reservoir hash."""

    def __init__(self, vq, decay=0.99, seed=0):
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError('decay must be in [0, 1], got %r' % (decay,))
        self.vq = vq
        self.decay = float(decay)
        self.seed = int(seed) & _MASK64
        self.k = int(vq.k)
        self.d = None
        self.threshold = None            # of the last reseed(): what summary() calls "live"
        self.last_mask = None            # int32 (k) host array: the codes the last reseed() replaced
        self._pending = None             # snapshot state that arrived before the device state existed
        W = vq.W.data
        if isinstance(W, DeviceArray):
            self._allocate(W.shape[1])

    # ------------------------------------------------------------------ state
    def _allocate(self, d):
        if backend._state.get('arena') is not None:
            # buffers taken now would belong to the recording, and their zero-fill would be replayed with every step
            raise RuntimeError('CodebookMonitor: the device state cannot be created while a step is being recorded; '
                               'attach the monitor after the codebook exists on the device, or run one eager step first')
        self.d = int(d)
        self.counts_dev = backend.zeros((self.k,), np.int32)
        self.usage_dev = backend.zeros((self.k,), np.float32)
        self.reservoir_dev = backend.zeros((self.k, self.d), np.float32)
        self.steps_seen_dev = backend.zeros((1,), np.int32)
        self.stats_dev = backend.zeros((_lib.CODEBOOK_STATS_WORDS,), np.float64)
        if self._pending is not None:
            state, self._pending = self._pending, None
            self.load_state(state)

    def _require_state(self):
        if self.d is None:
            raise RuntimeError('CodebookMonitor: nothing observed yet and the codebook has no device storage')

    # ------------------------------------------------------------------ the hook (VQ.__call__)
    def observe(self, z, indexes):
        """Enqueues one observation on the process stream: z (B, d, T[, 1]) latents, indexes (B, T[, 1]) int32."""
        if not (isinstance(z, DeviceArray) and isinstance(indexes, DeviceArray)):
            raise TypeError('CodebookMonitor.observe needs device arrays')
        B, d, T = z.shape[:3]
        if self.d is None:
            self._allocate(d)
        if d != self.d or indexes.size != B * T or indexes.dtype != np.int32 or z.dtype != np.float32:
            raise ValueError('CodebookMonitor.observe: latents %s %s / indexes %s %s do not fit a (%d, %d) codebook'
                             % (z.shape, z.dtype, indexes.shape, indexes.dtype, self.k, self.d))
        _lib.call('vqvae_codebook_observe', indexes.ptr, z.ptr, B, d, T, self.k, self.decay, self.seed,
                  self.counts_dev.ptr, self.usage_dev.ptr, self.reservoir_dev.ptr, self.steps_seen_dev.ptr, self.stats_dev.ptr,
                  backend.stream())

    # ------------------------------------------------------------------ reading
    def counts(self):
        """Host copy of the last observed step's histogram, int32 (k)."""
        self._require_state()
        return self.counts_dev.get()

    def usage(self):
        """Host copy of the running usage, float32 (k)."""
        self._require_state()
        return self.usage_dev.get()

    def steps_seen(self):
        self._require_state()
        return int(self.steps_seen_dev.get()[0])

    def summary(self, reset=False, threshold=None, prefix='main/'):
        """Means over the observations since the last reset, as an Evaluator result (LogReport.report takes it):
        ``perplexity`` exp(-sum p ln p) of the per-step code distribution, ``codes_used`` codes chosen at least once in a
        step, ``codes_live`` codes whose running usage is at or above ``threshold`` (default: the last reseed()'s; without
        one, above zero)."""
        self._require_state()
        st = self.stats_dev.get()
        n = max(st[4], 1.0)
        thr = self.threshold if threshold is None else threshold
        u = self.usage()
        live = int((u > 0).sum()) if thr is None else int((u >= np.float32(thr)).sum())
        if reset:
            self.stats_dev.fill_zero()
        return {prefix + 'perplexity': float(st[2] / n), prefix + 'codes_used': float(st[3] / n),
                prefix + 'codes_live': float(live)}

    # ------------------------------------------------------------------ repair
    def reseed(self, optimizer=None, threshold=1e-3, revived_usage=None, comm=None):
        """Replaces every code whose running usage is below ``threshold`` by its reservoir row (a latent the encoder
        produced at the last step), zeroes the Adam moments of the replaced rows (stale moments would drag the fresh vector
        back towards the dead one; with an EMACodebook on the link, its state of those rows restarts at N = 1, m = W for
        the same reason) and sets their usage to ``revived_usage`` (default: ``threshold``, so a revived code is
        not replaced again before it had a chance).  Returns the number of codes replaced.

        With a communicator of more than one rank the decision is taken on the usage summed over ranks, and code j takes
        the reservoir row of rank ``reservoir_owner(j, steps_seen, size)``: every rank ends with the same codebook.  After
        such a call ``usage`` holds the sum over ranks (the decay forgets it at the rate it forgets anything else)."""
        self._require_state()
        W = self.vq.W.data
        if not isinstance(W, DeviceArray) or tuple(W.shape) != (self.k, self.d):
            raise ValueError('CodebookMonitor.reseed: the codebook must be a (%d, %d) device array' % (self.k, self.d))
        revived = float(threshold if revived_usage is None else revived_usage)
        m = v = None
        if optimizer is not None and getattr(optimizer, 'm', None) is not None:
            named = dict(optimizer.target.namedparams())
            for name, off, size in optimizer.layout():
                if named.get(name) is self.vq.W and off + size <= optimizer.n_train:
                    m, v = optimizer.m.flat_view(off, size), optimizer.v.flat_view(off, size)
            if m is None:
                raise ValueError('CodebookMonitor.reseed: the optimizer does not hold this codebook')
        reservoir = self.reservoir_dev
        if comm is not None and comm.size > 1:
            comm.allreduce_grad(self.usage_dev.reshape(-1))
            step = self.steps_seen()
            first = (comm.rank - step) % comm.size              # this rank owns rows first, first + size, ...
            rows = len(range(first, self.k, comm.size))
            reservoir = backend.zeros((self.k, self.d), np.float32)
            if rows:
                pitch = comm.size * self.d * 4
                _lib.call('vqvae_memcpy2d_d2d', reservoir.ptr + first * self.d * 4, pitch,
                          self.reservoir_dev.ptr + first * self.d * 4, pitch, self.d * 4, rows, backend.stream())
            comm.allreduce_grad(reservoir.reshape(-1))
        n = DeviceArray((1,), np.int32)
        mask = DeviceArray((self.k,), np.int32)
        _lib.call('vqvae_codebook_reseed', W.ptr, None if m is None else m.ptr, None if v is None else v.ptr, self.k, self.d,
                  self.usage_dev.ptr, reservoir.ptr, float(threshold), revived, n.ptr, mask.ptr, backend.stream())
        core.bump_param_epoch('load')        # value-keyed caches (VQ search reuse, generation state) are stale; W did not move
        ema = getattr(self.vq, 'codebook_ema', None)
        if ema is not None:
            ema.reset(mask=mask)             # replaced rows restart at N = 1, m = W (else the next step pulls them back)
        self.threshold = float(threshold)
        self.last_mask = mask.get()
        return int(n.get()[0])

    # ------------------------------------------------------------------ snapshots (serializers.save_npz / load_npz)
    def state(self):
        out = {'seed': np.asarray(self.seed, np.uint64), 'decay': np.asarray(self.decay, np.float64)}
        if self.d is not None:
            out['usage'] = self.usage_dev.get()
            out['steps_seen'] = self.steps_seen_dev.get().reshape(())
        elif self._pending is not None:
            out.update(self._pending)
        return out

    def load_state(self, state):
        old = (self.seed, self.decay)
        if 'seed' in state:
            self.seed = int(state['seed']) & _MASK64
        if 'decay' in state:
            self.decay = float(state['decay'])
        if (self.seed, self.decay) != old:
            core.bump_param_epoch('monitor')     # both are kernel arguments of a recorded step
        if 'usage' not in state:
            return
        if self.d is None:
            self._pending = {k: np.array(state[k]) for k in ('usage', 'steps_seen') if k in state}
            return
        self.usage_dev.set(np.asarray(state['usage'], np.float32).reshape(self.k))
        self.steps_seen_dev.set(np.asarray(state['steps_seen'], np.int32).reshape(1))
