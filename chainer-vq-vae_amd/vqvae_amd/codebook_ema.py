"""EMACodebook -- the VQ-VAE paper's second codebook rule (van den Oord et al. 2017, appendix A.1): the codebook is not
trained by a gradient; every code tracks an exponential moving average of the encoder outputs assigned to it (online
k-means).  include/vqvae_vq_ema.h states the rule and csrc/vq_ema.hip computes it.

The reference moves the codebook by Adam on loss2 (net.py:90) only.  Opt-in and additive: a VQ link without an EMA
object runs exactly the launches it ran before.

    ema = EMACodebook(model.vq, decay=0.99, eps=1e-5)
    model.vq.codebook_ema = ema
    ...
    updater.update()          # accumulate() rides inside the forward, step() behind optimizer.update(), recorded or eager

With an EMA object on ``model.vq`` the updaters do not back-propagate loss2 (it has no one to train), so W's gradient slot
and Adam moments stay zero and W is a pure function of (ema_count, ema_sum).  A CodebookMonitor on the same link works
beside it; its reseed() ends with ``reset(mask)`` for the rows it replaced.

Device state (persistent, allocated once, never from a recorded step's arena): ``count_dev`` float32 (k), ``sum_dev``
float32 (k, d), ``stats_dev`` float32 (k * (d + 1)): the last step's n_j, then S_jc.
"""
import numpy as np

from . import _lib, backend, core
from .backend import DeviceArray

SNAPSHOT_PREFIX = 'updater/codebook_ema:main/'
STATE_KEYS = ('decay', 'eps', 'count', 'sum')


def attached_emas(link):
    """[(link path without slashes at the ends, EMA object)] of every VQ link under ``link`` that has one."""
    owners = [l for l in link.links() if getattr(l, 'codebook_ema', None) is not None]
    out = []
    for name, p in link.namedparams():
        for l in owners:
            if l.W is p:
                out.append((name[:-len('/W')].strip('/'), l.codebook_ema))
    return out


def step_attached(model, comm=None):
    """``step(comm)`` of every EMA object under ``model``: what the updaters call behind ``optimizer.update()``."""
    links = getattr(model, 'links', None)        # (the updaters also drive models that are not Links: nothing to step)
    for link in links() if links is not None else ():
        ema = getattr(link, 'codebook_ema', None)
        if ema is not None:
            ema.step(comm)


def _check_hyper(decay, eps):
    if not 0.0 <= float(decay) <= 1.0:
        raise ValueError('decay must be in [0, 1], got %r' % (decay,))
    if not float(eps) > 0.0:
        raise ValueError('eps must be positive, got %r' % (eps,))


class EMACodebook(object):
    """Moves the codebook of one VQ link.  ``decay``: weight of the past; ``eps``: Laplace smoothing of the counts."""

    def __init__(self, vq, decay=0.99, eps=1e-5):
        _check_hyper(decay, eps)
        self.vq = vq
        self.k = int(vq.k)
        self.d = None
        self._decay = float(decay)
        self._eps = float(eps)
        self._accumulated = False        # host-side: accumulate() ran since the last step()
        self._pending = None             # snapshot state that arrived before the device state existed
        W = vq.W.data
        if isinstance(W, DeviceArray):
            self._allocate(W)

    # ------------------------------------------------------------------ hyper-parameters (kernel arguments of a recorded step)
    @property
    def decay(self):
        return self._decay

    @decay.setter
    def decay(self, value):
        self._set_hyper(value, self._eps)

    @property
    def eps(self):
        return self._eps

    @eps.setter
    def eps(self, value):
        self._set_hyper(self._decay, value)

    def _set_hyper(self, decay, eps):
        _check_hyper(decay, eps)
        if (float(decay), float(eps)) != (self._decay, self._eps):
            self._decay, self._eps = float(decay), float(eps)
            core.bump_param_epoch('monitor')

    # ------------------------------------------------------------------ state
    def _allocate(self, W):
        if backend._state.get('arena') is not None:
            # buffers taken now would belong to the recording, and their initialisation would be replayed with every step
            raise RuntimeError('EMACodebook: the device state cannot be created while a step is being recorded; attach the '
                               'object after the codebook exists on the device, or run one eager step first')
        if tuple(W.shape)[0] != self.k:
            raise ValueError('EMACodebook: the codebook has %d rows, the link says k = %d' % (W.shape[0], self.k))
        self.d = int(W.shape[1])
        self.count_dev = backend.zeros((self.k,), np.float32)
        self.sum_dev = backend.zeros((self.k, self.d), np.float32)
        self.stats_dev = backend.zeros((self.k * (self.d + 1),), np.float32)
        self.reset()
        if self._pending is not None:
            state, self._pending = self._pending, None
            self.load_state(state)

    def _require_state(self):
        if self.d is None:
            W = self.vq.W.data
            if not isinstance(W, DeviceArray):
                raise RuntimeError('EMACodebook: the codebook has no device storage yet')
            self._allocate(W)

    def _codebook(self):
        W = self.vq.W.data
        if not isinstance(W, DeviceArray) or tuple(W.shape) != (self.k, self.d):
            raise ValueError('EMACodebook: the codebook must be a (%d, %d) device array' % (self.k, self.d))
        return W

    def reset(self, mask=None):
        """ema_count <- 1, ema_sum <- W: for every code, or for the codes whose entry of ``mask`` (int32 (k), device or
        host) is non-zero; the other codes keep their state bit for bit."""
        self._require_state()
        if mask is not None and not isinstance(mask, DeviceArray):
            mask = backend.to_device(np.ascontiguousarray(np.asarray(mask).reshape(self.k), np.int32))
        if mask is not None and (mask.size != self.k or mask.dtype != np.int32):
            raise ValueError('EMACodebook.reset: the mask must be int32 (%d,)' % self.k)
        _lib.call('vqvae_vq_ema_reset', self._codebook().ptr, self.count_dev.ptr, self.sum_dev.ptr, self.k, self.d,
                  None if mask is None else mask.ptr, backend.stream())

    # ------------------------------------------------------------------ the hooks (VQ.__call__, the updaters)
    def accumulate(self, z, indexes):
        """Enqueues the step's statistics on the process stream: z (B, d, T[, 1]) latents, indexes (B, T[, 1]) int32."""
        if not (isinstance(z, DeviceArray) and isinstance(indexes, DeviceArray)):
            raise TypeError('EMACodebook.accumulate needs device arrays')
        self._require_state()
        B, d, T = z.shape[:3]
        if d != self.d or indexes.size != B * T or indexes.dtype != np.int32 or z.dtype != np.float32:
            raise ValueError('EMACodebook.accumulate: latents %s %s / indexes %s %s do not fit a (%d, %d) codebook'
                             % (z.shape, z.dtype, indexes.shape, indexes.dtype, self.k, self.d))
        if B * T >= _lib.VQ_EMA_MAX_N:
            raise ValueError('EMACodebook.accumulate: %d rows; the float32 counts are exact below 2^24 rows only' % (B * T))
        ws = backend.workspace(_lib.load().vqvae_vq_ema_workspace_bytes(B, d, T, self.k))
        _lib.call('vqvae_vq_ema_accumulate', indexes.ptr, z.ptr, B, d, T, self.k, self.stats_dev.ptr, ws.ptr, ws.nbytes,
                  backend.stream())
        self._accumulated = True

    def step(self, comm=None):
        """Exchange (one float all-reduce of the statistics when ``comm`` has more than one rank) and apply the rule:
        W <- ema_sum / smoothed ema_count.  Call it behind ``optimizer.update()``; whatever the optimizer did to W in the
        same step is overwritten.

        The link's search reuse (``VQ._cache``) is keyed on the owning optimizer's step count (``W._owner_step``), which
        ``optimizer.update()`` has just advanced: the mechanism that covers Adam's in-place update covers this one, and no
        ``param_epoch('load')`` bump per step is needed (generation state keyed on that epoch packs the decoder's
        parameters only; the codebook reaches generation through freshly quantised latents).  For a link whose W no
        optimizer owns the cache is dropped here as well."""
        if not self._accumulated:
            raise RuntimeError('EMACodebook.step: nothing was accumulated since the previous step (the quantiser did not '
                               'run its search in train mode)')
        self._accumulated = False
        if comm is not None and comm.size > 1:
            comm.allreduce_grad(self.stats_dev)
        _lib.call('vqvae_vq_ema_apply', self._codebook().ptr, self.count_dev.ptr, self.sum_dev.ptr, self.stats_dev.ptr,
                  self.k, self.d, self._decay, self._eps, backend.stream())
        self.vq._cache = None

    # ------------------------------------------------------------------ reading
    def counts(self):
        """Host copy of the last statistics' n_j, float32 (k) (summed over ranks once ``step`` exchanged them)."""
        self._require_state()
        return self.stats_dev.get()[:self.k].copy()

    def sums(self):
        """Host copy of the last statistics' S_jc, float32 (k, d)."""
        self._require_state()
        return self.stats_dev.get()[self.k:].reshape(self.k, self.d).copy()

    # ------------------------------------------------------------------ snapshots (serializers.save_npz / load_npz)
    def state(self):
        out = {'decay': np.asarray(self._decay, np.float64), 'eps': np.asarray(self._eps, np.float64)}
        if self.d is not None:
            out['count'] = self.count_dev.get()
            out['sum'] = self.sum_dev.get()
        elif self._pending is not None:
            out.update(self._pending)
        return out

    def load_state(self, state):
        self._set_hyper(float(state['decay']) if 'decay' in state else self._decay,
                        float(state['eps']) if 'eps' in state else self._eps)
        if 'count' not in state or 'sum' not in state:
            return
        if self.d is None and not isinstance(self.vq.W.data, DeviceArray):
            self._pending = {k: np.array(state[k]) for k in ('count', 'sum')}
            return
        self._require_state()
        self.count_dev.set(np.asarray(state['count'], np.float32).reshape(self.k))
        self.sum_dev.set(np.asarray(state['sum'], np.float32).reshape(self.k, self.d))
