"""KMeansCodebookInit -- initialise the VQ layer's codebook by k-means over real encoder outputs: exact k-means++ seeding
followed by Lloyd iterations, all on the device (include/vqvae_kmeans.h, csrc/vq_kmeans.hip; the assignment step is the
training step's own exact search, the cluster sums are EMACodebook's ``accumulate``).

The reference draws the codebook from Chainer's default initialiser, which knows nothing about where the encoder's outputs
lie.  Opt-in and additive: without a call to this module nothing changes.

    init = KMeansCodebookInit(model.vq, rows=16 * 1920, iters=10, seed=0)
    while init.collect(z):                 # z: encoder output (B, d, T'[, 1]); returns the rows still missing
        ...
    report = init.run(optimizer=opt, comm=None)

    report = kmeans_init(model, iterator, rows=16 * 1920, iters=10, seed=0, optimizer=opt)      # the same, driven for you

Call it at a step boundary: before the first step or, better, after a warm-up (a random encoder's outputs are a poor
sample).  It is eager and never part of a recorded step; W is written in place, so a recorded step stays valid.
"""
import numpy as np

from . import _lib, backend, core
from .backend import DeviceArray

_MASK64 = (1 << 64) - 1


def _moments(optimizer, W, who):
    """(m, v) views of the Adam moments of the slot that holds parameter ``W`` (CodebookMonitor.reseed's lookup)."""
    if optimizer is None or getattr(optimizer, 'm', None) is None:
        return None, None
    named = dict(optimizer.target.namedparams())
    for name, off, size in optimizer.layout():
        if named.get(name) is W and off + size <= optimizer.n_train:
            return optimizer.m.flat_view(off, size), optimizer.v.flat_view(off, size)
    raise ValueError('%s: the optimizer does not hold this codebook' % who)


class KMeansCodebookInit(object):
    """Collects ``rows`` encoder outputs for one VQ link and replaces its codebook by their k-means centroids.
    ``iters``: Lloyd iterations after the seeding (0: seeding only); ``seed``: of the k-means++ draws."""

    def __init__(self, vq, rows, iters=10, seed=0):
        if int(rows) < 1:
            raise ValueError('rows must be at least 1, got %r' % (rows,))
        if int(rows) >= _lib.KMEANS_MAX_N:
            raise ValueError('rows must be below 2^24, got %r' % (rows,))
        if int(iters) < 0:
            raise ValueError('iters must not be negative, got %r' % (iters,))
        W = vq.W.data
        if W is not None and not isinstance(W, DeviceArray):
            raise ValueError('KMeansCodebookInit: the codebook is on the host; call to_gpu() first (there is no CPU path)')
        self.vq = vq
        self.k = int(vq.k)
        self.rows = int(rows)
        self.iters = int(iters)
        self.seed = int(seed) & _MASK64
        self.d = None
        self.pool = None                 # float32 (d, rows), allocated by the first collect()
        self.filled = 0
        self.rows_per_call = 0           # rows the first collect() was offered: one minibatch's worth

    @property
    def missing(self):
        return self.rows - self.filled

    def collect(self, z):
        """Appends the rows of ``z`` (Variable or DeviceArray, (B, d, T'[, 1]) float32; row n is z[n // T', :, n % T']) to
        the pool, as many as still fit.  Returns the number of rows still missing."""
        if isinstance(z, core.Variable):
            z = z.data
        if not isinstance(z, DeviceArray):
            backend.require_device(z)
        if z.ndim not in (3, 4) or (z.ndim == 4 and z.shape[3] != 1) or z.dtype != np.float32:
            raise ValueError('KMeansCodebookInit.collect: latents must be float32 (B, d, T[, 1]), got %s %s' % (z.shape, z.dtype))
        B, d, T = z.shape[:3]
        if self.d is None:
            if self.vq.W.data is None:            # a lazily shaped codebook: created as VQ.__call__ creates it
                self.vq._initialize_params(d)
                self.vq.W.to_gpu()
            if tuple(self.vq.W.data.shape) != (self.k, d):
                raise ValueError('KMeansCodebookInit.collect: latents of %d channels for a %s codebook' % (d, self.vq.W.data.shape))
            if backend._state.get('arena') is not None:
                raise RuntimeError('KMeansCodebookInit.collect: not while a step is being recorded')
            self.d = int(d)
            self.pool = DeviceArray((self.d, self.rows), np.float32)
            self.rows_per_call = B * T
        elif d != self.d:
            raise ValueError('KMeansCodebookInit.collect: latents of %d channels, the pool has %d' % (d, self.d))
        count = min(B * T, self.missing)
        if count > 0:
            _lib.call('vqvae_kmeans_collect', z.ptr, B, d, T, count, self.pool.ptr, self.rows, self.filled, backend.stream())
            self.filled += count
        return self.missing

    def run(self, optimizer=None, comm=None):
        """k-means++ seeding and ``iters`` Lloyd iterations over the pool, then W <- the centroids, IN PLACE.

        Returns ``{'inertia': [...], 'empty': [...], 'counts': float32 (k), 'rows': int32 (k)}``: ``inertia[i]`` is the sum
        of squared distances of the pool's rows to their nearest code before Lloyd iteration i, the last entry that of the
        codebook this call leaves; ``empty[i]`` the number of codes iteration i found without a row and re-drew from the
        pool; ``counts`` the rows per code of the final assignment; ``rows`` the pool rows the seeding chose.  Everything
        is read back once, at the end.

        Around W: the Adam moments of the codebook's slot are zeroed when ``optimizer`` is given (stale moments would
        drag the fresh codes back; the optimizer must hold this codebook), the search-reuse cache is dropped, an attached
        EMACodebook restarts at N = 1, m = W, and an attached CodebookMonitor's running usage becomes
        ``counts * rows_per_call / rows``: what one minibatch the size of the first collected one would have counted
        under the final assignment, i.e. the monitor's own unit.  A code that won pool rows thus starts well above a
        re-seeding threshold and the decay forgets the value at its usual rate; a code left empty starts at 0 and is the
        next ``reseed``'s to replace.

        With a communicator of more than one rank every rank calls this at the same step boundary with its own full
        pool; rank 0's k-means decides and its W reaches the others through ``comm.allreduce_grad`` (W zeroed on the
        other ranks, then summed: rank 0's bits everywhere).  On ranks other than 0 the report describes the shared
        codebook on that rank's pool: one inertia, no ``empty``, ``rows`` None."""
        if self.pool is None or self.missing:
            raise RuntimeError('KMeansCodebookInit.run: the pool is not full, %d of %d rows are missing' % (self.missing, self.rows))
        if backend._state.get('arena') is not None:
            raise RuntimeError('KMeansCodebookInit.run: not while a step is being recorded')
        W = self.vq.W.data
        if not isinstance(W, DeviceArray) or tuple(W.shape) != (self.k, self.d) or W.dtype != np.float32:
            raise ValueError('KMeansCodebookInit.run: the codebook must be a float32 (%d, %d) device array' % (self.k, self.d))
        m, v = _moments(optimizer, self.vq.W, 'KMeansCodebookInit.run')
        lib = _lib.load()
        N, d, k, st = self.rows, self.d, self.k, backend.stream()
        parallel = comm is not None and comm.size > 1
        decides = not parallel or comm.rank == 0
        need = max(lib.vqvae_kmeans_workspace_bytes(N, d, k), lib.vqvae_vq_workspace_bytes(1, d, N, k),
                   lib.vqvae_vq_ema_workspace_bytes(1, d, N, k))
        if not lib.vqvae_kmeans_workspace_bytes(N, d, k):
            raise ValueError('KMeansCodebookInit.run: N = %d, d = %d, k = %d is outside include/vqvae_kmeans.h' % (N, d, k))
        ws = DeviceArray((need,), np.uint8)
        idx = DeviceArray((N,), np.int32)
        stats = DeviceArray((k * (d + 1),), np.float32)
        inertia = backend.zeros((self.iters + 1,), np.float64)
        empty = backend.zeros((self.iters + 1,), np.int32)
        rows = mind = None

        def assign(slot):
            _lib.call('vqvae_vq_nearest_fwd', self.pool.ptr, W.ptr, 1, d, N, k, 0, idx.ptr, None, None, ws.ptr, ws.nbytes, st)
            _lib.call('vqvae_vq_ema_accumulate', idx.ptr, self.pool.ptr, 1, d, N, k, stats.ptr, ws.ptr, ws.nbytes, st)
            _lib.call('vqvae_kmeans_inertia', self.pool.ptr, W.ptr, idx.ptr, N, d, k, inertia.ptr + 8 * slot, ws.ptr,
                      ws.nbytes, st)

        if decides:
            rows = DeviceArray((k,), np.int32)
            mind = DeviceArray((N,), np.float32)
            _lib.call('vqvae_kmeans_seed', self.pool.ptr, N, d, k, self.seed, W.ptr, rows.ptr, mind.ptr, ws.ptr, ws.nbytes, st)
            for it in range(self.iters):
                assign(it)
                _lib.call('vqvae_kmeans_update', self.pool.ptr, N, d, k, stats.ptr, self.seed, it, W.ptr,
                          empty.ptr + 4 * it, st)
        else:
            _lib.call('vqvae_memset', W.ptr, 0, W.nbytes, st)
        if parallel:
            comm.allreduce_grad(W.reshape(-1))
        W.amax = None
        assign(self.iters if decides else 0)      # the report describes the W this call leaves
        if m is not None:
            _lib.call('vqvae_memset', m.ptr, 0, m.nbytes, st)
            _lib.call('vqvae_memset', v.ptr, 0, v.nbytes, st)
        core.bump_param_epoch('load')        # value-keyed caches (VQ search reuse, generation state) are stale; W did not move
        self.vq._cache = None
        ema = getattr(self.vq, 'codebook_ema', None)
        if ema is not None:
            ema.reset()
        mon = getattr(self.vq, 'monitor', None)
        if mon is not None:
            if mon.d is None:
                mon._allocate(d)
            _lib.call('vqvae_elementwise', _lib.EW_SCALE, k, stats.ptr, None, mon.usage_dev.ptr,
                      float(self.rows_per_call) / float(N), 0.0, st)
        report = {'inertia': [float(x) for x in inertia.get()[:self.iters + 1 if decides else 1]],
                  'empty': [int(x) for x in empty.get()[:self.iters]] if decides else [],
                  'counts': stats.get()[:k].copy(),
                  'rows': rows.get() if decides else None}
        self.pool = None                     # pool, workspace and scratch go back to the allocator
        self.filled = 0
        self.d = None
        return report


def kmeans_init(model, iterator, rows, iters=10, seed=0, optimizer=None, comm=None, converter=None, device=0):
    """Fills a KMeansCodebookInit for ``model.vq`` with ``model.encoder``'s outputs on minibatches of ``iterator``
    (evaluation mode, no graph) until ``rows`` rows are there, then runs it.  ``converter``: as the updaters'
    (default ``concat_examples``); the encoder's input is the converted minibatch's first array."""
    if converter is None:
        from .updaters import concat_examples as converter
    init = KMeansCodebookInit(model.vq, rows, iters, seed)
    missing = init.rows
    while missing:
        arrays = converter(iterator.next(), device)
        x_enc = arrays[0] if isinstance(arrays, (tuple, list)) else arrays
        with core.using_config('train', False), core.no_backprop_mode():
            z = model.encoder(x_enc)
        missing = init.collect(z)
    return init.run(optimizer=optimizer, comm=comm)
