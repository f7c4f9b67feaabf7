"""What the k-means codebook initialisation costs: vqvae_kmeans_seed (k rounds of two launches), one Lloyd iteration
(vqvae_vq_nearest_fwd + vqvae_vq_ema_accumulate + vqvae_kmeans_inertia + vqvae_kmeans_update) and a whole
KMeansCodebookInit.run (seeding, --iters iterations, the final assignment, one read-back) at configs[1] (N = 30 720,
k = 512, d = 64), at the reference's default model (N = 7 680, k = 128, d = 512) and at configs[3] (N = 524 288, k = 8 192,
d = 128).  One warm-up call, then `--repeats` windows between two device events (the whole run: a host clock around a call
that ends in its read-back); every window is printed.  Per round the seeding reads the pool once: the bytes/s column is
N * d * 4 * k / seeding time, the last column that rate over --copy-tbs (what a streaming copy reaches on this box).
Run it under `rocprofv3 --kernel-trace --stats -- python tools/vq_kmeans_prof.py` for the per-kernel times."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-vq-vae_amd'))

SHAPES = {'c1': (30720, 512, 64), 'default': (7680, 128, 512), 'c3': (524288, 8192, 128)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--shapes', default='c1,default,c3')
    ap.add_argument('--copy-tbs', type=float, default=6.3, help='streaming-copy rate for the last column, TB/s')
    args = ap.parse_args()
    import vqvae_amd as V
    from vqvae_amd import _lib, backend
    backend.init(0)
    lib = _lib.load()
    st = backend.stream()
    print('device: %s' % (backend.device_info(),))
    print('| shape | seeding, ms | us per round | pool read, TB/s | of the copy rate | one Lloyd iteration, ms | whole run (%d iterations), ms |'
          % args.iters)
    print('|---|---|---|---|---|---|---|')
    for name in args.shapes.split(','):
        N, k, d = SHAPES[name]
        rs = np.random.default_rng(2)
        host = rs.standard_normal((d, N), dtype=np.float32) + rs.integers(-3, 4, (d, N // 64)).repeat(64, 1).astype(np.float32)
        pool = backend.to_device(host)
        W, rows, mind = backend.empty((k, d)), backend.empty((k,), np.int32), backend.empty((N,))
        idx, stats = backend.empty((N,), np.int32), backend.empty((k * (d + 1),))
        out, empty = backend.zeros((1,), np.float64), backend.zeros((1,), np.int32)
        ws = backend.DeviceArray((max(lib.vqvae_kmeans_workspace_bytes(N, d, k), lib.vqvae_vq_workspace_bytes(1, d, N, k),
                                      lib.vqvae_vq_ema_workspace_bytes(1, d, N, k)),), np.uint8)

        def seeding():
            _lib.call('vqvae_kmeans_seed', pool.ptr, N, d, k, 0, W.ptr, rows.ptr, mind.ptr, ws.ptr, ws.nbytes, st)

        def lloyd():
            _lib.call('vqvae_vq_nearest_fwd', pool.ptr, W.ptr, 1, d, N, k, 0, idx.ptr, None, None, ws.ptr, ws.nbytes, st)
            _lib.call('vqvae_vq_ema_accumulate', idx.ptr, pool.ptr, 1, d, N, k, stats.ptr, ws.ptr, ws.nbytes, st)
            _lib.call('vqvae_kmeans_inertia', pool.ptr, W.ptr, idx.ptr, N, d, k, out.ptr, ws.ptr, ws.nbytes, st)
            _lib.call('vqvae_kmeans_update', pool.ptr, N, d, k, stats.ptr, 0, 0, W.ptr, empty.ptr, st)

        def timed(fn):
            fn()
            backend.synchronize()
            ms_all = []
            for _ in range(args.repeats):
                e0 = backend.Event().record(st)
                fn()
                e1 = backend.Event().record(st)
                backend.synchronize()
                ms = C.c_float()
                _lib.call('vqvae_event_elapsed_ms', C.byref(ms), e0.h, e1.h)
                ms_all.append(ms.value)
            return ms_all

        def whole():
            vq = V.VQ(k, d)
            vq.to_gpu()
            init = V.KMeansCodebookInit(vq, rows=N, iters=args.iters, seed=0)
            init.collect(pool.reshape(1, d, N))
            backend.synchronize()
            t0 = time.perf_counter()
            init.run()
            return (time.perf_counter() - t0) * 1e3
        t_seed = timed(seeding)
        t_lloyd = timed(lloyd)
        whole()
        t_whole = [whole() for _ in range(args.repeats)]
        rate = N * d * 4.0 * k / (min(t_seed) * 1e-3) / 1e12
        fmt = lambda v: ' / '.join('%.3f' % x for x in v)
        print('| %s (N %d, k %d, d %d) | %s | %.2f | %.2f | %.0f %% | %s | %s |'
              % (name, N, k, d, fmt(t_seed), min(t_seed) * 1e3 / k, rate, 100 * rate / args.copy_tbs, fmt(t_lloyd), fmt(t_whole)))
    print('one warm-up call, then %d windows per cell (all shown); per-round time and rate from the fastest window'
          % args.repeats)


if __name__ == '__main__':
    main()
