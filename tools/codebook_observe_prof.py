"""What CodebookMonitor.observe costs per step: vqvae_codebook_observe at configs[1] (N = 1 920, k = 512, d = 64) and at
configs[3] (N = 1 048 560, k = 8 192, d = 128), `--calls` back-to-back calls per shape between two device events.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/codebook_observe_prof.py` for the per-kernel times; the
printed bytes are what the histogram must move (the indices once, the bins once), for a rate over its kernel time."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-vq-vae_amd'))

SHAPES = {'c1': (2, 960, 512, 64), 'c3': (16, 65535, 8192, 128)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--shapes', default='c1,c3')
    args = ap.parse_args()
    from vqvae_amd import _lib, backend
    backend.init(0)
    for name in args.shapes.split(','):
        B, T, k, d = SHAPES[name]
        rs = np.random.RandomState(1)
        alive = rs.choice(k, k // 8, replace=False)
        idx = backend.to_device(alive[rs.randint(0, alive.size, (B, T))].astype(np.int32))
        z = backend.to_device(np.random.default_rng(2).random((B, d, T), dtype=np.float32))
        counts, usage = backend.zeros((k,), np.int32), backend.zeros((k,), np.float32)
        reservoir, steps = backend.zeros((k, d), np.float32), backend.zeros((1,), np.int32)
        stats = backend.zeros((_lib.CODEBOOK_STATS_WORDS,), np.float64)

        def run(n):
            for _ in range(n):
                _lib.call('vqvae_codebook_observe', idx.ptr, z.ptr, B, d, T, k, 0.99, 0, counts.ptr, usage.ptr, reservoir.ptr,
                          steps.ptr, stats.ptr, backend.stream())
        run(args.warmup)
        backend.synchronize()
        e0 = backend.Event().record(backend.stream())
        run(args.calls)
        e1 = backend.Event().record(backend.stream())
        backend.synchronize()
        ms = C.c_float()
        _lib.call('vqvae_event_elapsed_ms', C.byref(ms), e0.h, e1.h)
        print('%s: B %d T %d k %d d %d: %.2f us per observe call (%d calls back to back, three kernels each); histogram bytes '
              '%d (indices) + %d (bins); reservoir bytes written %d; perplexity %.2f'
              % (name, B, T, k, d, ms.value * 1e3 / args.calls, args.calls, B * T * 4, k * 4, k * d * 4, stats.get()[0]))


if __name__ == '__main__':
    main()
