"""What the EMA codebook rule costs per step, and what it replaces: vqvae_vq_ema_accumulate + vqvae_vq_ema_apply back to
back, and beside them vqvae_vq_grad_w (the fp64 scatter of the codebook loss, which a step with an EMA object no longer
runs), at configs[1] (N = 1 920, k = 512, d = 64), at the reference's default model (N = 480, k = 128, d = 512) and at
configs[3] (N = 1 048 560, k = 8 192, d = 128); `--calls` back-to-back calls per shape between two device events,
`--repeats` such windows.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/vq_ema_prof.py` for the
per-kernel times.  The printed floor is the time to read z once at the HBM rate given by --hbm-tbs."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-vq-vae_amd'))

SHAPES = {'c1': (2, 960, 512, 64), 'default': (4, 120, 128, 512), 'c3': (16, 65535, 8192, 128)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--shapes', default='c1,default,c3')
    ap.add_argument('--patterns', default='hot,one')
    ap.add_argument('--hbm-tbs', type=float, default=8.0, help='HBM rate for the read-z-once floor, TB/s')
    args = ap.parse_args()
    from vqvae_amd import _lib, backend
    backend.init(0)
    lib = _lib.load()
    print('| shape | pattern | accumulate + apply, us | accumulate, us | vq_grad_w, us | read z once, us | accumulate / floor |')
    print('|---|---|---|---|---|---|---|')
    for name in args.shapes.split(','):
        B, T, k, d = SHAPES[name]
        z = backend.to_device(np.random.default_rng(2).standard_normal((B, d, T), dtype=np.float32))
        W = backend.to_device(np.random.default_rng(3).standard_normal((k, d), dtype=np.float32))
        count, esum = backend.zeros((k,), np.float32), backend.zeros((k, d), np.float32)
        _lib.call('vqvae_vq_ema_reset', W.ptr, count.ptr, esum.ptr, k, d, None, backend.stream())
        stats, gW = backend.zeros((k * (d + 1),), np.float32), backend.zeros((k, d), np.float32)
        ws = backend.DeviceArray((max(lib.vqvae_vq_ema_workspace_bytes(B, d, T, k), lib.vqvae_vq_workspace_bytes(B, d, T, k)),),
                                 np.uint8)
        for pattern in args.patterns.split(','):
            rs = np.random.RandomState(1)
            if pattern == 'one':         # a collapsed codebook: every row on one code
                host = np.full((B, T), k // 3, np.int32)
            else:                        # an eighth of the codes alive, a few of them hot
                alive = rs.choice(k, k // 8, replace=False)
                host = alive[(rs.standard_exponential(B * T) * alive.size / 6).astype(np.int64) % alive.size] \
                    .reshape(B, T).astype(np.int32)
            idx = backend.to_device(host)

            def acc():
                _lib.call('vqvae_vq_ema_accumulate', idx.ptr, z.ptr, B, d, T, k, stats.ptr, ws.ptr, ws.nbytes, backend.stream())

            def both():
                acc()
                _lib.call('vqvae_vq_ema_apply', W.ptr, count.ptr, esum.ptr, stats.ptr, k, d, 0.99, 1e-5, backend.stream())

            def grad():
                _lib.call('vqvae_vq_grad_w', idx.ptr, z.ptr, B, d, T, k, gW.ptr, 0, ws.ptr, ws.nbytes, backend.stream())

            def timed(fn):
                best = []
                for _ in range(args.repeats):
                    for _ in range(args.warmup):
                        fn()
                    backend.synchronize()
                    e0 = backend.Event().record(backend.stream())
                    for _ in range(args.calls):
                        fn()
                    e1 = backend.Event().record(backend.stream())
                    backend.synchronize()
                    ms = C.c_float()
                    _lib.call('vqvae_event_elapsed_ms', C.byref(ms), e0.h, e1.h)
                    best.append(ms.value * 1e3 / args.calls)
                return best
            t_both, t_acc, t_grad = timed(both), timed(acc), timed(grad)
            floor = B * d * T * 4 / (args.hbm_tbs * 1e12) * 1e6
            fmt = lambda v: ' / '.join('%.1f' % x for x in v)
            print('| %s (N %d, k %d, d %d) | %s | %s | %s | %s | %.1f | %.1fx |'
                  % (name, B * T, k, d, pattern, fmt(t_both), fmt(t_acc), fmt(t_grad), floor, min(t_acc) / floor))
    print('%d calls back to back per window, %d windows per cell (all shown); floor = bytes of z / %.1f TB/s'
          % (args.calls, args.repeats, args.hbm_tbs))


if __name__ == '__main__':
    main()
