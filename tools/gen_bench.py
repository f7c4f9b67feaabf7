"""Throughput of the device-resident generation loop (generate.py:105-145) at BASELINE decoder sizes.
usage: python tools/gen_bench.py [--workload c2|c5|ref] [--n 1] [--steps 16000] [--graph-steps 8]
       python tools/gen_bench.py --workload ref --lockstep 128 [--group 128] [--steps 4000]
       python tools/gen_bench.py --workload ref --lengths-n 300 --lengths-seed 0 [--lengths-rate 16000] [--group 128]
           N utterances of gamma-distributed lengths (mean 3.6 s, clipped to 0.5-10 s at --lengths-rate samples per second;
           a lower rate keeps the list's shape and shrinks the run) through generate_lockstep twice: as sorted groups
           (refill=False) and with the columns refilled on the device (refill=True)
       python tools/gen_bench.py --workload ref --lockstep 128 --refill    equal lengths through the refilled kernels (tick cost)
       ... --lockstep N / --lengths-n N --latent-cond    the condition kept at the latent rate (generation.LatentCondition: random
           latents of ceil(T / 64) frames instead of the dense (N, Cc, T) array, which is never made); prints the bytes of
           both forms.  With --lengths-n, --refill runs the refilled road only
       ... --device-uniforms    the uniforms drawn inside the finishing kernels (vqvae_amd.DeviceUniforms) instead of a host
           array; without it the array's draw and upload are timed and printed
       ... [--temperature 0.8] [--top-k 32] [--top-p 0.95]   sampling controls (every sequence the same); with any of them
       generate_sequence runs the per-step kernels, and --batch refuses"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-vq-vae_amd'))


def gamma_lengths(n, seed, rate=16000.0):
    """Utterance lengths in samples: gamma(shape 2, mean 3.6 s) clipped to 0.5-10 s, at ``rate`` samples per second."""
    rs = np.random.RandomState(seed)
    return np.maximum((np.clip(rs.gamma(2.0, 1.8, n), 0.5, 10.0) * rate).astype(np.int64), 2)


def random_latents(backend, rs, tl, Cl, G, upscale=64):
    """A LatentCondition of random values, uploaded sequence by sequence."""
    from vqvae_amd.generation import LatentCondition
    latents = [backend.to_device(rs.standard_normal((Cl, int(t))).astype(np.float32)) for t in tl]
    return LatentCondition.from_latents(latents, backend.to_device(rs.standard_normal((len(tl), G)).astype(np.float32)), upscale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='c2', help='c2 / c5: BASELINE decoders (256 channels); ref: the reference\'s default '
                    'decoder (params.py: 3 x 10 blocks, 512 / 512 / 256, condition 640, softmax 256)')
    ap.add_argument('--dump', default='', help='write the sampled outputs to this .npy file (same seed = same file)')
    ap.add_argument('--n', type=int, default=1)
    ap.add_argument('--steps', type=int, default=16000)
    ap.add_argument('--graph-steps', type=int, default=8)
    ap.add_argument('--group', type=int, default=4)
    ap.add_argument('--streams', type=int, default=8)
    ap.add_argument('--batch', type=int, default=0, help='N sequences through generate_batch (concurrent groups of 4)')
    ap.add_argument('--lockstep', type=int, default=0, help='N sequences through generate_lockstep (groups of <= --group, default 128, '
                    'advancing together on the MFMA kernels); --graph-steps 0 = eager launches')
    ap.add_argument('--refill', action='store_true', help='--lockstep through generate_lockstep(refill=True)')
    ap.add_argument('--latent-cond', action='store_true', help='--lockstep / --lengths-n: the condition as a LatentCondition '
                    '(local latents 4/5 of the condition channels, x64), not the dense array')
    ap.add_argument('--lengths-n', type=int, default=0, help='N utterances of seeded gamma lengths, sorted groups against refill')
    ap.add_argument('--lengths-seed', type=int, default=0)
    ap.add_argument('--lengths-rate', type=float, default=16000.0, help='samples per second of the length list (default 16 kHz)')
    ap.add_argument('--per-step-kernels', action='store_true', help='hipGraph of per-step kernels instead of the persistent kernel')
    ap.add_argument('--temperature', type=float, default=None, help='sampling temperature (0 = greedy); default: none')
    ap.add_argument('--top-k', type=int, default=None, help='keep the k most likely classes; default: none')
    ap.add_argument('--top-p', type=float, default=None, help='nucleus mass in (0, 1]; default: none')
    ap.add_argument('--device-uniforms', action='store_true', help='the uniforms as a DeviceUniforms(0) drawn inside the kernels '
                    '(include/vqvae_gen_rng.h) instead of a host array; without it the array\'s draw and upload are timed and printed')
    a = ap.parse_args()
    ctl = dict(temperature=a.temperature, top_k=a.top_k, top_p=a.top_p)
    ctl_txt = ''.join(' %s=%g' % (k, v) for k, v in ctl.items() if v is not None) or ' no controls'
    from vqvae_amd import backend
    from vqvae_amd.wavenet import WaveNet
    backend.init(0)
    mol = a.workload == 'c5'
    ref = a.workload == 'ref'
    n_loop = 4 if mol else 3 if ref else 2
    Cc = 640 if ref else 192
    Cl = 512 if ref else 128                                 # --latent-cond: local channels; the rest is the speaker vector
    if ref:
        dec = WaveNet(n_loop, 10, 2, 256, 512, 512, 256, 256, False, 30, -40, Cc, 0)
    else:
        dec = WaveNet(n_loop, 10, 2, 1 if mol else 256, 256, 256, 256, 256, mol, 30, -40, Cc, 0)
    from vqvae_amd import functions as F
    from vqvae_amd.core import Variable
    # materialise the lazily initialised parameters with one tiny forward
    x = backend.zeros((1, 1 if mol else 256, 2048, 1))
    c = backend.zeros((1, Cc, 2048, 1))
    dec.to_gpu()
    dec(Variable(x), Variable(c))
    T = a.steps + 1

    def uniforms(rs, shape):
        """The (T, N, n_uniform) host draw, with the host time and bytes it and its upload cost, or a DeviceUniforms."""
        if a.device_uniforms:
            from vqvae_amd import DeviceUniforms
            print('uniforms: DeviceUniforms(0), %d bytes of stream ids; the host array would be %d bytes' % (8 * shape[1], 8 * int(np.prod(shape))))
            return DeviceUniforms(0)
        t0 = time.time()
        u = rs.uniform(0.01, 0.99, shape)
        t1 = time.time()
        d = backend.to_device(u.reshape(-1))
        backend.synchronize()
        t2 = time.time()
        del d
        print('uniforms: host array %s, %d bytes: draw %.3f s, upload %.3f s (the upload happens again inside the timed call)'
              % (shape, u.nbytes, t1 - t0, t2 - t1))
        return u

    if a.lengths_n:
        from vqvae_amd.generation import plan_lockstep, plan_refill, refill_slots
        group = a.group if a.group > 4 else 128
        lengths = gamma_lengths(a.lengths_n, a.lengths_seed, a.lengths_rate)
        N, T = a.lengths_n, int(lengths.max())
        steps, groups = plan_lockstep(N, T, lengths, group=group)
        ticks = dict(sorted=sum(g for _, g in groups), refill=plan_refill(steps, refill_slots((steps > 0).sum(), group))[0])
        rs = np.random.RandomState(0)
        if a.latent_cond:
            cond = random_latents(backend, rs, -(-lengths // 64), Cl, Cc - Cl)
            print('condition: latent %d bytes; dense (N, Cc, T) = (%d, %d, %d) would be %d bytes (%.1f GB), %.1fx'
                  % (cond.nbytes, N, Cc, T, 4 * N * Cc * T, 4e-9 * N * Cc * T, 4.0 * N * Cc * T / cond.nbytes))
        else:
            cond = backend.zeros((N, Cc, T), np.float32)
            for i in range(N):                               # row by row: the whole array may not fit the host twice
                cond.flat_view(i * Cc * T, Cc * T).set(rs.standard_normal(Cc * T).astype(np.float32))
        u = uniforms(rs, (T, N, 10 if mol else 1))
        short = np.minimum(lengths, 65)
        roads = (('refill', True),) if a.refill else (('sorted', False), ('refill', True))
        for _, refill in roads:                              # warm-up of the roads
            dec.generate_lockstep(cond, u, lengths=short, group=group, graph_steps=a.graph_steps, refill=refill, **ctl)
        print('lengths workload %s N=%d seed %d rate %g: %d samples, longest %d, group %d graph-steps %d,%s; lower bound %d ticks'
              % (a.workload, N, a.lengths_seed, a.lengths_rate, steps.sum(), steps.max(), group, a.graph_steps, ctl_txt,
                 max(int(steps.max()), -(-int(steps.sum()) // group))))
        res = {}
        for name, refill in roads:
            t0 = time.time()
            res[name] = dec.generate_lockstep(cond, u, lengths=lengths, group=group, graph_steps=a.graph_steps, refill=refill, **ctl)
            dt = time.time() - t0
            print('  %-6s %8d ticks in %8.3f s = %7.1f us/tick, %9.0f samples/s' % (name, ticks[name], dt, 1e6 * dt / ticks[name],
                                                                              steps.sum() / dt))
            res[name + '_dt'] = dt
        if a.dump:
            np.save(a.dump, res['refill'])
        if a.refill:
            return
        print('  ticks sorted / refill %.3f, wall sorted / refill %.3f, outputs equal: %s'
              % (ticks['sorted'] / ticks['refill'], res['sorted_dt'] / res['refill_dt'], np.array_equal(res['sorted'], res['refill'])))
        return
    if a.lockstep:
        group = a.group if a.group > 4 else 128
        rs = np.random.RandomState(0)
        if a.latent_cond:
            cond = random_latents(backend, rs, [-(-T // 64)] * a.lockstep, Cl, Cc - Cl)
            T = cond.shape[2]
            ctl = dict(ctl, lengths=np.full(a.lockstep, a.steps + 1))         # the dense run's steps, whatever 64 * frames is
            ctl_txt += ' latent condition (%d bytes, dense %d)' % (cond.nbytes, 4 * a.lockstep * Cc * (a.steps + 1))
        else:
            cond = backend.to_device(rs.standard_normal((a.lockstep, Cc, T)).astype(np.float32))
        u = uniforms(rs, (T, a.lockstep, 10 if mol else 1))
        if a.refill:
            ctl = dict(ctl, refill=True)
            ctl_txt += ' refill'
        if a.device_uniforms:
            ctl_txt += ' device uniforms'
        dec.generate_lockstep(cond, u, n_steps=64, group=group, graph_steps=a.graph_steps, **ctl)      # warm-up
        t0 = time.time()
        o = dec.generate_lockstep(cond, u, group=group, graph_steps=a.graph_steps, **ctl)
        dt = time.time() - t0
        if a.dump:
            np.save(a.dump, o)
        ngroups = (a.lockstep + group - 1) // group
        print('lockstep workload %s N=%d group %d graph-steps %d,%s: %d steps in %.3f s = %.1f us/step/group, %.0f steps/s, '
              '%.0f samples/s aggregate (%.1f sequences in real time at 16 kHz), distinct outputs %d'
              % (a.workload, a.lockstep, group, a.graph_steps, ctl_txt, a.steps, dt, 1e6 * dt / a.steps / ngroups, a.steps * ngroups / dt,
                 a.lockstep * a.steps / dt, a.lockstep * a.steps / dt / 16000, len(np.unique(o))))
        return
    if a.batch:
        rs = np.random.RandomState(0)
        cond = backend.to_device(rs.standard_normal((a.batch, Cc, T)).astype(np.float32))
        u = rs.uniform(0.01, 0.99, (T, a.batch, 10 if mol else 1))
        dec.generate_batch(cond, u, n_steps=64, group=a.group, max_streams=a.streams, **ctl)
        t0 = time.time()
        o = dec.generate_batch(cond, u, group=a.group, max_streams=a.streams, **ctl)
        dt = time.time() - t0
        if a.dump:
            np.save(a.dump, o)
        print('group %d streams %d: ' % (a.group, a.streams) + 'batch of %d sequences x %d steps in %.3f s = %.0f samples/s aggregate (%.1f sequences in real time at 16 kHz)'
              % (a.batch, a.steps, dt, a.batch * a.steps / dt, a.batch * a.steps / dt / 16000))
        return
    rs = np.random.RandomState(0)
    cond = backend.to_device(rs.standard_normal((a.n, Cc, T)).astype(np.float32))
    u = uniforms(rs, (T, a.n, 10 if mol else 1))
    pers = not a.per_step_kernels and all(v is None for v in ctl.values())     # controls leave the persistent kernel
    dec.generate_sequence(cond, u, n_steps=64, graph_steps=a.graph_steps, persistent=pers, **ctl)      # warm-up
    t0 = time.time()
    out = dec.generate_sequence(cond, u, graph_steps=a.graph_steps, persistent=pers, **ctl)
    dt = time.time() - t0
    o = out.get()
    if a.dump:
        np.save(a.dump, o)
    print('%s workload %s n=%d,%s: %d steps in %.3f s = %.1f us/step, %.0f samples/s per sequence (%.2fx real time at 16 kHz), '
          'distinct outputs %d' % ('persistent' if pers else 'per-step kernels', a.workload, a.n, ctl_txt, a.steps, dt, 1e6 * dt / a.steps, a.steps / dt,
                                   a.steps / dt / 16000, len(np.unique(o))))


if __name__ == '__main__':
    main()
