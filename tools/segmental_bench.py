"""Duration-penalised quantisation over a validation list: segmental.segment_many (csrc/segmental.h) through the default
model's front end, timed end to end and per launch, beside encode_many on the same list and the NumPy restatement on the
host CPU.
usage: python tools/segmental_bench.py [--rounds 3] [--utterances 300] [--seed 0] [--cpu-utterances 16] [--cpu-threads 16]
                                       [--step-timeout 300] [--out FILE]
       python tools/segmental_bench.py --parent DIR [--rounds 3] [--steps 30]
  Model: the default one (d = 512, k = 128), seeded weights (tools/frontend_bench.build_links).  Utterances: the list of
  DESIGN 7f, tools/gen_bench.gamma_lengths(300, seed 0) (gamma(shape 2, mean 3.6 s) clipped to 0.5 - 10 s at 16 kHz), host
  waves.  Penalties: multiples of s, the mean squared distance of a frame to its nearest code over the first utterances:
  P = 1 is [s / 64], P = 8 is s * [0, 1/4096, 1/1024, 1/256, 1/64, 1/16, 1/4, 1] (the seeded model's latents of an
  utterance lie close together: at s / 4 an utterance is one segment already).
  The GPU step is a fresh process of this file (--step gpu) under --step-timeout.
  (a) encode_many, segment_many with P = 1 and with P = 8, end to end on the host clock (upload, encoder, quantiser, table,
      DP, results back).
  (b) one more pass of each segment_many with device events round every vqvae_seg_segment call (table + DP) and round a
      vqvae_seg_distances call on the same operands (the table alone); the DP launch is the difference.
  (c) the rate / distortion figures of the P = 8 call.
  (d) the first --cpu-utterances utterances through tests/segmental_ref.py with P = 1 on --cpu-threads processes, scaled to
      the whole list by frames, and compared with the device's codes.
  Ranges over the rounds, not means.  Prints one JSON line; --out also writes the table as text.
  --parent DIR (a built tree of the parent commit): tools/frontend_bench.py's interleaved bench.py rounds."""
import argparse
import ctypes as C
import json
import multiprocessing
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-vq-vae_amd'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

MULTIPLES = (0.0, 1.0 / 4096, 1.0 / 1024, 1.0 / 256, 1.0 / 64, 1.0 / 16, 0.25, 1.0)


def _restate(job):
    import segmental_ref as R
    z, W, lam = job
    codes, n_seg, cost = R.viterbi(R.distances(z, W), lam)
    return codes, n_seg, float(cost)


def step(a):
    """The GPU step in this process; prints its JSON line and leaves the CPU's share in --dump."""
    import vqvae_amd as V
    from frontend_bench import build_links
    from gen_bench import gamma_lengths
    from resident_corpus_bench import synthetic_waves
    from vqvae_amd import _lib, backend, segmental
    backend.init(0)
    enc, vq, _ = build_links(a.seed + 3)
    waves = [(w / np.abs(w).max()).astype(np.float32) for w in synthetic_waves(gamma_lengths(a.utterances, a.seed), a.seed + 2)]
    st = backend.stream()
    n_cpu = min(a.cpu_utterances, a.utterances)
    _, first = V.encode_many(enc, vq, waves[:max(n_cpu, 1)], return_latents=True)
    s = float(np.mean([D.min(axis=1).mean() for D in segmental.distance_table(vq, first)]))
    p1, p8 = [s / 64.0], [s * m for m in MULTIPLES]

    def host_clock(fn):
        fn()                                                         # warm-up: allocator pool, code objects
        backend.synchronize()
        walls = []
        for _ in range(a.rounds):
            backend.synchronize()
            t0 = time.perf_counter()
            out = fn()
            backend.synchronize()
            walls.append(time.perf_counter() - t0)
        return out, [round(min(walls), 5), round(max(walls), 5)]

    out = {'step': 'gpu', 'penalty_unit': s}
    codes, out['encode_many_host_s'] = host_clock(lambda: V.encode_many(enc, vq, waves))
    seg1, out['segment_many_p1_host_s'] = host_clock(lambda: V.segment_many(enc, vq, waves, p1))
    seg8, out['segment_many_p8_host_s'] = host_clock(lambda: V.segment_many(enc, vq, waves, p8))
    out.update(frames=int(seg1.tl.astype(np.int64).sum()), longest=int(seg1.tl.max()), k=seg1.k, d=int(vq.W.data.shape[1]))

    def elapsed(e0, e1):
        el = C.c_float(0)
        _lib.call('vqvae_event_elapsed_ms', C.byref(el), e0.h, e1.h)
        return float(el.value)

    call0 = segmental.call
    for name, pen in (('p1', p1), ('p8', p8)):
        both, table, launches = [], [], 0
        for _ in range(a.rounds):
            marks = []

            def call(entry, *args):
                if entry != 'vqvae_seg_segment':
                    return call0(entry, *args)
                d, z, W = args[0], args[1], args[2]
                scratch = backend.DeviceArray((int(d._obj.ttot), int(d._obj.k)), np.float64)
                e0 = backend.Event().record(st)
                call0('vqvae_seg_distances', d, z, W, scratch.ptr, st)
                e1 = backend.Event().record(st)
                call0(entry, *args)
                marks.append((e0, e1, backend.Event().record(st)))
            segmental.call = call
            try:
                V.segment_many(enc, vq, waves, pen)
                backend.synchronize()
            finally:
                segmental.call = call0
            table.append(sum(elapsed(e0, e1) for e0, e1, e2 in marks))
            both.append(sum(elapsed(e1, e2) for e0, e1, e2 in marks))
            launches = len(marks)
        out['device_' + name] = {'calls': launches, 'table_ms': [round(min(table), 4), round(max(table), 4)],
                                 'table_and_dp_ms': [round(min(both), 4), round(max(both), 4)],
                                 'dp_ms': [round(min(b - t for b, t in zip(both, table)), 4), round(max(b - t for b, t in zip(both, table)), 4)]}
    out['curve'] = {'penalties': [float(v) for v in seg8.penalties], 'segments': seg8.n_segments.astype(np.int64).sum(axis=1).tolist(),
                    'mean_run': [float(v) for v in seg8.mean_run], 'segments_per_second': [float(v) for v in seg8.segments_per_second(16000)],
                    'distortion_per_frame': [float(v) for v in seg8.distortion.sum(axis=1) / out['frames']]}
    if a.dump:
        host = seg1.codes[0].to_host()
        np.savez(a.dump, W=vq.W.data.get(), lam=p1[0], n=n_cpu, **dict([('z%d' % i, first[i]) for i in range(n_cpu)] +
                                                                    [('c%d' % i, host[i]) for i in range(n_cpu)]))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default='', help='a built tree of the parent commit: interleave its bench.py with this tree\'s')
    ap.add_argument('--step', default='', choices=('', 'gpu'), help='(internal) run the GPU step in this process')
    ap.add_argument('--dump', default='', help='(internal) where the GPU step leaves the CPU\'s share')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--utterances', type=int, default=300)
    ap.add_argument('--cpu-utterances', type=int, default=16)
    ap.add_argument('--cpu-threads', type=int, default=16)
    ap.add_argument('--step-timeout', type=int, default=300)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.parent:
        from frontend_bench import against_parent
        return against_parent(a)
    if a.step:
        return step(a)
    out = {'tool': 'segmental_bench', 'utterances': a.utterances, 'rounds': a.rounds}
    with tempfile.TemporaryDirectory() as tmp:
        dump = os.path.join(tmp, 'cpu_share.npz')
        cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ['--step', 'gpu', '--dump', dump]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=a.step_timeout)
        if r.returncode != 0:
            raise SystemExit('segmental_bench: the GPU step failed (%d): %s' % (r.returncode, r.stderr.decode()[-2000:]))
        g = out['gpu'] = json.loads(r.stdout.decode().strip().splitlines()[-1])
        g.pop('step')
        with np.load(dump) as f:
            n_cpu, W, lam = int(f['n']), f['W'], float(f['lam'])
            jobs = [(f['z%d' % i], W, lam) for i in range(n_cpu)]
            device = [f['c%d' % i] for i in range(n_cpu)]
    if jobs:
        pool = multiprocessing.get_context('spawn').Pool(a.cpu_threads)
        t0 = time.perf_counter()
        rows = pool.map(_restate, jobs, chunksize=1)
        cpu_s = time.perf_counter() - t0
        pool.close()
        pool.join()
        frames = sum(j[0].shape[1] for j in jobs)
        out['cpu'] = {'numpy_host_cpu_s': round(cpu_s, 3), 'numpy_utterances': len(jobs), 'numpy_frames': frames, 'cpu_processes': a.cpu_threads,
                      'numpy_scaled_to_the_list_s': round(cpu_s * g['frames'] / max(frames, 1), 2),
                      'device_equals_numpy': bool(all(np.array_equal(r[0], c) for r, c in zip(rows, device)))}
    for name in ('p1', 'p8'):
        out['ratio_to_encode_many_' + name] = round(g['segment_many_%s_host_s' % name][0] / g['encode_many_host_s'][0], 3)
    print(json.dumps(out))
    if a.out:
        lines = ['tools/segmental_bench.py --rounds %d --utterances %d  (d = %d, k = %d, %d frames, longest utterance %d frames, penalty unit s = %.6g)'
                 % (a.rounds, a.utterances, g['d'], g['k'], g['frames'], g['longest'], g['penalty_unit']), '',
                 '(a) end to end, host clock, %d rounds: encode_many %.5f - %.5f s; segment_many P = 1 %.5f - %.5f s (x%.3f); P = 8 %.5f - %.5f s (x%.3f)'
                 % (a.rounds, g['encode_many_host_s'][0], g['encode_many_host_s'][1], g['segment_many_p1_host_s'][0], g['segment_many_p1_host_s'][1],
                    out['ratio_to_encode_many_p1'], g['segment_many_p8_host_s'][0], g['segment_many_p8_host_s'][1], out['ratio_to_encode_many_p8']), '',
                 '(b) P   calls   table alone, ms     table + DP, ms      DP (difference), ms']
        for name in ('p1', 'p8'):
            v = g['device_' + name]
            lines.append('    %s   %5d   %8.4f - %8.4f   %8.4f - %8.4f   %8.4f - %8.4f' % ((name[1:], v['calls']) + tuple(v['table_ms']) + tuple(v['table_and_dp_ms']) + tuple(v['dp_ms'])))
        lines += ['', '(c) penalty / s   segments   mean run   segments / s   distortion / frame']
        c = g['curve']
        for i, m in enumerate(MULTIPLES):
            lines.append('    %11.6f   %8d   %8.3f   %12.3f   %12.6g' % (m, c['segments'][i], c['mean_run'][i], c['segments_per_second'][i], c['distortion_per_frame'][i]))
        if 'cpu' in out:
            u = out['cpu']
            lines += ['', '(d) tests/segmental_ref.py, NumPy on the host CPU, the first %d utterances (%d frames), P = 1, on %d processes, once: %.3f s; scaled by '
                      'frames to the list: %.2f s; the device\'s codes equal it on those utterances: %s'
                      % (u['numpy_utterances'], u['numpy_frames'], u['cpu_processes'], u['numpy_host_cpu_s'], u['numpy_scaled_to_the_list_s'], u['device_equals_numpy'])]
        lines += ['', json.dumps(out)]
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
