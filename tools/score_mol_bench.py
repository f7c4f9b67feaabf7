"""Held-out likelihood of a corpus under a mixture-of-logistics decoder: scoring_mol.score_many_mol (the ragged decoder pass
with csrc/ragged_mol.hip's embed and NLL) beside the per-utterance loop over the EXISTING training forward -- decoder(x_dec,
cond) on the dense condition plus calculate_logistic_loss under no_backprop_mode, one utterance after the other.  The loop
over existing code is the yardstick.
usage: python tools/score_mol_bench.py [--rounds 3] [--utterances 100] [--seed 0] [--chunk-bytes 1073741824] [--matmul float32x2]
                                       [--step-timeout 600] [--pool-limit 103079215104]
       python tools/score_mol_bench.py --parent DIR [--rounds 3] [--steps 30]
  Model: BASELINE configs[4]'s decoder (4 x 10 blocks, 256 residual / 256 dilated / 256 skip channels, raw-sample input,
  10 logistics, condition 64 + 128), seeded weights with the head spread over the sample range.  Utterances:
  tools/gen_bench.gamma_lengths(N, seed) (gamma(shape 2, mean 3.6 s) clipped to 0.5 - 10 s at 16 kHz), each cut to 64 tl + 1
  samples so that both sides score the same 64 tl positions; the waves live on the device for both sides; the latent
  condition is seeded noise.
  The parent process runs the rounds interleaved, alternating who goes first, every GPU step a fresh child process under its
  own timeout: `--step loop`, `--step ragged` (one warm-up pass, one timed pass: host time, device span between two events,
  samples / s).  Ranges over the rounds are printed, not means.  Prints one JSON line.
  --parent DIR (a built tree of the parent commit): tools/score_bench.py's comparison of the two trees' bench.py."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-vq-vae_amd'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from score_bench import against_parent, last_json  # noqa: E402

DIMS = dict(n_loop=4, n_layer=10, R=256, D=256, S=256, Cl=64, G=128, M=10)


def build(a):
    """(wavenet on the device, LatentCondition, device waves per utterance, positions per utterance)."""
    import vqvae_amd as V
    from gen_bench import gamma_lengths
    from resident_corpus_bench import synthetic_waves
    from vqvae_amd import backend
    from vqvae_amd.wavenet import WaveNet
    m = DIMS
    M = m['M']
    wn = WaveNet(m['n_loop'], m['n_layer'], 2, 1, m['R'], m['D'], m['S'], 256, True, 3 * M, -40, m['Cl'] + m['G'], 0)
    rs = np.random.RandomState(a.seed + 3)
    for name, p in sorted(wn.namedparams()):
        sh = p.data.shape
        fan = int(np.prod(sh[1:])) if len(sh) > 1 else 1
        p.data = ((rs.standard_normal(sh) / np.sqrt(fan)) if len(sh) > 1 else 0.1 * rs.standard_normal(sh)).astype(np.float32)
    wn.proj2.W.data[M:2 * M] *= 20.0                       # a head whose mixture covers the sample range, not the 1e-12 floor
    wn.proj2.b.data[M:2 * M] = np.linspace(-100.0, 100.0, M)
    wn.proj2.b.data[2 * M:] = 3.0
    wn.to_gpu()
    lengths = gamma_lengths(a.utterances, a.seed)
    tl = np.maximum((np.asarray(lengths, np.int64) - 1) // 64, 1)
    lengths = 64 * tl + 1
    waves = backend.to_device_many([(w / np.abs(w).max()).astype(np.float32) for w in synthetic_waves(lengths, a.seed + 2)])
    local = [backend.to_device(np.maximum(rs.standard_normal((m['Cl'], int(t))), 0).astype(np.float32)) for t in tl]
    gv = backend.to_device(rs.standard_normal((a.utterances, m['G'])).astype(np.float32))
    cond = V.LatentCondition.from_latents(local, gv, 64)
    return wn, cond, waves, 64 * tl


def step(a):
    import vqvae_amd as V
    from vqvae_amd import _lib, backend, core
    from vqvae_amd.core import Variable
    backend.init(0)
    if a.matmul:
        backend.set_matmul_dtype(a.matmul)
    wn, cond, waves, n_pos = build(a)
    st = backend.stream()
    m = DIMS
    flushes = [0]

    def elapsed(e0, e1):
        el = C.c_float(0)
        _lib.call('vqvae_event_elapsed_ms', C.byref(el), e0.h, e1.h)
        return float(el.value)

    def loop():
        losses = []
        with core.using_config('train', False), core.no_backprop_mode():
            for i, (w, n) in enumerate(zip(waves, n_pos)):
                n = int(n)
                ci = V.LatentCondition.from_latents([cond.local.flat_view(int(cond.local_off[i]), m['Cl'] * int(cond.tl[i]), (m['Cl'], int(cond.tl[i])))],
                                                    cond.global_vec.flat_view(i * m['G'], m['G'], (1, m['G'])), 64)
                dense = ci.dense()
                x = w.flat_view(0, n, (1, 1, n, 1))                     # utils.py:104, 107: raw in, raw target
                t = w.flat_view(1, n, (1, 1, n, 1))
                y = wn(Variable(x), Variable(dense.reshape(1, m['Cl'] + m['G'], n, 1)))
                losses.append(wn.calculate_logistic_loss(y, t).data)
                del y, dense, x, t, ci
                # the existing forward keeps every block's gates and z and the allocator pool keeps a block of every size it
                # has seen: the pool is handed back when it passes --pool-limit
                if backend.memory_stats()['cached_bytes'] > a.pool_limit:
                    backend.synchronize()
                    backend.free_all_blocks()
                    flushes[0] += 1
        return losses

    def ragged():
        return V.score_many_mol(wn, cond, waves, chunk_bytes=a.chunk_bytes)

    def timed(fn):
        backend.synchronize()
        e0 = backend.Event().record(st)
        t0 = time.perf_counter()
        out = fn()
        host = time.perf_counter() - t0
        e1 = backend.Event().record(st)
        backend.synchronize()
        return out, {'host_s': host, 'device_span_s': 1e-3 * elapsed(e0, e1), 'wall_s': time.perf_counter() - t0}

    total = int(n_pos.sum())
    fn = loop if a.step == 'loop' else ragged
    timed(fn)                                            # warm-up: allocator pool, LDS opt-ins, weight packs
    flushes[0] = 0
    out, t = timed(fn)
    t['pool_flushes'] = flushes[0]
    bits = (np.array([float(l.get()) for l in out]) / np.log(2.0)) if a.step == 'loop' else out.bits_per_sample
    t.update(step=a.step, samples=total, samples_per_s=total / t['device_span_s'], bits_per_sample=[float(b) for b in bits])
    print(json.dumps(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default='', help="a built tree of the parent commit: interleave its bench.py with this tree's")
    ap.add_argument('--step', default='', choices=['', 'loop', 'ragged'], help='(a child process of this tool)')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--utterances', type=int, default=100)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--chunk-bytes', type=int, default=1 << 30)
    ap.add_argument('--matmul', default='', help='matmul mode (default: the process default)')
    ap.add_argument('--pool-limit', type=int, default=96 << 30, help='loop: hand the allocator pool back above this many cached bytes')
    ap.add_argument('--step-timeout', type=int, default=600, help='seconds every GPU step (child process) may take')
    a = ap.parse_args()
    if a.parent:
        return against_parent(a)
    if a.step:
        return step(a)
    common = ['--utterances', str(a.utterances), '--seed', str(a.seed), '--chunk-bytes', str(a.chunk_bytes),
              '--pool-limit', str(a.pool_limit)] + (['--matmul', a.matmul] if a.matmul else [])

    def child(which):
        cmd = [sys.executable, os.path.abspath(__file__), '--step', which] + common
        sys.stderr.write('score_mol_bench: %s\n' % ' '.join(cmd))
        sys.stderr.flush()
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=a.step_timeout)
        if r.returncode != 0:                                # a failed GPU step ends the run: nothing more is started
            raise SystemExit('score_mol_bench: step %s failed (%d): %s' % (which, r.returncode, r.stderr.decode()[-2000:]))
        return last_json(r.stdout.decode())
    rows = {'loop': [], 'ragged': []}
    for rnd in range(a.rounds):
        for which in (('loop', 'ragged') if rnd % 2 == 0 else ('ragged', 'loop')):
            rows[which].append(child(which))
    lb, rb = np.array(rows['loop'][0].pop('bits_per_sample')), np.array(rows['ragged'][0].pop('bits_per_sample'))
    for r in rows['loop'][1:] + rows['ragged'][1:]:
        r.pop('bits_per_sample')

    def rng(name, key):
        v = [r[key] for r in rows[name]]
        return [round(min(v), 4), round(max(v), 4)]
    keys = ('host_s', 'device_span_s', 'wall_s', 'samples_per_s')
    print(json.dumps({'tool': 'score_mol_bench',
                      'model': 'decoder 4 x 10 blocks, 256 / 256 / 256 channels, raw-sample input, 10 logistics, condition 64 + 128',
                      'matmul': a.matmul or 'process default', 'utterances': a.utterances, 'samples': rows['ragged'][0]['samples'],
                      'chunk_bytes': a.chunk_bytes, 'rounds': a.rounds,
                      'loop': dict((k, rng('loop', k)) for k in keys), 'ragged': dict((k, rng('ragged', k)) for k in keys),
                      'max_abs_difference_bits_per_sample': float(np.abs(lb - rb).max()),
                      'corpus_bits_per_sample': {'loop': float(lb.mean()), 'ragged': float(rb.mean())},
                      'all_rounds': rows}))


if __name__ == '__main__':
    main()
