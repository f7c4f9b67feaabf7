"""Held-out likelihood of a corpus: scoring.score_many (the ragged decoder pass of csrc/ragged_decoder.hip) beside the
per-utterance loop over the EXISTING forward -- decoder(x_dec, cond) on the dense condition plus softmax cross-entropy under
no_backprop_mode, one utterance after the other.  The loop over existing code is the yardstick.
usage: python tools/score_bench.py [--rounds 3] [--utterances 300] [--seed 0] [--chunk-bytes 1073741824] [--matmul float32x2]
                                   [--step-timeout 600] [--pool-limit 103079215104]
       python tools/score_bench.py --parent DIR [--rounds 3] [--steps 30]
  Model: the default decoder (3 x 10 blocks, 512 residual / 512 dilated / 256 skip channels, 256 classes, condition
  512 + 128), seeded weights.  Utterances: tools/gen_bench.gamma_lengths(300, seed 0) (gamma(shape 2, mean 3.6 s) clipped to
  0.5 - 10 s at 16 kHz), each cut to 64 tl + 1 samples so that both sides score the same 64 tl positions; the classes are
  binned once and live on the device for both sides; the latent condition is seeded noise.
  The parent process runs the rounds interleaved, alternating who goes first, every GPU step a fresh child process under its
  own timeout: `--step loop`, `--step ragged` (one warm-up pass, one timed pass: host time, device span between two events,
  samples / s), then `--step kernels` (device time between events around every launch of one ragged pass, and the bytes each
  launch must move: its inputs read once, its outputs written once).  Ranges over the rounds are printed, not means.
  Prints one JSON line.
  --parent DIR (a built tree of the parent commit): per round, as fresh child processes alternating who goes first, DIR's
  `bench.py` and this tree's; prints the rounds of ms_per_step and whether the ranges overlap."""
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

DIMS = dict(n_loop=3, n_layer=10, Q=256, R=512, D=512, S=256, Cl=512, G=128)


def last_json(text):
    return json.loads([l for l in text.split('\n') if l.startswith('{')][-1])


def against_parent(a):
    args = ['--gpus', '1', '--steps', str(a.steps), '--warmup', '5']
    rows = {'parent': [], 'this': []}
    for rnd in range(a.rounds):
        order = (('parent', os.path.abspath(a.parent)), ('this', ROOT))
        for who, root in (order if rnd % 2 == 0 else order[::-1]):
            cmd = [sys.executable, os.path.join(root, 'bench.py')] + args
            sys.stderr.write('score_bench: %s (in %s)\n' % (' '.join(cmd), root))
            sys.stderr.flush()
            r = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=a.step_timeout)
            if r.returncode != 0:
                raise SystemExit('score_bench: %s failed (%d): %s' % (cmd, r.returncode, r.stderr.decode()[-2000:]))
            rows[who].append(last_json(r.stdout.decode())['ms_per_step'])
    pa, tb = rows['parent'], rows['this']
    print(json.dumps({'tool': 'score_bench --parent', 'ms_per_step': rows, 'parent_range': [min(pa), max(pa)],
                      'this_range': [min(tb), max(tb)], 'ranges_overlap': bool(min(tb) <= max(pa) and min(pa) <= max(tb))}))


def build(a):
    """(wavenet on the device, LatentCondition, device classes per utterance, positions per utterance)."""
    import vqvae_amd as V
    from gen_bench import gamma_lengths
    from resident_corpus_bench import synthetic_waves
    from vqvae_amd import backend
    from vqvae_amd.inputs import DeviceInputPipeline
    from vqvae_amd.wavenet import WaveNet
    m = DIMS
    wn = WaveNet(m['n_loop'], m['n_layer'], 2, m['Q'], m['R'], m['D'], m['S'], m['Q'], False, 30, -40, m['Cl'] + m['G'], 0)
    rs = np.random.RandomState(a.seed + 3)
    for name, p in sorted(wn.namedparams()):
        sh = p.data.shape
        fan = int(np.prod(sh[1:])) if len(sh) > 1 else 1
        p.data = ((rs.standard_normal(sh) / np.sqrt(fan)) if len(sh) > 1 else 0.1 * rs.standard_normal(sh)).astype(np.float32)
    wn.to_gpu()
    lengths = gamma_lengths(a.utterances, a.seed)
    tl = np.maximum((np.asarray(lengths, np.int64) - 1) // 64, 1)
    lengths = 64 * tl + 1
    pipe = DeviceInputPipeline(m['Q'])
    classes = []
    for w in synthetic_waves(lengths, a.seed + 2):
        classes.append(pipe.bins((w / np.abs(w).max()).astype(np.float32)))
    local = [backend.to_device(np.maximum(rs.standard_normal((m['Cl'], int(t))), 0).astype(np.float32)) for t in tl]
    gv = backend.to_device(rs.standard_normal((a.utterances, m['G'])).astype(np.float32))
    cond = V.LatentCondition.from_latents(local, gv, 64)
    return wn, cond, classes, 64 * tl


def step(a):
    import vqvae_amd as V
    from vqvae_amd import _lib, backend, core, functions as F, scoring
    from vqvae_amd.core import Variable
    from vqvae_amd.inputs import IndexInput
    backend.init(0)
    if a.matmul:
        backend.set_matmul_dtype(a.matmul)
    wn, cond, classes, n_pos = build(a)
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
            for i, (q, n) in enumerate(zip(classes, n_pos)):
                n = int(n)
                ci = V.LatentCondition.from_latents([cond.local.flat_view(int(cond.local_off[i]), m['Cl'] * int(cond.tl[i]), (m['Cl'], int(cond.tl[i])))],
                                                    cond.global_vec.flat_view(i * m['G'], m['G'], (1, m['G'])), 64)
                dense = ci.dense()
                x = IndexInput((1, n), m['Q'])
                _lib.call('vqvae_memcpy_d2d', x.ptr, q.ptr, 4 * n, st)
                t = backend.DeviceArray((1, n, 1), np.int32)
                _lib.call('vqvae_memcpy_d2d', t.ptr, q.ptr + 4, 4 * n, st)
                y = wn(x, Variable(dense.reshape(1, m['Cl'] + m['G'], n, 1)))
                losses.append(F.softmax_cross_entropy(y, t).data)
                del y, dense, x, t, ci
                # the existing forward keeps every block's gates and z (25 GB for a 10 s utterance) and the allocator pool
                # keeps a block of every size it has seen: with 300 different lengths the pool is handed back when it passes
                # --pool-limit, or the loop runs out of memory
                if backend.memory_stats()['cached_bytes'] > a.pool_limit:
                    backend.synchronize()
                    backend.free_all_blocks()
                    flushes[0] += 1
        return losses

    def ragged():
        return V.score_many(wn, cond, classes, chunk_bytes=a.chunk_bytes)

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
    if a.step in ('loop', 'ragged'):
        fn = loop if a.step == 'loop' else ragged
        timed(fn)                                            # warm-up: allocator pool, LDS opt-ins, weight packs
        flushes[0] = 0
        out, t = timed(fn)
        t['pool_flushes'] = flushes[0]
        bits = (np.array([float(l.get()) for l in out]) / np.log(2.0)) if a.step == 'loop' else out.bits_per_sample
        t.update(step=a.step, samples=total, samples_per_s=total / t['device_span_s'], bits_per_sample=[float(b) for b in bits])
        print(json.dumps(t))
        return
    # --step kernels: device events around every launch of one ragged pass
    ragged()
    marks, call0, mine = [], _lib.call, _lib.HEADERS['vqvae_ragged_decoder.h'].prototypes

    def call(name, *args):
        if name in mine:
            e0 = backend.Event().record(st)
            call0(name, *args)
            marks.append((name, args[0]._obj, e0, backend.Event().record(st)))
        else:
            call0(name, *args)
    _lib.call = call
    try:
        ragged()
        backend.synchronize()
    finally:
        _lib.call = call0
    nb = m['n_loop'] * m['n_layer']
    Ch, M, Cc = m['D'] // 2, nb * m['D'], m['Cl'] + m['G']

    def must_move(name, d):          # bytes: the launch's inputs read once, its outputs written once
        T, TL = d.ttot, d.tltot
        return {'vqvae_rdec_embed': 4 * T + 8 * m['R'] * m['Q'] + 4 * m['R'] * T,
                'vqvae_rdec_cond_project': 4 * (m['Cl'] * TL + M * Cc + M * TL),
                'vqvae_rdec_cond_global': 4 * (d.n * m['G'] + M * Cc + d.n * M),
                'vqvae_rdec_gate': 4 * (m['R'] * T + 2 * m['D'] * m['R'] + m['D'] * TL + d.n * m['D'] + Ch * T),
                'vqvae_rdec_res_skip': 4 * (Ch * T + (m['R'] + m['S']) * Ch + 2 * m['R'] * T + 2 * m['S'] * T),
                'vqvae_rdec_head': 4 * (3 * m['S'] * T + m['S'] * m['S'] + m['Q'] * m['S'] + 3 * T),
                'vqvae_rdec_reduce': 8 * T + 16 * d.n}[name]
    flop = {'vqvae_rdec_cond_project': lambda d: 2.0 * M * m['Cl'] * d.tltot, 'vqvae_rdec_gate': lambda d: 2.0 * m['D'] * 2 * m['R'] * d.ttot,
            'vqvae_rdec_res_skip': lambda d: 2.0 * (m['R'] + m['S']) * Ch * d.ttot,
            'vqvae_rdec_head': lambda d: 2.0 * (m['S'] + m['Q']) * m['S'] * d.ttot}
    table = {}
    for name, d, e0, e1 in marks:
        row = table.setdefault(name, {'launches': 0, 'ms': 0.0, 'gbytes_must_move': 0.0, 'gflop': 0.0})
        row['launches'] += 1
        row['ms'] += elapsed(e0, e1)
        row['gbytes_must_move'] += 1e-9 * must_move(name, d)
        row['gflop'] += 1e-9 * flop.get(name, lambda d: 0.0)(d)
    for row in table.values():
        row['gbytes_per_s'] = round(row['gbytes_must_move'] / (1e-3 * row['ms']), 1)
        row['tflops'] = round(row['gflop'] / row['ms'], 2) if row['gflop'] else None
        row['ms'], row['gbytes_must_move'], row['gflop'] = round(row['ms'], 3), round(row['gbytes_must_move'], 3), round(row['gflop'], 1)
    print(json.dumps({'step': 'kernels', 'samples': total, 'kernels': table}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default='', help="a built tree of the parent commit: interleave its bench.py with this tree's")
    ap.add_argument('--step', default='', choices=['', 'loop', 'ragged', 'kernels'], help='(a child process of this tool)')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--utterances', type=int, default=300)
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
              '--pool-limit', str(a.pool_limit)] + \
        (['--matmul', a.matmul] if a.matmul else [])

    def child(which):
        cmd = [sys.executable, os.path.abspath(__file__), '--step', which] + common
        sys.stderr.write('score_bench: %s\n' % ' '.join(cmd))
        sys.stderr.flush()
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=a.step_timeout)
        if r.returncode != 0:                                # a failed GPU step ends the run: nothing more is started
            raise SystemExit('score_bench: step %s failed (%d): %s' % (which, r.returncode, r.stderr.decode()[-2000:]))
        return last_json(r.stdout.decode())
    rows = {'loop': [], 'ragged': []}
    for rnd in range(a.rounds):
        for which in (('loop', 'ragged') if rnd % 2 == 0 else ('ragged', 'loop')):
            rows[which].append(child(which))
    kernels = child('kernels')
    lb, rb = np.array(rows['loop'][0].pop('bits_per_sample')), np.array(rows['ragged'][0].pop('bits_per_sample'))
    for r in rows['loop'][1:] + rows['ragged'][1:]:
        r.pop('bits_per_sample')

    def rng(name, key):
        v = [r[key] for r in rows[name]]
        return [round(min(v), 4), round(max(v), 4)]
    keys = ('host_s', 'device_span_s', 'wall_s', 'samples_per_s')
    print(json.dumps({'tool': 'score_bench', 'model': 'decoder 3 x 10 blocks, 512 / 512 / 256 channels, 256 classes, condition 512 + 128',
                      'matmul': a.matmul or 'process default', 'utterances': a.utterances, 'samples': kernels['samples'],
                      'chunk_bytes': a.chunk_bytes, 'rounds': a.rounds,
                      'loop': dict((k, rng('loop', k)) for k in keys), 'ragged': dict((k, rng('ragged', k)) for k in keys),
                      'max_abs_difference_bits_per_sample': float(np.abs(lb - rb).max()),
                      'corpus_bits_per_sample': {'loop': float(lb.mean()), 'ragged': float(rb.mean())},
                      'all_rounds': rows, 'ragged_kernels': kernels['kernels']}))


if __name__ == '__main__':
    main()
