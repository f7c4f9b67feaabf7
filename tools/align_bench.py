"""Time-aligned metrics over a validation list: alignment.compare_aligned_many (include/vqvae_align.h: features of either
side, then per chunk the cepstra of either side, the DP launch and the path launch) timed end to end and per launch
family, beside metrics.compare_many on the same list cut to common length (what alignment adds) and beside the NumPy
restatement on the host CPU.
usage: python tools/align_bench.py [--rounds 3] [--utterances 300] [--seed 0] [--chunk-bytes 1073741824] [--cpu-utterances 32]
                                   [--cpu-threads 16] [--out FILE]
       python tools/align_bench.py --parent DIR [--rounds 3] [--steps 30]
  Utterances: the list of DESIGN 7f, tools/gen_bench.gamma_lengths(300, seed 0): gamma(shape 2, mean 3.6 s) clipped to
  0.5 - 10 s at 16 kHz, host float32 waves of seeded noise; the test side has lengths of its own, the reference's times a
  factor drawn uniformly from 0.8 - 1.25 (the DP's cost does not depend on the data, only on Fa and Fb).  Default
  MelConfig (n_fft 1024, hop 256, 80 mels, 13 coefficients).
  (a) compare_aligned_many end to end on the host clock (uploads, the feature launches, the alignment launches, the copy
      of the scores back), then one more pass with device events around every alignment launch: device time per family.
  (b) compare_many on the same two lists (it cuts every pair to its common length), host clock.
  (c) the first --cpu-utterances pairs through tests/alignment_ref.py (dtw_diagonals, float64 NumPy) from the device's
      log-mel features, on --cpu-threads processes, scaled to the whole list by cells, and compared bit for bit.
  Ranges over the rounds, not means.  Prints one JSON line; --out also writes the table as text.
  --parent DIR (a built tree of the parent commit): tools/frontend_bench.py's interleaved bench.py rounds."""
import argparse
import ctypes as C
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-vq-vae_amd'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

FAMILIES = ('vqvae_align_cepstra', 'vqvae_align_dtw', 'vqvae_align_path')


def _restate(job):
    import alignment_ref as R
    la, lb, dct = job
    r = R.align(la, lb, dct)
    return r['cost'], r['path_len'], r['diagonal_steps'], r['mcd_dtw_db'], r['log_mel_mae_dtw']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default='', help='a built tree of the parent commit: interleave its bench.py with this tree\'s')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--utterances', type=int, default=300)
    ap.add_argument('--cpu-utterances', type=int, default=32)
    ap.add_argument('--cpu-threads', type=int, default=16)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--chunk-bytes', type=int, default=1 << 30)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.parent:
        from frontend_bench import against_parent
        return against_parent(a)
    from gen_bench import gamma_lengths
    from vqvae_amd import _lib, alignment, backend, metrics
    n_cpu = min(a.cpu_utterances, a.utterances)
    pool = multiprocessing.get_context('spawn').Pool(a.cpu_threads) if n_cpu else None      # fresh children, started before the device is
    backend.init(0)
    cfg = metrics.MelConfig()
    len_a = gamma_lengths(a.utterances, a.seed)
    rs = np.random.RandomState(a.seed + 3)
    len_b = np.maximum((len_a * rs.uniform(0.8, 1.25, a.utterances)).astype(np.int64), cfg.n_fft)
    ref = [(0.1 * rs.standard_normal(int(n))).astype(np.float32) for n in len_a]
    test = [(0.1 * rs.standard_normal(int(n))).astype(np.float32) for n in len_b]
    st = backend.stream()

    def elapsed(e0, e1):
        el = C.c_float(0)
        _lib.call('vqvae_event_elapsed_ms', C.byref(el), e0.h, e1.h)
        return float(el.value)

    def aligned():
        return alignment.compare_aligned_many(ref, test, cfg, chunk_bytes=a.chunk_bytes)

    def plain():
        return metrics.compare_many(ref, test, cfg, chunk_bytes=a.chunk_bytes)

    def host_clock(fn):
        fn()                                                         # warm-up: allocator pool, code objects
        backend.synchronize()
        walls = []
        for _ in range(a.rounds):
            backend.synchronize()
            t0 = time.perf_counter()
            out = fn()
            walls.append(time.perf_counter() - t0)
        return out, walls

    al, walls_a = host_clock(aligned)
    _, walls_b = host_clock(plain)
    fa, fb = al.frames_a, al.frames_b
    cells = int((fa * fb).sum())
    chunks = alignment.plan_chunks(fa, fb, a.chunk_bytes)

    call0 = _lib.call
    fam_rounds = {k: [] for k in FAMILIES}
    launches = {k: 0 for k in FAMILIES}
    for _ in range(a.rounds):
        marks = []

        def call(name, *args):
            if name in FAMILIES:
                e0 = backend.Event().record(st)
                call0(name, *args)
                marks.append((name, e0, backend.Event().record(st)))
            else:
                call0(name, *args)
        _lib.call = call
        try:
            aligned()
            backend.synchronize()
        finally:
            _lib.call = call0
        for k in FAMILIES:
            fam_rounds[k].append(sum(elapsed(e0, e1) for name, e0, e1 in marks if name == k))
            launches[k] = sum(1 for name, _, _ in marks if name == k)
    families = {k: {'launches': launches[k], 'ms': [round(min(v), 3), round(max(v), 3)]} for k, v in fam_rounds.items()}
    dtw_ms = fam_rounds['vqvae_align_dtw']

    # (c) the host CPU, float64, once, from the device's own features
    cpu = {}
    if n_cpu:
        feats_a, feats_b = metrics.features_many(ref[:n_cpu], cfg), metrics.features_many(test[:n_cpu], cfg)
        dct = metrics.tables(cfg)[2]
        jobs = [(feats_a.utterance(i)[0], feats_b.utterance(i)[0], dct) for i in range(n_cpu)]
        t0 = time.perf_counter()
        rows = pool.map(_restate, jobs, chunksize=1)
        cpu_s = time.perf_counter() - t0
        pool.close()
        pool.join()
        cpu_cells = int((fa[:n_cpu] * fb[:n_cpu]).sum())
        same = all(np.float64(r[0]).view(np.uint64) == al.cost[i].view(np.uint64) and r[1] == al.path_len[i] and r[2] == al.diagonal_steps[i] and
                   np.float64(r[3]).view(np.uint64) == al.mcd_dtw_db[i].view(np.uint64) and
                   np.float64(r[4]).view(np.uint64) == al.log_mel_mae_dtw[i].view(np.uint64) for i, r in enumerate(rows))
        cpu = {'numpy_float64_host_cpu_s': round(cpu_s, 2), 'numpy_pairs': n_cpu, 'numpy_cells': cpu_cells, 'cpu_processes': a.cpu_threads,
               'numpy_scaled_to_the_list_s': round(cpu_s * cells / max(cpu_cells, 1), 1), 'device_equals_numpy_every_bit': bool(same)}

    out = {'tool': 'align_bench', 'config': repr(cfg), 'utterances': a.utterances, 'seconds_of_audio': [float(len_a.sum()) / cfg.sr, float(len_b.sum()) / cfg.sr],
           'frames': [int(fa.sum()), int(fb.sum())], 'mean_frames': [float(fa.mean()), float(fb.mean())], 'max_frames': [int(fa.max()), int(fb.max())],
           'cells': cells, 'diagonals_longest_pair': int((fa + fb - 1).max()), 'chunk_bytes': a.chunk_bytes, 'chunks': len(chunks), 'rounds': a.rounds,
           'compare_aligned_many_host_s': [round(min(walls_a), 4), round(max(walls_a), 4)],
           'compare_many_common_length_host_s': [round(min(walls_b), 4), round(max(walls_b), 4)],
           'families': families, 'dtw_gcells_per_s': [round(1e-6 * cells / max(dtw_ms), 2), round(1e-6 * cells / min(dtw_ms), 2)],
           'mean_mcd_dtw_db': float(al.mcd_dtw_db.mean()), 'mean_path_len': float(al.path_len.mean())}
    out.update(cpu)
    print(json.dumps(out))
    if a.out:
        lines = ['tools/align_bench.py --rounds %d --utterances %d  (%s)' % (a.rounds, a.utterances, repr(cfg)),
                 '%d pairs, %.0f s against %.0f s of audio, %d against %d frames (mean %.0f and %.0f, longest %d and %d), %d cells, '
                 '%d chunk(s) of at most %d bytes' % (a.utterances, out['seconds_of_audio'][0], out['seconds_of_audio'][1], fa.sum(), fb.sum(),
                                                      fa.mean(), fb.mean(), fa.max(), fb.max(), cells, len(chunks), a.chunk_bytes), '',
                 '(a) compare_aligned_many end to end, host clock (uploads, features, alignment, scores back), %d rounds: %.4f - %.4f s'
                 % (a.rounds, min(walls_a), max(walls_a)),
                 '(b) compare_many on the same lists cut to common length, host clock, %d rounds:                     %.4f - %.4f s'
                 % (a.rounds, min(walls_b), max(walls_b)), '',
                 'launch family            launches   device ms (range)']
        for k, f in families.items():
            lines.append('%-24s %8d   %8.3f - %8.3f' % (k, f['launches'], f['ms'][0], f['ms'][1]))
        lines += ['vqvae_align_dtw: %.2f - %.2f G cells/s over %d cells; the longest pair has %d anti-diagonals'
                  % (out['dtw_gcells_per_s'][0], out['dtw_gcells_per_s'][1], cells, out['diagonals_longest_pair']), '']
        if cpu:
            lines += ['(c) tests/alignment_ref.py (dtw_diagonals), float64 NumPy on the host CPU, the first %d pairs (%d cells) on %d processes, once: '
                      '%.2f s; scaled by cells to the list: %.0f s' % (n_cpu, cpu['numpy_cells'], a.cpu_threads, cpu['numpy_float64_host_cpu_s'],
                                                                      cpu['numpy_scaled_to_the_list_s']),
                      'device against it on those pairs, cost, path length, diagonal steps, mcd_dtw_db, log_mel_mae_dtw bit-equal: %s'
                      % cpu['device_equals_numpy_every_bit'], '']
        lines += ['mean mcd_dtw_db %.4f, mean path length %.1f' % (out['mean_mcd_dtw_db'], out['mean_path_len']), '', json.dumps(out)]
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
