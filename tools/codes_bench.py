"""Code statistics over a validation list: codestats.compare_codes_many and codestats.code_stats (include/vqvae_codes.h) timed
end to end and per launch family, beside the NumPy restatement of the edit distance on the host CPU.
usage: python tools/codes_bench.py [--rounds 3] [--utterances 300] [--seed 0] [--speakers 100] [--cpu-pairs 32]
                                   [--cpu-threads 16] [--step-timeout 300] [--out FILE]
       python tools/codes_bench.py --parent DIR [--rounds 3] [--steps 30]
  Utterances: the list of DESIGN 7f, tools/gen_bench.gamma_lengths(300, seed 0) (gamma(shape 2, mean 3.6 s) clipped to
  0.5 - 10 s at 16 kHz) at 64 samples per code; side b has lengths of its own, side a's times a factor drawn uniformly
  from 0.8 - 1.25.  Random codes, k = 128, in runs of geometric length (mean 3); host LatentCodes, uploaded once before
  the clock starts (codes are a product that lives on the device).
  Every GPU step is a fresh process of this file (--step NAME) under --step-timeout; a step that fails ends the run.
  (a) step compare: compare_codes_many end to end on the host clock (tables up, agreement, both collapses, the edit
      launch, results back), collapse=True and collapse=False.
  (b) step families: one more pass of each with device events around every launch: device time per family.
  (c) step stats: code_stats with --speakers speakers and bigrams, end to end on the host clock, and with 10 permutations.
  (d) the first --cpu-pairs raw pairs through tests/codestats_ref.py (edit_diagonals, vectorised along the anti-diagonals)
      on --cpu-threads processes, scaled to the whole list by cells, and compared with the device's distances.
  Ranges over the rounds, not means.  Prints one JSON line; --out also writes the table as text.
  --parent DIR (a built tree of the parent commit): tools/frontend_bench.py's interleaved bench.py rounds."""
import argparse
import ctypes as C
import json
import multiprocessing
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-vq-vae_amd'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

K = 128
FAMILIES = ('vqvae_codes_runs', 'vqvae_codes_hist', 'vqvae_codes_agree', 'vqvae_codes_edit')
STEPS = ('compare', 'families', 'stats')


def make_lists(a):
    """(utterances of side a, of side b, speakers): host int32 arrays."""
    from gen_bench import gamma_lengths
    len_a = np.maximum(gamma_lengths(a.utterances, a.seed) // 64, 1)
    rs = np.random.RandomState(a.seed + 5)
    len_b = np.maximum((len_a * rs.uniform(0.8, 1.25, a.utterances)).astype(np.int64), 1)

    def string(n):
        runs = rs.geometric(1.0 / 3.0, int(n))
        return np.repeat(rs.randint(0, K, int(n)), runs)[:int(n)].astype(np.int32)
    return [string(n) for n in len_a], [string(n) for n in len_b], rs.randint(0, a.speakers, a.utterances).astype(np.int32)


def _restate(job):
    import codestats_ref as R
    return R.edit_diagonals(*job)


def step(a):
    """One GPU step in this process; prints its JSON line."""
    from vqvae_amd import _lib, backend, codestats
    from vqvae_amd.frontend import LatentCodes
    backend.init(0)
    ua, ub, speakers = make_lists(a)
    ca = LatentCodes(np.array([len(u) for u in ua], np.int32), np.concatenate(ua), K)
    cb = LatentCodes(np.array([len(u) for u in ub], np.int32), np.concatenate(ub), K)
    ca.indices, cb.indices                                           # uploaded before any clock starts
    st = backend.stream()

    def host_clock(fn):
        fn()                                                         # warm-up: allocator pool, code objects
        backend.synchronize()
        walls = []
        for _ in range(a.rounds):
            backend.synchronize()
            t0 = time.perf_counter()
            out = fn()
            walls.append(time.perf_counter() - t0)
        return out, [round(min(walls), 5), round(max(walls), 5)]

    out = {'step': a.step}
    if a.step == 'compare':
        col, out['compare_collapsed_host_s'] = host_clock(lambda: codestats.compare_codes_many(ca, cb, collapse=True))
        raw, out['compare_raw_host_s'] = host_clock(lambda: codestats.compare_codes_many(ca, cb, collapse=False))
        out.update(cells_raw=int((raw.len_a * raw.len_b).sum()), cells_collapsed=int((col.len_a * col.len_b).sum()),
                   longest_raw=[int(raw.len_a.max()), int(raw.len_b.max())], diagonals_longest_raw=int((raw.len_a + raw.len_b - 1).max()),
                   mean_len_raw=[float(raw.len_a.mean()), float(raw.len_b.mean())], mean_len_collapsed=[float(col.len_a.mean()), float(col.len_b.mean())],
                   mean_error_rate=[float(raw.error_rate.mean()), float(col.error_rate.mean())],
                   first_raw=[[int(d), int(s)] for d, s in zip(raw.distance[:a.cpu_pairs], raw.subs[:a.cpu_pairs])])
    elif a.step == 'families':
        def elapsed(e0, e1):
            el = C.c_float(0)
            _lib.call('vqvae_event_elapsed_ms', C.byref(el), e0.h, e1.h)
            return float(el.value)
        call0 = _lib.call
        for name, fn in (('collapsed', lambda: codestats.compare_codes_many(ca, cb, collapse=True)),
                         ('raw', lambda: codestats.compare_codes_many(ca, cb, collapse=False)),
                         ('code_stats', lambda: codestats.code_stats(ca, speakers, a.speakers))):
            fn()
            rounds = {k: [] for k in FAMILIES}
            launches = {k: 0 for k in FAMILIES}
            for _ in range(a.rounds):
                marks = []

                def call(entry, *args):
                    if entry in FAMILIES:
                        e0 = backend.Event().record(st)
                        call0(entry, *args)
                        marks.append((entry, e0, backend.Event().record(st)))
                    else:
                        call0(entry, *args)
                _lib.call = call
                try:
                    fn()
                    backend.synchronize()
                finally:
                    _lib.call = call0
                for k in FAMILIES:
                    rounds[k].append(sum(elapsed(e0, e1) for entry, e0, e1 in marks if entry == k))
                    launches[k] = sum(1 for entry, _, _ in marks if entry == k)
            out[name] = {k: {'launches': launches[k], 'ms': [round(min(v), 4), round(max(v), 4)]} for k, v in rounds.items() if launches[k]}
    elif a.step == 'stats':
        s, out['code_stats_host_s'] = host_clock(lambda: codestats.code_stats(ca, speakers, a.speakers))
        _, out['code_stats_10_permutations_host_s'] = host_clock(lambda: codestats.code_stats(ca, speakers, a.speakers, permutations=10))
        out.update(positions=s.positions, transitions=s.transitions, runs=s.runs, mean_run=s.mean_run, mi_bits=s.mi_bits,
                   perplexity=s.perplexity)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default='', help='a built tree of the parent commit: interleave its bench.py with this tree\'s')
    ap.add_argument('--step', default='', choices=('',) + STEPS, help='(internal) run this GPU step in this process')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--utterances', type=int, default=300)
    ap.add_argument('--speakers', type=int, default=100)
    ap.add_argument('--cpu-pairs', type=int, default=32)
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
    out = {'tool': 'codes_bench', 'utterances': a.utterances, 'k': K, 'speakers': a.speakers, 'rounds': a.rounds}
    passed = [x for x in sys.argv[1:]]
    for name in STEPS:                                               # a fresh process per GPU step, each under its own limit
        cmd = [sys.executable, os.path.abspath(__file__)] + passed + ['--step', name]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=a.step_timeout)
        if r.returncode != 0:
            raise SystemExit('codes_bench: step %s failed (%d): %s' % (name, r.returncode, r.stderr.decode()[-2000:]))
        got = json.loads(r.stdout.decode().strip().splitlines()[-1])
        got.pop('step')
        out[name] = got
    n_cpu = min(a.cpu_pairs, a.utterances)
    if n_cpu:
        ua, ub, _ = make_lists(a)
        pool = multiprocessing.get_context('spawn').Pool(a.cpu_threads)
        t0 = time.perf_counter()
        rows = pool.map(_restate, list(zip(ua[:n_cpu], ub[:n_cpu])), chunksize=1)
        cpu_s = time.perf_counter() - t0
        pool.close()
        pool.join()
        cells = sum(len(x) * len(y) for x, y in zip(ua[:n_cpu], ub[:n_cpu]))
        first = out['compare'].pop('first_raw')
        out['cpu'] = {'numpy_host_cpu_s': round(cpu_s, 2), 'numpy_pairs': n_cpu, 'numpy_cells': cells, 'cpu_processes': a.cpu_threads,
                      'numpy_scaled_to_the_list_s': round(cpu_s * out['compare']['cells_raw'] / max(cells, 1), 1),
                      'device_equals_numpy': bool([list(r) for r in rows] == first[:n_cpu])}
    print(json.dumps(out))
    if a.out:
        c, s = out['compare'], out['stats']
        lines = ['tools/codes_bench.py --rounds %d --utterances %d --speakers %d  (k = %d, geometric runs of mean 3)' % (a.rounds, a.utterances, a.speakers, K),
                 '%d pairs; raw: mean %.0f and %.0f codes, longest %d and %d, %d cells, %d anti-diagonals in the longest pair; collapsed: mean %.0f and %.0f, %d cells'
                 % (a.utterances, c['mean_len_raw'][0], c['mean_len_raw'][1], c['longest_raw'][0], c['longest_raw'][1], c['cells_raw'],
                    c['diagonals_longest_raw'], c['mean_len_collapsed'][0], c['mean_len_collapsed'][1], c['cells_collapsed']), '',
                 '(a) compare_codes_many end to end, host clock, %d rounds: collapse=True %.5f - %.5f s, collapse=False %.5f - %.5f s'
                 % (a.rounds, c['compare_collapsed_host_s'][0], c['compare_collapsed_host_s'][1], c['compare_raw_host_s'][0], c['compare_raw_host_s'][1]), '',
                 '(b) call         launch family          launches   device ms (range)']
        for name, fams in out['families'].items():
            for k, f in fams.items():
                lines.append('    %-12s %-22s %8d   %8.4f - %8.4f' % (name, k, f['launches'], f['ms'][0], f['ms'][1]))
        lines += ['', '(c) code_stats, %d speakers, bigrams, host clock: %.5f - %.5f s; with 10 permutations %.5f - %.5f s  (%d positions, %d runs)'
                  % (a.speakers, s['code_stats_host_s'][0], s['code_stats_host_s'][1], s['code_stats_10_permutations_host_s'][0],
                     s['code_stats_10_permutations_host_s'][1], s['positions'], s['runs']), '']
        if 'cpu' in out:
            u = out['cpu']
            lines += ['(d) tests/codestats_ref.py (edit_diagonals), NumPy on the host CPU, the first %d raw pairs (%d cells) on %d processes, once: %.2f s; '
                      'scaled by cells to the list: %.1f s; the device\'s distance and substitutions equal it on those pairs: %s'
                      % (u['numpy_pairs'], u['numpy_cells'], u['cpu_processes'], u['numpy_host_cpu_s'], u['numpy_scaled_to_the_list_s'],
                         u['device_equals_numpy']), '']
        lines.append(json.dumps(out))
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
