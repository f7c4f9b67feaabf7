"""The audio metrics over a validation list: metrics.compare_many (include/vqvae_metrics.h: the ragged STFT / log-mel launch
and the distance launch, per chunk) timed per launch family, end to end, and beside the NumPy restatement on the host CPU.
usage: python tools/metrics_bench.py [--rounds 3] [--utterances 300] [--seed 0] [--chunk-bytes 1073741824] [--cpu-utterances 300]
                                     [--out FILE]
       python tools/metrics_bench.py --parent DIR [--rounds 3] [--steps 30]
  Utterances: the list of DESIGN 7f, tools/gen_bench.gamma_lengths(300, seed 0): gamma(shape 2, mean 3.6 s) clipped to
  0.5 - 10 s at 16 kHz, host float32 waves, peak-normalised; the test side is the reference without its last sample (what
  synthesize_many returns) plus noise at 0.05.  Default MelConfig (n_fft 1024, hop 256, 80 mels, 13 cepstral coefficients).
  Per round: compare_many end to end on the host clock (uploads, launches, the copy of the scores back), then one more pass
  with device events around every launch: device time per launch family, and the bytes each family must move (inputs read
  once, outputs written once) against 6.3 TB/s.  Ranges over the rounds are printed, not means.
  Once: the same list (the first --cpu-utterances of it) through tests/metrics_ref.py in float64 on the host CPU, for scale.
  Prints one JSON line; --out also writes the table as text.
  --parent DIR (a built tree of the parent commit): tools/frontend_bench.py's interleaved bench.py rounds."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-vq-vae_amd'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HBM = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default='', help='a built tree of the parent commit: interleave its bench.py with this tree\'s')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--utterances', type=int, default=300)
    ap.add_argument('--cpu-utterances', type=int, default=300)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--chunk-bytes', type=int, default=1 << 30)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.parent:
        from frontend_bench import against_parent
        return against_parent(a)
    import metrics_ref as R
    from gen_bench import gamma_lengths
    from resident_corpus_bench import synthetic_waves
    from vqvae_amd import _lib, backend, metrics
    backend.init(0)
    cfg = metrics.MelConfig()
    lengths = gamma_lengths(a.utterances, a.seed)
    ref = [(w / np.abs(w).max()).astype(np.float32) for w in synthetic_waves(lengths, a.seed + 2)]
    rs = np.random.RandomState(a.seed + 5)
    test = [(w[:-1] + np.float32(0.05) * rs.standard_normal(len(w) - 1).astype(np.float32)).astype(np.float32) for w in ref]
    st = backend.stream()

    def elapsed(e0, e1):
        el = C.c_float(0)
        _lib.call('vqvae_event_elapsed_ms', C.byref(el), e0.h, e1.h)
        return float(el.value)

    def compare():
        return metrics.compare_many(ref, test, cfg, chunk_bytes=a.chunk_bytes)

    compare()                                                    # warm-up: allocator pool, the LDS opt-in, the table cache
    backend.synchronize()
    walls = []
    for _ in range(a.rounds):
        backend.synchronize()
        t0 = time.perf_counter()
        scores = compare()
        walls.append(time.perf_counter() - t0)

    frames = scores['frames']
    common = np.array([min(len(x), len(y)) for x, y in zip(ref, test)], np.int64)
    chunks = metrics.plan_chunks(frames, 2 * (cfg.nb + cfg.n_mels), a.chunk_bytes)
    ftot, nb, nm = int(frames.sum()), cfg.nb, cfg.n_mels
    covered = int((cfg.n_fft + (frames - 1) * cfg.hop).sum())
    table_bytes = 4 * (2 * nb * cfg.n_fft + nm * nb)
    must = {'vqvae_metrics_stft_mel': 2 * (4 * covered + 4 * (nb + nm) * ftot) + 2 * len(chunks) * table_bytes,
            'vqvae_metrics_distances': 2 * 4 * (nb + nm) * ftot + 24 * len(frames)}
    flop = {'vqvae_metrics_stft_mel': 2 * ftot * (2.0 * 2 * nb * cfg.n_fft + 2.0 * nm * nb), 'vqvae_metrics_distances': 0.0}

    call0 = _lib.call
    fam_rounds = {k: [] for k in must}
    launches = {k: 0 for k in must}
    for _ in range(a.rounds):
        marks = []

        def call(name, *args):
            if name in must:
                e0 = backend.Event().record(st)
                call0(name, *args)
                marks.append((name, e0, backend.Event().record(st)))
            else:
                call0(name, *args)
        _lib.call = call
        try:
            compare()
            backend.synchronize()
        finally:
            _lib.call = call0
        for k in must:
            fam_rounds[k].append(sum(elapsed(e0, e1) for name, e0, e1 in marks if name == k))
            launches[k] = sum(1 for name, _, _ in marks if name == k)

    families = {}
    for k in must:
        lo, hi = min(fam_rounds[k]), max(fam_rounds[k])
        families[k] = {'launches': launches[k], 'ms': [round(lo, 3), round(hi, 3)], 'must_move_mb': round(must[k] / 1e6, 1),
                       'ms_at_6.3_TB_s': round(1e3 * must[k] / HBM, 3), 'gflop': round(1e-9 * flop[k], 1),
                       'tflops': [round(1e-9 * flop[k] / hi, 2), round(1e-9 * flop[k] / lo, 2)] if flop[k] else None}

    # the host CPU, float64, once: features of both sides and the three formulas
    tabs = metrics.tables(cfg)
    n_cpu = min(a.cpu_utterances, len(ref))
    t0 = time.perf_counter()
    cpu = np.zeros((n_cpu, 3))
    for i in range(n_cpu):
        L = int(common[i])
        ma, _, la, _ = R.features(ref[i][:L], tabs, cfg.n_fft, cfg.hop, cfg.floor)
        mb, _, lb, _ = R.features(test[i][:L], tabs, cfg.n_fft, cfg.hop, cfg.floor)
        cpu[i] = R.distances(la, lb, ma, mb, tabs[2])
    cpu_s = time.perf_counter() - t0
    dev = np.stack([scores['log_mel_mae'], scores['mcd_db'], scores['spectral_convergence']], axis=1)[:n_cpu]
    rel = (np.abs(dev - cpu) / np.abs(cpu)).max(axis=0)

    out = {'tool': 'metrics_bench', 'config': repr(cfg), 'utterances': a.utterances, 'samples': int(lengths.sum()),
           'seconds_of_audio': float(lengths.sum()) / 16000.0, 'frames': ftot, 'chunk_bytes': a.chunk_bytes, 'chunks': len(chunks),
           'rounds': a.rounds, 'compare_many_host_s': [round(min(walls), 4), round(max(walls), 4)], 'all_rounds_host_s': walls,
           'families': families, 'numpy_float64_host_cpu_s': round(cpu_s, 2), 'numpy_utterances': n_cpu,
           'cpu_threads': os.environ.get('OMP_NUM_THREADS', ''),
           'device_against_numpy_max_relative': {'log_mel_mae': float(rel[0]), 'mcd_db': float(rel[1]), 'spectral_convergence': float(rel[2])},
           'score_means': {'log_mel_mae': float(dev[:, 0].mean()), 'mcd_db': float(dev[:, 1].mean()),
                           'spectral_convergence': float(dev[:, 2].mean())}}
    print(json.dumps(out))
    if a.out:
        lines = ['tools/metrics_bench.py --rounds %d --utterances %d  (%s)' % (a.rounds, a.utterances, repr(cfg)),
                 '%d utterances, %d samples (%.0f s of audio), %d frames per side, %d chunk(s) of at most %d bytes'
                 % (a.utterances, lengths.sum(), lengths.sum() / 16000.0, ftot, len(chunks), a.chunk_bytes), '',
                 'compare_many end to end, host clock (uploads, launches, scores back), %d rounds: %.4f - %.4f s'
                 % (a.rounds, min(walls), max(walls)), '',
                 'launch family                launches   device ms (range)     must move   at 6.3 TB/s   GFLOP    TFLOP/s']
        for k, f in families.items():
            lines.append('%-28s %8d   %8.3f - %8.3f   %7.1f MB   %8.3f ms  %7.1f   %s'
                         % (k, f['launches'], f['ms'][0], f['ms'][1], f['must_move_mb'], f['ms_at_6.3_TB_s'], f['gflop'],
                            '-' if not f['tflops'] else '%.2f - %.2f' % tuple(f['tflops'])))
        lines += ['', 'tests/metrics_ref.py, float64 NumPy on the host CPU, %d utterances, once: %.2f s (OMP_NUM_THREADS=%s)'
                  % (n_cpu, cpu_s, out['cpu_threads']),
                  'device scores against it, max relative difference: log_mel_mae %.3g, mcd_db %.3g, spectral_convergence %.3g'
                  % tuple(rel), 'mean scores: log_mel_mae %.4f, mcd_db %.4f dB, spectral_convergence %.4f' % tuple(dev.mean(axis=0)), '',
                  json.dumps(out)]
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
