"""The pitch statistics over a validation list: pitch.compare_pitch_many (include/vqvae_pitch.h: the ragged YIN launch of
either side and the pair launch, per chunk) timed per launch family, end to end, and beside the NumPy restatement on the
host CPU.
usage: python tools/pitch_bench.py [--rounds 3] [--utterances 300] [--seed 0] [--chunk-bytes 1073741824] [--cpu-utterances 8]
                                   [--out FILE]
       python tools/pitch_bench.py --parent DIR [--rounds 3] [--steps 30]
  Utterances: the list of DESIGN 7f, tools/gen_bench.gamma_lengths(300, seed 0): gamma(shape 2, mean 3.6 s) clipped to
  0.5 - 10 s at 16 kHz, host float32 waves: a three-harmonic tone of a random F0 in 80 - 300 Hz over noise of 0.01, silent
  for its first fifth; the test side is the same a semitone up, without its last sample (what synthesize_many returns).
  Default PitchConfig (frame 1024, hop 256, 60 - 400 Hz: 267 lags of 757 terms).
  Per round: compare_pitch_many end to end on the host clock (uploads, launches, the copy of the scores back), then one
  more pass with device events around every launch: device time per launch family and, for the tracker, the float64
  operations of the difference function, 3 W (tau_max + 1) per frame, per second.  Ranges over the rounds, not means.
  Once: the first --cpu-utterances pairs through tests/pitch_ref.py in float64 on the host CPU, scaled to the whole list
  by frames, and compared with the device bit for bit.
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

SEMITONE = 2.0 ** (1.0 / 12.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default='', help='a built tree of the parent commit: interleave its bench.py with this tree\'s')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--utterances', type=int, default=300)
    ap.add_argument('--cpu-utterances', type=int, default=8)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--chunk-bytes', type=int, default=1 << 30)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.parent:
        from frontend_bench import against_parent
        return against_parent(a)
    import pitch_ref as R
    from gen_bench import gamma_lengths
    from vqvae_amd import _lib, backend, pitch
    backend.init(0)
    cfg = pitch.PitchConfig()
    conf = (cfg.sr, cfg.frame, cfg.hop, cfg.fmin, cfg.fmax)
    lengths = gamma_lengths(a.utterances, a.seed)
    rs = np.random.RandomState(a.seed + 2)
    ref, test = [], []
    for n in lengths:
        f = rs.uniform(80.0, 300.0)
        for side, shift in ((ref, 1.0), (test, SEMITONE)):
            w = R.tone(f * shift, int(n), cfg.sr, rs, noise=0.01)
            w[:int(n) // 5] = 0
            side.append(w)
    test = [w[:-1] for w in test]
    st = backend.stream()

    def elapsed(e0, e1):
        el = C.c_float(0)
        _lib.call('vqvae_event_elapsed_ms', C.byref(el), e0.h, e1.h)
        return float(el.value)

    def compare():
        return pitch.compare_pitch_many(ref, test, cfg, chunk_bytes=a.chunk_bytes)

    compare()                                                    # warm-up: allocator pool, code objects
    backend.synchronize()
    walls = []
    for _ in range(a.rounds):
        backend.synchronize()
        t0 = time.perf_counter()
        scores = compare()
        walls.append(time.perf_counter() - t0)

    frames = scores['frames']
    ftot = int(frames.sum())
    chunks = pitch.plan_chunks(frames, cfg, a.chunk_bytes, sides=2)
    flop = {'vqvae_pitch_yin': 2 * ftot * 3.0 * cfg.W * (cfg.tau_max + 1), 'vqvae_pitch_compare': 0.0}

    call0 = _lib.call
    fam_rounds = {k: [] for k in flop}
    launches = {k: 0 for k in flop}
    for _ in range(a.rounds):
        marks = []

        def call(name, *args):
            if name in flop:
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
        for k in flop:
            fam_rounds[k].append(sum(elapsed(e0, e1) for name, e0, e1 in marks if name == k))
            launches[k] = sum(1 for name, _, _ in marks if name == k)

    families = {}
    for k in flop:
        lo, hi = min(fam_rounds[k]), max(fam_rounds[k])
        families[k] = {'launches': launches[k], 'ms': [round(lo, 3), round(hi, 3)], 'gflop_float64': round(1e-9 * flop[k], 1),
                       'tflops_float64': [round(1e-9 * flop[k] / hi, 2), round(1e-9 * flop[k] / lo, 2)] if flop[k] else None}

    # the host CPU, float64, once: both tracks and the eight statistics of the first pairs, in the kernels' own order
    n_cpu = min(a.cpu_utterances, len(ref))
    rows = np.stack([scores[k] for k in R.COLUMNS], axis=1)
    t0 = time.perf_counter()
    cpu = np.zeros((n_cpu, len(R.COLUMNS)))
    for i in range(n_cpu):
        L = min(len(ref[i]), len(test[i]))
        cpu[i] = R.pair_stats(R.track(ref[i][:L], *conf)[0], R.track(test[i][:L], *conf)[0])
    cpu_s = time.perf_counter() - t0
    cpu_frames = int(frames[:n_cpu].sum())
    exact = bool(np.array_equal(rows[:n_cpu, :5].view(np.uint64), cpu[:, :5].view(np.uint64)))
    with np.errstate(invalid='ignore'):
        log_diff = float(np.nanmax(np.abs(rows[:n_cpu, 5:] - cpu[:, 5:])))

    out = {'tool': 'pitch_bench', 'config': repr(cfg), 'tau_min': cfg.tau_min, 'tau_max': cfg.tau_max, 'W': cfg.W,
           'utterances': a.utterances, 'samples': int(lengths.sum()), 'seconds_of_audio': float(lengths.sum()) / cfg.sr,
           'frames_per_side': ftot, 'chunk_bytes': a.chunk_bytes, 'chunks': len(chunks), 'rounds': a.rounds,
           'compare_pitch_many_host_s': [round(min(walls), 4), round(max(walls), 4)], 'all_rounds_host_s': walls,
           'families': families, 'numpy_float64_host_cpu_s': round(cpu_s, 2), 'numpy_utterances': n_cpu, 'numpy_frames_per_side': cpu_frames,
           'numpy_scaled_to_the_list_s': round(cpu_s * ftot / max(cpu_frames, 1), 1), 'cpu_threads': os.environ.get('OMP_NUM_THREADS', ''),
           'device_equals_numpy_counts_vuv_gross': exact, 'device_against_numpy_log_columns_max_abs': log_diff,
           'score_means': dict((k, float(np.nanmean(scores[k]))) for k in R.COLUMNS)}
    print(json.dumps(out))
    if a.out:
        lines = ['tools/pitch_bench.py --rounds %d --utterances %d  (%s: lags %d .. %d, W %d)'
                 % (a.rounds, a.utterances, repr(cfg), cfg.tau_min, cfg.tau_max, cfg.W),
                 '%d utterances, %d samples (%.0f s of audio), %d frames per side, %d chunk(s) of at most %d bytes'
                 % (a.utterances, lengths.sum(), lengths.sum() / float(cfg.sr), ftot, len(chunks), a.chunk_bytes), '',
                 'compare_pitch_many end to end, host clock (uploads, launches, scores back), %d rounds: %.4f - %.4f s'
                 % (a.rounds, min(walls), max(walls)), '',
                 'launch family            launches   device ms (range)     GFLOP float64   TFLOP/s float64']
        for k, f in families.items():
            lines.append('%-24s %8d   %8.3f - %8.3f   %13.1f   %s'
                         % (k, f['launches'], f['ms'][0], f['ms'][1], f['gflop_float64'],
                            '-' if not f['tflops_float64'] else '%.2f - %.2f' % tuple(f['tflops_float64'])))
        lines += ['', 'tests/pitch_ref.py, float64 NumPy on the host CPU, %d pairs (%d frames a side), once: %.2f s (OMP_NUM_THREADS=%s); '
                  'scaled by frames to the list: %.0f s' % (n_cpu, cpu_frames, cpu_s, out['cpu_threads'], out['numpy_scaled_to_the_list_s']),
                  'device against it on those pairs: counts, vuv_error, gross_error bit-equal: %s; log-based columns differ by at most %.3g'
                  % (exact, log_diff),
                  'mean scores: ' + ', '.join('%s %.4f' % (k, out['score_means'][k]) for k in R.COLUMNS), '', json.dumps(out)]
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
