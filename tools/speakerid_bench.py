"""Speaker identity over a validation list: speakerid.identify_many (csrc/speaker_id.h) timed end to end and per launch,
beside the NumPy restatement of the same rule on the host CPU.
usage: python tools/speakerid_bench.py [--rounds 3] [--utterances 300] [--seed 0] [--speakers 100] [--cpu-threads 16]
                                       [--step-timeout 300] [--out FILE]
       python tools/speakerid_bench.py --parent DIR [--rounds 3] [--steps 30]
  Utterances: the list of DESIGN 7f as tools/frontend_bench.py draws it, tools/gen_bench.gamma_lengths(300, seed 0)
  (gamma(shape 2, mean 3.6 s) clipped to 0.5 - 10 s at 16 kHz), host float32 waves, each normalised to peak 1; utterance i
  is speaker i mod --speakers.  MelConfig(): n_fft 1024, hop 256, 80 mel bands, 13 cepstra; deltas, D = 26; no gate;
  ridge 1e-6.  The list is both enrolment and test.
  Every GPU step is a fresh process of this file (--step NAME) under --step-timeout; a step that fails ends the run.
  (a) step identify: identify_many from host waves end to end on the host clock (two features_many, the features, the
      statistics, the host fit, the score launch, results back).
  (b) step launches: one more pass with device events around each of the three entry points: device time per launch,
      and the score launch's float64 rate: kept frames * models * (2 T + 3 D) operations, T = D (D + 1) / 2.
  (c) tests/speakerid_ref.py on the device's own log-mel (written by step identify to a scratch directory) on
      --cpu-threads processes: features and statistics per utterance, the fit, the scores; compared with the device's q.
  Ranges over the rounds, not means.  Prints one JSON line; --out also writes the table as text.
  --parent DIR (a built tree of the parent commit): tools/frontend_bench.py's interleaved bench.py rounds."""
import argparse
import ctypes as C
import hashlib
import json
import multiprocessing
import os
import shutil
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

ENTRIES = ('vqvae_spk_features', 'vqvae_spk_stats', 'vqvae_spk_score')
STEPS = ('identify', 'launches')
RIDGE = 1e-6


def make_list(a):
    from gen_bench import gamma_lengths
    from resident_corpus_bench import synthetic_waves
    lengths = gamma_lengths(a.utterances, a.seed)
    waves = [(w / np.abs(w).max()).astype(np.float32) for w in synthetic_waves(lengths, a.seed + 2)]
    return waves, (np.arange(a.utterances) % a.speakers).astype(np.int64)


def digest(q):
    return hashlib.sha1(np.ascontiguousarray(q, np.float64).tobytes()).hexdigest()


def step(a):
    """One GPU step in this process; prints its JSON line."""
    from vqvae_amd import _lib, backend, metrics, speakerid
    backend.init(0)
    cfg = metrics.MelConfig()
    waves, speakers = make_list(a)
    st = backend.stream()
    run = lambda: speakerid.identify_many(waves, speakers, waves, cfg, a.speakers, ridge=RIDGE)
    out = {'step': a.step}
    if a.step == 'identify':
        run()                                                            # warm-up: allocator pool, code objects, tables
        backend.synchronize()
        walls = []
        for _ in range(a.rounds):
            backend.synchronize()
            t0 = time.perf_counter()
            sc = run()
            walls.append(time.perf_counter() - t0)
        feats = metrics.features_many(waves, cfg)
        np.save(os.path.join(a.scratch, 'log_mel.npy'), feats.log_mel.get())
        np.save(os.path.join(a.scratch, 'frames.npy'), feats.frames)
        out.update(identify_many_host_s=[round(min(walls), 5), round(max(walls), 5)], frames=int(feats.frames.sum()),
                   longest=int(feats.frames.max()), kept=int(sc.count.sum()), D=sc.D, models=sc.G, accuracy=sc.accuracy(speakers),
                   q_sha1=digest(sc.q))
    else:
        def elapsed(e0, e1):
            el = C.c_float(0)
            _lib.call('vqvae_event_elapsed_ms', C.byref(el), e0.h, e1.h)
            return float(el.value)
        call0 = speakerid.call
        sc = run()
        rounds = {k: [] for k in ENTRIES}
        launches = {k: 0 for k in ENTRIES}
        for _ in range(a.rounds):
            marks = []

            def call(entry, *args):
                e0 = backend.Event().record(st)
                call0(entry, *args)
                marks.append((entry, e0, backend.Event().record(st)))
            speakerid.call = call
            try:
                sc = run()
                backend.synchronize()
            finally:
                speakerid.call = call0
            for k in ENTRIES:
                rounds[k].append([elapsed(e0, e1) for entry, e0, e1 in marks if entry == k])
                launches[k] = len(rounds[k][-1])
        # identify_many launches features twice (enrolment, test), statistics once, score once
        out['launches'] = {k: {'launches': launches[k], 'ms_each': [round(min(min(r) for r in v), 4), round(max(max(r) for r in v), 4)]}
                           for k, v in rounds.items()}
        D, T = sc.D, sc.D * (sc.D + 1) // 2
        ops = float(sc.count.sum()) * sc.G * (2 * T + 3 * D)
        ms = out['launches']['vqvae_spk_score']['ms_each']
        out.update(score_ops=ops, score_tflops=[round(ops / (ms[1] * 1e-3) / 1e12, 3), round(ops / (ms[0] * 1e-3) / 1e12, 3)])
    print(json.dumps(out))


_MODELS = None


def _first(job):
    import speakerid_ref as R
    log_mel, dct = job
    x, keep = R.features(log_mel, dct)
    return (x, keep) + R.stats(x, keep)


def _init_second(mu, linv):
    global _MODELS
    _MODELS = (mu, linv)


def _second(job):
    import speakerid_ref as R
    return R.score(job[0], job[1], _MODELS[0], _MODELS[1])[0]


def restate(a, scratch):
    """(seconds, sha1 of q): the restatement over the device's log-mel on a.cpu_threads processes."""
    import speakerid_ref as R
    from vqvae_amd import metrics
    dct = metrics.tables(metrics.MelConfig())[2]
    log_mel, frames = np.load(os.path.join(scratch, 'log_mel.npy')), np.load(os.path.join(scratch, 'frames.npy'))
    off = np.concatenate([[0], np.cumsum(frames)])
    blocks = [np.ascontiguousarray(log_mel[:, int(s):int(e)]) for s, e in zip(off[:-1], off[1:])]
    speakers = np.arange(a.utterances) % a.speakers
    ctx = multiprocessing.get_context('spawn')
    pool = ctx.Pool(a.cpu_threads)
    pool.map(_first, [(blocks[0], dct)] * a.cpu_threads)                 # the workers' imports are not on the clock
    t0 = time.perf_counter()
    rows = pool.map(_first, [(b, dct) for b in blocks], chunksize=1)
    pool.close()
    pool.join()
    fit = R.fit(*R.speaker_sums([r[2:] for r in rows], speakers, a.speakers), ridge=RIDGE)
    pool = ctx.Pool(a.cpu_threads, _init_second, (fit['mu'], fit['linv']))
    q = np.stack(pool.map(_second, [r[:2] for r in rows], chunksize=1))
    wall = time.perf_counter() - t0
    pool.close()
    pool.join()
    return wall, digest(q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default='', help='a built tree of the parent commit: interleave its bench.py with this tree\'s')
    ap.add_argument('--step', default='', choices=('',) + STEPS, help='(internal) run this GPU step in this process')
    ap.add_argument('--scratch', default='', help='(internal) where step identify leaves the log-mel for the restatement')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--utterances', type=int, default=300)
    ap.add_argument('--speakers', type=int, default=100)
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
    out = {'tool': 'speakerid_bench', 'utterances': a.utterances, 'speakers': a.speakers, 'rounds': a.rounds, 'ridge': RIDGE}
    scratch = tempfile.mkdtemp(prefix='speakerid_bench')
    try:
        for name in STEPS:                                               # a fresh process per GPU step, each under its own limit
            cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ['--step', name, '--scratch', scratch]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=a.step_timeout)
            if r.returncode != 0:
                raise SystemExit('speakerid_bench: step %s failed (%d): %s' % (name, r.returncode, r.stderr.decode()[-2000:]))
            got = json.loads(r.stdout.decode().strip().splitlines()[-1])
            got.pop('step')
            out[name] = got
        if a.cpu_threads:
            wall, sha = restate(a, scratch)
            out['cpu'] = {'numpy_host_cpu_s': round(wall, 2), 'cpu_processes': a.cpu_threads,
                          'device_equals_numpy': bool(sha == out['identify']['q_sha1'])}
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    print(json.dumps(out))
    if a.out:
        i, l = out['identify'], out['launches']
        lines = ['tools/speakerid_bench.py --rounds %d --utterances %d --speakers %d' % (a.rounds, a.utterances, a.speakers),
                 '%d utterances, %d frames (%d kept), the longest %d; D = %d, %d models; accuracy on the enrolment list %.3f'
                 % (a.utterances, i['frames'], i['kept'], i['longest'], i['D'], i['models'], i['accuracy']), '',
                 '(a) identify_many from host waves end to end, host clock, %d rounds: %.5f - %.5f s'
                 % (a.rounds, i['identify_many_host_s'][0], i['identify_many_host_s'][1]), '',
                 '(b) entry point            launches a call   device ms each (range)']
        for k, f in l['launches'].items():
            lines.append('    %-22s %8d          %8.4f - %8.4f' % (k, f['launches'], f['ms_each'][0], f['ms_each'][1]))
        lines += ['    the score launch: %.4g float64 operations, %.3f - %.3f TFLOP/s (the YIN tracker measured 14)'
                  % (l['score_ops'], l['score_tflops'][0], l['score_tflops'][1]), '']
        if 'cpu' in out:
            u = out['cpu']
            lines += ['(c) tests/speakerid_ref.py, NumPy on the host CPU, the same list on %d processes, once: %.2f s; the device\'s q '
                      'equals it in every bit: %s' % (u['cpu_processes'], u['numpy_host_cpu_s'], u['device_equals_numpy']), '']
        lines.append(json.dumps(out))
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
