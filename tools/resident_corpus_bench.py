"""The training step fed from a device-resident corpus (vqvae_amd.ResidentCorpus / ResidentCorpusIterator) beside the two
feeds bench.py times: the minibatch already on the device (`ms_per_step`) and a fresh host minibatch every step through
inputs.StreamingInputIterator (`ms_per_step_with_input`).
usage: python tools/resident_corpus_bench.py [--rounds 3] [--steps 30] [--utterances 2000] [--seed 0] [--draws 200]
       python tools/resident_corpus_bench.py --parent DIR [--rounds 3] [--steps 30]
  Model: BASELINE configs[1] (bench.py's CFG: B = 16, L = 7680), one GPU, the step replayed as a hipGraph.
  Corpus: synthetic, --utterances waveforms whose lengths follow the gamma law of tools/gen_bench.py (shape 2, mean
  3.6 s) clipped to 1-10 s at 16 kHz.
  Per round, interleaved in one process: `resident` (two device minibatches alternated), `streaming` (fresh host
  minibatch per step), `corpus` (every minibatch drawn on the device).  Ranges over the rounds are printed, not means.
  Also: the draw launch alone between device events, the host time of next(), the corpus's bytes.
  Prints one JSON line.
  --parent DIR (a built tree of the parent commit): per round, as fresh child processes one after the other, (a) DIR's
  `bench.py --full`, (b) this tree's `bench.py --full`, (c) this tool with --rounds 1; prints the three rounds of
  ms_per_step / ms_per_step_with_input of (a) and (b), (c)'s legs, and the two comparisons against (a)'s own spread."""
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


def corpus_lengths(n, seed, rate=16000.0):
    """gamma(shape 2, mean 3.6 s) as tools/gen_bench.gamma_lengths, clipped to 1-10 s."""
    rs = np.random.RandomState(seed)
    return (np.clip(rs.gamma(2.0, 1.8, n), 1.0, 10.0) * rate).astype(np.int64)


def synthetic_waves(lengths, seed):
    """Three sinusoids and a little noise per utterance (bench.synth_examples's signal), float32, not normalised."""
    rs = np.random.RandomState(seed)
    for n in lengths:
        t = np.arange(n, dtype=np.float32) / np.float32(16000.0)
        f, ph, a = rs.uniform(80, 4000, 3), rs.uniform(0, 2 * np.pi, 3), rs.uniform(0.2, 1.0, 3)
        w = sum(np.float32(a[i]) * np.sin(np.float32(2 * np.pi * f[i]) * t + np.float32(ph[i])) for i in range(3))
        yield (w + np.float32(0.05) * rs.standard_normal(n).astype(np.float32)).astype(np.float32)


def last_json(text):
    return json.loads([l for l in text.split('\n') if l.startswith('{')][-1])


def child(cmd, cwd):
    sys.stderr.write('resident_corpus_bench: %s (in %s)\n' % (' '.join(cmd), cwd))
    sys.stderr.flush()
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    if r.returncode != 0:
        raise SystemExit('resident_corpus_bench: %s failed (%d): %s' % (cmd, r.returncode, r.stderr.decode()[-2000:]))
    return last_json(r.stdout.decode())


def against_parent(a):
    """Three interleaved rounds of (a) the parent's bench.py --full, (b) this tree's, (c) this tool's legs."""
    bench_args = ['--gpus', '1', '--full', '--steps', str(a.steps), '--warmup', '5', '--no-cpu-baseline', '--no-kernel-table']
    rows = {'parent': [], 'this': [], 'corpus': []}
    for _ in range(a.rounds):
        for who, root in (('parent', os.path.abspath(a.parent)), ('this', ROOT)):
            d = child([os.path.join(root, 'bench.py')] + bench_args, root)
            rows[who].append({'ms_per_step': d['ms_per_step'], 'ms_per_step_with_input': d['ms_per_step_with_input']})
        rows['corpus'].append(child([os.path.abspath(__file__), '--rounds', '1', '--steps', str(a.steps), '--utterances',
                                     str(a.utterances), '--seed', str(a.seed), '--draws', str(a.draws)], ROOT))
    pa = [r['ms_per_step'] for r in rows['parent']]
    pw = [r['ms_per_step_with_input'] for r in rows['parent']]
    tb = [r['ms_per_step'] for r in rows['this']]
    c = [r['ms_per_step_corpus'][0] for r in rows['corpus']]
    out = {'tool': 'resident_corpus_bench --parent', 'rounds': rows,
           'parent_ms_per_step_range': [min(pa), max(pa)], 'parent_with_input_range': [min(pw), max(pw)],
           'this_ms_per_step_range': [min(tb), max(tb)], 'corpus_ms_per_step_range': [min(c), max(c)],
           # (b) inside (a)'s round-to-round spread; (c) above (a)'s with-input figure of the same round by at most (a)'s spread
           'this_inside_parent_spread': bool(min(pa) <= min(tb) and max(tb) <= max(pa)),
           'corpus_minus_parent_with_input': [ci - wi for ci, wi in zip(c, pw)],
           'parent_with_input_spread': max(pw) - min(pw),
           'corpus_within_parent_with_input_plus_spread': bool(all(ci - wi <= max(pw) - min(pw) for ci, wi in zip(c, pw)))}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default='', help='a built tree of the parent commit: interleave its bench.py --full with this tree\'s')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--utterances', type=int, default=2000)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--draws', type=int, default=200, help='draw launches timed alone between device events')
    a = ap.parse_args()
    if a.parent:
        return against_parent(a)
    import bench
    import vqvae_amd as V
    from vqvae_amd import _lib, backend
    from vqvae_amd.inputs import DeviceInputPipeline, StreamingInputIterator
    backend.init(0)
    cfg = dict(bench.CFG)
    B, L = cfg['batch_per_gpu'], cfg['length']
    model, opt = bench.build(cfg, 1)
    model.to_gpu(0)
    opt.setup(model)

    host = []
    for s in range(8):
        ex = bench.synth_examples(B, cfg, seed=71 + s)
        host.append((np.stack([e[0][0, :, 0] for e in ex]), np.array([e[2] for e in ex], np.int32)))
    pipe = DeviceInputPipeline(cfg['quantize'])
    resident = bench.ResidentIterator([pipe(*host[0]), pipe(*host[1])])
    cyc = [0]

    def source():
        cyc[0] += 1
        return host[cyc[0] % len(host)]
    streaming = StreamingInputIterator(source, B, L, cfg['quantize'])

    lengths = corpus_lengths(a.utterances, a.seed)
    t0 = time.perf_counter()
    rs = np.random.RandomState(a.seed + 1)
    corpus = V.ResidentCorpus(synthetic_waves(lengths, a.seed + 2), rs.randint(0, cfg['n_speaker'], a.utterances))
    backend.synchronize()
    ingest_s = time.perf_counter() - t0
    drawn = V.ResidentCorpusIterator(corpus, B, L, seed=71, quantize=cfg['quantize'])

    upd = V.VQVAE_ParallelUpdater(resident, opt, converter=bench.resident_converter, device=0, graph=True)
    for _ in range(8):
        upd.update()
        if upd._graphed is not None:
            break
    if upd._graphed is None:
        raise SystemExit('resident_corpus_bench: no recording after the warm-up steps')
    feeds = (('resident', resident), ('streaming', streaming), ('corpus', drawn))
    ms = dict((name, []) for name, _ in feeds)
    for _ in range(a.rounds):
        for name, it in feeds:
            upd._iterators['main'] = it
            for _ in range(2):
                upd.update()
            backend.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                upd.update()
            backend.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / a.steps)

    # the draw alone: device events around every launch, and the host time of next() with nothing to wait for
    st = backend.stream()
    dev_us, host_us = [], []
    for _ in range(a.draws):
        e0 = backend.Event().record(st)
        t0 = time.perf_counter()
        batch = drawn.next()
        host_us.append(1e6 * (time.perf_counter() - t0))
        e1 = backend.Event().record(st)
        _lib.call('vqvae_event_synchronize', e1.h)
        el = C.c_float(0)
        _lib.call('vqvae_event_elapsed_ms', C.byref(el), e0.h, e1.h)
        dev_us.append(1e3 * el.value)
        del batch
    dev_us, host_us = np.sort(dev_us[10:]), np.sort(host_us[10:])

    def rng(v):
        return [round(float(min(v)), 3), round(float(max(v)), 3)]
    out = {'tool': 'resident_corpus_bench', 'workload': 'BASELINE configs[1]: B %d, L %d, one GPU, hipGraph step' % (B, L),
           'rounds': a.rounds, 'steps': a.steps,
           'ms_per_step_resident': rng(ms['resident']), 'ms_per_step_streaming': rng(ms['streaming']),
           'ms_per_step_corpus': rng(ms['corpus']), 'ms_per_step_all_rounds': ms,
           'draw_launch_us_between_events': {'min': float(dev_us[0]), 'median': float(np.median(dev_us)), 'max': float(dev_us[-1])},
           'next_host_us': {'min': float(host_us[0]), 'median': float(np.median(host_us)), 'max': float(host_us[-1])},
           'dispatches_per_step_added': 1,
           'corpus': {'utterances': len(corpus), 'hours': corpus.hours(16000), 'bytes': corpus.nbytes, 'ingest_s': ingest_s,
                      'epochs_drawn': drawn.epoch_detail}}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
