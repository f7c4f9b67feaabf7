"""ABX discriminability over a validation list: abx.abx_many (csrc/abx.h) through the default model's front end, timed end
to end and per entry point, beside encode_many on the same list and the NumPy restatement on the host CPU.
usage: python tools/abx_bench.py [--rounds 3] [--utterances 300] [--seed 0] [--labels 40] [--speakers 20] [--max-per-group 8]
                                 [--cpu-pairs 512] [--cpu-threads 16] [--step-timeout 300] [--out FILE]
       python tools/abx_bench.py --parent DIR [--rounds 3] [--steps 30]
  Model: the default one (d = 512, k = 128), seeded weights (tools/frontend_bench.build_links).  Utterances: the list of
  DESIGN 7f, tools/gen_bench.gamma_lengths(300, seed 0) (gamma(shape 2, mean 3.6 s) clipped to 0.5 - 10 s at 16 kHz), host
  waves.  Items: SYNTHETIC -- every utterance's latent frames cut end to end into items of 3 to 30 frames (uniform), each
  with a random label of --labels; utterance u is of speaker u % --speakers; no contexts.  The labels carry no information
  about the frames, so the error itself says nothing (it is near 0.5); the work is what is measured.  Task: within speakers,
  --max-per-group triples of every group.
  The GPU step is a fresh process of this file (--step gpu) under --step-timeout.
  (a) the plan on the host, once; encode_many, abx_many(plan=...) over the latents and over the codes, end to end on the
      host clock (upload, encoder, quantiser, norms, local costs, DP, results back, scores).
  (b) one more pass of each with device events round every vqvae_abx_norms, vqvae_abx_local and vqvae_abx_dtw call, split
      by the DP's form; the local entry point's float64 rate over the latents: cells * d * 2 operations (a product and an
      addition per channel and cell) over its device time.
  (c) the first --cpu-pairs pairs through tests/abx_ref.py on --cpu-threads processes, scaled to the list by cells * d,
      and compared with the device's distances.
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


def _restate(job):
    import abx_ref as R
    xa, xb = job
    dist, cost, K = R.pair(xa, xb, 'cosine')
    return float(dist), float(cost), int(K)


def synthetic_items(tl, labels, speakers, seed):
    from vqvae_amd import abx
    rs = np.random.RandomState(seed)
    utt, start, stop = [], [], []
    for u, t in enumerate(tl):
        at = 0
        while at + 3 <= t:
            F = min(int(rs.randint(3, 31)), int(t) - at)
            utt.append(u), start.append(at), stop.append(at + F)
            at += F
    utt = np.array(utt)
    return abx.Items(utt, start, stop, rs.randint(0, labels, utt.size), utt % speakers)


def step(a):
    """The GPU step in this process; prints its JSON line and leaves the CPU's share in --dump."""
    import vqvae_amd as V
    from frontend_bench import build_links
    from gen_bench import gamma_lengths
    from resident_corpus_bench import synthetic_waves
    from vqvae_amd import _lib, abx, backend, frontend
    backend.init(0)
    enc, vq, _ = build_links(a.seed + 3)
    waves = [(w / np.abs(w).max()).astype(np.float32) for w in synthetic_waves(gamma_lengths(a.utterances, a.seed), a.seed + 2)]
    tl = frontend._wave_lengths([w.size for w in waves], 6, 'abx_bench')[1]
    items = synthetic_items(tl, a.labels, a.speakers, a.seed + 5)
    st = backend.stream()

    def host_clock(fn, rounds=a.rounds):
        fn()                                                         # warm-up: allocator pool, code objects
        backend.synchronize()
        walls = []
        for _ in range(rounds):
            backend.synchronize()
            t0 = time.perf_counter()
            out = fn()
            backend.synchronize()
            walls.append(time.perf_counter() - t0)
        return out, [round(min(walls), 5), round(max(walls), 5)]

    out = {'step': 'gpu'}
    t0 = time.perf_counter()
    plan = abx.plan_abx(items, max_per_group=a.max_per_group, seed=a.seed)
    out['plan_host_s'] = round(time.perf_counter() - t0, 4)
    kw = dict(plan=plan)                                             # planned once, as for several snapshots of one item list
    _, out['encode_many_host_s'] = host_clock(lambda: V.encode_many(enc, vq, waves))
    sc_lat, out['abx_many_latents_host_s'] = host_clock(lambda: abx.abx_many(enc, vq, waves, items, what='latents', **kw))
    sc_cod, out['abx_many_codes_host_s'] = host_clock(lambda: abx.abx_many(enc, vq, waves, items, what='codes', **kw))
    pd = sc_lat.pairs
    cells = pd.frames_a * pd.frames_b
    short = np.minimum(pd.frames_a, pd.frames_b)
    out.update(frames=int(tl.sum()), items=len(items), triples=int(plan.tri_a.size), pairs=len(pd), groups=len(plan.groups),
               cells=int(cells.sum()), cells_block_form=int(cells[short > abx.WAVE_SHORT].sum()), d=int(vq.W.data.shape[1]),
               k=int(vq.W.data.shape[0]), item_frames=[int((items.stop - items.start).min()), int((items.stop - items.start).max())],
               error_latents=sc_lat.error, error_codes=sc_cod.error)

    def elapsed(e0, e1):
        el = C.c_float(0)
        _lib.call('vqvae_event_elapsed_ms', C.byref(el), e0.h, e1.h)
        return float(el.value)

    call0 = abx.call
    for what in ('latents', 'codes'):
        rows = []
        for _ in range(a.rounds):
            marks = []

            def call(entry, *args):
                e0 = backend.Event().record(st)
                call0(entry, *args)
                form = ''
                if entry == 'vqvae_abx_dtw':
                    form = '_wave' if args[0]._obj.max_short <= abx.WAVE_SHORT else '_block'
                marks.append((entry[len('vqvae_abx_'):] + form, e0, backend.Event().record(st)))
            abx.call = call
            try:
                abx.abx_many(enc, vq, waves, items, what=what, **kw)
                backend.synchronize()
            finally:
                abx.call = call0
            row = {}
            for name, e0, e1 in marks:
                row[name] = row.get(name, 0.0) + elapsed(e0, e1)
                row[name + '_calls'] = row.get(name + '_calls', 0) + 1
            rows.append(row)
        dev = {}
        for name in rows[0]:
            vals = [r[name] for r in rows]
            dev[name] = vals[0] if name.endswith('_calls') else [round(min(vals), 4), round(max(vals), 4)]
        out['device_' + what] = dev
    local_ms = out['device_latents']['local'][0]
    out['local_float64_gflops'] = round(out['cells'] * out['d'] * 2 / (local_ms * 1e-3) / 1e9, 1)
    if a.dump:
        n = min(a.cpu_pairs, len(pd))
        lat = V.encode_many(enc, vq, waves, return_latents=True)[1]
        cut = lambda m: lat[int(items.utterance[m])][:, int(items.start[m]):int(items.stop[m])]
        np.savez(a.dump, n=n, distance=pd.distance[:n], cost=pd.cost[:n], path_len=pd.path_len[:n],
                 **dict([('a%d' % p, cut(pd.ia[p])) for p in range(n)] + [('b%d' % p, cut(pd.ib[p])) for p in range(n)]))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default='', help='a built tree of the parent commit: interleave its bench.py with this tree\'s')
    ap.add_argument('--step', default='', choices=('', 'gpu'), help='(internal) run the GPU step in this process')
    ap.add_argument('--dump', default='', help='(internal) where the GPU step leaves the CPU\'s share')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--utterances', type=int, default=300)
    ap.add_argument('--labels', type=int, default=40)
    ap.add_argument('--speakers', type=int, default=20)
    ap.add_argument('--max-per-group', type=int, default=8)
    ap.add_argument('--cpu-pairs', type=int, default=512)
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
    out = {'tool': 'abx_bench', 'utterances': a.utterances, 'rounds': a.rounds}
    with tempfile.TemporaryDirectory() as tmp:
        dump = os.path.join(tmp, 'cpu_share.npz')
        cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ['--step', 'gpu', '--dump', dump]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=a.step_timeout)
        if r.returncode != 0:
            raise SystemExit('abx_bench: the GPU step failed (%d): %s' % (r.returncode, r.stderr.decode()[-2000:]))
        g = out['gpu'] = json.loads(r.stdout.decode().strip().splitlines()[-1])
        g.pop('step')
        with np.load(dump) as f:
            n = int(f['n'])
            jobs = [(f['a%d' % p], f['b%d' % p]) for p in range(n)]
            device = list(zip(f['distance'].tolist(), f['cost'].tolist(), f['path_len'].tolist()))
    if jobs:
        pool = multiprocessing.get_context('spawn').Pool(a.cpu_threads)
        t0 = time.perf_counter()
        rows = pool.map(_restate, jobs, chunksize=8)
        cpu_s = time.perf_counter() - t0
        pool.close()
        pool.join()
        cells = sum(j[0].shape[1] * j[1].shape[1] for j in jobs)
        out['cpu'] = {'numpy_host_cpu_s': round(cpu_s, 3), 'numpy_pairs': len(jobs), 'numpy_cells': cells, 'cpu_processes': a.cpu_threads,
                      'numpy_scaled_to_the_list_s': round(cpu_s * g['cells'] / max(cells, 1), 1),
                      'device_equals_numpy': bool(all(tuple(r) == tuple(d) for r, d in zip(rows, device)))}
    for what in ('latents', 'codes'):
        out['ratio_to_encode_many_' + what] = round(g['abx_many_%s_host_s' % what][0] / g['encode_many_host_s'][0], 3)
    print(json.dumps(out))
    if a.out:
        lines = ['tools/abx_bench.py --rounds %d --utterances %d --labels %d --speakers %d --max-per-group %d  (d = %d, k = %d, %d frames, '
                 '%d synthetic items of %d - %d frames, %d groups, %d triples, %d unique ordered pairs, %d cells, %d of them in the 256-lane form)'
                 % (a.rounds, a.utterances, a.labels, a.speakers, a.max_per_group, g['d'], g['k'], g['frames'], g['items'], g['item_frames'][0],
                    g['item_frames'][1], g['groups'], g['triples'], g['pairs'], g['cells'], g['cells_block_form']), '',
                 '(a) end to end, host clock, %d rounds: encode_many %.5f - %.5f s; abx_many latents %.5f - %.5f s (x%.3f); codes %.5f - %.5f s (x%.3f); '
                 'the plan alone, host, once: %.4f s' % (a.rounds, g['encode_many_host_s'][0], g['encode_many_host_s'][1],
                                                         g['abx_many_latents_host_s'][0], g['abx_many_latents_host_s'][1], out['ratio_to_encode_many_latents'],
                                                         g['abx_many_codes_host_s'][0], g['abx_many_codes_host_s'][1], out['ratio_to_encode_many_codes'],
                                                         g['plan_host_s']), '',
                 '(b) device time between events, ms, summed over the calls (calls)']
        for what in ('latents', 'codes'):
            v = g['device_' + what]
            lines.append('    %-8s' % what + '   '.join('%s %.4f - %.4f (%d)' % (name, v[name][0], v[name][1], v[name + '_calls'])
                                                       for name in ('table', 'norms', 'local', 'dtw_wave', 'dtw_block') if name in v))
        lines += ['    local over the latents: %d cells * %d channels * 2 float64 operations / %.4f ms = %.1f GFLOP/s'
                  % (g['cells'], g['d'], g['device_latents']['local'][0], g['local_float64_gflops']),
                  '    synthetic labels: error %.4f over the latents, %.4f over the codes (chance is 0.5)' % (g['error_latents'], g['error_codes'])]
        if 'cpu' in out:
            u = out['cpu']
            lines += ['', '(c) tests/abx_ref.py, NumPy on the host CPU, the first %d pairs (%d cells), cosine over the latents, on %d processes, once: %.3f s; '
                      'scaled by cells to the list: %.1f s; the device\'s distance, cost and path_len equal it on those pairs: %s'
                      % (u['numpy_pairs'], u['numpy_cells'], u['cpu_processes'], u['numpy_host_cpu_s'], u['numpy_scaled_to_the_list_s'], u['device_equals_numpy'])]
        lines += ['', json.dumps(out)]
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
