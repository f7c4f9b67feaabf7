"""What the optimizer hooks cost per recorded step at configs[1] (bench.py's model, batch 16, length 7680), on one box in
one call: `--rounds` interleaved rounds of {no hooks, clipping that never triggers, clipping that always triggers, all
three hooks}, each variant a fresh child process, ms per replayed step for every run.

    python tools/optim_hooks_bench.py [--steps 30] [--rounds 3] [--out profiles/optim_hooks/bench.json]

The per-kernel numbers (the norm pass's achieved TB/s, the hooked Adam's time next to adam_kernel's) come from a
kernel trace of two of the children, a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/optim_hooks_bench.py --child --variant all --steps 20
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/optim_hooks_bench.py --child --variant none --steps 20
    python tools/optim_hooks_bench.py --stats DIR/.../*_kernel_stats.csv          # the rows that matter, with TB/s
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'chainer-vq-vae_amd'))

VARIANTS = ('none', 'clip_never', 'clip_always', 'all')
KERNELS = ('optim_sumsq_kernel', 'optim_finalise_kernel', 'adam_hooked_kernel', 'adam_kernel')


def child(a):
    import bench
    import vqvae_amd as V
    from vqvae_amd import backend
    cfg = dict(bench.CFG)
    backend.init(0)
    model, opt = bench.build(cfg, 1)
    model.to_gpu()
    opt.setup(model)
    if a.variant == 'clip_never':
        opt.add_hook(V.GradientClipping(1e30))
    elif a.variant == 'clip_always':
        opt.add_hook(V.GradientClipping(1e-3))
    elif a.variant == 'all':
        opt.add_hook(V.GradientClipping(1e-3))
        opt.add_hook(V.NonFiniteGuard())
        opt.add_hook(V.GradientNorms())
    shards = [V.concat_examples(bench.synth_examples(cfg['batch_per_gpu'], cfg, 71), device=0)]
    upd = V.VQVAE_ParallelUpdater(bench.ResidentIterator(shards), opt, converter=bench.resident_converter, device=0,
                                  graph=True)
    for _ in range(8):                   # lazily shaped parameters appear at step 1, the recording at step 3
        upd.update()
        if upd._graphed is not None:
            break
    if upd._graphed is None:
        raise SystemExit('optim_hooks_bench: no recording of the step after the warm-up')
    for _ in range(3):
        upd.update()
    backend.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        upd.update()
    backend.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    out = {'variant': a.variant, 'ms_per_step': ms, 'n_train': int(opt.n_train),
           'losses': [float(l.data.get()) for l in upd.last_losses]}
    if a.variant != 'none':
        st = opt.hook_state()
        out.update(grad_norm=st['norm'], scale=float(st['scale']), skipped=opt.skipped_steps(),
                   work_items=opt._hook_dev['n_items'])
    print(json.dumps(out))


def stats_rows(paths):
    """The hook kernels' rows (and adam_kernel's) of rocprofv3's *_kernel_stats.csv files."""
    rows = []
    for path in paths:
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r.get('Name', '')
                hit = [k for k in KERNELS if k in name and (k != 'adam_kernel' or 'hooked' not in name)]
                if hit:
                    rows.append({'file': os.path.basename(path), 'kernel': hit[0], 'calls': int(r['Calls']),
                                 'avg_us': float(r['AverageNs']) * 1e-3, 'min_us': float(r['MinNs']) * 1e-3,
                                 'max_us': float(r['MaxNs']) * 1e-3})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--variant', default='none', choices=VARIANTS)
    ap.add_argument('--timeout', type=int, default=240, help='seconds per child process')
    ap.add_argument('--stats', nargs='*', default=None, help='*_kernel_stats.csv files of a rocprofv3 run: print the hook kernels')
    ap.add_argument('--n-train', type=int, default=0, help='with --stats: gradients in the arena, for the TB/s column')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.stats is not None:
        for r in stats_rows(a.stats):
            tbs = ''
            if a.n_train and r['kernel'] == 'optim_sumsq_kernel':
                tbs = '  %.2f TB/s at the average, %.2f at the best' % (4e-6 * a.n_train / r['avg_us'], 4e-6 * a.n_train / r['min_us'])
            print('%(file)s  %(kernel)s  %(calls)d calls  avg %(avg_us).1f us  min %(min_us).1f  max %(max_us).1f' % r + tbs)
        return
    runs = {v: [] for v in VARIANTS}
    for _ in range(a.rounds):
        for v in VARIANTS:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--variant', v, '--steps', str(a.steps)],
                                 stdout=subprocess.PIPE, timeout=a.timeout, check=True)
            runs[v].append(json.loads(out.stdout.decode().strip().splitlines()[-1]))
            print('%-12s %.3f ms per step' % (v, runs[v][-1]['ms_per_step']), flush=True)
    res = {'workload': 'configs[1], batch 16, length 7680, recorded step', 'steps': a.steps, 'rounds': a.rounds, 'runs': runs,
           'ms_per_step': {v: [r['ms_per_step'] for r in runs[v]] for v in VARIANTS}}
    print(json.dumps(res['ms_per_step']))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
