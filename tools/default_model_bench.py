"""Training step of the reference's DEFAULT model (params.py: d = 512, k = 128, WaveNet 3 x 10 blocks with 512 residual /
512 dilated / 256 skip channels, condition 512 + 128, 109 speakers) at batch 4, length 7680, 'float32x2': the float32x2
pre-split chain (vqvae_set_presplit(7), the default) against the generic path with every tensor of the chain fp32
(vqvae_set_presplit(0)) -- three interleaved rounds, every measurement in a fresh child process on the same device, the
step replayed as one hipGraph.  Then a per-kernel table from the library's event profiler (eager launches, each kernel timed
by its own dispatch's events), every kernel of the chain set against its roofline: max(FLOP / the three-product MFMA
ceiling, algorithmic HBM bytes / HBM bandwidth) / measured time.  No torch, no reference: runs on the GPU box alone.
usage: python tools/default_model_bench.py [--steps 10] [--rounds 3] [--batch 4] [--length 7680] [--out profiles/...json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'chainer-vq-vae_amd'))

CFG = dict(d=512, k=128, n_loop=3, n_layer=10, filter_size=2, input_dim=256, quantize=256,
           residual=512, dilated=512, skip=256, local_dim=512, global_dim=128, n_speaker=109,
           length=7680, beta=0.25, lr=2e-4, ema_mu=0.9999, batch_per_gpu=4)
MFMA_CEILING_TFLOPS = 2500.0 / 3.0      # three fp16 MFMA products per fp32 product
HBM_TBS = 8.0
TAGS = {1: 'gate GEMM (fwd)', 2: 'residual 1x1 (fwd)', 3: 'gate derivative (gz -> gh)', 4: 'backward-data (gx)',
        11: 'skip sum', 12: 'dilated weight gradients', 13: 'res / skip weight gradients',
        7: 'other convs fwd', 8: 'other convs bwd-data', 9: 'other convs wgrad', 10: 'vq nearest'}


def chain_rooflines(cfg, B, presplit):
    """(FLOP, algorithmic HBM bytes) per LAUNCH of the chain's kernels: N = B T columns; a pre-split or fp32 element is 4
    bytes either way -- what the pre-split chain saves in bytes is the tanh half of the gates (GATES_SIG)."""
    N = B * cfg['length']
    Cr, Cd, Cs, K = cfg['residual'], cfg['dilated'], cfg['skip'], cfg['filter_size']
    Ch = Cd // 2
    saved = 1.0 if presplit & 4 else 1.5
    return {
        1: (2.0 * N * K * Cr * Cd, 4.0 * (N * Cr + N * saved * Cd + K * Cr * Cd)),
        2: (2.0 * N * Ch * Cr, 4.0 * (N * Ch + 2 * N * Cr)),
        3: (2.0 * N * Ch * (Cr + Cs), 4.0 * (N * (Cr + Cs) + N * (saved - 0.5) * Cd + N * Cd)),
        4: (2.0 * N * K * Cd * Cr, 4.0 * (N * Cd + 2 * N * Cr)),
    }


def child(a):
    import bench
    import vqvae_amd as V
    from vqvae_amd import _lib, backend
    cfg = dict(CFG, batch_per_gpu=a.batch, length=a.length)
    backend.init(0)
    backend.set_matmul_dtype('float32x2')
    backend.set_presplit(a.presplit)
    lib = _lib.load()
    d = _lib.ResblockDesc(a.batch, a.length, cfg['residual'], cfg['dilated'], cfg['skip'],
                          cfg['local_dim'] + cfg['global_dim'], cfg['filter_size'], 1, 0)
    bits = lib.vqvae_resblock_f16x2_storage(C.byref(d))
    model, opt = bench.build(cfg, 1)
    model.to_gpu()
    opt.setup(model)
    shards = [V.concat_examples(bench.synth_examples(a.batch, cfg, 71), device=0)]
    upd = V.VQVAE_ParallelUpdater(bench.ResidentIterator(shards), opt, converter=bench.resident_converter, device=0, graph=True)
    for _ in range(8):                   # lazily shaped parameters appear at step 1, the recording at step 3
        upd.update()
        if upd._graphed is not None:
            break
    if upd._graphed is None:
        raise SystemExit('default_model_bench: no recording of the step after the warm-up')
    upd.update()
    backend.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        upd.update()
    backend.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    losses = [float(l.data.get()) for l in upd.last_losses]
    # the same step, launched eagerly, every tagged kernel timed by its own dispatch's events
    upd.graph = False
    upd.update()
    backend.synchronize()
    lib.vqvae_prof_reset()
    lib.vqvae_prof_enable(-1)
    k = min(a.steps, 3)
    for _ in range(k):
        upd.update()
    backend.synchronize()
    lib.vqvae_prof_enable(0)
    kernels = {}
    for tag in sorted(TAGS):
        tot, cnt = C.c_double(0), C.c_int(0)
        _lib.call('vqvae_prof_read', tag, C.byref(tot), C.byref(cnt))
        if cnt.value:
            kernels[tag] = {'launches_per_step': cnt.value / k, 'us_per_launch': 1e3 * tot.value / cnt.value,
                            'ms_per_step': tot.value / k}
    rep = backend.f32x2_contract_violations()
    print(json.dumps({'presplit': a.presplit, 'storage_bits': bits, 'ms_per_step': ms, 'losses': losses, 'kernels': kernels,
                      'f32x2_contract': {'violations': rep['violations'], 'checked': rep['checked']}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batch', type=int, default=CFG['batch_per_gpu'])
    ap.add_argument('--length', type=int, default=CFG['length'])
    ap.add_argument('--presplit', type=int, default=7)
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--timeout', type=int, default=240, help='seconds per child process')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = {0: [], 7: []}
    for _ in range(a.rounds):
        for mask in (0, 7):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--presplit', str(mask), '--steps', str(a.steps),
                                  '--batch', str(a.batch), '--length', str(a.length)], stdout=subprocess.PIPE, timeout=a.timeout, check=True)
            runs[mask].append(json.loads(out.stdout.decode().strip().splitlines()[-1]))
            print('presplit %d: %.3f ms per step (storage bits %d)' % (mask, runs[mask][-1]['ms_per_step'], runs[mask][-1]['storage_bits']), flush=True)
    cfg = dict(CFG, batch_per_gpu=a.batch, length=a.length)
    res = {'model': 'params.py default (d 512, k 128, 3 x 10 blocks, 512 / 512 / 256, condition 640)', 'batch': a.batch,
           'length': a.length, 'matmul': 'float32x2', 'steps': a.steps, 'rounds': a.rounds,
           'mfma_ceiling_tflops': MFMA_CEILING_TFLOPS, 'hbm_tb_s': HBM_TBS, 'paths': {}}
    for mask, name in ((0, 'generic (presplit 0)'), (7, 'pre-split chain (presplit 7)')):
        rs = runs[mask]
        ms = sorted(r['ms_per_step'] for r in rs)
        roof = chain_rooflines(cfg, a.batch, mask)
        table = {}
        for tag, label in TAGS.items():
            rows = [r['kernels'][str(tag)] for r in rs if str(tag) in r['kernels']]
            if not rows:
                continue
            us = sorted(x['us_per_launch'] for x in rows)[len(rows) // 2]
            row = {'kernel': label, 'launches_per_step': rows[0]['launches_per_step'], 'us_per_launch': us,
                   'ms_per_step': us * rows[0]['launches_per_step'] * 1e-3, 'share_of_step': us * rows[0]['launches_per_step'] * 1e-3 / ms[len(ms) // 2]}
            if tag in roof:
                fl, by = roof[tag]
                t_roof = max(fl / (MFMA_CEILING_TFLOPS * 1e12), by / (HBM_TBS * 1e12)) * 1e6
                row.update({'gflop': fl * 1e-9, 'mbytes': by * 1e-6, 'roofline_us': t_roof, 'frac_of_roofline': t_roof / us,
                            'bound': 'MFMA' if fl / (MFMA_CEILING_TFLOPS * 1e12) > by / (HBM_TBS * 1e12) else 'HBM'})
            table[str(tag)] = row
        res['paths'][name] = {'ms_per_step': ms, 'median_ms_per_step': ms[len(ms) // 2], 'storage_bits': rs[0]['storage_bits'],
                              'losses': rs[0]['losses'], 'f32x2_contract': rs[0]['f32x2_contract'], 'kernels': table}
    g, p = res['paths']['generic (presplit 0)'], res['paths']['pre-split chain (presplit 7)']
    res['speedup'] = g['median_ms_per_step'] / p['median_ms_per_step']
    for name, path in res['paths'].items():
        print('\n%s: %s ms per step' % (name, ' / '.join('%.3f' % m for m in path['ms_per_step'])))
        for row in path['kernels'].values():
            print('  %-30s %5.1f x %8.1f us = %7.3f ms (%4.1f %%)%s' % (
                row['kernel'], row['launches_per_step'], row['us_per_launch'], row['ms_per_step'], 100 * row['share_of_step'],
                ('   %.2f of its %s roofline (%.1f us)' % (row['frac_of_roofline'], row['bound'], row['roofline_us'])) if 'roofline_us' in row else ''))
    print('\npre-split chain against generic: x %.3f' % res['speedup'])
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write('\n')


if __name__ == '__main__':
    main()
