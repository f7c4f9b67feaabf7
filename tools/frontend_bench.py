"""The front half of synthesize_many for a corpus: the per-utterance loop (encoder, quantiser and ConditionEmbed with n = 1,
one utterance after the other, as the call runs without ``batched_frontend``) beside frontend.frontend_many (the ragged
convs of include/vqvae_ragged.h: every stage one launch per chunk).
usage: python tools/frontend_bench.py [--rounds 3] [--utterances 300] [--seed 0] [--chunk-bytes 1073741824] [--matmul float32x2]
       python tools/frontend_bench.py --parent DIR [--rounds 3] [--steps 30]
  Model: the default one (d = 512, k = 128, Cl = 512, G = 128, 109 speakers), seeded weights.
  Utterances: the list of DESIGN 7f, tools/gen_bench.gamma_lengths(300, seed 0): gamma(shape 2, mean 3.6 s) clipped to
  0.5 - 10 s at 16 kHz, host float32 waves.
  Per round, interleaved in one process: `loop` (the per-utterance front end: host time until the last launch is enqueued,
  and the device span between two events), `batched` (frontend_many on the same list: the same two figures).  Ranges over
  the rounds are printed, not means.  Then one more batched pass with device events around every launch: the per-stage table.
  Prints one JSON line.
  --parent DIR (a built tree of the parent commit): per round, as fresh child processes one after the other, DIR's
  `bench.py` and this tree's; prints the rounds of ms_per_step and whether this tree's lie inside the parent's spread."""
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


def last_json(text):
    return json.loads([l for l in text.split('\n') if l.startswith('{')][-1])


def against_parent(a):
    args = ['--gpus', '1', '--steps', str(a.steps), '--warmup', '5']
    rows = {'parent': [], 'this': []}
    for rnd in range(a.rounds):
        order = (('parent', os.path.abspath(a.parent)), ('this', ROOT))
        for who, root in (order if rnd % 2 == 0 else order[::-1]):      # alternate who goes first: the chip warms up over a visit
            cmd = [sys.executable, os.path.join(root, 'bench.py')] + args
            sys.stderr.write('frontend_bench: %s (in %s)\n' % (' '.join(cmd), root))
            sys.stderr.flush()
            r = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
            if r.returncode != 0:
                raise SystemExit('frontend_bench: %s failed (%d): %s' % (cmd, r.returncode, r.stderr.decode()[-2000:]))
            rows[who].append(last_json(r.stdout.decode())['ms_per_step'])
    pa, tb = rows['parent'], rows['this']
    print(json.dumps({'tool': 'frontend_bench --parent', 'ms_per_step': rows, 'parent_range': [min(pa), max(pa)],
                      'this_range': [min(tb), max(tb)], 'this_inside_parent_spread': bool(min(pa) <= min(tb) and max(tb) <= max(pa))}))


def build_links(seed, d=512, k=128, Cl=512, G=128, n_speaker=109):
    import vqvae_amd as V
    rs = np.random.RandomState(seed)
    enc, vq, ce = V.Encoder(d), V.VQ(k, d), V.ConditionEmbed(n_speaker, G, Cl)

    def fill(conv, co, ci, K):
        conv.W.data = (rs.standard_normal((co, ci, K, 1)) / np.sqrt(ci * K)).astype(np.float32)
        conv.b.data = (0.1 * rs.standard_normal(co)).astype(np.float32)
    ci = 1
    for s in range(1, 7):
        fill(getattr(enc, 'conv%d' % s), d, ci, 4)
        ci = d
    vq.W.data = (0.1 * rs.standard_normal((k, d))).astype(np.float32)
    ci = d
    for i in range(1, 6):
        fill(getattr(ce, 'local_embed%d' % i), Cl, ci, 3)
        ci = Cl
    ce.global_embed.W.data = rs.standard_normal((n_speaker, G)).astype(np.float32)
    for link in (enc, vq, ce):
        link.to_gpu()
    return enc, vq, ce


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default='', help='a built tree of the parent commit: interleave its bench.py with this tree\'s')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--utterances', type=int, default=300)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--chunk-bytes', type=int, default=1 << 30)
    ap.add_argument('--matmul', default='', help='matmul mode (default: the process default)')
    a = ap.parse_args()
    if a.parent:
        return against_parent(a)
    import vqvae_amd as V
    from gen_bench import gamma_lengths
    from resident_corpus_bench import synthetic_waves
    from vqvae_amd import _lib, backend, core, frontend
    from vqvae_amd.core import Variable
    from vqvae_amd.generation import LatentCondition
    from vqvae_amd.synthesis import _latent_condition
    backend.init(0)
    if a.matmul:
        backend.set_matmul_dtype(a.matmul)
    enc, vq, ce = build_links(a.seed + 3)
    lengths = gamma_lengths(a.utterances, a.seed)
    waves = []
    for w in synthetic_waves(lengths, a.seed + 2):
        waves.append((w / np.abs(w).max()).astype(np.float32))
    speakers = np.random.RandomState(a.seed + 1).randint(0, 109, a.utterances).astype(np.int32)
    st = backend.stream()

    def elapsed(e0, e1):
        el = C.c_float(0)
        _lib.call('vqvae_event_elapsed_ms', C.byref(el), e0.h, e1.h)
        return float(el.value)

    def loop():                                              # synthesize_many's front end without batched_frontend
        conds = []
        with core.using_config('train', False), core.no_backprop_mode():
            for w, spk in zip(waves, speakers):
                xd = backend.to_device(np.asarray(w, np.float32))
                xd = xd.reshape(1, 1, xd.size, 1)
                e = vq(enc(Variable(xd)))
                c = ce(e, Variable(backend.to_device(np.array([spk], np.int32)))).data
                conds.append(_latent_condition(c, ce))
        return LatentCondition.concatenate(conds)

    def batched():
        return V.frontend_many(enc, vq, ce, waves, speakers, chunk_bytes=a.chunk_bytes)

    def timed(fn):
        backend.synchronize()
        e0 = backend.Event().record(st)
        t0 = time.perf_counter()
        out = fn()
        host = time.perf_counter() - t0
        e1 = backend.Event().record(st)
        backend.synchronize()
        wall = time.perf_counter() - t0
        return out, {'host_s': host, 'device_span_s': 1e-3 * elapsed(e0, e1), 'wall_s': wall}

    ref, _ = timed(loop)                                     # warm-up of both (allocator pool, LDS opt-ins, weight packs)
    got, _ = timed(batched)
    # the two front ends round z differently, so a latent frame that lies within rounding of the border between two
    # codes takes the other code and moves the 63 condition frames around it: counted, not hidden in a maximum
    a_, b_ = ref.local.get().reshape(-1), got.local.get().reshape(-1)
    scale, frames, moved = max(float(np.abs(a_).max()), 1e-30), 0, 0
    for o, t in zip(ref.local_off, ref.tl):
        blk = slice(int(o), int(o) + ref.Cl * int(t))
        diff = np.abs(a_[blk] - b_[blk]).reshape(ref.Cl, int(t)).max(axis=0)
        frames, moved = frames + int(t), moved + int((diff > 1e-4 * scale).sum())
    agree = {'latent_frames': frames, 'frames_beyond_1e-4_of_scale': moved}
    del ref, got
    rows = {'loop': [], 'batched': []}
    for _ in range(a.rounds):
        for name, fn in (('loop', loop), ('batched', batched)):
            out, t = timed(fn)
            del out
            rows[name].append(t)

    # the per-stage table: device events around every launch of one more batched pass
    marks = []
    conv0, call0 = frontend._conv, _lib.call

    def conv(tb, x_ptr, x_cstride, off_in_ptr, s_in, s_out, W, b, y_ptr, window, relu, blocked=False):
        e0 = backend.Event().record(st)
        conv0(tb, x_ptr, x_cstride, off_in_ptr, s_in, s_out, W, b, y_ptr, window, relu, blocked)
        name = 'encoder stage %d' % s_out if window[0] == 4 else 'condition conv dil %d' % window[3]
        marks.append((name, e0, backend.Event().record(st), 2.0 * W.shape[0] * W.shape[1] * window[0] * tb.ttot(s_out)))

    def call(name, *args):
        if name in ('vqvae_vq_nearest_fwd', 'vqvae_ragged_speaker_gather'):
            e0 = backend.Event().record(st)
            call0(name, *args)
            marks.append((name, e0, backend.Event().record(st), 0.0))
        else:
            call0(name, *args)
    frontend._conv, _lib.call = conv, call
    try:
        chunks = len(frontend.plan_chunks(lengths, [1] + [512] * 6, a.chunk_bytes))
        batched()
        backend.synchronize()
    finally:
        frontend._conv, _lib.call = conv0, call0
    table = {}
    for name, e0, e1, flop in marks:
        row = table.setdefault(name, {'launches': 0, 'ms': 0.0, 'gflop': 0.0})
        row['launches'] += 1
        row['ms'] += elapsed(e0, e1)
        row['gflop'] += 1e-9 * flop
    for row in table.values():
        row['tflops'] = round(row['gflop'] / row['ms'], 2) if row['ms'] and row['gflop'] else None
        row['ms'], row['gflop'] = round(row['ms'], 3), round(row['gflop'], 1)

    def rng(name, key):
        v = [r[key] for r in rows[name]]
        return [round(min(v), 4), round(max(v), 4)]
    out = {'tool': 'frontend_bench', 'model': 'd 512, k 128, Cl 512, G 128', 'matmul': a.matmul or backend.default_matmul_dtype(),
           'utterances': a.utterances, 'samples': int(lengths.sum()), 'seconds_of_audio': float(lengths.sum()) / 16000.0,
           'chunk_bytes': a.chunk_bytes, 'chunks': chunks, 'rounds': a.rounds,
           'loop': dict((k, rng('loop', k)) for k in ('host_s', 'device_span_s', 'wall_s')),
           'batched': dict((k, rng('batched', k)) for k in ('host_s', 'device_span_s', 'wall_s')),
           'all_rounds': rows, 'loop_against_batched': agree, 'batched_stages': table}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
