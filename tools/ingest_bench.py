"""Corpus ingest on the device (vqvae_amd.ingest, include/vqvae_ingest.h): raw 48 kHz int16 audio in host memory to a
ResidentCorpus at 16 kHz, resampled (kaiser_fast), silence-trimmed and peak-normalised by three launches per batch.
usage: python tools/ingest_bench.py [--rounds 3] [--utterances 2000] [--seed 0] [--batch-mib 64] [--res-type kaiser_fast]
  Corpus: synthetic, --utterances waveforms whose lengths follow the gamma law of tools/resident_corpus_bench.py (shape 2,
  mean 3.6 s, clipped to 1-10 s), at 48 kHz, int16 mono, three sinusoids and a little noise between 0.15 s of faint noise
  at both ends (so the trim has something to cut); about 2 hours, 0.7 GB of raw audio.
  Per round: ResidentCorpus.from_arrays end to end (wall clock, arrays already in host memory: no file is read), and per
  batch, between device events, the host-to-device copy of the raw audio and the resample, bounds (two kernels) and pack
  launches.  Ranges over the rounds are printed, not means.  The one condition: in every batch the three launches together
  take less device time than that batch's host-to-device copy.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-vq-vae_amd'))


def corpus_lengths(n, seed, rate):
    rs = np.random.RandomState(seed)
    return (np.clip(rs.gamma(2.0, 1.8, n), 1.0, 10.0) * rate).astype(np.int64)


def synthetic_raws(lengths, seed, rate):
    rs = np.random.RandomState(seed)
    edge = int(0.15 * rate)
    out = []
    for n in lengths:
        t = np.arange(n, dtype=np.float32) / np.float32(rate)
        f, ph, a = rs.uniform(80, 4000, 3), rs.uniform(0, 2 * np.pi, 3), rs.uniform(0.05, 0.3, 3)
        w = sum(np.float32(a[i]) * np.sin(np.float32(2 * np.pi * f[i]) * t + np.float32(ph[i])) for i in range(3))
        w[:edge] = 0
        w[n - edge:] = 0
        w += np.float32(1e-3) * rs.standard_normal(n).astype(np.float32)
        out.append(np.clip(np.round(w * 32768), -32768, 32767).astype(np.int16))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--utterances', type=int, default=2000)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--batch-mib', type=int, default=64)
    ap.add_argument('--res-type', default='kaiser_fast')
    ap.add_argument('--sr-in', type=int, default=48000)
    a = ap.parse_args()
    import vqvae_amd as V
    from vqvae_amd import backend
    from vqvae_amd import ingest as G
    backend.init(0)
    lengths = corpus_lengths(a.utterances, a.seed, float(a.sr_in))
    raws = synthetic_raws(lengths, a.seed + 2, a.sr_in)
    speakers = np.random.RandomState(a.seed + 1).randint(0, 100, a.utterances)
    raw_bytes = int(sum(r.nbytes for r in raws))
    hours_in = float(lengths.sum()) / a.sr_in / 3600.0

    # from_arrays with the front end's event timing switched on
    rounds = []
    for _ in range(a.rounds + 1):                       # the first round warms the pool, the page-locked buffer and the code objects
        front = G.DeviceIngest(16000, a.res_type, 20)
        front.timings = timings = []
        backend.synchronize()
        t0 = time.perf_counter()
        items = [G._Array(raw, a.sr_in, 'wave %d' % i) for i, raw in enumerate(raws)]      # what from_arrays does
        corpus = V.ResidentCorpus._from_items(items, speakers, front, a.batch_mib << 20, False, lambda i: i)
        backend.synchronize()
        wall = time.perf_counter() - t0
        launches = [t['resample'] + t['bounds'] + t['pack'] for t in timings]
        rounds.append({'wall_s': wall, 'hours_per_s': hours_in / wall, 'batches': len(timings),
                       'h2d_ms': sum(t['h2d'] for t in timings), 'resample_ms': sum(t['resample'] for t in timings),
                       'bounds_ms': sum(t['bounds'] for t in timings), 'pack_ms': sum(t['pack'] for t in timings),
                       'h2d_gb_per_s': [round(1e-6 * t['h2d_bytes'] / t['h2d'], 2) for t in timings],
                       'launches_over_h2d_per_batch': [round(l / t['h2d'], 4) for l, t in zip(launches, timings)],
                       'smallest_batch': min(({'bytes': t['h2d_bytes'], 'utterances': t['utterances'], 'h2d_ms': round(t['h2d'], 4),
                                               'resample_ms': round(t['resample'], 4), 'bounds_ms': round(t['bounds'], 4),
                                               'pack_ms': round(t['pack'], 4)} for t in timings), key=lambda d: d['bytes']),
                       'launches_below_h2d_in_every_batch': bool(all(l < t['h2d'] for l, t in zip(launches, timings)))})
        kept_hours, n_kept, skipped = corpus.hours(16000), len(corpus), len(corpus.skipped)
        del corpus
    rounds = rounds[1:]

    def rng(key):
        v = [r[key] for r in rounds]
        return [round(float(min(v)), 4), round(float(max(v)), 4)]
    out = {'tool': 'ingest_bench', 'rounds': a.rounds, 'utterances': a.utterances, 'sr_in': a.sr_in, 'res_type': a.res_type,
           'raw_bytes': raw_bytes, 'hours_in': round(hours_in, 4), 'hours_kept': round(kept_hours, 4), 'kept': n_kept,
           'skipped': skipped, 'batch_mib': a.batch_mib,
           'wall_s': rng('wall_s'), 'hours_of_audio_per_s': rng('hours_per_s'), 'h2d_ms': rng('h2d_ms'),
           'resample_ms': rng('resample_ms'), 'bounds_ms': rng('bounds_ms'), 'pack_ms': rng('pack_ms'),
           'launches_below_h2d_in_every_batch': bool(all(r['launches_below_h2d_in_every_batch'] for r in rounds)),
           'all_rounds': rounds}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
