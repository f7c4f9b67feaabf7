"""The draw rule of the device-resident corpus (include/vqvae_corpus.h), restated independently of the package from the
header's text alone: plain Python integers, one draw at a time; Philox is tests/gen_rng_ref.block.  The reference of
tests/test_host_resident_corpus.py and tests/test_gpu_resident_corpus.py; it is pinned by the header's known answers.

  key      (seed & 0xffffffff, seed >> 32);  n = n_view
  d        iteration * global_batch + global_row;  e = d div n, p = d mod n
  q        p without shuffle, else pi(seed, e, p): n == 1 -> 0; w = max(2, bit_length(n - 1)) rounded up to even, h = w / 2,
           mask = 2^h - 1; from x = p repeat { (l, r) = (x >> h, x & mask); four rounds i = 0..3 of
           f = word0(Philox((r, i, e, 0x50455231))) & mask, (l, r) = (r, l ^ f); x = (l << h) | r } until x < n
  u        view[q] (q without a view);  count = length[u] - L1
  start    0 when count <= 0, else (v * count) >> 64 with v = (w0 << 32) | w1 of Philox((d & 0xffffffff, d >> 32, 0, 0x43524F31))
  row      x[i] = samples[offset[u] + start + i] when start + i < length[u], else 0.0;  x_enc = x;  bins of x: x_dec = bins[:-1],
           t = bins[1:];  speaker_out = speaker[u]
"""
import numpy as np

import gen_rng_ref as G

TAG_PERM = 0x50455231
TAG_CROP = 0x43524F31
M32 = 0xFFFFFFFF


def _key(seed):
    return (int(seed) & M32, int(seed) >> 32)


def width(n):
    """w: max(2, bit_length(n - 1)) rounded up to even."""
    w = max(2, (int(n) - 1).bit_length())
    return w + (w & 1)


def pi_walks(seed, e, p, n):
    """(pi(seed, e, p), the number of walks it took)."""
    n, p, e = int(n), int(p), int(e)
    assert 0 <= p < n and 0 <= e <= M32
    if n == 1:
        return 0, 0
    h = width(n) // 2
    mask = (1 << h) - 1
    key = _key(seed)
    x, walks = p, 0
    while True:
        l, r = x >> h, x & mask
        for i in range(4):
            f = G.block((r, i, e, TAG_PERM), key)[0] & mask
            l, r = r, l ^ f
        x = (l << h) | r
        walks += 1
        if x < n:
            return x, walks


def pi(seed, e, p, n):
    return pi_walks(seed, e, p, n)[0]


def start_of(seed, d, count):
    """The crop offset of draw d in an utterance with `count` = length - L1 (0 on the padding branch)."""
    d, count = int(d), int(count)
    if count <= 0:
        return 0
    w = G.block((d & M32, d >> 32, 0, TAG_CROP), _key(seed))
    return ((((w[0] << 32) | w[1]) * count) >> 64)


def draw(seed, d, lengths, L1, shuffle=True, view=None):
    """(u, start) of draw d."""
    n = len(lengths) if view is None else len(view)
    e, p = divmod(int(d), n)
    q = pi(seed, e, p, n) if shuffle else p
    u = q if view is None else int(view[q])
    return u, start_of(seed, d, int(lengths[u]) - int(L1))


def plan(seed, iteration, global_batch, lengths, L1, shuffle=True, view=None, rows=None):
    """The (u, start) rows of global batch `iteration`; `rows`: the global rows wanted (default: all of them)."""
    rows = range(global_batch) if rows is None else rows
    return [draw(seed, int(iteration) * int(global_batch) + int(g), lengths, L1, shuffle, view) for g in rows]


def batch(waves, speakers, rows, L1, quantize=256):
    """The four arrays of the (u, start) rows by slicing and zero padding: x_enc float32 (R, L1), x_dec int32 (R, L1 - 1),
    speaker int32 (R,), t int32 (R, L1 - 1).  The bins are the reference transform's (oracle MuLaw), not the thresholds'."""
    import vqvae_oracle as O
    x = np.zeros((len(rows), L1), np.float32)
    for j, (u, s) in enumerate(rows):
        piece = np.asarray(waves[u], np.float32)[s:s + L1]
        x[j, :len(piece)] = piece
    bins = O.MuLaw(quantize).transform(x).astype(np.int32)
    spk = np.array([speakers[u] for u, _ in rows], np.int32)
    return x, np.ascontiguousarray(bins[:, :-1]), spk, np.ascontiguousarray(bins[:, 1:])
