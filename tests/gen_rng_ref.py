"""The uniforms of generation drawn on the device (include/vqvae_gen_rng.h), restated independently of the package: plain
Python integers, one block at a time, written from the header's definition.  The reference of tests/test_host_gen_rng.py
and tests/test_gpu_gen_rng.py; it is pinned by the two known answers of the header.

  Philox4x32-10, multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85
  round:   (c0, c1, c2, c3), (k0, k1) -> (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)); then the key advances
  key:     (seed low, seed high)         counter: (t, j >> 1, id low, id high)
  double:  words (a, b) = (w[2 (j & 1)], w[2 (j & 1) + 1]) -> ((a >> 5) * 2**26 + (b >> 6)) / 2**53
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def block(counter, key):
    """One Philox4x32-10 block: counter (4 words), key (2 words) -> 4 words, all Python ints."""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def to_double(a, b):
    """Two words -> the 53-bit double in [0, 1).  (a >> 5) * 2**26 + (b >> 6) < 2**53 is exact in an int and in a double."""
    return float((int(a) >> 5) * 67108864 + (int(b) >> 6)) / 9007199254740992.0


def uniform(seed, stream_id, t, j):
    w = block((t, j >> 1, stream_id & MASK, stream_id >> 32), (seed & MASK, seed >> 32))
    h = 2 * (j & 1)
    return to_double(w[h], w[h + 1])


def uniforms(seed, ids, steps, n_uniform=1, t0=0):
    """float64 (steps, len(ids), n_uniform): row s is step t0 + s, column q the stream ids[q]."""
    ids = [int(i) for i in ids]
    out = np.empty((steps, len(ids), n_uniform), np.float64)
    for s in range(steps):
        for q, sid in enumerate(ids):
            for j in range(n_uniform):
                out[s, q, j] = uniform(int(seed), sid, t0 + s, j)
    return out
