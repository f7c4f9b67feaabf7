"""NumPy restatement of the summation order of include/vqvae_optim.h (the optimizer hooks' norm pass and finalise
launch), the way tests/vq_kmeans_ref.py restates the k-means tree.  Every operation below is one IEEE float64
operation in the order the header states; the device kernels must give the same bits.

    chunk [s, e) of the arena, q0 = s // 4:  lane t takes the aligned quads q0 + t, q0 + t + 256, ... in order and the
    elements of a quad in ascending order, elements outside [s, e) counting +0;  the 256 lane sums are folded in
    halves (h = 128 .. 1: v[t] += v[t + h]);  S_p adds a parameter's chunk partials in ascending order;  S adds the
    S_p in layout order;  a group adds its members' S_p in the order given.
"""
import numpy as np

CHUNK = 4096
THREADS = 256


def chunks_of(sizes, chunk=CHUNK):
    """[(parameter index, start, length)] in table order, from the sizes alone."""
    out, off = [], 0
    for p, size in enumerate(sizes):
        for s in range(0, int(size), chunk):
            out.append((p, off + s, min(chunk, int(size) - s)))
        off += int(size)
    return out


def chunk_partial(g, s, e):
    """The partial of chunk [s, e) of the float32 arena ``g``."""
    q0 = s // 4
    q1 = (e + 3) // 4
    rows = -(-(q1 - q0) // THREADS)
    sq = np.zeros(rows * THREADS * 4, np.float64)
    lo = q0 * 4
    x = g[s:e].astype(np.float64)
    sq[s - lo:e - lo] = x * x                      # exact: 48 bits; everything else stays +0
    sq = sq.reshape(rows, THREADS, 4)
    acc = np.zeros(THREADS, np.float64)
    for r in range(rows):
        for k in range(4):
            acc = acc + sq[r, :, k]
    h = THREADS // 2
    while h >= 1:
        acc = acc[:h] + acc[h:2 * h]
        h //= 2
    return acc[0]


def param_sumsq(g, sizes):
    """S_p for every parameter, float64 (n_params)."""
    g = np.ascontiguousarray(g, np.float32).reshape(-1)
    out = np.zeros(len(sizes), np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        for p, s, n in chunks_of(sizes):
            out[p] = out[p] + chunk_partial(g, s, s + n)
    return out


def total(sp):
    S = np.float64(0.0)
    with np.errstate(over='ignore', invalid='ignore'):
        for v in sp:
            S = S + v
    return S


def finalise(sp, threshold=np.inf, groups=()):
    """The state block's fields from the S_p: dict(S, norm, rate, scale, nonfinite, group_norms)."""
    S = total(sp)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        norm = np.sqrt(S)
        rate = np.float64(threshold) / norm
        scale = np.float32(rate) if rate < 1.0 else np.float32(1.0)
        gn = np.asarray([np.float32(np.sqrt(total(sp[list(m)]))) for m in groups], np.float32)
    return {'S': S, 'norm': norm, 'rate': rate, 'scale': scale, 'nonfinite': int(not np.isfinite(S)),
            'group_norms': gn}
