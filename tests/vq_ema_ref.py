"""NumPy restatement of the EMA codebook rule (include/vqvae_vq_ema.h) for tests/test_host_vq_ema.py and
tests/test_gpu_vq_ema.py: the statistics in the header's summation order (bit-exact) and as a plain float64 sum, and the
update itself with every float32 operation rounded on its own."""
import numpy as np

PIECE = 512


def rows_of(z):
    """z (B, d, T) -> (B*T, d): row n is z[n // T, :, n % T]."""
    z = np.asarray(z)
    B, d, T = z.shape[:3]
    return np.ascontiguousarray(z.reshape(B, d, T).transpose(0, 2, 1).reshape(B * T, d))


def _piece_sum(rows):
    """(len <= PIECE, d) float32 -> (d,) float64 in the order of one wave: lane l adds entries l, l + 64, ...; the 64
    lane sums are folded 32, 16, ..., 1."""
    n, d = rows.shape
    pad = np.zeros((PIECE, d), np.float64)
    pad[:n] = rows
    lanes = np.zeros((64, d), np.float64)
    for i in range(PIECE // 64):
        lanes = lanes + pad[i * 64:(i + 1) * 64]
    h = 32
    while h:
        lanes = lanes[:h] + lanes[h:2 * h]
        h >>= 1
    return lanes[0]


def accumulate(idx, z, k, ordered=True):
    """(n float32 (k), S float32 (k, d)).  ordered: the header's order (what the kernels must reproduce bit for bit);
    otherwise float32(plain float64 sum)."""
    r = rows_of(z)
    flat = np.asarray(idx).reshape(-1)
    d = r.shape[1]
    n = np.zeros(k, np.float32)
    S = np.zeros((k, d), np.float32)
    order = np.argsort(flat, kind='stable')
    sorted_idx = flat[order]
    lo = np.searchsorted(sorted_idx, np.arange(k), 'left')
    hi = np.searchsorted(sorted_idx, np.arange(k), 'right')
    for j in np.nonzero(hi > lo)[0]:
        mine = r[order[lo[j]:hi[j]]]                 # ascending rows (stable sort)
        n[j] = mine.shape[0]
        if ordered:
            tot = np.zeros(d, np.float64)
            for p0 in range(0, mine.shape[0], PIECE):
                tot = tot + _piece_sum(mine[p0:p0 + PIECE])
        else:
            tot = mine.astype(np.float64).sum(0)
        S[j] = tot.astype(np.float32)
    return n, S


def stats_of(n, S):
    return np.concatenate([np.asarray(n, np.float32).reshape(-1), np.asarray(S, np.float32).reshape(-1)])


def apply(W, N, m, n, S, decay, eps):
    """One application of the rule; returns new (W, N, m), float32."""
    f = np.float32
    decay, k = f(decay), N.shape[0]
    w1 = f(1.0) - decay
    N = (decay * N.astype(f)).astype(f) + (w1 * n.astype(f)).astype(f)
    m = (decay * m.astype(f)).astype(f) + (w1 * S.astype(f)).astype(f)
    total = np.float64(0.0)
    for v in N.astype(np.float64):
        total = total + v
    if total == 0.0:
        return W.copy(), N, m
    eps64 = np.float64(f(eps))
    with np.errstate(all='ignore'):
        Nt = ((N.astype(np.float64) + eps64) / (total + np.float64(k) * eps64) * total).astype(f)
        W = (m / Nt[:, None]).astype(f)
    return W, N, m
