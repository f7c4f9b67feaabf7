"""NumPy restatement of the codebook's k-means initialisation (include/vqvae_kmeans.h) for tests/test_host_vq_kmeans.py and
tests/test_gpu_vq_kmeans.py: the hash, the float32 distance in the exact search's order, the float64 summation tree and the
walk down it, the seeding, the centroid update and the inertia, every one bit for bit what the kernels must produce."""
import numpy as np

BLOCK = 256
M64 = (1 << 64) - 1


def hash64(seed, word, j):
    """x of the header's hash for counter (word, j); j may be an array.  uint64 arithmetic wraps."""
    with np.errstate(over='ignore'):
        ctr = (np.uint64(int(word) & 0xFFFFFFFF) << np.uint64(32)) | (np.asarray(j, np.uint64) & np.uint64(0xFFFFFFFF))
        x = np.uint64(int(seed) & M64) + (ctr + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return x


def uniform(x):
    """u of the header: the top 24 bits of x, exact in float64."""
    return np.float64(int(x) >> 40) * np.float64(2.0 ** -24)


def dist(pool, c):
    """pool (d, N) float32, c (d,) float32 or (d, N) (a centre per row) -> (N,) float32: sequential over the channels,
    sub, mul and add each rounded to float32."""
    pool = np.asarray(pool, np.float32)
    c = np.asarray(c, np.float32)
    acc = np.zeros(pool.shape[1], np.float32)
    for ch in range(pool.shape[0]):
        df = (pool[ch] - c[ch]).astype(np.float32)
        acc = (acc + (df * df).astype(np.float32)).astype(np.float32)
    return acc


def tree(values):
    """The levels of the summation tree over `values` padded with +0 to a power of two: levels[0] the leaves (float64),
    levels[-1] the root."""
    v = np.asarray(values, np.float32).astype(np.float64)
    P = 1
    while P < v.size:
        P *= 2
    lv = np.zeros(P, np.float64)
    lv[:v.size] = v
    levels = [lv]
    while lv.size > 1:
        lv = lv[0::2] + lv[1::2]
        levels.append(lv)
    return levels


def tree_sum(values):
    return tree(values)[-1][0]


def descend(levels, t):
    """The walk of the header from the root with target t; returns the leaf."""
    i = 0
    for lv in levels[-2::-1]:
        L, R = lv[2 * i], lv[2 * i + 1]
        if t < L or not R > 0.0:
            i = 2 * i
        else:
            t = t - L
            i = 2 * i + 1
    return i


def seed(pool, k, seed_):
    """(W (k, d), rows (k,) int32, mind (N,) float32, totals: the tree's root of every round j >= 1)."""
    pool = np.asarray(pool, np.float32)
    d, N = pool.shape
    rows = np.zeros(k, np.int32)
    D = np.full(N, np.inf, np.float32)
    totals = []
    for j in range(k):
        x = hash64(seed_, 0, j)
        row = int(x % np.uint64(N))
        if j > 0:
            levels = tree(D)
            total = levels[-1][0]
            totals.append(total)
            if total > 0.0:
                row = descend(levels, uniform(x) * total)
        rows[j] = row
        D = np.minimum(D, dist(pool, pool[:, row]))
    return np.ascontiguousarray(pool[:, rows].T), rows, D, totals


def update(pool, n, S, seed_, it):
    """(W (k, d), number of empty codes) from the counts n (k,) and sums S (k, d) of vq_ema_ref.accumulate."""
    pool = np.asarray(pool, np.float32)
    N = pool.shape[1]
    n = np.asarray(n, np.float32)
    S = np.asarray(S, np.float32)
    k = n.size
    W = np.zeros(S.shape, np.float32)
    live = n > 0
    W[live] = (S[live] / n[live, None]).astype(np.float32)
    rows = (hash64(seed_, it + 1, np.arange(k)) % np.uint64(N)).astype(np.int64)
    W[~live] = pool[:, rows[~live]].T
    return W, int((~live).sum())


def inertia(pool, W, idx):
    pool = np.asarray(pool, np.float32)
    idx = np.asarray(idx).reshape(-1)
    k = W.shape[0]
    ok = (idx >= 0) & (idx < k)
    D = dist(pool, np.asarray(W, np.float32)[np.where(ok, idx, 0)].T)
    return tree_sum(np.where(ok, D, np.float32(0)))


def argmin_exact(pool, W):
    """numpy.argmin over the float32 distances in the search's order (first minimum wins): what vqvae_vq_nearest_fwd
    returns."""
    D = np.stack([dist(pool, w) for w in np.asarray(W, np.float32)])
    return D.argmin(0).astype(np.int32)
