"""NumPy restatement of the rule of csrc/segmental.h: the float64 distance table, the forward recursion with its stay bits
and lowest-index minima, the backtrack; and two independent statements it is checked against on the host -- a brute force
over all k^T paths (the objective) and a textbook Viterbi with the full k x k transition matrix.

Everything is float64 with one rounding per operation, in the header's order: the table adds its terms j ascending from
0.0; ``min`` is exact, np.argmin returns the lowest index of the smallest value."""
import itertools

import numpy as np


def distances(z, W):
    """D (T, k) float64 of z (d, T) float32 and W (k, d) float32: sum_j ((double)z[j, t] - (double)W[c, j])^2, j ascending."""
    z, W = np.asarray(z), np.asarray(W)
    assert z.dtype == np.float32 and W.dtype == np.float32 and z.shape[0] == W.shape[1]
    z64, W64 = z.astype(np.float64), W.astype(np.float64)
    D = np.zeros((z.shape[1], W.shape[0]), np.float64)
    for j in range(z.shape[0]):
        diff = z64[j][:, None] - W64[:, j][None, :]
        D = D + diff * diff
    return D


def viterbi(D, lam):
    """(codes (T,) int32, n_seg, cost) of one utterance's table under one penalty: steps 2 and 3 of the rule."""
    D = np.asarray(D, np.float64)
    lam = np.float64(lam)
    T, k = D.shape
    V = D[0].copy()
    stay = np.ones((T, k), bool)
    a = np.zeros(T, np.int64)
    with np.errstate(over='ignore', invalid='ignore'):
        for t in range(1, T):
            a[t - 1] = int(np.argmin(V))
            sw = V[a[t - 1]] + lam
            stay[t] = V <= sw
            V = D[t] + np.where(stay[t], V, sw)
    codes = np.zeros(T, np.int32)
    codes[T - 1] = int(np.argmin(V))
    cost = V[codes[T - 1]]
    for t in range(T - 1, 0, -1):
        codes[t - 1] = codes[t] if stay[t, codes[t]] else a[t - 1]
    n_seg = 1 + int(np.count_nonzero(codes[1:] != codes[:-1]))
    return codes, n_seg, np.float64(cost)


def segment(latents, W, penalties):
    """The restated module: per penalty and utterance (codes, n_seg, cost), as result[p][i]."""
    tables = [distances(z, W) for z in latents]
    return [[viterbi(D, lam) for D in tables] for lam in np.asarray(penalties, np.float64).reshape(-1)]


def path_cost(D, path, lam):
    """The objective of one path, summed in path order: distortion + lam * changes of code."""
    path = np.asarray(path)
    return float(D[np.arange(len(path)), path].sum() + lam * np.count_nonzero(path[1:] != path[:-1]))


def brute_force(D, lam):
    """(best path, its objective) over all k^T paths; the first of equal bests in lexicographic order."""
    T, k = D.shape
    best, best_path = None, None
    for path in itertools.product(range(k), repeat=T):
        c = path_cost(D, path, lam)
        if best is None or c < best:
            best, best_path = c, path
    return np.array(best_path, np.int32), best


def viterbi_full(D, lam):
    """The textbook statement: V[t, c] = D[t, c] + min_c' (V[t - 1, c'] + lam [c' != c]) over the full k x k matrix,
    a tie between staying and switching going to staying, then to the lowest c'.  (codes, cost)."""
    D = np.asarray(D, np.float64)
    T, k = D.shape
    V = D[0].copy()
    back = np.zeros((T, k), np.int64)
    off_diagonal = np.float64(lam) * (1.0 - np.eye(k))
    for t in range(1, T):
        M = V[:, None] + off_diagonal                       # [c', c]
        best = M.min(axis=0)
        back[t] = np.where(np.diag(M) <= best, np.arange(k), M.argmin(axis=0))
        V = D[t] + best
    codes = np.zeros(T, np.int32)
    codes[T - 1] = int(np.argmin(V))
    for t in range(T - 1, 0, -1):
        codes[t - 1] = back[t, codes[t]]
    return codes, np.float64(V[codes[T - 1]])


def planted(k, d, runs, spacing, noise, seed):
    """Latents that are codebook rows in planted runs plus noise.  ``runs``: [(code, frames), ...].  The codebook rows are
    ``spacing`` apart along their own axis (row c is spacing * e_c, k <= d), the noise uniform in [-noise, noise] per
    component.  Returns (W (k, d) float32, z (d, T) float32, the planted codes (T,) int32)."""
    assert k <= d
    rs = np.random.RandomState(seed)
    W = np.zeros((k, d), np.float32)
    W[np.arange(k), np.arange(k)] = spacing
    want = np.concatenate([np.full(n, c, np.int32) for c, n in runs])
    z = W[want].T + rs.uniform(-noise, noise, (d, want.size))
    return W, np.ascontiguousarray(z, np.float32), want


# Integer-valued latents and a codebook with duplicated rows (1 repeats 0, 3 repeats 2): D is exact, so every tie is.  The
# host and the device tests share the case.
TIE_W = np.array([[1, 0], [1, 0], [3, 0], [3, 0], [1, 2]], np.float32)
TIE_Z = [np.array([[1, 3, 2, 2, 1, 1, 3], [0, 0, 0, 1, 1, 2, 0]], np.float32), np.array([[2], [0]], np.float32),
         np.array([[2, 2, 2, 0], [0, 0, 0, 0]], np.float32)]
