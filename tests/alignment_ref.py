"""The rule of include/vqvae_align.h restated in float64 NumPy, twice: ``dtw_loops`` is a plain double loop over the cells,
``dtw_diagonals`` the same recurrence an anti-diagonal at a time (what the larger shapes are checked with).  Both return
(cost, K, diagonal_steps, ia, ib).  ``cepstra`` and ``local_cost`` are steps 1 and 2, ``path_mae`` the along-path reduce
with the header's lane order, ``align`` the whole of a pair from its two float32 log-mel blocks.

NumPy's elementwise float64 +, -, *, / and sqrt round once each, as the device's do; nothing here calls a sum or a dot
whose order NumPy chooses."""
import numpy as np

C_DB = 4.3429448190325175          # 10 / ln 10, the constant of csrc/audio_metrics.hip
LANES = 256


def cepstra(log_mel, dct):
    """(F, n_mcep) float64: c[f, q] = sum_m (double)dct[q, m] * (double)log_mel[m, f], m ascending."""
    lm = np.asarray(log_mel, np.float32).astype(np.float64)
    dc = np.asarray(dct, np.float32).astype(np.float64)
    c = np.zeros((lm.shape[1], dc.shape[0]), np.float64)
    for m in range(lm.shape[0]):
        c = c + dc[:, m][None, :] * lm[m][:, None]
    return c


def local_cost(ca, cb):
    """(Fa, Fb) float64: d(i, j) = C * sqrt(2 * sum_q (0.5 * (ca[i, q] - cb[j, q]))^2), q ascending."""
    s = np.zeros((ca.shape[0], cb.shape[0]), np.float64)
    for q in range(ca.shape[1]):
        h = 0.5 * (ca[:, q][:, None] - cb[:, q][None, :])
        s = s + h * h
    return C_DB * np.sqrt(2.0 * s)


def backtrack(direction, K):
    Fa, Fb = direction.shape
    ia, ib = np.zeros(K, np.int32), np.zeros(K, np.int32)
    i, j = Fa - 1, Fb - 1
    for s in range(K):
        ia[K - 1 - s], ib[K - 1 - s] = i, j
        dr = direction[i, j]
        if dr == 0:
            i, j = i - 1, j - 1
        elif dr == 1:
            i -= 1
        elif dr == 2:
            j -= 1
        else:
            assert s == K - 1 and (i, j) == (0, 0)
    return ia, ib


def dtw_loops(d):
    """The recurrence cell by cell."""
    Fa, Fb = d.shape
    D = np.zeros((Fa, Fb), np.float64)
    K = np.zeros((Fa, Fb), np.int64)
    G = np.zeros((Fa, Fb), np.int64)
    direction = np.full((Fa, Fb), 3, np.int8)
    for i in range(Fa):
        for j in range(Fb):
            if i == 0 and j == 0:
                D[0, 0], K[0, 0] = d[0, 0], 1
                continue
            best, dr = None, 3
            if i > 0 and j > 0:
                best, dr = D[i - 1, j - 1], 0
            if i > 0 and (best is None or D[i - 1, j] < best):
                best, dr = D[i - 1, j], 1
            if j > 0 and (best is None or D[i, j - 1] < best):
                best, dr = D[i, j - 1], 2
            pi, pj = (i - 1, j - 1) if dr == 0 else (i - 1, j) if dr == 1 else (i, j - 1)
            D[i, j] = best + d[i, j]
            K[i, j] = K[pi, pj] + 1
            G[i, j] = G[pi, pj] + (1 if dr == 0 else 0)
            direction[i, j] = dr
    k = int(K[-1, -1])
    return (D[-1, -1], k, int(G[-1, -1])) + backtrack(direction, k)


def dtw_diagonals(d):
    """The recurrence an anti-diagonal i + j = k at a time; the cells of a diagonal read the two before it only."""
    Fa, Fb = d.shape
    D = np.zeros((Fa, Fb), np.float64)
    K = np.zeros((Fa, Fb), np.int64)
    G = np.zeros((Fa, Fb), np.int64)
    direction = np.full((Fa, Fb), 3, np.int8)
    D[0, 0], K[0, 0] = d[0, 0], 1
    for k in range(1, Fa + Fb - 1):
        i = np.arange(max(0, k - (Fb - 1)), min(k, Fa - 1) + 1)
        j = k - i
        iu, ju = np.maximum(i - 1, 0), np.maximum(j - 1, 0)
        has = (i > 0) & (j > 0)
        best = np.where(has, D[iu, ju], np.inf)
        dr = np.where(has, 0, 3)
        pi, pj = np.where(has, iu, i), np.where(has, ju, j)
        for code, ok, ci, cj in ((1, i > 0, iu, j), (2, j > 0, i, ju)):
            v = D[ci, cj]
            take = ok & ((dr == 3) | (v < best))
            best, dr = np.where(take, v, best), np.where(take, code, dr)
            pi, pj = np.where(take, ci, pi), np.where(take, cj, pj)
        D[i, j] = best + d[i, j]
        K[i, j] = K[pi, pj] + 1
        G[i, j] = G[pi, pj] + (dr == 0)
        direction[i, j] = dr
    kk = int(K[-1, -1])
    return (D[-1, -1], kk, int(G[-1, -1])) + backtrack(direction, kk)


def reduce_order(values, lanes=LANES):
    """Lane t adds elements t, t + lanes, ... in ascending order to 0.0, then s[k] += s[k + h] for h = lanes / 2 .. 1."""
    v = np.asarray(values, np.float64).reshape(-1)
    pad = (-v.size) % lanes
    rows = np.concatenate([v, np.zeros(pad, np.float64)]).reshape(-1, lanes)
    s = np.zeros(lanes, np.float64)
    for row in rows:
        s = s + row
    h = lanes // 2
    while h >= 1:
        s[:h] = s[:h] + s[h:2 * h]
        h //= 2
    return s[0]


def path_mae(log_mel_a, log_mel_b, ia, ib):
    """log_mel_mae_dtw: term k * n_mels + m is |la[m, ia[k]] - lb[m, ib[k]]| in float64."""
    la = np.asarray(log_mel_a, np.float32).astype(np.float64)
    lb = np.asarray(log_mel_b, np.float32).astype(np.float64)
    terms = np.abs(la[:, ia] - lb[:, ib]).T.reshape(-1)
    return reduce_order(terms) / np.float64(terms.size)


def path_sum(d, ia, ib):
    """d summed along the path in ascending order, as the recurrence adds it."""
    s = d[ia[0], ib[0]]
    for i, j in zip(ia[1:], ib[1:]):
        s = s + d[i, j]
    return s


def align(log_mel_a, log_mel_b, dct, dtw=dtw_diagonals):
    """dict of every quantity of a pair."""
    d = local_cost(cepstra(log_mel_a, dct), cepstra(log_mel_b, dct))
    cost, K, G, ia, ib = dtw(d)
    return dict(cost=cost, path_len=K, diagonal_steps=G, ia=ia, ib=ib, mcd_dtw_db=cost / np.float64(K),
                log_mel_mae_dtw=path_mae(log_mel_a, log_mel_b, ia, ib), d=d)


def tie_break_path(Fa, Fb):
    """The path when every candidate ties (all local costs equal): every cell with a diagonal predecessor chooses it, so
    the walk back from (Fa - 1, Fb - 1) is diagonal while possible and then runs along the remaining side to (0, 0).
    Written ascending, the path first stays on frame 0 of the shorter side for |Fa - Fb| steps and is diagonal after:
    Fa < Fb: (0, 0), (0, 1) .. (0, Fb - Fa), (1, Fb - Fa + 1) .. (Fa - 1, Fb - 1);
    Fa > Fb: (0, 0), (1, 0) .. (Fa - Fb, 0), (Fa - Fb + 1, 1) .. (Fa - 1, Fb - 1).  K = max(Fa, Fb), min(Fa, Fb) - 1 diagonal steps."""
    n, extra = min(Fa, Fb), abs(Fa - Fb)
    along, held = list(range(max(Fa, Fb))), [0] * extra + list(range(n))
    ia, ib = (held, along) if Fa <= Fb else (along, held)
    return np.array(ia, np.int32), np.array(ib, np.int32)
