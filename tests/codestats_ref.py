"""The rule of include/vqvae_codes.h restated in NumPy: ``runs`` and ``run_hist``; the counts twice, ``counts_loops`` by plain
loops over the positions and ``counts_add_at`` by np.add.at; the edit distance twice, ``edit_loops`` cell by cell over the
whole (La + 1) x (Lb + 1) matrix and ``edit_diagonals`` an anti-diagonal at a time keeping three diagonals only (what the
larger shapes are checked with); ``agreement``; and the derived figures of vqvae_amd.codestats.figures written again from
their definitions, term by term with math.log2.  Everything up to the figures is integer work: there is no tolerance."""
import math

import numpy as np


# ---- runs ---------------------------------------------------------------------------------------------------------------
def runs(c):
    """(u, dur) int32 of one utterance's codes: a run starts at 0 and wherever c[t] != c[t-1]."""
    c = np.asarray(c).reshape(-1)
    u, dur = [], []
    for t in range(len(c)):
        if t == 0 or c[t] != c[t - 1]:
            u.append(int(c[t]))
            dur.append(1)
        else:
            dur[-1] += 1
    return np.array(u, np.int32), np.array(dur, np.int32)


def run_hist(durations, max_run):
    """(max_run,) int64 over the durations of a whole list: a run of length L counts in bucket min(L, max_run) - 1."""
    h = np.zeros(max_run, np.int64)
    for d in durations:
        for L in np.asarray(d).reshape(-1):
            h[min(int(L), max_run) - 1] += 1
    return h


# ---- counts -------------------------------------------------------------------------------------------------------------
def counts_loops(utts, groups, k, G, bigrams=True):
    """(uni (G, k), big (k, k) or None, invalid) by plain loops.  A code outside [0, k) adds to invalid only and drops its
    two transitions; a group outside [0, G) makes the whole utterance invalid positions."""
    uni, big, invalid = np.zeros((G, k), np.int64), np.zeros((k, k), np.int64) if bigrams else None, 0
    for c, g in zip(utts, groups):
        c = [int(x) for x in np.asarray(c).reshape(-1)]
        if not 0 <= g < G:
            invalid += len(c)
            continue
        for t, x in enumerate(c):
            if not 0 <= x < k:
                invalid += 1
                continue
            uni[g, x] += 1
            if bigrams and t + 1 < len(c) and 0 <= c[t + 1] < k:
                big[x, c[t + 1]] += 1
    return uni, big, invalid


def counts_add_at(utts, groups, k, G, bigrams=True):
    """The same tables by np.add.at over whole utterances."""
    uni, big, invalid = np.zeros((G, k), np.int64), np.zeros((k, k), np.int64) if bigrams else None, 0
    for c, g in zip(utts, groups):
        c = np.asarray(c, np.int64).reshape(-1)
        if not 0 <= g < G:
            invalid += c.size
            continue
        ok = (c >= 0) & (c < k)
        invalid += int((~ok).sum())
        np.add.at(uni[g], c[ok], 1)
        if bigrams:
            both = ok[:-1] & ok[1:]
            np.add.at(big, (c[:-1][both], c[1:][both]), 1)
    return uni, big, invalid


# ---- the edit distance ----------------------------------------------------------------------------------------------------
def edit_loops(a, b):
    """(dist, subs) cell by cell: diagonal, step along a, step along b, a later candidate only when strictly smaller."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    La, Lb = len(a), len(b)
    D = np.zeros((La + 1, Lb + 1), np.int64)
    S = np.zeros((La + 1, Lb + 1), np.int64)
    D[:, 0] = np.arange(La + 1)
    D[0, :] = np.arange(Lb + 1)
    for i in range(1, La + 1):
        for j in range(1, Lb + 1):
            ne = int(a[i - 1] != b[j - 1])
            d, s = D[i - 1, j - 1] + ne, S[i - 1, j - 1] + ne
            if D[i - 1, j] + 1 < d:
                d, s = D[i - 1, j] + 1, S[i - 1, j]
            if D[i, j - 1] + 1 < d:
                d, s = D[i, j - 1] + 1, S[i, j - 1]
            D[i, j], S[i, j] = d, s
    return int(D[La, Lb]), int(S[La, Lb])


def edit_diagonals(a, b):
    """The same recurrence an anti-diagonal i + j = k of the whole matrix at a time; three diagonals are kept, indexed
    by i.  The cells of a diagonal read the two before it only."""
    a, b = np.asarray(a, np.int64).reshape(-1), np.asarray(b, np.int64).reshape(-1)
    La, Lb = len(a), len(b)
    D = [np.zeros(La + 1, np.int64) for _ in range(3)]
    S = [np.zeros(La + 1, np.int64) for _ in range(3)]
    for k in range(La + Lb + 1):
        Dc, Dp, Dq = D[k % 3], D[(k - 1) % 3], D[(k - 2) % 3]
        Sc, Sp, Sq = S[k % 3], S[(k - 1) % 3], S[(k - 2) % 3]
        lo, hi = max(0, k - Lb), min(k, La)
        if lo == 0:
            Dc[0], Sc[0] = k, 0                               # D(0, j) = j
        if hi == k:
            Dc[k], Sc[k] = k, 0                               # D(i, 0) = i
        i0, i1 = max(lo, 1), min(hi, k - 1)                   # the cells with i > 0 and j > 0
        if i0 > i1:
            continue
        ne = (a[i0 - 1:i1] != b[k - i1 - 1:k - i0][::-1]).astype(np.int64)        # a[i - 1] against b[k - i - 1]
        d, s = Dq[i0 - 1:i1] + ne, Sq[i0 - 1:i1] + ne
        for Dn, Sn in ((Dp[i0 - 1:i1], Sp[i0 - 1:i1]), (Dp[i0:i1 + 1], Sp[i0:i1 + 1])):     # (i - 1, j), then (i, j - 1)
            take = Dn + 1 < d
            d, s = np.where(take, Dn + 1, d), np.where(take, Sn, s)
        Dc[i0:i1 + 1], Sc[i0:i1 + 1] = d, s
    return int(D[(La + Lb) % 3][La]), int(S[(La + Lb) % 3][La])


def derive(dist, subs, La, Lb):
    """(dels, ins, matches) from the two outputs: both divisions are exact."""
    assert (dist - subs + La - Lb) % 2 == 0 and (dist - subs - La + Lb) % 2 == 0
    dels, ins = (dist - subs + La - Lb) // 2, (dist - subs - La + Lb) // 2
    return dels, ins, La - dels - subs


def agreement(a, b):
    """(agree, overlap) over the raw codes."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    n = min(len(a), len(b))
    return int((a[:n] == b[:n]).sum()), n


# ---- the derived figures, from their definitions ---------------------------------------------------------------------------
def _entropy(counts):
    n = float(sum(counts))
    return -sum((c / n) * math.log2(c / n) for c in counts if c > 0)


def entropy_bits(uni):
    return _entropy([int(x) for x in np.asarray(uni).sum(axis=0)])


def mi_bits(uni):
    uni = np.asarray(uni, np.int64)
    n_g, n_c, n = uni.sum(axis=1), uni.sum(axis=0), int(uni.sum())
    return sum((int(uni[g, c]) / n) * math.log2(int(uni[g, c]) * n / (int(n_g[g]) * int(n_c[c])))
               for g in range(uni.shape[0]) for c in range(uni.shape[1]) if uni[g, c] > 0)


def speaker_entropy_bits(uni):
    return _entropy([int(x) for x in np.asarray(uni).sum(axis=1)])


def js_bits(uni):
    uni = np.asarray(uni, np.int64)
    G, k = uni.shape
    out = np.full((G, G), np.nan)
    for g in range(G):
        for h in range(G):
            ng, nh = int(uni[g].sum()), int(uni[h].sum())
            if ng == 0 or nh == 0:
                continue
            t = 0.0
            for c in range(k):
                p, q = int(uni[g, c]) / ng, int(uni[h, c]) / nh
                m = 0.5 * (p + q)
                if p > 0:
                    t += 0.5 * p * math.log2(p / m)
                if q > 0:
                    t += 0.5 * q * math.log2(q / m)
            out[g, h] = t
    return out


def self_share(big):
    big = np.asarray(big, np.int64)
    return int(np.trace(big)) / int(big.sum())


def next_entropy_bits(big):
    """H(c' | c) = - sum p(c, c') log2 p(c' | c)."""
    big = np.asarray(big, np.int64)
    T = int(big.sum())
    return -sum((int(big[c, d]) / T) * math.log2(int(big[c, d]) / int(big[c].sum()))
                for c in range(big.shape[0]) for d in range(big.shape[1]) if big[c, d] > 0)
