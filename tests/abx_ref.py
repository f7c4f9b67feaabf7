"""NumPy restatement of the rule of csrc/abx.h: the norms, the local cost under both metrics and from a table, the DTW
recurrence -- stated twice, row by row and by anti-diagonals -- and, for the host side of vqvae_amd.abx, the triples of
both tasks by brute force, their scores and the means.  A brute force over all monotone paths is the objective the
recurrence is checked against.

Everything is float64 with one rounding per operation, in the header's order: every sum adds its terms j ascending from
0.0; the candidates of a cell are tried diagonal, up, left and a later one wins only when strictly smaller."""
import numpy as np


# ---- steps 1 and 2 ---------------------------------------------------------------------------------------------------------------
def norms(x):
    """n (F,) float64 of x (D, F) float32: sum_j x[j, f]^2, j ascending."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    x64 = x.astype(np.float64)
    n = np.zeros(x.shape[1], np.float64)
    for j in range(x.shape[0]):
        n = n + x64[j] * x64[j]
    return n


def local(xa, xb, metric):
    """d (Fa, Fb) float64 of xa (D, Fa) and xb (D, Fb) float32."""
    xa, xb = np.asarray(xa), np.asarray(xb)
    assert xa.dtype == np.float32 and xb.dtype == np.float32 and xa.shape[0] == xb.shape[0]
    a64, b64 = xa.astype(np.float64), xb.astype(np.float64)
    acc = np.zeros((xa.shape[1], xb.shape[1]), np.float64)
    if metric == 'euclidean':
        for j in range(xa.shape[0]):
            diff = a64[j][:, None] - b64[j][None, :]
            acc = acc + diff * diff
        return np.sqrt(acc)
    assert metric == 'cosine'
    for j in range(xa.shape[0]):
        acc = acc + a64[j][:, None] * b64[j][None, :]
    q = norms(xa)[:, None] * norms(xb)[None, :]
    with np.errstate(divide='ignore', invalid='ignore'):
        d = 1.0 - acc / np.sqrt(q)
    d = np.where(d < 0.0, 0.0, d)
    return np.where(q == 0.0, 1.0, d)


def code_table(W, metric):
    """(k, k) float64: the dense rule over the rows of W (k, d) float32."""
    Wt = np.ascontiguousarray(np.asarray(W).T)
    return local(Wt, Wt, metric)


def local_codes(ca, cb, table):
    return np.asarray(table, np.float64)[np.asarray(ca)[:, None], np.asarray(cb)[None, :]]


# ---- step 3, twice -------------------------------------------------------------------------------------------------------------
def dtw_rows(d):
    """(cost, path_len) of a local-cost table (Fa, Fb), row by row."""
    d = np.asarray(d, np.float64)
    Fa, Fb = d.shape
    D = np.zeros((Fa, Fb), np.float64)
    K = np.zeros((Fa, Fb), np.int64)
    for i in range(Fa):
        for j in range(Fb):
            have, best, kb = False, 0.0, 0
            for ok, pi, pj in ((i > 0 and j > 0, i - 1, j - 1), (i > 0, i - 1, j), (j > 0, i, j - 1)):
                if ok and (not have or D[pi, pj] < best):
                    have, best, kb = True, D[pi, pj], K[pi, pj]
            D[i, j] = best + d[i, j] if have else d[i, j]
            K[i, j] = kb + 1
    return D[-1, -1], int(K[-1, -1])


def dtw_diagonals(d):
    """The same by anti-diagonals i + j = k, every diagonal at once from the two before it."""
    d = np.asarray(d, np.float64)
    Fa, Fb = d.shape
    D = np.full((Fa + 1, Fb + 1), np.inf)                      # a border that never wins: row and column 0
    K = np.zeros((Fa + 1, Fb + 1), np.int64)
    for k in range(Fa + Fb - 1):
        i = np.arange(max(0, k - (Fb - 1)), min(k, Fa - 1) + 1)
        j = k - i
        if k == 0:
            D[1, 1], K[1, 1] = d[0, 0], 1
            continue
        best, kb = D[i, j].copy(), K[i, j].copy()             # (i-1, j-1)
        have = (i > 0) & (j > 0)
        for ok, pi, pj in ((i > 0, i, j + 1), (j > 0, i + 1, j)):       # (i-1, j), (i, j-1) in the bordered arrays
            take = ok & (~have | (D[pi, pj] < best))
            best, kb = np.where(take, D[pi, pj], best), np.where(take, K[pi, pj], kb)
            have = have | ok
        D[i + 1, j + 1] = best + d[i, j]
        K[i + 1, j + 1] = kb + 1
    return D[Fa, Fb], int(K[Fa, Fb])


def dtw(d):
    """(distance, cost, path_len)."""
    cost, K = dtw_diagonals(d)
    return cost / np.float64(K), cost, K


def brute_force(d):
    """The smallest summed cost over all monotone paths (steps (1, 1), (1, 0), (0, 1)) from (0, 0) to the end."""
    d = np.asarray(d, np.float64)
    Fa, Fb = d.shape
    best = [np.inf]

    def walk(i, j, s):
        s = s + d[i, j]
        if i == Fa - 1 and j == Fb - 1:
            best[0] = min(best[0], s)
            return
        if i + 1 < Fa and j + 1 < Fb:
            walk(i + 1, j + 1, s)
        if i + 1 < Fa:
            walk(i + 1, j, s)
        if j + 1 < Fb:
            walk(i, j + 1, s)

    walk(0, 0, 0.0)
    return best[0]


def pair(xa, xb, metric):
    return dtw(local(xa, xb, metric))


# ---- the triples ----------------------------------------------------------------------------------------------------------------
def triples(label, speaker=None, context=None, across=False):
    """Every (A, B, X, group key) of the task, by brute force over all item triples."""
    M = len(label)
    spk = np.zeros(M, int) if speaker is None else np.asarray(speaker)
    ctx = np.zeros(M, int) if context is None else np.asarray(context)
    out = []
    for x in range(M):
        for a in range(M):
            for b in range(M):
                if a == x or label[a] != label[x] or label[b] == label[x] or spk[a] != spk[b]:
                    continue
                if not (ctx[a] == ctx[b] == ctx[x]):
                    continue
                if (spk[x] != spk[a]) != bool(across):
                    continue
                out.append((a, b, x, (int(label[x]), int(label[b]), int(ctx[x]), int(spk[a]), int(spk[x]))))
    return out


def scores(tri, distance):
    """(error, by_label_pair, {group key: (triples, errors, ties)}) from ``triples`` and distance(a, x) -> float64."""
    groups = {}
    for a, b, x, key in tri:
        n, e, t = groups.get(key, (0, 0, 0))
        dax, dbx = distance(a, x), distance(b, x)
        groups[key] = (n + 1, e + int(dax > dbx), t + int(dax == dbx))
    sums, counts = {}, {}
    for key in sorted(groups):
        n, e, t = groups[key]
        rate = np.float64(2 * e + t) / np.float64(2 * n)
        sums[key[:2]] = sums.get(key[:2], 0.0) + float(rate)
        counts[key[:2]] = counts.get(key[:2], 0) + 1
    by = dict((lp, sums[lp] / float(counts[lp])) for lp in sorted(sums))
    total = 0.0
    for lp in sorted(by):
        total = total + by[lp]
    return total / float(len(by)), by, groups


# ---- the constructed set ------------------------------------------------------------------------------------------------------
def constructed(noise, seed=0, d=16, labels=3, speakers=2, tokens=4):
    """3 labels x 2 speakers x 4 tokens of 3 to 8 frames over label prototypes: (features per item, one utterance each,
    label, speaker).  Every frame of an item is its label's prototype plus ``noise`` * randn."""
    rs = np.random.RandomState(seed)
    proto = rs.randn(labels, d)
    feats, label, speaker = [], [], []
    for lab in range(labels):
        for s in range(speakers):
            for t in range(tokens):
                F = int(rs.randint(3, 9))
                feats.append((proto[lab][:, None] + noise * rs.randn(d, F)).astype(np.float32))
                label.append(lab)
                speaker.append(s)
    return feats, np.array(label), np.array(speaker)
