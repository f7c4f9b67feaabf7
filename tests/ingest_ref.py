"""NumPy restatement of the ingest rule of include/vqvae_ingest.h, written from the header and independent of
vqvae_amd/ingest.py: decode to mono, the tap table, the resampler, the frame energies in the rule's order, the silence
bounds, the peak and the normalisation.  Every sum is accumulated in float64 in the order the header gives."""
from fractions import Fraction

import numpy as np

F, H, AMIN = 2048, 512, 1e-10
FILTERS = {'kaiser_fast': (16, 0.85, 8.555504641634386), 'kaiser_best': (64, 0.9475937167399596, 14.769656459379492)}


def ratio(sr_in, sr_out, res_type='kaiser_fast'):
    """(L, M, J)"""
    Z = (FILTERS[res_type] if isinstance(res_type, str) else res_type)[0]
    f = Fraction(sr_out, sr_in)
    L, M = f.numerator, f.denominator
    if L == M:
        return 1, 1, 1
    J = Z
    while J * min(L, M) < Z * M:         # the smallest integer with J * s >= Z, s = min(1, L / M)
        J += 1
    return L, M, J


def taps(sr_in, sr_out, res_type='kaiser_fast'):
    """float32 (L, 2J), row p, column j + J - 1"""
    Z, rho, beta = FILTERS[res_type] if isinstance(res_type, str) else res_type
    L, M, J = ratio(sr_in, sr_out, res_type)
    s = min(1.0, L / M)
    out = np.zeros((L, 2 * J), np.float32)
    js = np.arange(-J + 1, J + 1).astype(np.float64)
    for p in range(L):
        u = s * (np.float64(p) / np.float64(L) - js)
        v = u / Z
        w = np.zeros_like(u)
        ok = np.abs(v) < 1
        w[ok] = np.i0(beta * np.sqrt(1 - v[ok] * v[ok])) / np.i0(beta)
        out[p] = (((s * rho) * np.sinc(rho * u)) * w).astype(np.float32)
    return out


def mono(raw):
    """float32 (frames,) of int16 / float32 (frames, channels) or (frames,)"""
    raw = np.asarray(raw)
    raw = raw[:, None] if raw.ndim == 1 else raw
    x = raw.astype(np.float64) / 32768.0 if raw.dtype == np.int16 else raw.astype(np.float32).astype(np.float64)
    acc = np.zeros(raw.shape[0], np.float64)
    for c in range(raw.shape[1]):
        acc = acc + x[:, c]
    return (acc / np.float64(raw.shape[1])).astype(np.float32)


def n_out_of(n_in, L, M):
    return -((-int(n_in) * L) // M)


def resample(x, h, L, M, J):
    """x float32 mono; h the table"""
    x = np.asarray(x, np.float32)
    if L == M:
        return x.copy()
    n_out = n_out_of(len(x), L, M)
    o = np.arange(n_out, dtype=np.int64)
    q, p = (o * M) // L, (o * M) % L
    padded = np.concatenate((np.zeros(J, np.float64), x.astype(np.float64), np.zeros(J + 1, np.float64)))
    hd = h.astype(np.float64)
    acc = np.zeros(n_out, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for col in range(2 * J):                   # j = col - J + 1, ascending: x[q + j] sits at padded[q + j + J]
            acc = acc + padded[q + col + 1] * hd[p, col]
        return acc.astype(np.float32)


def frame_energies(y):
    y = np.asarray(y, np.float32)
    n = len(y)
    assert n >= F // 2 + 1
    nf = 1 + n // H
    i = np.arange(nf, dtype=np.int64)[:, None] * H + np.arange(F, dtype=np.int64)[None, :] - F // 2
    i = np.where(i < 0, -i, i)
    i = np.where(i >= n, 2 * (n - 1) - i, i)
    with np.errstate(invalid='ignore', over='ignore'):
        v = y[i].astype(np.float64)
        sq = (v * v).reshape(nf, F // 64, 64)      # sample m = l + 64 r sits at [r, l]
        a = np.zeros((nf, 64), np.float64)
        for r in range(F // 64):
            a = a + sq[:, r, :]
        stride = 32
        while stride >= 1:
            a[:, :stride] = a[:, :stride] + a[:, stride:2 * stride]
            stride //= 2
    return a[:, 0].copy()


def bounds(y, r):
    """(start, end, peak float32, status)"""
    y = np.asarray(y, np.float32)
    n = len(y)
    if not np.isfinite(y).all():
        return 0, n, np.float32(0), 1
    mse = frame_energies(y) / np.float64(F)
    floored = np.maximum(AMIN, mse)
    ref = max(AMIN, float(mse.max()))
    loud = np.nonzero(floored > ref * r)[0]
    if loud.size == 0:
        return 0, 0, np.float32(0), 4 | 2
    start, end = H * int(loud[0]), min(n, H * (int(loud[-1]) + 1))
    peak = np.abs(y[start:end]).max() if end > start else np.float32(0)
    return start, end, np.float32(peak), (4 if end <= start else 0) | (2 if peak == 0 else 0)


def top_db_ratio(top_db):
    return 10.0 ** (-top_db / 10.0)


def normalise(y, start, end, peak):
    return (y[start:end] / np.float32(peak)).astype(np.float32)


def resampled(raw, sr_in, sr_out=16000, res_type='kaiser_fast'):
    L, M, J = ratio(sr_in, sr_out, res_type)
    return resample(mono(raw), taps(sr_in, sr_out, res_type) if L != M else None, L, M, J)


def process(raw, sr_in, sr_out=16000, res_type='kaiser_fast', top_db=20):
    """The whole rule for one utterance: (wave float32, status)"""
    y = resampled(raw, sr_in, sr_out, res_type)
    start, end, peak, status = bounds(y, top_db_ratio(top_db))
    if status:
        return None, status
    return normalise(y, start, end, peak), 0
