"""NumPy restatements for the audio metrics (include/vqvae_metrics.h, vqvae_amd.metrics); nothing here imports the package.

``features``         the rule of the header in float64 (or, with dtype=float32, a plain float32 NumPy evaluation of it),
                     run on the float32 tables.
``distances_exact``  the distance kernel's arithmetic in its own order, fed the float32 log_mel / mag it is given: equal
                     to the device in every bit.
``distances``        the three formulas in float64 from float64 features, any order (np.sum).
``plan_chunks``      the greedy chunk planner, written as a plain loop.
``utterance_list``   the utterance list of tests/test_gpu_metrics.py.
"""
import numpy as np

THREADS = 256
DB = 4.3429448190325175           # 10 / ln 10, the header's double


def frame_count(length, n_fft, hop):
    """Brute force: slide the window until it no longer fits."""
    f = 0
    while f * hop + n_fft <= length:
        f += 1
    return f


def frame_matrix(x, n_fft, hop, frames, dtype=np.float64):
    x = np.asarray(x, dtype)
    return np.stack([x[f * hop:f * hop + n_fft] for f in range(frames)], axis=1)        # (n_fft, F)


def features(x, tabs, n_fft, hop, floor, dtype=np.float64):
    """(mag (nb, F), mel (n_mels, F), log_mel (n_mels, F), pw (nb, F)) of one utterance, in ``dtype``."""
    dft, mel = np.asarray(tabs[0], dtype), np.asarray(tabs[1], dtype)
    nb = n_fft // 2 + 1
    frames = 1 + (len(x) - n_fft) // hop
    X = frame_matrix(x, n_fft, hop, frames, dtype)
    re, im = dft[:nb] @ X, dft[nb:] @ X
    pw = re * re + im * im
    melp = mel @ pw
    return np.sqrt(pw), melp, np.log(np.maximum(melp, dtype(floor))), pw


def window_l1(x, tabs, n_fft, hop):
    """A_f = sum_k |w[k] x[f hop + k]| in float64, (F,); w is row 0 of the dft table."""
    frames = 1 + (len(x) - n_fft) // hop
    return np.abs(np.asarray(tabs[0][0], np.float64)[:, None] * frame_matrix(x, n_fft, hop, frames)).sum(axis=0)


def _strided_sum(vals):
    """Thread t adds elements t, t + 256, ... in order from 0; then p[t] += p[t + h] for h = 128 .. 1."""
    vals = np.asarray(vals, np.float64).reshape(-1)
    pad = (-len(vals)) % THREADS
    rows = np.concatenate([vals, np.zeros(pad)]).reshape(-1, THREADS)       # x + 0.0 == x for every partial that occurs
    p = np.zeros(THREADS)
    for r in rows:
        p = p + r
    h = THREADS // 2
    while h >= 1:
        p[:h] = p[:h] + p[h:2 * h]
        h //= 2
    return p[0]


def distances_exact(la, lb, ma, mb, dct):
    """One pair: float32 blocks (n_mels, F) and (nb, F) -> [log_mel_mae, mcd_db, spectral_convergence] as the kernel
    computes them."""
    assert la.dtype == lb.dtype == ma.dtype == mb.dtype == np.float32
    n_mels, F = la.shape
    d = la.astype(np.float64) - lb.astype(np.float64)
    mae = _strided_sum(np.abs(d).T) / np.float64(F * n_mels)             # element index f * n_mels + m
    dct = np.asarray(dct, np.float32).astype(np.float64)
    s = np.zeros(F)
    for q in range(dct.shape[0]):
        c = np.zeros(F)
        for m in range(n_mels):
            c = c + dct[q, m] * (0.5 * d[m])
        s = s + c * c
    mcd = _strided_sum(DB * np.sqrt(2.0 * s)) / np.float64(F)
    va, vb = ma.astype(np.float64), mb.astype(np.float64)
    dm = va - vb
    with np.errstate(divide='ignore', invalid='ignore'):
        sc = np.sqrt(_strided_sum((dm * dm).T)) / np.sqrt(_strided_sum((va * va).T))
    return np.array([mae, mcd, sc])


def distances(la, lb, ma, mb, dct):
    """The formulas in float64 from float64 features."""
    d = la - lb
    c = np.asarray(dct, np.float64) @ (0.5 * d)
    return np.array([np.abs(d).mean(), (DB * np.sqrt(2.0 * (c * c).sum(axis=0))).mean(),
                     np.sqrt(((ma - mb) ** 2).sum()) / np.sqrt((ma ** 2).sum())])


def plan_chunks(frames, width, chunk_bytes):
    chunks, start = [], 0
    while start < len(frames):
        stop, total = start + 1, frames[start]
        while stop < len(frames) and 4 * width * (total + frames[stop]) <= chunk_bytes:
            total += frames[stop]
            stop += 1
        chunks.append((start, stop))
        start = stop
    return chunks


FRAME_COUNTS = [1, 1, 2, 31, 32, 33, 65, 3]
CONFIGS = [(64, 16, 8, 4), (96, 25, 5, 3), (256, 64, 20, 13), (1024, 256, 80, 13)]      # (n_fft, hop, n_mels, n_mcep)


def utterance_list(n_fft, hop, sr=16000):
    """The list of the GPU tests: L = n_fft + hop (F - 1), plus hop - 1 trailing samples for odd F; two tones over a noise
    floor, peak-normalised, all drawn from one RandomState(1)."""
    rs = np.random.RandomState(1)
    waves = []
    for F in FRAME_COUNTS:
        L = n_fft + hop * (F - 1) + (hop - 1 if F % 2 else 0)
        t = np.arange(L) / float(sr)
        x = 0.5 * np.sin(2 * np.pi * 440 * t) + 0.25 * np.sin(2 * np.pi * 2900 * t + 1) + 0.1 * rs.randn(L)
        waves.append((x / np.abs(x).max()).astype(np.float32))
    return waves
