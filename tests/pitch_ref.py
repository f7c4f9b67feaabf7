"""NumPy restatements for the pitch tracker and the pair statistics (include/vqvae_pitch.h, vqvae_amd.pitch); nothing here
imports the package.

``lags``          tau_min, tau_max, W of a configuration, and ``lags_brute`` the same by counting with exact rationals.
``track``         the header's rule in float64 in the header's order: equal to the device in every bit.
``pair_stats``    the pair kernel's arithmetic in its own order.  Counts, vuv_error and gross_error are equal to the device in
                  every bit; the three log-based columns use NumPy's log / log2 where the device uses its own.
``pair_bounds``   what those three may differ by, from a stated accuracy of the device functions in ulp.
``tone`` / ``tone_set`` / ``utterance_list``   the signals of the tests.
"""
import math
from fractions import Fraction

import numpy as np

import metrics_ref as M

THREADS = 256
COLUMNS = ('voiced_ref', 'voiced_test', 'voiced_both', 'vuv_error', 'gross_error', 'f0_rmse_cents', 'log_f0_mean_ref',
           'log_f0_mean_test')
FRAME_COUNTS = M.FRAME_COUNTS
# (sr, frame, hop, fmin, fmax); the first three are those of the truth tests, the last has nothing round
CONFIGS = [(4000, 160, 40, 100.0, 400.0), (8000, 320, 80, 100.0, 500.0), (16000, 1024, 256, 60.0, 400.0),
           (4000, 150, 25, 90.0, 410.0)]
TRUTH_CONFIGS = [(16000, 1024, 256, 60.0, 400.0), (8000, 320, 80, 100.0, 500.0), (4000, 160, 40, 100.0, 400.0)]
THRESHOLD, MIN_POWER = 0.15, 1e-8


def lags(sr, frame, fmin, fmax):
    """(tau_min, tau_max, W) by the header's formulas: float64 divisions, floor and ceil."""
    tau_min, tau_max = int(math.floor(sr / float(fmax))), int(math.ceil(sr / float(fmin)))
    return tau_min, tau_max, frame - tau_max


def lags_brute(sr, frame, fmin, fmax):
    """The same by counting: the largest tau with tau * fmax <= sr and the smallest with tau * fmin >= sr, exactly."""
    fmin, fmax = Fraction(float(fmin)), Fraction(float(fmax))
    tau_min = 0
    while (tau_min + 1) * fmax <= sr:
        tau_min += 1
    tau_max = 0
    while tau_max * fmin < sr:
        tau_max += 1
    return tau_min, tau_max, frame - tau_max


def frame_count(length, frame, hop):
    return M.frame_count(length, frame, hop)


def _sum4(terms):
    """The header's order S along the last axis: term j goes to accumulator j mod 4, j ascending, each from 0.0; the sum is
    (a0 + a1) + (a2 + a3).  The padding adds +0.0 to sums of non-negative terms, which changes no bit."""
    W = terms.shape[-1]
    pad = (-W) % 4
    if pad:
        terms = np.concatenate([terms, np.zeros(terms.shape[:-1] + (pad,))], axis=-1)
    rows = terms.reshape(terms.shape[:-1] + (-1, 4))
    acc = np.zeros(terms.shape[:-1] + (4,))
    for r in range(rows.shape[-2]):
        acc = acc + rows[..., r, :]
    return (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])


def normalised_difference(frames, tau_max):
    """(d' (F, tau_max + 1) with d'(0) = 1, power (F,)) of float64 frames (F, frame)."""
    F, frame = frames.shape
    W = frame - tau_max
    win = np.lib.stride_tricks.sliding_window_view(frames, W, axis=1)[:, :tau_max + 1]      # [f, tau, j] = x[j + tau]
    diff = win[:, :1] - win[:, 1:]
    d = _sum4(diff * diff)                                                                   # tau = 1 .. tau_max
    power = _sum4(frames[:, :W] * frames[:, :W]) / np.float64(W)
    c = np.cumsum(d, axis=1)                                                                 # sequential, ascending
    tau = np.arange(1, tau_max + 1, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        dp = np.where(c == 0.0, 1.0, (d * tau) / c)
    return np.concatenate([np.ones((F, 1)), dp], axis=1), power


def track(x, sr, frame, hop, fmin, fmax, threshold=THRESHOLD, min_power=MIN_POWER, block=32):
    """(f0 (F,) float32, aperiodicity (F,) float32, lag (F,) int: the chosen tau, 0 for an unvoiced frame) of one utterance."""
    tau_min, tau_max, W = lags(sr, frame, fmin, fmax)
    x = np.asarray(x, np.float32).astype(np.float64)
    F = 1 + (len(x) - frame) // hop
    f0, ap, lag = np.zeros(F, np.float32), np.zeros(F, np.float32), np.zeros(F, np.int64)
    for f_lo in range(0, F, block):
        f_hi = min(F, f_lo + block)
        frames = np.stack([x[f * hop:f * hop + frame] for f in range(f_lo, f_hi)])
        dps, power = normalised_difference(frames, tau_max)
        for f in range(f_lo, f_hi):
            dp = dps[f - f_lo]
            if power[f - f_lo] < min_power:
                ap[f] = 1.0
                continue
            below = np.nonzero(dp[tau_min:tau_max + 1] < threshold)[0]
            if below.size == 0:
                ap[f] = np.float32(dp[tau_min:tau_max + 1].min())
                continue
            tau = tau_min + int(below[0])
            while tau + 1 <= tau_max and dp[tau + 1] < dp[tau]:
                tau += 1
            ts = np.float64(tau)
            if tau - 1 >= 1 and tau + 1 <= tau_max:
                a, b, c = dp[tau - 1], dp[tau], dp[tau + 1]
                q = (a - 2.0 * b) + c
                if q > 0.0:
                    ts = np.float64(tau) + (0.5 * (a - c)) / q
            with np.errstate(divide='ignore'):
                f0[f] = np.float32(np.float64(sr) / ts)
            ap[f] = np.float32(dp[tau])
            lag[f] = tau
    return f0, ap, lag


def _terms(f0_a, f0_b):
    fa, fb = np.asarray(f0_a, np.float32).astype(np.float64), np.asarray(f0_b, np.float32).astype(np.float64)
    va, vb = fa > 0.0, fb > 0.0
    both = va & vb
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(both, fb / np.where(both, fa, 1.0), 1.0)
        cents = np.where(both, 1200.0 * np.log2(r), 0.0)
        la, lb = np.where(va, np.log(np.where(va, fa, 1.0)), 0.0), np.where(vb, np.log(np.where(vb, fb, 1.0)), 0.0)
    return va, vb, both, r, cents, la, lb


def pair_stats(f0_a, f0_b):
    """One pair: the eight columns as the kernel computes them (a frame outside a set adds +0.0 here and nothing there:
    the same bits, as no partial sum is -0.0)."""
    va, vb, both, r, cents, la, lb = _terms(f0_a, f0_b)
    F = np.float64(len(va))
    na, nb, nboth = np.float64(va.sum()), np.float64(vb.sum()), np.float64(both.sum())
    gross = np.float64((both & (np.abs(r - 1.0) > 0.2)).sum())
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.array([na, nb, nboth, np.float64((va != vb).sum()) / F, gross / nboth,
                         np.sqrt(M._strided_sum(cents * cents) / nboth), M._strided_sum(la) / na, M._strided_sum(lb) / nb])


def pair_bounds(f0_a, f0_b, ulps=4.0):
    """What f0_rmse_cents, log_f0_mean_ref and log_f0_mean_test of the device may differ from ``pair_stats`` by, when the
    device's log and log2 are within ``ulps`` ulp of the true value and NumPy's within 1 ulp: (3,) float64.
    Per term t = log f: |dt| <= (ulps + 1) ulp(t).  A sum of n terms formed in the same order on both sides: the terms'
    differences add up, and each of the n additions (and the tree's) may round differently once its inputs differ, by at
    most one ulp of the largest partial sum, which is at most sum |t|:  dS <= sum |dt| + (n + 8) ulp(sum |t|).  The mean
    adds half an ulp of itself for the division.
    Per term c^2 with c = 1200 log2 r: |dc| <= 1200 (ulps + 1) ulp(log2 r) + ulp(c); |d(c^2)| <= 2 |c| |dc| + dc^2 +
    ulp(c^2); the sum as above; rmse = sqrt(S / n) moves by at most dS / (2 n rmse) + 2 ulp(rmse) (and not at all when
    every r is exactly 1: log2(1) is exactly 0 on both sides)."""
    va, vb, both, r, cents, la, lb = _terms(f0_a, f0_b)
    u = ulps + 1.0

    def sum_bound(terms, dterms, n):
        return dterms.sum() + (n + 8) * np.spacing(np.abs(terms).sum())

    out = np.zeros(3)
    n = int(both.sum())
    if n and (r[both] != 1.0).any():
        lg = np.abs(cents) / 1200.0
        dc = 1200.0 * u * np.spacing(lg) + np.spacing(np.abs(cents))
        sq = cents * cents
        dS = sum_bound(sq, 2.0 * np.abs(cents) * dc + dc * dc + np.spacing(sq), n)
        rmse = np.sqrt(sq.sum() / n)
        out[0] = dS / (2.0 * n * rmse) + 2.0 * np.spacing(rmse)
    for k, (v, t) in enumerate(((va, la), (vb, lb))):
        n = int(v.sum())
        if n:
            out[1 + k] = sum_bound(t, u * np.spacing(np.abs(t)) * v, n) / n + np.spacing(np.abs(t).sum() / n)
    return out


# ---- signals ---------------------------------------------------------------------------------------------------------
def tone(f, length, sr, rs=None, noise=1e-3, phase=0.0):
    """Three harmonics of amplitudes 1, 0.5, 0.25 over white noise, float32."""
    t = np.arange(length) / float(sr)
    x = np.sin(2 * np.pi * f * t + phase) + 0.5 * np.sin(2 * np.pi * 2 * f * t + 2 * phase) + 0.25 * np.sin(2 * np.pi * 3 * f * t)
    if rs is not None and noise:
        x = x + noise * rs.standard_normal(length)
    return x.astype(np.float32)


def tone_set(sr, frame, hop, fmin, fmax, frames=5, count=23, seed=0):
    """[(f, wave)]: ``count`` tones between 1.15 fmin and 0.9 fmax (geometrically spaced), ``frames`` frames each, noise of
    1e-3 from RandomState(seed)."""
    rs = np.random.RandomState(seed)
    return [(f, tone(f, frame + hop * (frames - 1), sr, rs)) for f in np.geomspace(1.15 * fmin, 0.9 * fmax, count)]


def cents(f0, f):
    return 1200.0 * np.log2(np.asarray(f0, np.float64) / f)


def list_tones(fmin, fmax, shift=1.0):
    """{utterance: true frequency} of the plain tones of ``utterance_list``."""
    return {3: 1.3 * fmin * shift, 7: 1.1 * np.sqrt(fmin * fmax) * shift}


def utterance_list(sr, frame, hop, fmin, fmax, shift=1.0):
    """The list of the GPU tests, one utterance per entry of FRAME_COUNTS: L = frame + hop (F - 1), plus hop - 1 trailing
    samples for odd F.  ``shift`` multiplies every tone's frequency (the test side of a pair).
      0  a wave of period exactly tau_max (the best lag is the last one: no refinement)
      1  a wave of period exactly tau_min
      2  exact zeros
      3  a tone low in the range
      4  white noise
      5  zeros, then a tone that starts halfway through
      6  a tone high in the range followed by one in the middle
      7  a tone in the middle"""
    tau_min, tau_max, _ = lags(sr, frame, fmin, fmax)
    rs = np.random.RandomState(1)
    lo, mid, hi = 1.3 * fmin * shift, np.sqrt(fmin * fmax) * shift, 0.8 * fmax * shift
    waves = []
    for u, F in enumerate(FRAME_COUNTS):
        L = frame + hop * (F - 1) + (hop - 1 if F % 2 else 0)
        n = np.arange(L)
        if u == 0:
            x = (np.sin(2 * np.pi * n * shift / tau_max) + 0.3 * np.sin(4 * np.pi * n * shift / tau_max)).astype(np.float32)
        elif u == 1:
            x = np.sin(2 * np.pi * n * shift / tau_min).astype(np.float32)
        elif u == 2:
            x = np.zeros(L, np.float32)
        elif u == 3:
            x = tone(lo, L, sr, rs)
        elif u == 4:
            x = (0.3 * rs.standard_normal(L)).astype(np.float32)
        elif u == 5:
            x = tone(mid, L, sr, rs, phase=0.5)
            x[:L // 2] = 0
        elif u == 6:
            x = np.concatenate([tone(hi, L // 2, sr, rs), tone(mid, L - L // 2, sr, rs, phase=1.0)])
        else:
            x = tone(mid * 1.1, L, sr, rs)
        waves.append(x)
    return waves
