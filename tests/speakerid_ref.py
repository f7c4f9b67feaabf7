"""The rule of csrc/speaker_id.h restated in float64 NumPy, with explicit loops wherever the order matters, and a second,
independent evaluation of what the rule is for.

The restatement: ``cepstra``, ``deltas``, ``energy`` / ``gate`` and ``features`` are steps 1 to 3 for one utterance from
its float32 log-mel block; ``reduce_kept`` is the lane reduce R; ``stats`` step 5; ``score`` step 6; ``fit`` the host half
(per-speaker sums in list order, mean, covariance, Cholesky factor, its inverse, log-determinant).  NumPy's elementwise
float64 +, -, * and / round once each, as the device's do; nothing on these paths calls a sum or a dot whose order NumPy
chooses.

The independent evaluation: ``moments_direct`` (np.mean / np.cov-style moments of the kept frames) and ``score_direct``
(np.linalg.solve on the covariance itself): no lanes, no Cholesky factor, NumPy's own summation orders.

``voices`` is the synthetic identification fixture: 4 speakers, harmonic tones through a speaker-specific formant envelope
and F0 range, another "sentence" (F0 contour and amplitude pattern) per utterance.
"""
import numpy as np

LANES = 256
LN10 = np.log(np.float64(10.0))


# ---- steps 1 to 3 ---------------------------------------------------------------------------------------------------------------
def cepstra(log_mel, dct):
    """(F, n_mcep): c[f, q] = sum_m (double)dct[q, m] * (double)log_mel[m, f], m ascending from 0.0."""
    lm = np.asarray(log_mel, np.float32).astype(np.float64)
    dc = np.asarray(dct, np.float32).astype(np.float64)
    c = np.zeros((lm.shape[1], dc.shape[0]), np.float64)
    for m in range(lm.shape[0]):
        c = c + dc[:, m][None, :] * lm[m][:, None]
    return c


def deltas(c):
    """d[f] = 0.5 * (c[min(f + 1, F - 1)] - c[max(f - 1, 0)]): one subtraction, then one product."""
    F = c.shape[0]
    nxt = np.minimum(np.arange(F) + 1, F - 1)
    prv = np.maximum(np.arange(F) - 1, 0)
    return 0.5 * (c[nxt] - c[prv])


def energy(log_mel):
    """e[f] = sum_m (double)log_mel[m, f], m ascending from 0.0."""
    lm = np.asarray(log_mel, np.float32).astype(np.float64)
    e = np.zeros(lm.shape[1], np.float64)
    for m in range(lm.shape[0]):
        e = e + lm[m]
    return e


def threshold(n_mels, gate_db):
    """thr = n_mels * gate_db / 10 * ln 10, left to right in float64; None without a gate."""
    if gate_db is None:
        return None
    return np.float64(n_mels) * np.float64(gate_db) / np.float64(10.0) * LN10


def gate(log_mel, thr):
    e = energy(log_mel)
    if thr is None:
        return np.ones(e.size, bool)
    return e >= e.max() - np.float64(thr)


def features(log_mel, dct, with_deltas=True, thr=None):
    """(x (F, D) float64, keep (F,) bool) of one utterance."""
    c = cepstra(log_mel, dct)
    x = np.concatenate([c, deltas(c)], axis=1) if with_deltas else c
    return x, gate(log_mel, thr)


# ---- steps 4 to 6 ---------------------------------------------------------------------------------------------------------------
def reduce_kept(values, keep, lanes=LANES):
    """R over one utterance for every trailing column of ``values`` (F, ...): lane t = f mod lanes adds its kept frames'
    terms in ascending f to 0.0, then s[k] += s[k + h] for h = lanes / 2 .. 1.  A frame that is not kept adds nothing."""
    v = np.asarray(values, np.float64)
    k = np.asarray(keep, bool)
    F, tail = v.shape[0], v.shape[1:]
    pad = (-F) % lanes
    v = np.concatenate([v, np.zeros((pad,) + tail, np.float64)]).reshape((-1, lanes) + tail)
    k = np.concatenate([k, np.zeros(pad, bool)]).reshape(-1, lanes)
    s = np.zeros((lanes,) + tail, np.float64)
    for row, kr in zip(v, k):
        kr = kr.reshape((lanes,) + (1,) * len(tail))
        s = np.where(kr, s + row, s)
    h = lanes // 2
    while h >= 1:
        s[:h] = s[:h] + s[h:2 * h]
        h //= 2
    return s[0]


def stats(x, keep):
    """(cnt, s1 (D,), s2 (D (D + 1) / 2,)): the upper triangle row-major."""
    x = np.asarray(x, np.float64)
    D = x.shape[1]
    p, q = np.triu_indices(D)
    return int(np.count_nonzero(keep)), reduce_kept(x, keep), reduce_kept(x[:, p] * x[:, q], keep)


def frame_distances(x, mu, linv):
    """(G, F): qf of every frame under every model; y_r = sum_{c <= r} linv[g, r, c] * (x[f, c] - mu[g, c]), c ascending;
    qf = sum_r y_r * y_r, r ascending."""
    x, mu, linv = np.asarray(x, np.float64), np.asarray(mu, np.float64), np.asarray(linv, np.float64)
    G, D = mu.shape
    z = x[None, :, :] - mu[:, None, :]                       # (G, F, D)
    qf = np.zeros((G, x.shape[0]), np.float64)
    for r in range(D):
        y = np.zeros((G, x.shape[0]), np.float64)
        for c in range(r + 1):
            y = y + linv[:, r, c][:, None] * z[:, :, c]
        qf = qf + y * y
    return qf


def score(x, keep, mu, linv):
    """(q (G,), cnt): q[g] = R(qf) / (double)cnt."""
    cnt = int(np.count_nonzero(keep))
    qf = frame_distances(x, mu, linv)
    return reduce_kept(qf.T, keep) / np.float64(cnt), cnt


def log_likelihood(q, logdet, D):
    return -0.5 * (np.asarray(q, np.float64) + np.asarray(logdet, np.float64)[None, :] + D * np.log(2.0 * np.pi))


# ---- the host half -------------------------------------------------------------------------------------------------------------
def speaker_sums(per_utt, speakers, G):
    """Per-speaker (cnt (G,), S1, S2) from per-utterance (cnt, s1, s2), added in list order, each from 0.0."""
    D, T = per_utt[0][1].size, per_utt[0][2].size
    C, S1, S2 = np.zeros(G, np.int64), np.zeros((G, D), np.float64), np.zeros((G, T), np.float64)
    for (cnt, s1, s2), g in zip(per_utt, speakers):
        C[g] += cnt
        S1[g] = S1[g] + s1
        S2[g] = S2[g] + s2
    return C, S1, S2


def fit(C, S1, S2, ridge=0.0):
    """dict of mu, cov, L, linv (lower), logdet from the raw sums."""
    G, D = S1.shape
    p, q = np.triu_indices(D)
    n = C.astype(np.float64)
    mu = S1 / n[:, None]
    full = np.zeros((G, D, D), np.float64)
    full[:, p, q] = S2
    full[:, q, p] = S2
    cov = full / n[:, None, None] - mu[:, :, None] * mu[:, None, :]
    if ridge:
        cov = cov + (ridge * np.trace(cov, axis1=1, axis2=2) / D)[:, None, None] * np.eye(D)[None]
    L = np.stack([np.linalg.cholesky(c) for c in cov])
    linv = np.stack([np.tril(np.linalg.inv(l)) for l in L])
    logdet = 2.0 * np.log(np.diagonal(L, axis1=1, axis2=2)).sum(axis=1)
    return dict(mu=mu, cov=cov, L=L, linv=linv, logdet=logdet, count=C)


# ---- the independent evaluation -----------------------------------------------------------------------------------------------
def moments_direct(blocks):
    """(mu, cov) of the kept frames of a list of (x, keep) blocks taken together: np.mean and the biased np.cov."""
    rows = np.concatenate([np.asarray(x, np.float64)[np.asarray(k, bool)] for x, k in blocks])
    return rows.mean(axis=0), np.atleast_2d(np.cov(rows, rowvar=False, bias=True))


def score_direct(x, keep, mu, cov):
    """The mean of (x - mu)^T cov^-1 (x - mu) over the kept frames, by np.linalg.solve on cov itself."""
    z = np.asarray(x, np.float64)[np.asarray(keep, bool)] - mu
    return float(np.mean(np.sum(z * np.linalg.solve(cov, z.T).T, axis=1)))


def kl_gauss(mu_a, cov_a, mu_b, cov_b):
    """KL(a || b) of two Gaussians, nats."""
    D = mu_a.size
    dm = mu_b - mu_a
    ib = np.linalg.inv(cov_b)
    return 0.5 * (np.trace(ib.dot(cov_a)) + dm.dot(ib).dot(dm) - D + np.linalg.slogdet(cov_b)[1] - np.linalg.slogdet(cov_a)[1])


# ---- the synthetic voices -------------------------------------------------------------------------------------------------------
VOICE_CFG = dict(sr=16000, n_fft=256, hop=64, n_mels=24, n_mcep=6)
# per speaker: the F0 range in Hz and three formants (centre Hz, width Hz)
VOICES = (((95.0, 125.0), ((500.0, 120.0), (1500.0, 200.0), (2500.0, 300.0))),
          ((180.0, 230.0), ((750.0, 150.0), (1150.0, 200.0), (3000.0, 350.0))),
          ((120.0, 160.0), ((300.0, 100.0), (2200.0, 250.0), (3300.0, 300.0))),
          ((210.0, 270.0), ((400.0, 120.0), (900.0, 150.0), (2700.0, 300.0))))


def voice(speaker, sentence, seconds=0.5, sr=16000):
    """One utterance: harmonics of a slowly moving F0 inside the speaker's range, each weighted by the speaker's formant
    envelope at its frequency, under the sentence's amplitude pattern, plus a little noise; float32, peak 0.5."""
    (f_lo, f_hi), formants = VOICES[speaker]
    rs = np.random.RandomState(1000 + 97 * sentence + speaker)
    n = int(seconds * sr)
    t = np.arange(n) / float(sr)
    knots = rs.uniform(f_lo, f_hi, 6)
    f0 = np.interp(t, np.linspace(0.0, seconds, 6), knots)
    phase = 2.0 * np.pi * np.cumsum(f0) / sr
    amp = np.interp(t, np.linspace(0.0, seconds, 9), rs.uniform(0.3, 1.0, 9))
    wave = np.zeros(n)
    for h in range(1, 40):
        fh = h * f0
        if fh.min() > 0.45 * sr:
            break
        env = sum(np.exp(-0.5 * ((fh - fc) / bw) ** 2) for fc, bw in formants) + 0.02
        wave += env * np.sin(h * phase + rs.uniform(0, 2 * np.pi)) * (fh < 0.45 * sr)
    wave = amp * wave + 0.003 * rs.standard_normal(n)
    return (0.5 * wave / np.abs(wave).max()).astype(np.float32)


def voices(enrol=3, test=2):
    """(enrol waves, enrol speakers, test waves, targets): ``enrol`` + ``test`` utterances of every voice, all of other
    sentences."""
    ew, es, tw, ts = [], [], [], []
    for s in range(len(VOICES)):
        for k in range(enrol):
            ew.append(voice(s, k))
            es.append(s)
        for k in range(test):
            tw.append(voice(s, enrol + k))
            ts.append(s)
    return ew, np.array(es, np.int64), tw, np.array(ts, np.int64)
