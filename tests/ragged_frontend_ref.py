"""Float64 restatement of the ragged front end (vqvae_amd.frontend, include/vqvae_ragged.h), built from the oracle's own
functions: every utterance is run SEPARATELY through encoder_fwd, the sequential float32 argmin of vq_forward and
cond_embed_fwd's conv stack, which is what "an utterance never sees its neighbours" means.  Also the length rule and the
chunk planner, restated independently of the package."""
import numpy as np

import vqvae_oracle as O

DEPTH = 6
CAP = 1 << 31


def length_rule(t):
    """One encoder stage: K = 4, stride 2, pad 1."""
    return (int(t) - 2) // 2 + 1 if int(t) >= 2 else 0


def stage_lengths(t, depth=DEPTH):
    out = [int(t)]
    for _ in range(depth):
        out.append(length_rule(out[-1]))
    return out


def latent_length(t):
    return stage_lengths(t)[-1]


def plan_chunks(lengths, widths, chunk_bytes):
    """Greedy, in input order: a run is closed in front of the utterance that would push one stage past chunk_bytes or
    to 2^31 elements; an oversize utterance stands alone."""
    chunks, start = [], 0
    sums = [0] * len(widths)
    for u, t in enumerate(lengths):
        per = [w * l for w, l in zip(widths, stage_lengths(t, len(widths) - 1))]
        new = [a + b for a, b in zip(sums, per)]
        if u > start and (4 * max(new) > chunk_bytes or max(new) >= CAP):
            chunks.append((start, u))
            start, new = u, per
        sums = new
    if len(lengths) > start:
        chunks.append((start, len(lengths)))
    return chunks


def _f64(p):
    return dict((n, tuple(None if a is None else np.asarray(a, np.float64) for a in v) if isinstance(v, tuple)
                 else np.asarray(v, np.float64)) for n, v in p.items())


def encode(enc_params, wave):
    """z (d, tl) in float64 of ONE utterance."""
    z, _ = O.encoder_fwd(_f64(enc_params), np.asarray(wave, np.float64).reshape(1, 1, -1))
    return z[0]


def argmin_f32(z, W):
    """The sequential float32 argmin of vq_forward over the columns of z (d, T): indices (T,) int32."""
    _, idx = O.vq_forward(np.ascontiguousarray(z, np.float32)[None], np.ascontiguousarray(W, np.float32))
    return idx[0].astype(np.int32)


def distance_gaps(z, W):
    """Per column of the float64 z: (best, second best) squared distance to the rows of W."""
    d2 = ((np.asarray(z, np.float64).T[:, None, :] - np.asarray(W, np.float64)[None]) ** 2).sum(axis=2)
    part = np.sort(d2, axis=1)
    return part[:, 0], part[:, 1], d2.argmin(axis=1).astype(np.int32)


def condition_stack(cond_params, e):
    """The five dilated convs + ReLU of cond_embed_fwd on ONE utterance's e (d, tl), float64: (Cl, tl)."""
    p = _f64(cond_params)
    _, hs = O.cond_embed_fwd(p, np.asarray(e, np.float64)[None], np.zeros(1, np.int32), upscale=1)
    return hs[-1][0]


def frontend(P, wave):
    """One utterance: (z float64 (d, tl), indices of the float64 z, local float64 (Cl, tl) from e = W[indices])."""
    z = encode(P['encoder'], wave)
    _, _, idx = distance_gaps(z, P['vq'])
    e = np.asarray(P['vq'], np.float64)[idx].T
    return z, idx, condition_stack(P['condition_embed'], e)
