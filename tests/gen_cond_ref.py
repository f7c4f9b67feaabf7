"""NumPy restatement of the condition-column rule of include/vqvae_gen_cond.h (csrc/generate_cond.hip): row (q, t) of the
compact column that a lockstep step reads when the condition is kept at the latent rate.  Float64 where the header says
float64, float32 products and sum each rounded on their own."""
import numpy as np


def position(t, tl, upscale):
    """(inside, v0, v1, w0, w1) of step ``t`` of a sequence of ``tl`` latent frames: the scalar rule, as one thread of the
    kernel evaluates it."""
    T = upscale * tl
    if t >= T:
        return False, 0, 0, np.float32(0), np.float32(1)
    if tl == 1:
        return True, 0, 0, np.float32(0), np.float32(1)
    v = np.float64(t) * (np.float64(tl - 1) / np.float64(T - 1))
    if t == T - 1:
        v = np.float64(tl - 1)
    v0 = min(max(int(np.floor(v)), 0), tl - 2)
    v1 = v0 + 1
    return True, v0, v1, np.float32(np.float64(v1) - v), np.float32(v - np.float64(v0))


def tables(tl, upscale):
    """The rule for every t < upscale * tl at once: (v0, v1, w0, w1) arrays."""
    T = upscale * tl
    if tl == 1:
        return np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T, np.float32), np.ones(T, np.float32)
    v = np.arange(T, dtype=np.float64) * (np.float64(tl - 1) / np.float64(T - 1))
    v[T - 1] = tl - 1
    v0 = np.clip(np.floor(v).astype(np.int64), 0, tl - 2).astype(np.int32)
    v1 = v0 + 1
    return v0, v1, (v1.astype(np.float64) - v).astype(np.float32), (v - v0.astype(np.float64)).astype(np.float32)


def column(x, g, t, upscale):
    """Row (q, t): x (Cl, tl) the sequence's latent block, g (G,) its speaker vector -> (Cl + G,) float32."""
    x = np.asarray(x, np.float32)
    inside, v0, v1, w0, w1 = position(t, x.shape[1], upscale)
    if inside:
        loc = (w0 * x[:, v0]).astype(np.float32) + (w1 * x[:, v1]).astype(np.float32)
    else:
        loc = np.zeros(x.shape[0], np.float32)
    return np.concatenate([loc.astype(np.float32), np.asarray(g, np.float32)])


def dense(x, g, upscale):
    """The whole (Cl + G, upscale * tl) expansion of one sequence, from the vectorised tables."""
    x = np.asarray(x, np.float32)
    v0, v1, w0, w1 = tables(x.shape[1], upscale)
    loc = (w0[None, :] * x[:, v0]).astype(np.float32) + (w1[None, :] * x[:, v1]).astype(np.float32)
    return np.concatenate([loc, np.repeat(np.asarray(g, np.float32)[:, None], loc.shape[1], axis=1)], axis=0)
