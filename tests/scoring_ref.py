"""The rule of include/vqvae_ragged_decoder.h restated per utterance in float64 NumPy, on the oracle's own functions: the dense
condition of cond_embed_fwd (align-corners up-sampling of the local block, the speaker vector broadcast), wavenet_fwd
over the one-hot input and softmax_xent_fwd.  Nothing here restates a kernel: no tiles, no splits, no latent-rate
projection.  The reduce's order IS restated, exactly (reduce_order), because the device promises those bits.

tests/test_host_scoring.py holds score_utterance to vae_forward's loss1 at 1e-12."""
import numpy as np

import vqvae_oracle as O

LANES = 256


def cast_tree(p, dtype):
    if isinstance(p, dict):
        return dict((k, cast_tree(v, dtype)) for k, v in p.items())
    if isinstance(p, list):
        return [cast_tree(v, dtype) for v in p]
    if isinstance(p, tuple):
        return tuple(cast_tree(v, dtype) for v in p)
    return np.asarray(p).astype(dtype)


def positions(L, tl, upscale=64):
    """n = min(upscale * tl, L - 1)."""
    return min(int(upscale) * int(tl), int(L) - 1)


def dense_condition(local, gvec, upscale=64):
    """(1, Cl + G, upscale * tl) from the utterance's (Cl, tl) local block and (G,) speaker vector: what
    O.cond_embed_fwd builds behind its convs."""
    local = np.asarray(local)
    T = int(upscale) * local.shape[1]
    loc = O.upsample_fwd(local[None], T)
    glob = np.broadcast_to(np.asarray(gvec, local.dtype)[None, :, None], (1, len(gvec), T))
    return np.concatenate((loc, glob), axis=1)


def score_utterance(dec, q, local, gvec, n_loop, n_layer, upscale=64, dtype=np.float64):
    """dec: the oracle's decoder parameter tree; q (L,) classes; local (Cl, tl); gvec (G,).
    -> dict(n, nll (n,), logits (Q, n), hit (n,) bool, gap (n,): the top-two logit gap)."""
    dec = cast_tree(dec, dtype)
    q = np.asarray(q).reshape(-1).astype(np.int64)
    Q = dec['embed'][0].shape[1]
    n = positions(len(q), np.asarray(local).shape[1], upscale)
    assert n >= 1
    x = np.ascontiguousarray(np.identity(Q, dtype=dtype)[q[:n]].T[None])             # the input at j is q[j]
    cond = np.ascontiguousarray(dense_condition(np.asarray(local, dtype), np.asarray(gvec, dtype), upscale)[:, :, :n])
    y, _ = O.wavenet_fwd(dec, x, cond, n_loop, n_layer)
    t = q[1:n + 1]                                                                   # the target is q[j + 1]
    _, logp = O.softmax_xent_fwd(y, t[None].astype(np.int32))
    nll = -logp[0, t, np.arange(n)]
    top = np.sort(y[0], axis=0)
    return dict(n=n, nll=nll, logits=y[0], hit=np.argmax(y[0], axis=0) == t, gap=top[-1] - top[-2] if Q > 1 else np.full(n, np.inf))


def reduce_order(values, lanes=LANES):
    """The device reduce's order (include/vqvae_ragged_decoder.h): lane t adds elements t, t + lanes, ... in ascending order
    (float64, or int64 for integers), then s[k] += s[k + h] for h = lanes / 2, lanes / 4 .. 1."""
    v = np.asarray(values).reshape(-1)
    acc = np.float64 if v.dtype.kind == 'f' else np.int64
    s = np.zeros(lanes, acc)
    for a in range(0, v.size, lanes):
        row = v[a:a + lanes].astype(acc)
        s[:row.size] = s[:row.size] + row
    h = lanes // 2
    while h >= 1:
        s[:h] = s[:h] + s[h:2 * h]
        h //= 2
    return s[0]
