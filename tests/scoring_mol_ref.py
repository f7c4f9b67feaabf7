"""The rule of csrc/ragged_mol.h restated per utterance in float64 NumPy, on the oracle's own functions: the dense condition
(scoring_ref.dense_condition), wavenet_fwd over the raw-sample or one-hot input and _mol_terms.  Nothing here restates a
kernel: no tiles, no splits, no latent-rate projection.  Two things ARE restated exactly, because the device promises their
bits: the sample-form embed (embed_bits) and the reduce's order (scoring_ref.reduce_order).

tests/test_host_scoring_mol.py holds score_utterance_mol to vae_forward(loss_kind='mol')'s loss1 at 1e-12 and its
per-position terms to the reference's own tests/golden/ref_mol_loss.npz."""
import numpy as np

import vqvae_oracle as O
from scoring_ref import LANES, cast_tree, dense_condition, positions, reduce_order  # noqa: F401


def mol_nll(y, t, quantize=256, log_scale_min=-40.0):
    """The per-position negative log-likelihoods of _mol_terms (modules.py:173-228 without the mean): y (B, 3 M, T),
    t (B, 1, T) -> (B, T), in y's dtype."""
    return -O._mol_terms(y, np.asarray(t, y.dtype), quantize, log_scale_min)['lse'][:, 0]


def at_floor(y, t, quantize=256, log_scale_min=-40.0):
    """(B, T) bool: positions between the tails whose EVERY component's cdf_delta is at or below the 1e-12 floor."""
    c = O._mol_terms(y, np.asarray(t, y.dtype), quantize, log_scale_min)
    inner = ~(c['left'] | c['right'])
    return (inner & (c['cdf_delta'] <= 1e-12)).all(axis=1)


def score_utterance_mol(dec, w, local, gvec, n_loop, n_layer, upscale=64, quantize=256, log_scale_min=-40.0, dtype=np.float64):
    """dec: the oracle's decoder parameter tree; w (L,) float32 samples; local (Cl, tl); gvec (G,).
    -> dict(n, nll (n,), params (3 M, n), floor (n,) bool).  An embed of Qin > 1 input channels reads the one-hot of
    MuLaw(Qin) classes; the target is the sample in both forms."""
    dec = cast_tree(dec, dtype)
    w = np.asarray(w, np.float32).reshape(-1)
    Qin = dec['embed'][0].shape[1]
    n = positions(len(w), np.asarray(local).shape[1], upscale)
    assert n >= 1
    if Qin == 1:
        x = np.ascontiguousarray(w[:n].astype(dtype)[None, None])                     # the input at j is w[j]
    else:
        q = O.MuLaw(Qin).transform(w).astype(np.int64)
        x = np.ascontiguousarray(np.identity(Qin, dtype=dtype)[q[:n]].T[None])
    cond = np.ascontiguousarray(dense_condition(np.asarray(local, dtype), np.asarray(gvec, dtype), upscale)[:, :, :n])
    y, _ = O.wavenet_fwd(dec, x, cond, n_loop, n_layer)
    t = w[1:n + 1].astype(dtype)[None, None]                                          # the target is w[j + 1]
    return dict(n=n, nll=mol_nll(y, t, quantize, log_scale_min)[0], params=y[0], floor=at_floor(y, t, quantize, log_scale_min)[0])


def embed_bits(W, b, waves, n_pos):
    """The sample-form embed in float32, bit for bit: W (R, 1, 2), b (R,) or None, a list of (L_i,) float32 waves and
    their n_i -> (R, sum n_i).  Two products, one sum, the bias; at jl = 0 the second product alone, then the bias."""
    W = np.asarray(W, np.float32).reshape(-1, 2)
    cols = []
    for w, n in zip(waves, n_pos):
        w = np.asarray(w, np.float32).reshape(-1)
        p1 = W[:, 1:2] * w[None, :n]
        v = p1.copy()
        v[:, 1:] = W[:, 0:1] * w[None, :n - 1] + p1[:, 1:]
        if b is not None:
            v = v + np.asarray(b, np.float32)[:, None]
        assert v.dtype == np.float32
        cols.append(v)
    return np.concatenate(cols, axis=1)
