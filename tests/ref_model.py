"""Reading side of the reference-model fixtures (tests/golden/ref_*.npz, written by
tests/golden/make_golden_model.py from the reference's own code executed on a Chainer stand-in) and the
comparisons the host and the GPU tests share.  NumPy only."""
import json
import os

import numpy as np

from helpers import assert_close, assert_close_scaled

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

MARGIN = 1e-3          # VQ rows: (second-best - best) / best squared distance must exceed this
WHOLE_MAX = 4096       # gradients up to this many elements are stored whole ...
N_GRAD = 512           # ... larger ones at this many seeded flat positions (plus sum and sum of squares of all)
N_EMA = 256            # EMA parameters: whole up to this many elements, else this many positions
N_COND = 256
N_Y = 1024
MAX_BYTES = 330751     # no new fixture is larger than the largest older one (vq_train.npz)


def positions(seed, stream, size, n):
    """The seeded flat positions a tensor is sampled at: regenerated, not stored."""
    return np.sort(np.random.RandomState([seed, stream]).choice(size, n, replace=False))


def decay_tag(decay):
    return ('%g' % decay).replace('.', 'p')


def load(name):
    fx = dict(np.load(os.path.join(GOLD, name)))
    for key in list(fx):
        if key.endswith('meta_json'):
            fx[key[:-5]] = json.loads(str(fx[key]))
    return fx


def crafted_mol_inputs(seed):
    """test_mol_nll's recipe at (2, 30, 64): targets at exactly -1 and +1, on both sides of +-0.999, a log-scale
    below log_scale_min, a mean so far off that cdf_delta < 1e-12."""
    rs = np.random.RandomState(seed)
    B, nm, T = 2, 10, 64
    t = rs.uniform(-0.99, 0.99, (B, 1, T)).astype(np.float32)
    t[0, 0, :3] = -1.0
    t[1, 0, :3] = 1.0
    t[0, 0, 3:7] = [-0.9995, -0.9985, 0.9985, 0.9995]
    t[1, 0, 3:7] = [0.9995, 0.9985, -0.9985, -0.9995]
    y = rs.standard_normal((B, 3 * nm, T)).astype(np.float32)
    y[:, nm:2 * nm] = 127.5 * t + 30 * rs.standard_normal((B, nm, T)).astype(np.float32)
    y[:, 2 * nm:] = rs.uniform(0.5, 3.5, (B, nm, T)).astype(np.float32)
    y[0, 2 * nm, 9] = -50.0                              # clamped scale
    y[1, 2 * nm + 3, 1] = -41.0                          # ... on an edge-branch target
    y[1, nm + 1, 11] = 127.5 * t[1, 0, 11] + 4000.0      # far-off mean: saturated term
    return y, t


def perturb(meta, arrays):
    """The recorded move of the EMA fixture's target parameters between its two calls, in place, on the decoder's
    arrays in namedparams() order (the draws do not depend on a trailing axis of length 1)."""
    rs = np.random.RandomState(meta['perturb_seed'])
    for a in arrays:
        a[...] = a + meta['perturb_scale'] * rs.standard_normal(a.shape)


def sampled(fx, key, stream, arr, whole_max, n):
    """(got values at the stored positions, stored values) of one tensor."""
    flat = np.asarray(arr).reshape(-1)
    want = fx[key]
    if flat.size > whole_max:
        flat = flat[positions(fx['meta']['sample_seed'], stream, flat.size, n)]
    assert flat.shape == want.shape, '%s: %s vs %s' % (key, flat.shape, want.shape)
    return flat, want


def compare_step(fx, losses, idx, grads, tol=1e-4, grad_tol=1e-4, z=None, e=None, cond=None, y=None, what=''):
    """One VQVAE_StandardUpdater step against a ref_model_*.npz fixture.  ``grads``: Chainer parameter name ->
    gradient array, a parameter whose gradient is None ABSENT (or None).  Raises AssertionError."""
    names = [str(n) for n in fx['names']]
    for i, (a, b) in enumerate(zip(losses, fx['losses'])):
        assert_close(float(a), float(b), tol, '%s loss%d' % (what, i + 1))
    np.testing.assert_array_equal(np.asarray(idx).reshape(fx['idx'].shape), fx['idx'], what + ' VQ indices')
    if z is not None:
        assert_close(np.asarray(z).reshape(-1), fx['z'].reshape(-1), tol, what + ' z')
    if e is not None:
        assert_close(np.asarray(e).reshape(-1), fx['e'].reshape(-1), tol, what + ' e')
    if cond is not None:
        assert_close(*sampled(fx, 'cond_val', 1000, cond, 0, N_COND), tol, what + ' condition')
    if y is not None:
        assert_close(*sampled(fx, 'y_val', 1001, y, 0, N_Y), tol, what + ' y')
    got_none = sorted(n for n in names if grads.get(n) is None)
    want_none = sorted(n for n, m in zip(names, fx['grad_none']) if m)
    assert got_none == want_none, '%s parameters without a gradient: %s, the reference leaves %s' % (what, got_none, want_none)
    assert sorted(k for k in grads if grads[k] is not None) == sorted(set(names) - set(want_none)), what + ' gradient names'
    for i, n in enumerate(names):
        if fx['grad_none'][i]:
            continue
        g = np.asarray(grads[n], np.float64)
        got, want = sampled(fx, 'g%03d' % i, i, g, WHOLE_MAX, N_GRAD)
        assert_close_scaled(got, want, grad_tol, '%s grad %s' % (what, n))
        # Every element enters the two sums.  The bar above allows each element err = grad_tol * max|g_ref|, hence
        #   |sum g - sum g_ref|     <= size * err
        #   |sum g^2 - sum g_ref^2| =  |sum (g - g_ref)(g + g_ref)| <= err * (2 sum|g_ref| + size * err)
        #                           <= err * (2 sqrt(size * sumsq_ref) + size * err)        (Cauchy-Schwarz)
        err = grad_tol * fx['grad_absmax'][i]
        assert abs(g.sum() - fx['grad_sum'][i]) <= g.size * err, \
            '%s grad %s: sum %.9e vs %.9e' % (what, n, g.sum(), fx['grad_sum'][i])
        assert abs((g * g).sum() - fx['grad_sumsq'][i]) <= err * (2 * np.sqrt(g.size * fx['grad_sumsq'][i]) + g.size * err), \
            '%s grad %s: sum of squares %.9e vs %.9e' % (what, n, (g * g).sum(), fx['grad_sumsq'][i])


def grad_errors(fx, grads):
    """name -> max |got - want| / max |want| at the stored positions (what assert_close_scaled bounds)."""
    out = {}
    for i, n in enumerate(str(s) for s in fx['names']):
        if fx['grad_none'][i] or grads.get(n) is None:
            continue
        got, want = sampled(fx, 'g%03d' % i, i, np.asarray(grads[n], np.float64), WHOLE_MAX, N_GRAD)
        out[n] = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))
    return out
