"""NumPy restatement of the sampling controls of include/vqvae_sampling.h (temperature, top-k, top-p, greedy), the way
tests/optim_hooks_ref.py restates the optimizer hooks' summation order.  One sequence at one step:

    l[0, O) float32 logits, u the uniform double in [0, 1) that oracle.choice_from_uniform would get,
    temperature (float32, >= 0), top_k (int32, 0 or >= O = off), top_p (float32, >= 1 = off).

  Rank.   Classes are totally ordered by (logit descending, index ascending); equal logits go to the lower index.
  Greedy. temperature == 0 returns the rank-0 class; u is not read.
  top-k.  Ranks < top_k are kept, decided on the raw float32 logits.
  Temperature.  x = l * (1.0f / temperature) in float32; over the kept classes m = max x, e = expf(x - m),
          p = e / sum(e) in float32 (classes outside hold e = 0 and stay in the sum, where they change nothing).
  top-p.  After top-k, on p: walk the kept classes in rank order adding p in float64; keep the shortest prefix whose mass
          is >= top_p.  The prefix is never empty: rank 0 is always in it.
  Draw.   Classes outside the kept set get probability 0; then oracle.choice_from_uniform: float64 cumulative sum in
          index order, divided by its last element, the number of entries <= u.  The rank-0 class has e = 1, so the
          last element is positive, every entry in front of the first kept class is 0 <= u, and the entry of the LAST
          kept class and all behind it are 1 > u: with u < 1 the count is the index of an entry that is larger than the
          one in front of it, which is a class with p > 0, which is a kept class.  (A kept class whose e underflows to 0
          can never be drawn; it is still "kept".)

With all three controls neutral this is oracle.choice_from_uniform(oracle.softmax_axis1(l), u).
"""
import numpy as np

import vqvae_oracle as O


def rank_order(l):
    """Class indices in rank order: logit descending, index ascending (-0 equals +0)."""
    l = np.asarray(l, np.float32)
    return np.lexsort((np.arange(l.size), -l))            # the last key is the primary one


def filtered(l, temperature=1.0, top_k=0, top_p=1.0):
    """(p, kept, mass): p float32 (O,) = what the draw's cumulative sum adds up (0 outside the kept set), kept = boolean
    mask of the kept classes, mass = the float64 rank-order cumulative masses the nucleus was decided on (None without
    top-p)."""
    l = np.asarray(l, np.float32).reshape(-1)
    n_cls = l.size
    T, tp, k = np.float32(temperature), np.float32(top_p), int(top_k)
    order = rank_order(l)
    if T == 0:                                             # greedy: the rank-0 class alone
        T, k, tp = np.float32(1), 1, np.float32(1)
    if k <= 0 or k > n_cls:
        k = n_cls
    kept = np.zeros(n_cls, bool)
    kept[order[:k]] = True
    x = l * (np.float32(1.0) / T)
    m = x[kept].max()
    with np.errstate(under='ignore'):
        e = np.exp(x - m)
        e[~kept] = 0
        p = e / e.sum()
    assert p.dtype == np.float32
    mass = None
    if tp < 1:
        mass = p[order[:k]].astype(np.float64).cumsum()    # sequential, like the device's one-thread walk
        reach = np.flatnonzero(mass >= np.float64(tp))
        n_keep = int(reach[0]) + 1 if reach.size else k
        drop = order[n_keep:k]
        kept[drop] = False
        p[drop] = 0
    return p, kept, mass


def probs(l, temperature=1.0, top_k=0, top_p=1.0):
    """What vqvae_sample_logits writes to probs_out: (float)(p / last element of the float64 cumulative sum)."""
    p, _, _ = filtered(l, temperature, top_k, top_p)
    return (p.astype(np.float64) / p.astype(np.float64).cumsum()[-1]).astype(np.float32)


def sample(l, u, temperature=1.0, top_k=0, top_p=1.0):
    """The class drawn."""
    if np.float32(temperature) == 0:
        return int(rank_order(l)[0])
    p, _, _ = filtered(l, temperature, top_k, top_p)
    return O.choice_from_uniform(p, u)


def ambiguous(l, u, temperature=1.0, top_k=0, top_p=1.0, margin=1e-5):
    """True when two float32 evaluations of the same rule may legitimately differ: u within ``margin`` of an edge of the
    restated cdf, or a rank-order cumulative mass within ``margin`` of top_p.  Never for greedy / top_k == 1."""
    if np.float32(temperature) == 0 or int(top_k) == 1:
        return False
    p, _, mass = filtered(l, temperature, top_k, top_p)
    if mass is not None and np.abs(mass - np.float64(np.float32(top_p))).min() <= margin:
        return True
    cdf = p.astype(np.float64).cumsum()
    cdf /= cdf[-1]
    return bool(np.abs(cdf - u).min() <= margin)


def mol_sample(out, u, temperature, log_scale_min=-40.0):
    """oracle.mol_sample_from_uniform (generate.py:113-133) with a temperature per row (> 0): the mixture weights are
    softmax(logit_probs * (1.0f / temperature)), each scale is exp(max(log_scale, log_scale_min)) * temperature, both
    float32; the rest is unchanged.  out (n, 3 * nr_mix) float32, u (n, nr_mix) float64 in (0, 1)."""
    out = np.asarray(out, np.float32)
    T = np.broadcast_to(np.asarray(temperature, np.float32), (out.shape[0],)).reshape(-1, 1)
    assert (T > 0).all()
    nr = out.shape[1] // 3
    logit_probs = out[:, :nr] * (np.float32(1.0) / T)
    means = out[:, nr:2 * nr]
    log_scales = np.maximum(out[:, 2 * nr:3 * nr], np.float32(log_scale_min))
    scales = np.exp(log_scales) * T
    assert logit_probs.dtype == np.float32 and scales.dtype == np.float32
    rand = means + scales * (np.log(u) - np.log(1 - u))               # float64
    rand = rand * O.softmax_axis1(logit_probs)
    value = rand.sum(axis=1).astype(np.float32)
    value /= 127.5
    return np.clip(value, -1, 1)
