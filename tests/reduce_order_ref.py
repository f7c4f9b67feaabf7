"""NumPy float32 restatements of the fixed summation orders of the library's partial-sum reduces (csrc/wgrad.hip
wgrad_reduce_kernel, csrc/conv_api.hip pullback_reduce_kernel).  float32 + float32 in NumPy is the IEEE operation the
device performs, so a result computed here from the partials the device left is the device's result bit for bit, or
the order moved."""
import numpy as np

TILE = 128                # slab tiles are TILE x TILE floats, bias slabs rows of TILE-padded length


def cdiv(a, b):
    return (a + b - 1) // b


def wgrad_reduce(parts):
    """parts: float32 (nsplit, ...) -> float32 (...).  Four groups g = 0..3; group g adds splits g, g+16, ... into v0,
    g+4, g+20, ... into v1, g+8, ... into v2 and g+12, ... into v3 while sp + 12 < nsplit, its leftover splits (stepping
    by 4) all into v0; the group is (v0+v1)+(v2+v3), the result (g0+g1)+(g2+g3).  Every accumulator starts at +0."""
    parts = np.asarray(parts)
    assert parts.dtype == np.float32
    nsplit = parts.shape[0]
    groups = []
    with np.errstate(all='ignore'):
        for g in range(4):
            v = [np.zeros(parts.shape[1:], np.float32) for _ in range(4)]
            sp = g
            while sp + 12 < nsplit:
                for j in range(4):
                    v[j] = v[j] + parts[sp + 4 * j]
                sp += 16
            while sp < nsplit:
                v[0] = v[0] + parts[sp]
                sp += 4
            groups.append((v[0] + v[1]) + (v[2] + v[3]))
        return (groups[0] + groups[1]) + (groups[2] + groups[3])


def wgrad_slab_floats(M, cins):
    """floats of one split's weight slabs ([tile row][tile column][TILE][TILE]; every segment starts a new tile column)"""
    return cdiv(M, TILE) * sum(cdiv(c, TILE) for c in cins) * TILE * TILE


def wgrad_bias_floats(M, nseg):
    """floats of one split's bias slabs ([segment][TILE-padded M])"""
    return nseg * cdiv(M, TILE) * TILE


def wgrad_outputs(ws, nsplit, M, cins, with_bias):
    """What the reduce writes, recomputed from the workspace a weight-gradient launch left (float32, flat): the slabs
    [nsplit][tile row][tile column][TILE][TILE] from its start, then (launches with a bias output) the bias slabs
    [nsplit][segment][padded M].  Returns ([segment] -> (M, cin) float32, [segment] -> (M,) float32 or None)."""
    tm, nseg = cdiv(M, TILE), len(cins)
    tn = sum(cdiv(c, TILE) for c in cins)
    nslab = nsplit * tm * tn * TILE * TILE
    slabs = ws[:nslab].reshape(nsplit, tm, tn, TILE, TILE)
    full = wgrad_reduce(slabs).transpose(0, 2, 1, 3).reshape(tm * TILE, tn * TILE)
    gw, col = [], 0
    for c in cins:
        gw.append(full[:M, col:col + c])
        col += cdiv(c, TILE) * TILE
    gb = None
    if with_bias:
        b = wgrad_reduce(ws[nslab:nslab + nsplit * nseg * tm * TILE].reshape(nsplit, nseg, tm * TILE))
        gb = [b[s, :M] for s in range(nseg)]
    return gw, gb


def pullback_reduce(part, v0, Tl):
    """part: float32 (nblocks, B, nt, Cd, 4), the sums every 128-column tile left for the four latent positions
    v0[128 n] .. v0[128 n] + 3 under it -> (B, nblocks, Cd, Tl): every output starts at +0 and collects its tiles in
    ascending tile order (positions >= Tl are dropped)."""
    part = np.asarray(part)
    assert part.dtype == np.float32
    nblocks, B, nt, Cd, _ = part.shape
    out = np.zeros((nblocks, B, Cd, Tl), np.float32)
    with np.errstate(all='ignore'):
        for n in range(nt):
            vb = int(v0[n * TILE])
            for k in range(4):
                if vb + k < Tl:
                    out[:, :, :, vb + k] = out[:, :, :, vb + k] + part[:, :, n, :, k]
    return out.transpose(1, 0, 2, 3)
