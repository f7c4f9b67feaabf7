"""Shared reference of the vector quantiser's domain tests (test_host_vq_domain.py, test_gpu_vq_domain.py): plain NumPy.

* seq_argmin      -- the reference's argmin (utils.py:189-207) restated over row blocks: float32 distances summed
                     sequentially over the channels, numpy.argmin's first minimum.
* make_inputs     -- seeded latents and codebook of a row of ROWS: ordinary rows, rows near a code, near-tie pairs
                     around the certainty band of the row's sweep, groups of exactly equal codes, and the scale /
                     degenerate variants.
* expected_paths  -- what csrc/vq.hip launches for a shape, restated from its predicates (NOT read from the library:
                     vqvae_vq_paths is compared with it).
* ROWS            -- one pytest.param per edge of those predicates.
"""
import zlib

import numpy as np
import pytest

# include/vqvae_hip.h VQVAE_VQ_PATH_*
PATH_X2, PATH_X3, PATH_REG, PATH_LDS4, PATH_LDS2, PATH_LDS1 = 0x001, 0x002, 0x004, 0x008, 0x010, 0x020
PATH_CAND, PATH_R8, PATH_TILE, PATH_SORT = 0x040, 0x080, 0x100, 0x200
PATH_BITS = dict(SWEEP_X2=PATH_X2, SWEEP_X3=PATH_X3, SWEEP_REG=PATH_REG, SWEEP_LDS4=PATH_LDS4, SWEEP_LDS2=PATH_LDS2,
                 SWEEP_LDS1=PATH_LDS1, CANDIDATES=PATH_CAND, RECHECK_R8=PATH_R8, GATHER_TILE=PATH_TILE, GRAD_SORT=PATH_SORT)
SWEEPS = PATH_X2 | PATH_X3 | PATH_REG | PATH_LDS4 | PATH_LDS2 | PATH_LDS1
MATMUL_CODES = {'float32': 0, 'bfloat16': 1, 'float32x3': 2, 'float32x2': 3}       # backend._MATMUL_CODES
REF_COST_MAX = 2.5e9            # N k d of a row: seq_argmin stays within ~3 s
U = 2.0 ** -24


def seq_argmin(rows, W):
    """rows (N, d), W (k, d) float32 -> (N,) int32: dist = 0; for c: dist = dist + (r[:, c, None] - W[None, :, c]) ** 2,
    everything float32, then argmin(axis=1) -- the order in which numpy.sum(axis=2) of utils.py:202 adds the channels of
    its (B, k, d, T', 1) operand (a reduction over an axis that is not the contiguous one adds slice by slice)."""
    rows, W = np.asarray(rows), np.asarray(W)
    assert rows.dtype == np.float32 and W.dtype == np.float32 and rows.shape[1] == W.shape[1]
    N, d = rows.shape
    k = W.shape[0]
    Wt = np.ascontiguousarray(W.T)
    out = np.empty(N, np.int32)
    step = max(1, (1 << 22) // k)
    for s in range(0, N, step):
        r = np.ascontiguousarray(rows[s:s + step].T)            # (d, n)
        dist = np.zeros((r.shape[1], k), np.float32)
        tmp = np.empty_like(dist)
        for c in range(d):
            np.subtract(r[c][:, None], Wt[c][None, :], out=tmp)
            np.multiply(tmp, tmp, out=tmp)
            np.add(dist, tmp, out=dist)
        out[s:s + step] = np.argmin(dist, axis=1)
    return out


def band_constant(d, dtype):
    """The certainty band of the sweep a shape takes is c (d + 4) u S (csrc/vq.hip): c = 16 for the fp32 MFMA sweeps,
    24 for the six bf16 products (d 64 / 128, matmul dtype 2), 17 for the three fp16 products (dtype 3)."""
    if d in (64, 128) and dtype >= 2:
        return 24.0 if dtype == 2 else 17.0
    return 16.0


def expected_paths(B, d, T, k, mode, dtype):
    """csrc/vq.hip's dispatch restated: the VQVAE_VQ_PATH_* bits of (B, d, T, k) under matmul dtype 0..3, -1 where mode 0
    refuses d."""
    N = B * T
    p = 0
    if mode == 0:
        dpad = d + (d & 1)
        if d in (64, 128):
            p |= PATH_X2 if dtype == 3 else PATH_X3 if dtype == 2 else PATH_REG
            if dtype >= 2 and k >= 1024 and N >= 1024:
                p |= PATH_CAND
        else:
            # NW wavefronts of 32 columns: dpad 32 NW + 32 (dpad + 1) floats within 150 KB of LDS
            for nw, bit in ((4, PATH_LDS4), (2, PATH_LDS2), (1, PATH_LDS1)):
                if dpad * (nw + 1) + 1 <= 1200:
                    p |= bit
                    break
            else:
                return -1
        if N > 8192:
            p |= PATH_R8
    if N >= 16384 and d <= 254 and B <= 65535:
        p |= PATH_TILE
    if not (N <= 8192 and N * k <= 2 ** 26):
        p |= PATH_SORT
    return p


# ---- rows ------------------------------------------------------------------------------------------------------------
# (name, kind, B, T, d, k, variant).  kind: 'once' (forward + gradient, the process's matmul mode), 'modes' (the same
# under the matmul_mode fixture), 'grad' (vqvae_vq_grad_w alone on seeded indices).
def _p(name, kind, B, T, d, k, variant='mix'):
    return pytest.param((name, kind, B, T, d, k, variant), id=name)


VARIANTS = ['scale-55', 'scale-40', 'scale40', 'codebook-20', 'code12', 'component12', 'zero_codebook', 'zero_latents', 'one_code']
ROWS = [
    # the LDS-staged sweep (every d but 64 / 128)
    _p('smallest_d1', 'once', 3, 7, 1, 5),
    _p('ragged_code_tile_d33', 'once', 2, 50, 33, 31),              # k < 32; batch boundary inside a column tile
    _p('d66_mod4_2', 'once', 3, 43, 66, 97),
    _p('nw4_d238', 'once', 2, 75, 238, 300),
    _p('nw2_d239', 'once', 2, 75, 239, 300),
    _p('nw2_d398', 'once', 2, 60, 398, 70),
    _p('nw1_d399', 'once', 2, 60, 399, 70),
    _p('default_model_d512', 'once', 4, 120, 512, 128),
    _p('widest_d598', 'once', 1, 40, 598, 33),
    _p('k1', 'once', 2, 9, 20, 1),
    _p('k2', 'once', 2, 9, 20, 2),
    # d 64 / 128: one of three sweeps by matmul mode
    _p('k1000_ragged_tile_wn4', 'modes', 2, 120, 64, 1000),         # k % 4 == 0, k % 64 != 0
    _p('cand_off_k1023', 'modes', 8, 128, 64, 1023),
    _p('cand_off_N1023', 'modes', 1, 1023, 64, 1024),
    _p('cand_on_1024', 'modes', 8, 128, 64, 1024),
    _p('cand_scalar_wn_k1026', 'modes', 11, 100, 128, 1026),        # k % 4 != 0, ragged 256-row block
    _p('k37_below_a_tile', 'modes', 2, 100, 128, 37),
    # re-check and gather tiers
    _p('recheck2_N8192', 'once', 2, 4096, 66, 97),
    _p('recheck8_N8193', 'once', 3, 2731, 66, 97),
    _p('gather_tile_d254', 'once', 2, 8192, 254, 33),
    _p('gather_plain_d255', 'once', 2, 8192, 255, 33),
    _p('N65600_grid_stride', 'once', 1, 65600, 8, 19),              # mode 1 beyond 65 535 rows, five sort chunks (T = 1025 x 64: whole gather tiles)
    _p('gather_tile_ragged', 'once', 1, 16400, 8, 19),              # a last gather tile of 16 rows, two sort chunks
]
for _v in VARIANTS:
    ROWS.append(_p('d64_' + _v, 'modes', 2, 120, 64, 512, _v))
    ROWS.append(_p('d128_' + _v, 'modes', 2, 120, 128, 1024, _v))
    ROWS.append(_p('d33_' + _v, 'once', 2, 50, 33, 31, _v))
ROWS += [
    _p('grad_scan_k8192', 'grad', 1, 8192, 4, 8192, 'random'),      # N k == 2^26
    _p('grad_sort_k8193', 'grad', 1, 8192, 4, 8193, 'random'),      # one chunk, N <= 8192
    _p('grad_one_chunk', 'grad', 1, 16384, 8, 40, 'random'),
    _p('grad_two_chunks', 'grad', 1, 16385, 8, 40, 'random'),
    _p('grad_8_pieces', 'grad', 1, 40000, 16, 3, 'code1'),          # 40 000 rows on code 1: the cap of 8 pieces (2048 each would be 20)
    _p('grad_sort_d300_k1100', 'grad', 2, 4200, 300, 1100, 'random'),   # ragged second channel slab, second 1024-code scan block
    _p('grad_scan_d300', 'grad', 2, 300, 300, 40, 'random'),
    _p('grad_scan_d66_P3', 'grad', 2, 300, 66, 40, 'random'),
    _p('grad_scan_d512', 'grad', 2, 300, 512, 128, 'random'),
]
FWD_ONCE = [p for p in ROWS if p.values[0][1] == 'once']
FWD_MODES = [p for p in ROWS if p.values[0][1] == 'modes']
GRAD_ROWS = [p for p in ROWS if p.values[0][1] == 'grad']
# equal codes in different MFMA tiles, half-waves and re-check threads; + (k-3, k-2) at the codebook's end, so that the LAST
# code stays one of a kind and can win: a row is planted beside it (a sweep that drops the end of a ragged tile shows there)
GROUPS = [(3, 35), (10, 74), (5, 261)]


def near_tie_pair(rs, row, gap):
    """Two codes at squared distance 1 and 1 + gap from `row` in random directions (float64 construction, rounded to
    float32): the pair of test_vq_near_ties_around_the_certainty_band for any d."""
    d = row.shape[0]
    ua, ub = rs.standard_normal(d), rs.standard_normal(d)
    ua /= np.linalg.norm(ua)
    ub /= np.linalg.norm(ub)
    return (row + ua).astype(np.float32), (row + np.sqrt(1.0 + gap) * ub).astype(np.float32)


def _groups(k):
    g = [p for p in GROUPS if p[1] < k - 3]
    if k >= 4:
        g.append((k - 3, k - 2))
    elif k >= 2:
        g.append((k - 2, k - 1))
    return g


def make_inputs(row, dtype=3, scale=None):
    """Seeded inputs of a forward row -> dict(z (B, d, T), W (k, d), rows (N, d) = the latents row-major, planted: the
    row ids that sit on a group of equal codes or between a near-tie pair, first: {row id: first code of its group}).
    dtype: the matmul dtype whose sweep sets the band the near-tie gaps are multiples of.  scale: a power of two applied
    to both tensors (default: the row's variant decides)."""
    name, kind, B, T, d, k, variant = row
    assert kind != 'grad'
    rs = np.random.RandomState(zlib.crc32(repr(row).encode()))
    N = B * T
    rows = rs.standard_normal((N, d)).astype(np.float32)
    W = (2.0 * rs.standard_normal((k, d))).astype(np.float32)          # far codes: squared distance ~ 5 d
    order = rs.permutation(N)
    groups = _groups(k)
    taken = set(j for g in groups for j in g) | {k - 1}
    free = [j for j in rs.permutation(k) if j not in taken]
    # a quarter of the rows (as far as the free codes reach) get a near-tie pair of their own
    npair = min(N // 4, len(free) // 2 - 1) if len(free) >= 4 else 0
    first, planted = {}, []
    for gi, (a, b) in enumerate(groups):
        W[b] = W[a]
        if gi < N:
            n = int(order[gi])
            rows[n] = W[a]                                              # exactly on both: the first must win
            first[n] = a
            planted.append(n)
    pair_rows = [int(n) for n in order[len(groups):len(groups) + npair]]
    last_row = int(order[-1]) if k >= 4 and N > len(groups) + npair else None
    if last_row is not None:                                            # beside the last code (not `planted`: no tie to re-check)
        rows[last_row] = W[k - 1] + np.float32(0.25) * rs.standard_normal(d).astype(np.float32)
    # near a code (golden.make_golden.stress_inputs): half of what is left
    rest = order[len(groups) + npair:N - 1] if last_row is not None else order[len(groups) + npair:]
    near = rest[:len(rest) // 2]
    far_codes = free[2 * npair:]
    if len(near) and len(far_codes):
        j = np.asarray(far_codes)[rs.randint(0, len(far_codes), len(near))]
        rows[near] = W[j] + np.float32(0.5) * rs.standard_normal((len(near), d)).astype(np.float32)
    # the pairs: gaps relative to the band of this row's sweep, c (d + 4) u S_n with S_n = |z_n|^2 + max_j |w_j|^2 as the
    # kernels take it (the planted codes stay below the far codes' largest norm except by chance; S_n is recomputed below)
    c = band_constant(d, dtype)
    mult = np.array([1e-7, 1e-4, 0.5, 0.9, 1.1, 2.0, 8.0])[rs.randint(0, 7, max(npair, 1))]
    wmax = float((W.astype(np.float64) ** 2).sum(1).max())
    seeds = rs.randint(0, 2 ** 31 - 1, max(npair, 1))
    for i, n in enumerate(pair_rows):
        S_n = float((rows[n].astype(np.float64) ** 2).sum()) + wmax
        gap = mult[i] if mult[i] < 1e-3 else mult[i] * c * (d + 4) * U * S_n
        W[free[2 * i]], W[free[2 * i + 1]] = near_tie_pair(np.random.RandomState(seeds[i]), rows[n], gap)
        planted.append(n)
    # |values| <= 2 before the variant, so that scale 2^40 stays at 2^41
    top = max(float(np.abs(rows).max()), float(np.abs(W).max()))
    shrink = np.float32(2.0 ** -int(np.ceil(np.log2(top / 2.0)))) if top > 2.0 else np.float32(1.0)
    rows, W = rows * shrink, W * shrink
    if variant == 'codebook-20':
        W = W * np.float32(2.0 ** -20)
    elif variant == 'code12':
        W[free[-1]] *= np.float32(2.0 ** 12)
    elif variant == 'component12':
        rows[order[::4], rs.randint(0, d)] *= np.float32(2.0 ** 12)
    elif variant == 'zero_codebook':
        W = np.zeros_like(W)
    elif variant == 'zero_latents':
        rows = np.zeros_like(rows)
    elif variant == 'one_code':
        W = np.repeat(W[free[-1]][None], k, axis=0)
    if scale is None:
        scale = 2.0 ** int(variant[5:]) if variant.startswith('scale') else 1.0
    rows, W = np.ascontiguousarray(rows * np.float32(scale)), np.ascontiguousarray(W * np.float32(scale))
    assert np.isfinite(rows).all() and np.isfinite(W).all()
    assert max(np.abs(rows).max(), np.abs(W).max()) <= 2.0 ** 41
    z = np.ascontiguousarray(rows.reshape(B, T, d).transpose(0, 2, 1))
    if variant != 'mix' and not variant.startswith('scale'):
        first = {}                                                      # the variant moved the codes: seq_argmin alone decides
    return dict(z=z, W=W, rows=rows, planted=np.array(sorted(planted), np.int64), first=first, last_row=last_row)


def recheck_facts(inp, d):
    """From the final tensors, in float64: (must, has_far).  must: the planted rows (on a group of equal codes, or between
    a near-tie pair) whose two nearest codes are closer than 0.9 x the fp32 band 16 (d + 4) u S_n -- every sweep's band
    is at least that wide, and its distances are within a small part of it, so each of them is re-checked.  has_far: some
    row's two nearest codes are more than 4 x the widest band (24) apart, so it cannot be: n_rechecked < N."""
    rows, W = inp['rows'].astype(np.float64), inp['W'].astype(np.float64)
    k = W.shape[0]
    if k < 2:
        return 0, True
    wn = (W ** 2).sum(1)
    zn = (rows ** 2).sum(1)
    S = zn + wn.max()
    must, far = 0, False
    planted = set(inp['planted'].tolist())
    for s in range(0, rows.shape[0], 4096):
        r = rows[s:s + 4096]
        dist = ((r[:, None, :] - W[None]) ** 2).sum(2) if r.shape[0] * k * W.shape[1] <= 1 << 24 else \
            np.maximum(zn[s:s + 4096, None] - 2.0 * r @ W.T + wn[None], 0.0)
        two = np.partition(dist, 1, axis=1)[:, :2]
        gap = two[:, 1] - two[:, 0]
        far = far or bool((gap > 4 * 24.0 * (d + 4) * U * S[s:s + 4096]).any())
        near = gap < 0.9 * 16.0 * (d + 4) * U * S[s:s + 4096]
        must += sum(1 for i in np.nonzero(near)[0] if s + int(i) in planted)
    return must, far


def grad_inputs(row, idx=None):
    """Seeded gy (B, d, T) whose channels span 10^+-3, and for a gradient-only row its indices (B, T)."""
    name, kind, B, T, d, k, variant = row
    rs = np.random.RandomState(zlib.crc32(('gy' + repr(row)).encode()))
    if idx is None:
        idx = rs.randint(0, k, size=(B, T)).astype(np.int32)
        if variant == 'code1':
            idx[:] = 1
    gy = (rs.standard_normal((B, d, T)) * 10.0 ** rs.uniform(-3, 3, size=(B, d, 1))).astype(np.float32)
    return np.ascontiguousarray(idx.reshape(B, T).astype(np.int32)), gy


def grad_reference(idx, gy, k):
    """gW = onehot(idx)^T gy accumulated in float64 (utils.py:227-228) -> (float64 (k, d), the codes in use)."""
    B, d, T = gy.shape
    want = np.zeros((k, d), np.float64)
    np.add.at(want, idx.reshape(-1), gy.transpose(0, 2, 1).reshape(-1, d).astype(np.float64))
    used = np.zeros(k, bool)
    used[idx.reshape(-1)] = True
    return want, used


# ---- the C ABI on resident arrays (GPU tests) ---------------------------------------------------------------------
def vq_indices(gpu, z_dev, W_dev, B, d, T, k, mode, e_dev=None):
    """vqvae_vq_nearest_fwd through the C ABI on resident inputs -> (idx host (B, T), rows re-checked)."""
    from vqvae_amd import _lib
    from vqvae_amd.backend import DeviceArray
    idx = DeviceArray((B, T), np.int32)
    nre = DeviceArray((1,), np.int32)
    ws = gpu.workspace(_lib.load().vqvae_vq_workspace_bytes(B, d, T, k))
    _lib.call('vqvae_vq_nearest_fwd', z_dev.ptr, W_dev.ptr, B, d, T, k, mode, idx.ptr, None if e_dev is None else e_dev.ptr,
              nre.ptr, ws.ptr, ws.nbytes, gpu.stream())
    return idx.get(), int(nre.get()[0])
