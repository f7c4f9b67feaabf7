"""The reduces that finish a split launch add their partial results in a documented, fixed order (the step's
determinism rests on it).  Each test lets a public entry point run, reads the partials back -- they stay in the caller's
workspace -- recomputes every output from them in the restated order (tests/reduce_order_ref.py) and compares BITS."""
import ctypes as C

import numpy as np
import pytest

import reduce_order_ref as R

pytestmark = pytest.mark.gpu

MODES = {3: 'float32x2', 2: 'float32x3', 0: 'float32'}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _nsplit_from_workspace(lib, _lib, M, B, T, cin, K, nblocks):
    """The split count of the weight-gradient launch over nblocks * K segments of `cin` input channels, M output rows and
    (B, T) positions, from the workspace the library asks for: vqvae_resstack_dil_wgrad_workspace_bytes is that launch's
    slabs (nsplit x (weight slabs + bias slabs)) + 256, and the generic conv plans its launch from the same numbers."""
    d = _lib.ResblockDesc(B, T, cin, M, 64, 64, K, 1)
    by = int(lib.vqvae_resstack_dil_wgrad_workspace_bytes(C.byref(d), nblocks)) - 256
    nseg = nblocks * K
    per = 4 * (R.wgrad_slab_floats(M, [cin] * nseg) + R.wgrad_bias_floats(M, nseg))
    assert by > 0 and by % per == 0, (by, per)
    return by // per


# (entry point, matmul mode, B, T, M, cin, K, blocks, accumulate, bias, nsplit this (B, T) gives)
# nsplit: one split per 4 K steps of 32 positions while tiles x splits stay below one residency round, i.e. B T / 128
# here -- 1, 2, 3 (a group with no split at all, the tail loop alone), 4, 5, 13 (tails of 4, 3, 3, 3), 16 (one full
# round of the unrolled loop, no tail), 17 (one round for group 0 ... and a tail), 29 and 30 (a round, then 13 / 14 left:
# group 0 (and 1) takes a second round, the others tail)
WGRAD_CASES = [
    ('conv', 3, 1, 128, 64, 64, 1, 1, 0, True, 1),
    ('conv', 2, 1, 256, 192, 192, 2, 1, 0, False, 2),
    ('conv', 0, 1, 384, 256, 128, 3, 1, 1, True, 3),
    ('conv', 3, 2, 256, 256, 256, 1, 1, 0, True, 4),
    ('conv', 2, 1, 640, 64, 192, 1, 1, 1, False, 5),
    ('conv', 0, 1, 640, 64, 130, 1, 1, 0, True, 5),            # a row of outputs that ends inside a lane's four
    ('dil', 2, 1, 1664, 192, 128, 2, 2, 0, True, 13),
    ('dil', 0, 2, 1024, 256, 64, 2, 2, 1, False, 16),
    ('dil', 3, 1, 2176, 64, 256, 2, 1, 0, True, 17),
    ('dil', 2, 2, 1856, 256, 192, 2, 2, 1, True, 29),
    ('conv', 3, 1, 3840, 192, 64, 2, 1, 0, True, 30),
]


@pytest.mark.parametrize('case', WGRAD_CASES, ids=lambda c: '%s_m%d_B%d_T%d_M%d_c%d_K%d_n%d_acc%d_b%d_ns%d' % c)
def test_weight_gradient_reduce_order(gpu, case):
    """vqvae_conv1d_bwd_weight (one segment per tap, output strides K) and vqvae_resstack_dil_wgrad (blocks x taps
    segments, one bias output per block): every weight- and bias-gradient entry is the restated sum of the partial slabs
    the launch left in the workspace, to the bit -- M = 64 / 192 / 256 (padded slab rows), cin = 64 / 128 / 192 / 256
    (padded columns, a second tile per segment), accumulate over a non-zero gradient, with and without bias outputs,
    matmul modes 3, 2 and 0."""
    from vqvae_amd import _lib
    from vqvae_amd.backend import DeviceArray
    lib = _lib.load()
    kind, mode, B, T, M, cin, K, nblocks, acc, bias, want_ns = case
    gpu.set_matmul_dtype(MODES[mode])
    gpu.set_f32x2_min_gflop(0.0)
    try:
        nsplit = _nsplit_from_workspace(lib, _lib, M, B, T, cin, K, nblocks)
        assert nsplit == want_ns
        rs = np.random.RandomState(B * T + M + cin)
        x = [gpu.to_device(rs.standard_normal((B, cin, T)).astype(np.float32)) for _ in range(nblocks)]
        gy = [gpu.to_device(rs.standard_normal((B, M, T)).astype(np.float32)) for _ in range(nblocks)]
        gW0 = [rs.standard_normal((M, cin, K)).astype(np.float32) for _ in range(nblocks)]
        gb0 = [rs.standard_normal(M).astype(np.float32) for _ in range(nblocks)]
        gW = [gpu.to_device(a) for a in gW0]
        gb = [gpu.to_device(a) for a in gb0] if bias else None
        if kind == 'conv':
            d = _lib.Conv1dDesc(B, cin, T, M, T, K, 1, K - 1, 1, 0)
            ws = DeviceArray((lib.vqvae_conv1d_workspace_bytes(C.byref(d)) // 4 + 1,), np.float32)
            _lib.call('vqvae_conv1d_bwd_weight', C.byref(d), x[0].ptr, gy[0].ptr, gW[0].ptr, gb[0].ptr if bias else None,
                      acc, ws.ptr, ws.nbytes, gpu.stream())
            bias_seg = [0]
        else:
            d = _lib.ResblockDesc(B, T, cin, M, 64, 64, K, 1)
            ws = DeviceArray((lib.vqvae_resstack_dil_wgrad_workspace_bytes(C.byref(d), nblocks) // 4 + 1,), np.float32)
            dils = (C.c_int * nblocks)(*[2 ** i for i in range(nblocks)])
            _lib.call('vqvae_resstack_dil_wgrad', C.byref(d), nblocks, dils, _lib.ptr_array(x), _lib.ptr_array(gy),
                      _lib.ptr_array(gW), _lib.ptr_array(gb) if bias else None, acc, ws.ptr, ws.nbytes, None, None,
                      gpu.stream())
            bias_seg = [l * K for l in range(nblocks)]
        want_w, want_b = R.wgrad_outputs(ws.get().reshape(-1), nsplit, M, [cin] * (nblocks * K), bias)
        assert all(np.isfinite(w).all() and np.abs(w).max() > 0 for w in want_w)
        for l in range(nblocks):
            got = gW[l].get().reshape(M, cin, K)
            for j in range(K):
                w = want_w[l * K + j]
                if acc:
                    w = gW0[l][:, :, j] + w
                np.testing.assert_array_equal(_bits(got[:, :, j]), _bits(w), 'gW, block %d tap %d' % (l, j))
            if bias:
                b = want_b[bias_seg[l]]
                assert np.abs(b).max() > 0
                if acc:
                    b = gb0[l] + b
                np.testing.assert_array_equal(_bits(gb[l].get().reshape(M)), _bits(b), 'gb, block %d' % l)
    finally:
        gpu.set_f32x2_min_gflop(8.0)
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())


# (blocks, B, T, Cd, Tl, non-finite partials)
PULLBACK_CASES = [(1, 1, 128, 64, 2, False), (3, 2, 384, 128, 6, False), (1, 2, 384, 64, 2, False),
                  (3, 1, 128, 128, 2, False), (3, 2, 384, 64, 6, True)]


@pytest.mark.parametrize('case', PULLBACK_CASES, ids=lambda c: 'n%d_B%d_T%d_Cd%d_Tl%d_inf%d' % c)
def test_pullback_reduce_order(gpu, case):
    """vqvae_pullback_reduce_into on seeded random partials: every output is 0 + its tiles in ascending tile order, to
    the bit.  The last case plants an inf and values near the float32 maximum: the sums overflow or not, and turn NaN or
    not, by the order they are taken in, so order and not value is what is compared."""
    from vqvae_amd import _lib, functions as F
    nblocks, B, T, Cd, Tl, nonfinite = case
    nt = T // 128
    rs = np.random.RandomState(nblocks * 1000 + B * 100 + T + Tl)
    part = rs.standard_normal((nblocks, B, nt, Cd, 4)).astype(np.float32)
    if nonfinite:
        with np.errstate(over='ignore'):
            part *= np.float32(1.5e38)                     # two of a sign overflow: (a + b) + c != a + (b + c)
        part[1, 0, 1, 5, 2] = np.inf
        part[2, 1, 0, 7, 1] = -np.inf
    tb = F.resize_tables(Tl, T)
    v0 = F.resize_tables_host(Tl, T)['v0']
    bstride = nblocks * Cd * Tl + 8                        # a batch stride wider than the rows written
    gP = gpu.to_device(np.full((B, bstride), 7.0, np.float32))
    _lib.call('vqvae_pullback_reduce_into', gpu.to_device(part).ptr, tb['v0'].ptr, nblocks, B, T, Cd, Tl, gP.ptr, bstride,
              gpu.stream())
    got = gP.get().reshape(B, bstride)
    want = R.pullback_reduce(part, v0, Tl).reshape(B, nblocks * Cd * Tl)
    if nonfinite:
        assert np.isinf(want).any() and np.isnan(want).any() and np.isfinite(want).any()
    np.testing.assert_array_equal(_bits(got[:, :nblocks * Cd * Tl]), _bits(want))
    np.testing.assert_array_equal(got[:, nblocks * Cd * Tl:], 7.0)
