"""The vector quantiser (csrc/vq.hip) through the C ABI, one row per edge of its dispatch (tests/vq_domain_ref.py ROWS): the
three sweep families and the LDS sweep's three tiers, ragged code tiles, the candidate pass, both re-check batchings, both
gathers, mode 1's grid stride, both forms of the codebook gradient with their chunking, pieces and channel slabs, and
inputs far from O(1).  The reference is vq_domain_ref.seq_argmin -- the reference's float32 order and numpy.argmin, checked
against the oracle and the golden files in test_host_vq_domain.py -- and numpy.add.at in float64 for the gradient: neither
is the code under test nor its mode 1.  Every row first asserts the path it is here for (vqvae_vq_paths against the
restated predicates), so a row that drifts onto another kernel fails instead of passing vacuously."""
import numpy as np
import pytest

import vq_domain_ref as R

pytestmark = pytest.mark.gpu

_CASES, _GRADS = {}, {}


def _L():
    from vqvae_amd import _lib
    return _lib


def _case(row, dtype):
    """Inputs and references of a forward row; they depend on the matmul dtype only through the band constant the
    near-tie gaps are multiples of, so the modes that share a sweep share the reference."""
    name, kind, B, T, d, k, variant = row
    key = (row, R.band_constant(d, dtype))
    if key not in _CASES:
        inp = R.make_inputs(row, dtype)
        inp['ref'] = R.seq_argmin(inp['rows'], inp['W'])
        assert 0 <= inp['ref'].min() and inp['ref'].max() < k
        for n, j in inp['first'].items():
            assert inp['ref'][n] == j                   # the first of a group of equal codes
        if inp['last_row'] is not None and variant == 'mix':
            assert inp['ref'][inp['last_row']] == k - 1  # the row planted beside the last code
        inp['must'], inp['far'] = R.recheck_facts(inp, d)
        for a in ('z', 'W', 'rows', 'ref'):
            inp[a].setflags(write=False)
        _CASES[key] = inp
    return _CASES[key]


def _grad_case(row, idx=None):
    name, kind, B, T, d, k, variant = row
    key = (row, None if idx is None else idx.tobytes())
    if key not in _GRADS:
        idx, gy = R.grad_inputs(row, idx)
        want64, used = R.grad_reference(idx, gy, k)
        _GRADS[key] = (idx, gy, want64.astype(np.float32), used)
    return _GRADS[key]


def _check_paths(row, mode, dtype):
    name, kind, B, T, d, k, variant = row
    p = _L().load().vqvae_vq_paths(B, d, T, k, mode)
    assert p == R.expected_paths(B, d, T, k, mode, dtype), (name, mode, hex(p))
    return p


def _check_gradient(gpu, row, idx, tag):
    """Step 6: vqvae_vq_grad_w == the float64 scatter-add rounded once, bit for bit (float64 sums of a few 10^4 float32
    terms differ between summation orders by < 2^-40 relative: another float32 rounding needs a sum that close to a
    rounding boundary), accumulate 0 and 1, unused codes exactly 0 / untouched, two calls identical."""
    name, kind, B, T, d, k, variant = row
    idx, gy, want, used = _grad_case(row, idx)
    assert idx.min() >= 0 and idx.max() < k
    lib = _L()
    sort = bool(lib.load().vqvae_vq_paths(B, d, T, k, 1) & R.PATH_SORT)
    assert sort == (not (B * T <= 8192 and B * T * k <= 2 ** 26)), name
    d_idx, d_gy = gpu.to_device(idx), gpu.to_device(gy)
    ws = gpu.workspace(lib.load().vqvae_vq_workspace_bytes(B, d, T, k))
    outs = []
    for _ in range(2):
        gW = gpu.to_device(np.full((k, d), np.nan, np.float32))
        lib.call('vqvae_vq_grad_w', d_idx.ptr, d_gy.ptr, B, d, T, k, gW.ptr, 0, ws.ptr, ws.nbytes, gpu.stream())
        outs.append(gW.get())
    np.testing.assert_array_equal(outs[0], outs[1])
    mism = int((outs[0] != want).sum())
    print('%s %s: gW entries off the float64 scatter-add: %d of %d' % (name, tag, mism, want.size))
    assert mism == 0, '%s %s: %d of %d entries differ from the float64 scatter-add' % (name, tag, mism, want.size)
    assert not outs[0][~used].any()
    iW = np.random.RandomState(k + d).standard_normal((k, d)).astype(np.float32)
    gW = gpu.to_device(iW)
    lib.call('vqvae_vq_grad_w', d_idx.ptr, d_gy.ptr, B, d, T, k, gW.ptr, 1, ws.ptr, ws.nbytes, gpu.stream())
    got = gW.get()
    np.testing.assert_array_equal(got, iW + want)               # one float32 rounding
    np.testing.assert_array_equal(got[~used], iW[~used])


def _run_forward_row(gpu, row):
    name, kind, B, T, d, k, variant = row
    N = B * T
    dtype = _L().load().vqvae_get_matmul_dtype()
    # 1. the path this row is here for
    p0, p1 = _check_paths(row, 0, dtype), _check_paths(row, 1, dtype)
    assert p0 >= 0 and bin(p0 & R.SWEEPS).count('1') == 1 and not p1 & (R.SWEEPS | R.PATH_CAND | R.PATH_R8)
    inp = _case(row, dtype)
    ref = inp['ref'].reshape(B, T)
    zd, Wd = gpu.to_device(inp['z']), gpu.to_device(inp['W'])
    # 2. + 3. indices alone (e = NULL): inside [0, k) before anything else sees them, then the reference's, row for row
    nre = {}
    for mode in (0, 1):
        idx, nre[mode] = R.vq_indices(gpu, zd, Wd, B, d, T, k, mode)
        assert idx.shape == (B, T) and idx.min() >= 0 and idx.max() < k, (name, mode, int(idx.min()), int(idx.max()))
        bad = np.nonzero(idx.reshape(-1) != inp['ref'])[0]
        print('%s mode %d: %d of %d indices off the reference, %d rows re-checked' % (name, mode, bad.size, N, nre[mode]))
        assert bad.size == 0, '%s mode %d: %d of %d rows differ from the reference, first %s (got %s, want %s)' % (
            name, mode, bad.size, N, bad[:5], idx.reshape(-1)[bad[:5]], inp['ref'][bad[:5]])
    # 4. with the gather
    want_e = np.ascontiguousarray(inp['W'][ref].transpose(0, 2, 1))
    for mode in (0, 1):
        e = gpu.to_device(np.full((B, d, T), np.nan, np.float32))
        idx, _ = R.vq_indices(gpu, zd, Wd, B, d, T, k, mode, e)
        np.testing.assert_array_equal(idx, ref)
        got = e.get()
        assert got.tobytes() == want_e.tobytes(), '%s mode %d: e is not W[idx] bit for bit' % (name, mode)
    # 5. the rows that had to take the exact re-check did
    assert nre[1] == 0
    assert inp['must'] <= nre[0] <= N, (name, nre[0], inp['must'])
    if inp['far']:
        assert nre[0] < N, (name, nre[0])
    # 6. the codebook gradient on these indices
    _check_gradient(gpu, row, ref, 'dtype %d' % dtype)


@pytest.mark.parametrize('row', R.FWD_ONCE)
def test_vq_row(gpu, row):
    _run_forward_row(gpu, row)


@pytest.mark.parametrize('row', R.FWD_MODES)
def test_vq_row_in_three_matmul_modes(gpu, matmul_mode, row):
    name, kind, B, T, d, k, variant = row
    assert _L().load().vqvae_get_matmul_dtype() == R.MATMUL_CODES[matmul_mode]
    sweep = {'float32x2': R.PATH_X2, 'float32x3': R.PATH_X3, 'float32': R.PATH_REG}[matmul_mode]
    assert _L().load().vqvae_vq_paths(B, d, T, k, 0) & R.SWEEPS == sweep
    _run_forward_row(gpu, row)


@pytest.mark.parametrize('row', R.GRAD_ROWS)
def test_vq_grad_row(gpu, row):
    name, kind, B, T, d, k, variant = row
    _check_gradient(gpu, row, None, 'seeded indices')
    if variant == 'code1':
        idx, gy, want, used = _grad_case(row)
        assert used.tolist() == [False, True, False]            # codes 0 and 2 stayed exactly zero above


def test_vq_d599_mode0_refuses_and_the_rest_works(gpu):
    """One channel beyond the widest LDS-staged sweep: mode 0 returns an error that names d and writes nothing; mode 1 and
    the gradient have no such limit."""
    row = ('d599', 'once', 2, 30, 599, 40, 'mix')
    name, kind, B, T, d, k, variant = row
    lib = _L().load()
    assert lib.vqvae_vq_paths(B, d, T, k, 0) == -1 and lib.vqvae_vq_paths(B, d, T, k, 1) == 0
    inp = _case(row, lib.vqvae_get_matmul_dtype())
    zd, Wd = gpu.to_device(inp['z']), gpu.to_device(inp['W'])
    idx = gpu.to_device(np.full((B, T), -7, np.int32))
    ws = gpu.workspace(lib.vqvae_vq_workspace_bytes(B, d, T, k))
    rc = lib.vqvae_vq_nearest_fwd(zd.ptr, Wd.ptr, B, d, T, k, 0, idx.ptr, None, None, ws.ptr, ws.nbytes, gpu.stream())
    assert rc != 0
    msg = lib.vqvae_last_error_string().decode()
    assert 'd=599' in msg, msg
    assert (idx.get() == -7).all()
    e = gpu.to_device(np.full((B, d, T), np.nan, np.float32))
    got, nre = R.vq_indices(gpu, zd, Wd, B, d, T, k, 1, e)
    assert got.min() >= 0 and got.max() < k
    np.testing.assert_array_equal(got.reshape(-1), inp['ref'])
    assert nre == 0
    np.testing.assert_array_equal(e.get(), inp['W'][got].transpose(0, 2, 1))
    _check_gradient(gpu, row, got, 'after mode 1')
