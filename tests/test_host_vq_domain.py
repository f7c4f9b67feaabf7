"""The vector quantiser's domain rows without a GPU: the shared reference (vq_domain_ref.seq_argmin) against the oracle's
verbatim restatement of the reference and its golden files, the dispatch query vqvae_vq_paths against the predicates
restated in Python, and the coverage of tests/test_gpu_vq_domain.py's rows -- every path bit is reached and every tier bit
is also absent somewhere, so no row of the GPU file passes vacuously."""
import os
import re

import numpy as np
import pytest

import vq_domain_ref as R
import vqvae_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
ALL = [p.values[0] for p in R.ROWS]


def _lib():
    from vqvae_amd import _lib
    return _lib.load()


def _oracle_idx(rows, W, B, T):
    d = rows.shape[1]
    z = np.ascontiguousarray(rows.reshape(B, T, d).transpose(0, 2, 1))
    return O.vq_forward(z, W)[1].reshape(-1)


@pytest.mark.parametrize('name', ['vq_train', 'vq_3d', 'vq_ties'])
def test_seq_argmin_equals_the_golden_indices(name):
    """The three golden shapes: indices written by the reference's own code (tests/golden/make_golden.py)."""
    g = np.load(os.path.join(GOLD, name + '.npz'))
    z = g['z'].reshape(g['z'].shape[:3])
    B, d, T = z.shape
    rows = np.ascontiguousarray(z.transpose(0, 2, 1).reshape(-1, d))
    np.testing.assert_array_equal(R.seq_argmin(rows, g['W']), g['idx'].reshape(-1))
    np.testing.assert_array_equal(R.seq_argmin(rows, g['W']), _oracle_idx(rows, g['W'], B, T))


@pytest.mark.parametrize('B,T,d,k', [(3, 7, 1, 5), (2, 1, 9, 40), (1, 1, 64, 70), (2, 9, 20, 1), (2, 9, 20, 2), (2, 50, 33, 31),
                                     (3, 43, 66, 97), (1, 40, 250, 100), (2, 120, 17, 300)])
def test_seq_argmin_equals_the_oracle_on_planted_ties(B, T, d, k):
    """make_inputs' mix (equal codes, near-tie pairs down to 1e-7 relative, rows near a code) plus 1-ulp perturbations of
    duplicated codes, on shapes small enough for oracle.vq_forward's (B, k, d, T) temporaries.  T = 1 is included: the
    two agree there as well (numpy.sum(axis=2) adds the channels slice after slice, not pairwise); ROWS still keeps
    T >= 2, the layout the golden files pin."""
    inp = R.make_inputs(('host', 'once', B, T, d, k, 'mix'))
    rows, W = inp['rows'].copy(), inp['W'].copy()
    rs = np.random.RandomState(B * 1000 + k)
    for _ in range(min(k // 2, 8)):                      # a copy of a code, one component moved by one ulp, and a row on the original
        a, b = rs.randint(0, k, 2)
        if a == b:
            continue
        W[b] = W[a]
        c = rs.randint(0, d)
        W[b, c] = np.nextafter(W[a, c], np.float32(np.inf if rs.randint(0, 2) else -np.inf))
        rows[rs.randint(0, B * T)] = W[a]
    got = R.seq_argmin(rows, W)
    np.testing.assert_array_equal(got, _oracle_idx(rows, W, B, T))
    assert got.min() >= 0 and got.max() < k
    # the unperturbed inputs: a row on a group of equal codes returns the first of them
    ref = R.seq_argmin(inp['rows'], inp['W'])
    for n, j in inp['first'].items():
        assert ref[n] == j, (n, j, ref[n])
    if k >= 4:
        assert inp['first']


def test_scale_is_exact_and_keeps_the_reference_index():
    """A power-of-two scale of both tensors changes no float32 relation while nothing under- or overflows: 2^40 and
    2^-40 leave the reference's indices where they are (2^-55 squares into the subnormals and may not)."""
    row = ('host_scale', 'once', 2, 50, 33, 31, 'mix')
    base = R.make_inputs(row)
    want = R.seq_argmin(base['rows'], base['W'])
    for s in (2.0 ** 40, 2.0 ** -40):
        inp = R.make_inputs(row, scale=s)
        np.testing.assert_array_equal(inp['rows'], base['rows'] * np.float32(s))
        np.testing.assert_array_equal(R.seq_argmin(inp['rows'], inp['W']), want)


def test_header_bits_are_the_modules():
    text = open(os.path.join(ROOT, 'include', 'vqvae_hip.h')).read()
    bits = {m.group(1): int(m.group(2), 16) for m in re.finditer(r'#define VQVAE_VQ_PATH_(\w+) (0x[0-9a-fA-F]+)', text)}
    assert bits == R.PATH_BITS
    assert sorted(bits.values()) == [1 << i for i in range(10)]


@pytest.mark.parametrize('dtype', [0, 1, 2, 3])
def test_paths_query_equals_the_restated_predicates(dtype):
    lib = _lib()
    before = lib.vqvae_get_matmul_dtype()
    assert lib.vqvae_set_matmul_dtype(dtype) == 0
    try:
        for name, kind, B, T, d, k, variant in ALL:
            for mode in (0, 1):
                assert lib.vqvae_vq_paths(B, d, T, k, mode) == R.expected_paths(B, d, T, k, mode, dtype), (name, mode, dtype)
        # the tier edges on their own, beside the rows: every d around them, every threshold of N and k from both sides
        for d in (1, 2, 63, 64, 65, 127, 128, 129, 237, 238, 239, 240, 397, 398, 399, 400, 597, 598):
            for (B, T, k) in [(1, 1023, 1024), (1, 1024, 1023), (1, 1024, 1024), (2, 4096, 8192), (1, 8193, 3), (1, 16383, 3),
                              (1, 16384, 3), (65536, 1, 3), (65535, 1, 3), (1, 8192, 8193)]:
                for mode in (0, 1):
                    assert lib.vqvae_vq_paths(B, d, T, k, mode) == R.expected_paths(B, d, T, k, mode, dtype), (B, d, T, k, mode)
    finally:
        lib.vqvae_set_matmul_dtype(before)


def test_d599_is_refused_by_the_sweep_alone():
    lib = _lib()
    for d in (599, 600, 1000):
        assert R.expected_paths(2, d, 30, 40, 0, 3) == -1
        assert lib.vqvae_vq_paths(2, d, 30, 40, 0) == -1
        assert lib.vqvae_vq_paths(2, d, 30, 40, 1) == 0 == R.expected_paths(2, d, 30, 40, 1, 3)
    assert lib.vqvae_vq_paths(2, 598, 30, 40, 0) == R.PATH_LDS1
    assert lib.vqvae_vq_paths(0, 64, 30, 40, 0) == -1          # no such problem


def test_rows_reach_every_path_and_every_absence():
    """The union over the rows as the GPU file runs them ('once' and gradient rows: the default matmul dtype 3; 'modes':
    dtypes 3, 2 and 0): every bit set somewhere; candidate pass, R = 8, tiled gather and sorted gradient each also absent
    from a mode-0 row; R = 2 and R = 8, tiled and plain gather each with a d that is no multiple of 4."""
    seen, absent = 0, 0
    for name, kind, B, T, d, k, variant in ALL:
        for dtype in ((3, 2, 0) if kind == 'modes' else (3,)):
            p = R.expected_paths(B, d, T, k, 0, dtype)
            assert p >= 0, name
            assert bin(p & R.SWEEPS).count('1') == 1, name
            if kind == 'grad':
                p &= R.PATH_SORT
                absent |= ~p & R.PATH_SORT
            else:
                absent |= ~p & (R.PATH_CAND | R.PATH_R8 | R.PATH_TILE | R.PATH_SORT)
                if d in (64, 128) and dtype >= 2:
                    assert (p & R.PATH_CAND != 0) == (k >= 1024 and B * T >= 1024), name
            seen |= p
    assert seen == sum(R.PATH_BITS.values()), hex(seen)
    assert absent == R.PATH_CAND | R.PATH_R8 | R.PATH_TILE | R.PATH_SORT, hex(absent)
    odd = {(bool(R.expected_paths(B, d, T, k, 0, 3) & R.PATH_R8), bool(R.expected_paths(B, d, T, k, 0, 3) & R.PATH_TILE))
           for name, kind, B, T, d, k, variant in ALL if kind == 'once' and d % 4}
    assert {(False, False), (True, False), (True, True)} <= odd
    # gradient rows: both forms with more than 256 channels, the scan form's P = 3, k beyond one scan block on the sort
    g = [(R.expected_paths(B, d, T, k, 1, 3) & R.PATH_SORT != 0, B * T, d, k) for name, kind, B, T, d, k, variant in ALL if kind == 'grad']
    assert any(s and d > 256 and d % 256 and k > 1024 for s, N, d, k in g) and any(not s and d > 256 and d % 256 for s, N, d, k in g)
    assert any(not s and 256 // d == 3 for s, N, d, k in g) and any(s and N <= 8192 for s, N, d, k in g)
    assert any(s and 16384 < N <= 32768 for s, N, d, k in g) and any(s and N == 16384 for s, N, d, k in g)
    assert any(kind == 'grad' and variant == 'code1' and B * T > 8 * 2048 and R.expected_paths(B, d, T, k, 1, 3) & R.PATH_SORT
               for name, kind, B, T, d, k, variant in ALL)          # every row on one code: more than 8 pieces of 2048 rows
    assert len({p.id for p in R.ROWS}) == len(R.ROWS)


@pytest.mark.parametrize('row', R.ROWS)
def test_reference_cost_of_a_row(row):
    name, kind, B, T, d, k, variant = row
    # seq_argmin costs N k d; a gradient-only row's reference is one float64 scatter-add of N d terms and never forms the
    # distances (grad_sort_d300_k1100's N k d is 2.8e9: its reference takes 20 ms)
    assert B * T * (d if kind == 'grad' else k * d) <= R.REF_COST_MAX
    if kind != 'grad':
        assert T >= 2                   # (oracle.vq_forward is the stated reference of seq_argmin: see the T = 1 note above)
