"""CPU tests of tests/call_accuracy_ref.py, the yardstick of tests/test_gpu_call_accuracy.py:

  the references     each float64 function reproduces the oracle's (conv1d_fwd / _bwd through crop, ReLU and the mask,
                     softmax_xent_*, upsample_bwd, the embed conv) to 1e-12 of scale; a swapped tap order or a transposed weight
                     is off by O(1).  (mol wraps the oracle's own functions: nothing to compare.)
  e32                NumPy's float32 evaluation of every quantity of every GPU row is not exact and stays inside its cap: 1e-6
                     for the contractions (as in the chain's host test), for the others the cap written beside them in CAPS;
  the dispatch       vqvae_conv1d_forms on the library loaded without a GPU equals expected_forms: every GPU row in every
                     mode, and a sweep across every predicate's edge; the rows reach the forms they are in the suite for;
  the emulation      on the contraction of each conv row (its first 64 output rows x 96 columns, K as in the row) faithful split
                     arithmetic passes the bar and one dropped product of float32x3 fails it;
  the scalars        the two-stage reduce in its stated order, run in NumPy float32 on the rows' inputs, passes the error model
                     the GPU test judges a device scalar against; the same with one workgroup's partial left out fails it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import call_accuracy_ref as R
import vqvae_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CONV = [r[0] for r in R.CONV_ROWS if r[0] != 'wide']            # `wide` (64 MB of output) is kept to the tests that need it


def _lib():
    from vqvae_amd import _lib
    return _lib


def _scaled(got, want):
    return R.metrics(got, want)[1]


# ---------------------------------------------------------------------------------------------------------------------------
# the references against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def _oracle_conv(inp, d, relu=False, x_relu=None):
    B, Cin, Tin, Cout, Tout, K, stride, pad, dil = d
    f = lambda a: a.astype(np.float64)
    x = f(inp['x'] if x_relu is None else x_relu)
    y = O.conv1d_fwd(x, f(inp['W']), f(inp['b']), stride, pad, dil)
    nat = y.shape[2]
    gfull = np.zeros((B, Cout, nat))
    gfull[:, :, :Tout] = inp['gy']
    gx, gW, gb = O.conv1d_bwd(x, f(inp['W']), gfull, stride, pad, dil)
    y = y[:, :, :Tout]
    return (np.maximum(y, 0) if relu else y), gx, gW, gb


@pytest.mark.parametrize('name', HOST_CONV)
def test_conv_references_reproduce_the_oracle(name):
    _, row, opt = R.CONV_BY_NAME[name]
    d = R.desc_of(row)
    inp = R.conv_inputs(name)
    r = R.conv_refs(name, inp, np.float64)
    y, gx, gW, gb = _oracle_conv(inp, d)
    worst = 0.0
    for q, want in (('y', y), ('gx', gx), ('gW', gW), ('gb', gb)):
        assert r[q].dtype == np.float64
        worst = max(worst, _scaled(r[q], want))
        assert _scaled(r[q], want) <= 1e-12, (name, q)
    if opt.get('relu'):
        assert _scaled(r['y_relu'], np.maximum(y, 0)) <= 1e-12
        xr = np.maximum(inp['x'], 0)
        assert _scaled(r['gx_relu'], _oracle_conv(inp, d, x_relu=xr)[1] * (xr > 0)) <= 1e-12
    if opt.get('acc'):
        for q, want, add in (('gx+', gx, inp['ax']), ('gW+', gW, inp['aW']), ('gb+', gb, inp['ab'])):
            assert _scaled(r[q], want + add) <= 1e-12, (name, q)
    print('CALL_SELF %s: worst %.3e of scale' % (name, worst))


def test_a_swapped_tap_order_or_a_transposed_weight_is_seen():
    name = 'two_tap'
    _, row, _ = R.CONV_BY_NAME[name]
    B, Cin, Tin, Cout, Tout, K, stride, pad, dil = R.desc_of(row)
    inp = R.conv_inputs(name)
    y, gx, gW, gb = _oracle_conv(inp, R.desc_of(row))
    assert _scaled(R.conv_fwd(inp['x'], inp['W'], inp['b'], stride, pad, dil, Tout), y) <= 1e-12
    assert _scaled(R.conv_fwd(inp['x'], inp['W'][:, :, ::-1], inp['b'], stride, pad, dil, Tout), y) > 1e-2
    assert Cin == Cout
    assert _scaled(R.conv_fwd(inp['x'], inp['W'].transpose(1, 0, 2), inp['b'], stride, pad, dil, Tout), y) > 1e-2
    assert _scaled(R.conv_bwd_data(inp['W'][:, :, ::-1], inp['gy'], stride, pad, dil, Tin), gx) > 1e-2
    assert _scaled(R.conv_bwd_weight(inp['x'], inp['gy'], K, stride, pad, dil)[0][:, :, ::-1], gW) > 1e-2


@pytest.mark.parametrize('row', R.STACK_ROWS, ids=str)
def test_stack_references_reproduce_the_oracle(row):
    """Layer by layer in float64 from the float64 output of the layer before: the oracle's chain of conv1d_fwd + relu, and its
    backward."""
    B, Cc, T, dils = row
    inp = R.stack_inputs(row)
    f = lambda a: a.astype(np.float64)
    hs, pre = [], []
    h = f(inp['x'])
    for W, b, dil in zip(inp['W'], inp['b'], dils):
        p = O.conv1d_fwd(h, f(W), f(b), 1, dil, dil)
        mine = R.convstack_layer(h, W, b, dil)
        assert _scaled(mine, np.maximum(p, 0)) <= 1e-12
        h = mine
        hs.append(h)
        pre.append(p)
    gx, gWs, gbs = R.convstack_bwd(inp['x'], inp['W'], hs, dils, inp['gy'])
    g = f(inp['gy'])
    for l in range(len(dils) - 1, -1, -1):
        g = g * (pre[l] > 0)
        g_in, gW, gb = O.conv1d_bwd(f(inp['x']) if l == 0 else hs[l - 1], f(inp['W'][l]), g, 1, dils[l], dils[l])
        assert _scaled(gWs[l], gW) <= 1e-12 and _scaled(gbs[l], gb) <= 1e-12, l
        g = g_in
    assert _scaled(gx, g) <= 1e-12


@pytest.mark.parametrize('row', R.S2_ROWS, ids=str)
def test_stage_backward_reference_reproduces_the_oracle(row):
    B, Tin, mask = row
    inp = R.s2_inputs(row)
    f = lambda a: a.astype(np.float64)
    nat = R.conv_out_len(Tin, 4, 2, 1, 1)
    assert nat == inp['Tout']
    gx, gW, gb = O.conv1d_bwd(f(inp['x']), f(inp['W']), f(inp['gy']), 2, 1, 1)
    mine = R.conv_s2_bwd(inp['x'], inp['W'], inp['gy'], mask)
    assert _scaled(mine[0], gx * (inp['x'] > 0) if mask else gx) <= 1e-12
    assert _scaled(mine[1], gW) <= 1e-12 and _scaled(mine[2], gb) <= 1e-12


@pytest.mark.parametrize('row', R.ONEHOT_ROWS, ids=str)
def test_embed_references_reproduce_the_oracle(row):
    B, Cout, q, K, T = row
    inp = R.onehot_inputs(row, 'dense')
    f = lambda a: a.astype(np.float64)
    want = O.conv1d_fwd(f(inp['x']), f(inp['W']), f(inp['b']), 1, K - 1, 1)[:, :, :T]
    assert _scaled(R.embed_fwd(inp['x'], inp['W'], inp['b']), want) <= 1e-12
    gfull = np.zeros((B, Cout, T + K - 1))
    gfull[:, :, :T] = inp['gy']
    _, gW, gb = O.conv1d_bwd(f(inp['x']), f(inp['W']), gfull, 1, K - 1, 1)
    mine = R.embed_wgrad(inp['x'], inp['gy'], K)
    assert _scaled(mine[0], gW) <= 1e-12 and _scaled(mine[1], gb) <= 1e-12


@pytest.mark.parametrize('row', R.XENT_ROWS[:4], ids=str)
def test_xent_reference_reproduces_the_oracle(row):
    inp = R.xent_inputs(row)
    y = inp['y'].astype(np.float64)
    loss, logp = O.softmax_xent_fwd(y, inp['t'])
    r = R.xent(inp['y'], inp['t'], R.XENT_GLOSS)
    assert abs(r['loss'] - loss) <= 1e-12 * abs(loss)
    assert _scaled(r['lse'], (y - logp)[:, 0, :]) <= 1e-12
    assert _scaled(r['gy'], O.softmax_xent_bwd(logp, inp['t'], R.XENT_GLOSS)) <= 1e-12


@pytest.mark.parametrize('Tin,Tout', [(3, 24), (15, 961), (64, 256), (1, 64)])
def test_upsample_adjoint_reproduces_the_oracle(Tin, Tout):
    rs = np.random.RandomState(Tin + Tout)
    gy = rs.standard_normal((2, 3, Tout))
    v0, v1, w0, w1 = O.resize_tables(Tin, Tout, np.float64)
    assert _scaled(R.upsample_bwd(gy, dict(v0=v0, v1=v1, w0=w0, w1=w1), Tin), O.upsample_bwd(gy, Tin)) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------------
# e32 of every row of the GPU test
# ---------------------------------------------------------------------------------------------------------------------------
CONTRACTION_CAP = 1e-6
# quantity -> (cap l2, cap max) where a row's own e32 is above 1e-6: twice the largest e32 measured here (NumPy float32 on
# this module's inputs), the measured figure in the comment
CAPS = {
    # the fp32 conditioning of cdf_plus - cdf_min; the max metric is set by one element and is not asserted (nor on the device)
    'mol gy logits': (3.94e-6, None),       # l2 1.968e-06 at (2, 1, 300000); 1.05e-6 .. 1.13e-6 at the other rows
    'mol gy means': (2.24e-6, None),        # l2 1.116e-06 at (10, 3, 63)
    'mol gy log-scales': (3.86e-6, None),   # l2 1.928e-06 at (2, 1, 300000)
}


def _inside(what, key, e32, cap=(CONTRACTION_CAP, CONTRACTION_CAP)):
    cap = CAPS.get(key, cap)
    print('CALL_REF %s %s: e32 l2 %.3e max %.3e' % (what, key, e32[0], e32[1]))
    assert e32[0] > 0 and e32[1] > 0, (what, key)
    assert e32[0] <= cap[0], (what, key, e32)
    assert cap[1] is None or e32[1] <= cap[1], (what, key, e32)


@pytest.mark.parametrize('name', [r[0] for r in R.CONV_ROWS])
def test_float32_error_of_the_conv_rows(name):
    inp = R.conv_inputs(name)
    r64, r32 = R.conv_refs(name, inp, np.float64), R.conv_refs(name, inp, np.float32)
    assert sorted(r64) == sorted(r32)
    for q in sorted(r64):
        assert r32[q].dtype == np.float32 and r64[q].dtype == np.float64
        _inside(name, q, R.metrics(r32[q], r64[q]))


def test_float32_error_of_the_latent_and_embed_rows():
    for row in R.STACK_ROWS:
        inp = R.stack_inputs(row)
        hs, h = [], inp['x']
        for W, b, dil in zip(inp['W'], inp['b'], row[3]):
            h = R.convstack_layer(h, W, b, dil, np.float32)       # what a faultless device would hand on
            hs.append(h)
        for l, dil in enumerate(row[3]):
            prev = inp['x'] if l == 0 else hs[l - 1]
            _inside(row, 'h[%d]' % l, R.metrics(R.convstack_layer(prev, inp['W'][l], inp['b'][l], dil, np.float32),
                                                 R.convstack_layer(prev, inp['W'][l], inp['b'][l], dil)))
        b64, b32 = (R.convstack_bwd(inp['x'], inp['W'], hs, row[3], inp['gy'], dt) for dt in (np.float64, np.float32))
        _inside(row, 'gx', R.metrics(b32[0], b64[0]))
        for l in range(len(row[3])):
            _inside(row, 'gW[%d]' % l, R.metrics(b32[1][l], b64[1][l]))
            _inside(row, 'gb[%d]' % l, R.metrics(b32[2][l], b64[2][l]))
    for row in R.S2_ROWS:
        inp = R.s2_inputs(row)
        b64, b32 = (R.conv_s2_bwd(inp['x'], inp['W'], inp['gy'], row[2], dt) for dt in (np.float64, np.float32))
        for q, a, b in zip(('gx', 'gW', 'gb'), b32, b64):
            if not (row == (1, 2, 0) and q == 'gb'):               # one term per channel: float32 is exact there
                _inside(row, q, R.metrics(a, b))
    for row in R.ONEHOT_ROWS:
        for kind in ('dense',):                                     # a one-hot input selects weights: float32 sums of K terms
            inp = R.onehot_inputs(row, kind)
            _inside(row, 'y', R.metrics(R.embed_fwd(inp['x'], inp['W'], inp['b'], np.float32), R.embed_fwd(inp['x'], inp['W'], inp['b'])))
            g64, g32 = (R.embed_wgrad(inp['x'], inp['gy'], row[3], dt) for dt in (np.float64, np.float32))
            _inside(row, 'gW', R.metrics(g32[0], g64[0]))
            _inside(row, 'gb', R.metrics(g32[1], g64[1]))


def test_float32_error_of_the_loss_rows():
    for row in R.XENT_ROWS:
        inp = R.xent_inputs(row)
        r64 = R.xent(inp['y'], inp['t'], R.XENT_GLOSS)
        r32 = R.xent(inp['y'], inp['t'], R.XENT_GLOSS, dtype=np.float32)
        _inside(row, 'xent lse', R.metrics(r32['lse'], r64['lse']))
        _inside(row, 'xent gy', R.metrics(r32['gy'], r64['gy']))
    for row in R.MOL_ROWS:
        nm = row[0]
        inp = R.mol_inputs(row)
        g64, g32 = R.mol(inp['y'], inp['t'])['gy'], R.mol(inp['y'], inp['t'], dtype=np.float32)['gy']
        for i, part in enumerate(('logits', 'means', 'log-scales')):
            _inside(row, 'mol gy ' + part, R.metrics(g32[:, i * nm:(i + 1) * nm], g64[:, i * nm:(i + 1) * nm]))


# ---------------------------------------------------------------------------------------------------------------------------
# the dispatch query
# ---------------------------------------------------------------------------------------------------------------------------
def test_header_bits_are_the_modules():
    text = open(os.path.join(ROOT, 'include', 'vqvae_hip.h')).read()
    bits = {m.group(1): int(m.group(2), 0) for m in re.finditer(r'#define VQVAE_CONV_FORM_(\w+) (0x[0-9a-fA-F]+|\d+)', text)}
    assert bits == R.FORM_BITS
    fam = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define VQVAE_CONV_(GEMM_\w+|WGRAD_\w+) (\d+)', text)}
    assert fam == dict(GEMM_LIN128=R.GEMM_LIN128, GEMM_TILED=R.GEMM_TILED, GEMM_FP32=R.GEMM_FP32, WGRAD_W3=R.WGRAD_W3,
                       WGRAD_W2=R.WGRAD_W2, WGRAD_GENERIC=R.WGRAD_GENERIC)
    L = _lib()
    assert all(getattr(L, 'CONV_FORM_' + k) == v for k, v in R.FORM_BITS.items())


def _forms(lib, d, which, relu=0):
    return lib.vqvae_conv1d_forms(C.byref(_lib().Conv1dDesc(*(tuple(d) + (relu,)))), which)


def _sweep():
    """Shapes on both sides of every predicate: M = 255 / 256 / 257 (256-row tiles), cin = 63 / 64 / 96 / 128 (the halved 1x1 and
    lin128's K), T % 64 and T % 4 (lin128, the vector loads, the fast weight gradient, the phase split), nblk2 = 255 / 256
    (256-column tiles), the split-K plan's edges (tiles = 128 / 129, nk = 31 / 32, 8 steps per split), K = 1 .. 4 and a K the
    entry points refuse, strides 1 .. 3, an oversize crop."""
    out = []
    for M in (255, 256, 257, 512):
        for cin in (63, 64, 96, 128, 130):
            for T in (62, 63, 64, 128, 200):
                out.append((2, cin, T, M, T, 1, 1, 0, 1))
                out.append((2, M, T, cin, T, 1, 1, 0, 1))
    for K in (1, 2, 3, 4, 5):
        for stride in (1, 2, 3):
            for Tin in (7, 8, 64, 255, 256):
                for dil in (1, 2):
                    pad = dil * (K - 1) // 2
                    Tout = R.conv_out_len(Tin, K, stride, pad, dil)
                    for cin, M in ((64, 64), (256, 256), (48, 256), (1, 64)):
                        if Tout > 0:
                            out.append((2, cin, Tin, M, Tout, K, stride, pad, dil))
    for B, T in ((255, 256), (256, 256), (1, 255 * 256), (1, 256 * 256), (128, 257), (4, 16384)):     # nblk2 around 256
        out.append((B, 32, T, 256, T, 1, 1, 0, 1))
        out.append((B, 32, T, 256, T, 2, 1, 1, 1))
        out.append((B, 256, T, 32, T, 1, 1, 0, 1))            # ... of the backward-data GEMM
    for B, T, cin in ((128, 128, 512), (129, 128, 512), (2, 120, 496), (2, 120, 512), (2, 120, 1280), (1, 100, 4096),
                      (64, 128, 256), (65, 128, 256), (16, 128, 8192)):                                # the split-K plan
        out.append((B, cin, T, 192, T, 1, 1, 0, 1))
        out.append((B, 192, T, cin, T, 1, 1, 0, 1))
    out.append((2, 64, 64, 64, 65, 1, 1, 0, 1))              # Tout above the natural length: refused
    out.append((0, 64, 64, 64, 64, 1, 1, 0, 1))
    return out


@pytest.mark.parametrize('mode', R.ACC_MODES + ('bfloat16',))
def test_forms_query_equals_the_restated_predicates(mode):
    lib = _lib().load()
    before = lib.vqvae_get_matmul_dtype()
    assert lib.vqvae_set_matmul_dtype(R.MODES[mode]) == 0
    try:
        for gflop in (0.0, 8.0):
            assert lib.vqvae_set_f32x2_min_gflop(gflop) == 0
            cases = [(R.desc_of(row), opt.get('relu', False)) for _, row, opt in R.CONV_ROWS] + [(d, False) for d in _sweep()]
            for d, relu in cases:
                for which in (0, 1, 2, 3):
                    for r in ((0, 1) if relu else (0,)):
                        got, want = _forms(lib, d, which, r), R.expected_forms(d, which, mode, gflop, r)
                        assert got == want, '%r which %d relu %d %s gflop %g: the library says %s, the predicates %s' % (
                            d, which, r, mode, gflop, R.describe(got), R.describe(want))
    finally:
        lib.vqvae_set_f32x2_min_gflop(8.0)
        lib.vqvae_set_matmul_dtype(before)
    assert lib.vqvae_conv1d_forms(None, 0) == -1


def test_sweep_crosses_every_predicate():
    """No edge of the sweep is vacuous: over it (float32x3 and float32x2) every bit is set somewhere and absent somewhere, in
    each direction it can occur in; refusals occur."""
    seen, absent, refused = [0, 0, 0], [0, 0, 0], 0
    fam = [set(), set(), set()]
    for mode in ('float32x3', 'float32x2', 'float32'):
        for d in _sweep():
            for which in (0, 1, 2):
                w = R.expected_forms(d, which, mode)
                if w < 0:
                    refused += 1
                    continue
                seen[which] |= w
                absent[which] |= ~w
                fam[which].add(w & R.FAMILY)
    gemm = R.ROWS256 | R.WIDE | R.TAP2 | R.LEAN | R.HALVED | R.SPLIT | R.STRIDED
    wg = R.ROWS256 | R.PHASES | R.SPLIT | R.STRIDED
    for which, bits in ((0, gemm), (1, gemm), (2, wg)):
        assert seen[which] & bits == bits and absent[which] & bits == bits, (which, hex(seen[which]), hex(absent[which]))
    assert fam[0] == fam[1] == {R.GEMM_LIN128, R.GEMM_TILED, R.GEMM_FP32} and fam[2] == {R.WGRAD_W3, R.WGRAD_W2, R.WGRAD_GENERIC}
    assert refused


@pytest.mark.parametrize('name', [r[0] for r in R.CONV_ROWS])
def test_rows_reach_the_forms_they_are_here_for(name):
    assert set(R.ROW_FORMS) == set(R.CONV_BY_NAME)
    d = R.desc_of(R.CONV_BY_NAME[name][1])
    for mode in R.ACC_MODES:
        R.check_row_forms(name, mode, lambda which: R.expected_forms(d, which, mode))
    # the weight-gradient kernels between them: wgrad3_kernel<2, 1, 3> / <2, 1, 2> (128-row tiles), wgrad2_kernel, wgrad_kernel<false>
    w = {(n, m): R.expected_forms(R.desc_of(R.CONV_BY_NAME[n][1]), 2, m) for n in R.CONV_BY_NAME for m in R.ACC_MODES}
    np_of = lambda v: (v & R.NP_MASK) >> R.NP_SHIFT
    for np_, m in ((3, 'float32x3'), (2, 'float32x2')):
        assert any(v & R.FAMILY == R.WGRAD_W3 and not v & R.ROWS256 and np_of(v) == np_ for (n, mm), v in w.items() if mm == m)
        assert any(v & R.FAMILY == R.WGRAD_W3 and v & R.ROWS256 and np_of(v) == np_ for (n, mm), v in w.items() if mm == m)
    assert any(v & R.FAMILY == R.WGRAD_W2 for v in w.values()) and any(v & R.FAMILY == R.WGRAD_GENERIC for v in w.values())


# ---------------------------------------------------------------------------------------------------------------------------
# the emulation on the rows' own contractions
# ---------------------------------------------------------------------------------------------------------------------------
def _contraction(name, M=64, N=96):
    """A (M, Kp) = the first M output channels' weights, taps side by side; Bm (Kp, N) = the matching input windows of batch
    item 0 at outputs t = 8 .. 8 + N (inside every row's Tout); K = K Cin as in the row, zero-padded to whole 16-deep steps."""
    _, row, _ = R.CONV_BY_NAME[name]
    B, Cin, Tin, Cout, Tout, K, stride, pad, dil = R.desc_of(row)
    inp = R.conv_inputs(name)
    M, N = min(M, Cout), min(N, Tout - 8)
    xp = np.pad(inp['x'][0], ((0, 0), (pad, pad + stride * Tout + dil * K)))
    A = np.concatenate([inp['W'][:M, :, j] for j in range(K)], 1)
    Bm = np.concatenate([xp[:, j * dil + 8 * stride: j * dil + (8 + N) * stride: stride] for j in range(K)], 0)
    want_y = R.conv_fwd(inp['x'][:1], inp['W'][:M], None, stride, pad, dil, Tout)[0, :, 8:8 + N]
    assert np.abs(np.matmul(A.astype(np.float64), Bm.astype(np.float64)) - want_y).max() <= 1e-12 * np.abs(want_y).max()
    Kp = -(-A.shape[1] // 16) * 16
    return (np.ascontiguousarray(np.pad(A, ((0, 0), (0, Kp - A.shape[1])))),
            np.ascontiguousarray(np.pad(Bm, ((0, Kp - Bm.shape[0]), (0, 0)))), K * Cin)


@pytest.mark.parametrize('name', HOST_CONV + ['wide'])
def test_emulated_split_products_pass_the_bar_and_emulated_defects_fail_it(name):
    A, Bm, Ktot = _contraction(name)
    want = np.matmul(A.astype(np.float64), Bm.astype(np.float64))
    e32 = R.metrics(np.matmul(A, Bm), want)
    if Ktot > 1:
        assert all(e > 0 for e in e32)
    forms = dict(x3=R.emulate_x3(A, Bm), x2=R.emulate_x2(A, Bm), x3_no_lh=R.emulate_x3(A, Bm, 'lh'), x3_no_mm=R.emulate_x3(A, Bm, 'mm'))
    for form, got in sorted(forms.items()):
        err = R.metrics(got, want)
        print('CALL_EMU %s K %d %s: l2 %.3e (e32 %.3e) max %.3e (e32 %.3e)' % (name, Ktot, form, err[0], e32[0], err[1], e32[1]))
        ok = [e <= R.bar(r) for e, r in zip(err, e32)]
        if form.startswith('x3_no'):
            assert not any(ok), '%s: the defect passes the bar: %r against e32 %r' % (form, err, e32)
        else:
            assert all(ok), '%s: faithful arithmetic misses the bar: %r against e32 %r' % (form, err, e32)


# ---------------------------------------------------------------------------------------------------------------------------
# the scalars
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', R.SCALAR_N)
def test_two_stage_sum_passes_its_model_and_a_lost_partial_fails_it(n):
    inp = R.scalar_inputs(n)
    d = (inp['a'] - inp['b']).astype(np.float32)
    for what, terms, scale in (('sum', inp['x'], 0.5), ('sqdiff', (d * d).astype(np.float32), 1.0 / n)):
        t64 = terms.astype(np.float64)
        want, mass = t64.sum() * scale, np.abs(t64).sum() * abs(scale)
        allow = R.scalar_model(n) * mass
        got = float(R.two_stage_sum(terms, np.float32(scale)))
        print('CALL_SCALAR %s n %d: err %.3e allowed %.3e' % (what, n, abs(got - want), allow))
        assert abs(got - want) <= allow, (what, n)
        nwg = R.grid_for(n)
        lost = float(R.two_stage_sum(terms, np.float32(scale), leave_out=nwg // 2))
        assert abs(lost - want) > allow, (what, n, 'a lost partial passes the model')
