"""Every call of a training step OUTSIDE the decoder chain and the vector quantiser held to fp32 accuracy on its own arithmetic.

The neighbouring tests of these entry points (test_conv1d_fwd_bwd, test_conv1d_random_shapes_vs_oracle, test_conv1d_contract,
test_conv_stack_fused_vs_oracle, test_encoder_stage_backward_fused_vs_oracle, test_latent_fusions_contract, test_softmax_xent*,
test_mol_nll*) assert 1e-4 or 1e-5 against the oracle: a lost product of 'float32x3' (2.4e-6 .. 2.8e-6 relative L2) passes them
forty times over.  Here every call is compared with tests/call_accuracy_ref.py's float64 evaluation of THAT call's function
over the values the call was handed, two metrics per quantity (relative L2 error, max error over the tensor's scale), each for
the device (`err`) and for NumPy's float32 evaluation of the same function over the same values (`e32`):

    err <= 3 e32 + 1e-7          chain_accuracy_ref.bar, the decoder chain's bar

Conv rows run in the three modes of the matmul_mode fixture, and each first asserts, through vqvae_conv1d_forms, the kernel
forms it is in the suite for (call_accuracy_ref.ROW_FORMS) and that the query equals the restated predicates.  The fused latent
kernels use fp32 MFMA in every mode and run once.  The mixture-of-logistics gradient is asserted in the L2 metric only, per
third of the channels (cdf_plus - cdf_min cancels in fp32: the max metric's e32 is set by one element; it is printed).  A
scalar (the two losses, vqvae_sum, vqvae_sqdiff_mean) is not judged against e32 -- one float32 evaluation can land on the
float64 value by luck -- but against call_accuracy_ref.scalar_model, the error model of the kernel's stated summation order,
which tests/test_host_call_accuracy.py shows a NumPy run of that order to pass and a lost partial to fail.

One line per call and quantity (pytest -s):  CALL_ACC <row> <mode> <entry point> <quantity> l2 err e32 ratio max err e32 ratio

MARGINS.  The L2 bar is the plain one for every quantity in every mode.  One group of quantities carries an addition to its MAX
bar, derived where it is passed from chain_accuracy_ref.seq_error over the K the kernel keeps in one accumulator: h_l and gx of
the conv stack (STACK MARGIN in test_convstack_call_accuracy); it was not taken from a device figure.  The generic conv carries
none: the split-K rows and the 65536-position weight gradient of `wide`, where one was expected, sit under e32 in every mode
(splitk / splitk_t 0.40 .. 1.00, gW of wide 0.55 .. 0.88).

MEASURED, one run on an MI355X (bit-reproducible: a second run printed the same 389 lines): the worst err / e32 per quantity
and mode over all rows, relative L2 then max-over-scale (one column where the call does not depend on the matmul mode):

    quantity                                     float32x2    float32x3    float32
    conv1d_fwd y                                 1.67  1.91   1.52  2.28   1.86  2.50
    conv1d_fwd y (ReLU, head)                    0.67  0.72   0.82  0.75   1.00  1.00
    conv1d_bwd_data gx                           1.75  2.04   2.04  2.45   2.61  3.60
    conv1d_bwd_data gx + addend                  1.07  1.26   1.17  2.02   1.40  1.86
    conv1d_bwd_data_relu gx (head)               0.66  0.48   0.82  0.87   1.00  1.00
    conv1d_bwd_weight gW                         1.50  1.58   1.50  1.58   1.67  1.54
    conv1d_bwd_weight gb                         1.04  1.07   1.04  1.07   1.04  1.07
    conv1d_bwd_weight gW + addend                1.42  1.54   1.42  1.54   1.42  1.54
    conv1d_bwd_weight gb + addend                0.93  0.96   0.93  0.96   0.93  0.96
    convstack_fwd h                              3.44  5.43 *
    convstack_bwd gx                             1.91  2.67
    convstack_bwd gW                             2.08  2.14
    convstack_bwd gb                             2.35  3.35
    conv_s2_bwd gx                               2.25  2.07
    conv_s2_bwd gW                               1.00  1.00
    conv_s2_bwd gb                               2.05  3.22
    embed_onehot_fwd y, one-hot / one class      1.00  1.00   1.00  1.00   1.00  1.00
    embed_onehot_wgrad gW, one-hot / one class   1.00  1.00   1.00  1.00   1.00  1.00
    embed_onehot_wgrad gb, one-hot / one class   1.30  1.26   1.30  1.26   1.30  1.26
    embed_onehot_fwd y, dense                    1.16  1.34   1.16  1.34   1.32  1.60
    embed_onehot_wgrad gW, dense                 1.78  2.00   1.78  2.00   1.78  2.00
    embed_onehot_wgrad gb, dense                 1.24  1.21   1.24  1.21   1.24  1.21
    softmax_xent_fwd lse                         1.00  1.01
    softmax_xent_bwd gy                          0.96  1.00
    mol_nll_bwd gy logits                        0.96  1.11
    mol_nll_bwd gy means                         1.03  1.17
    mol_nll_bwd gy log-scales                    0.98  2.06
    upsample_linear_bwd gx                       0.82  0.89
    embed_broadcast_bwd gE                       1.47  1.28
    embed_broadcast_bwd gE + addend              1.62  1.34
    scalars, err / allowed:  xent loss 0.010, mol loss 0.020, vqvae_sum 0.000, vqvae_sqdiff_mean 0.030

(a ratio above 3 passes where 1e-7 carries it: gx of enc1 in 'float32', 4.17e-7 against 3 x 1.16e-7 + 1e-7, and the bias sums of the
fused latent kernels.)  * = outside the plain bar, max metric only: h[0] of the (1, 64, 5) conv stack, 4.73e-7 against
3 x 8.7e-8 + 1e-7 (STACK MARGIN: 192 terms in one fp32 accumulator, seq_error 3.4e-7, against a NumPy matmul of a 64 x 64 by
64 x 5 block).  It is no defect of the kernel -- no product is left out, no operand rounded early -- and no kernel was changed.
The scalar models are far from tight (they bound every tree level by sum |term|); tests/test_host_call_accuracy.py shows they
still fail a lost workgroup partial.

SHOWN ABLE TO FAIL where the 1e-4 / 1e-5 bars could not.  Five value-only mutations (a product or a rounding; no address, bound,
barrier or launch geometry) in disjoint kernels of a scratch copy of csrc/, built into ONE scratch library (their quantities do
not overlap) and run once against this file and once against the old tests of the same calls (test_conv1d_fwd_bwd,
test_conv1d_random_shapes_vs_oracle, test_conv1d_contract, test_float32x3_is_as_accurate_as_fp32_mfma,
test_conv_stack_fused_vs_oracle, test_encoder_stage_backward_fused_vs_oracle, test_latent_fusions_contract,
test_conv_s2_bwd_contract, test_softmax_xent*); never committed.  This file: 27 of 104 fail.
  float32x3 K loop, 128-row tiles:  a_l * b_h dropped from the product chain of the plain (non-TAP2) loop of
      conv_gemm_x3_kernel<.., WM = 2, .., NP = 3>.  test_conv_call_accuracy[float32x3] fails at every row that runs that form --
      enc1, enc_odd, ragged, splitk (y), splitk_t, cond_proj, lin128, lin128_T200, three_tap (their gx on 128-row tiles) -- with y
      at 6.7 .. 40 e32 (relative L2 1.6e-6 .. 1.7e-6) and gx at 6.6 .. 30 e32 (2.4e-6 .. 2.5e-6); head, two_tap and wide (256-row
      tiles) pass.  The dense road of test_embed_onehot_call_accuracy fails in 'float32x3' and 'float32x2' (its conv runs under a
      skip flag, hence six products in both): y at 9 .. 32 e32.  Old tests in 'float32x3': test_conv1d_fwd_bwd,
      test_conv1d_random_shapes_vs_oracle and test_conv1d_contract pass; test_float32x3_is_as_accurate_as_fp32_mfma, the one fp32-class
      check there was, fails at 5 of its 8 shapes.
  wgrad3_kernel<2, 1, 3>:  a_l * b_h dropped from its plain product chain.  gW of enc1 (every mode whose weight gradient takes the
      phase split on six products: 'float32x3' and 'float32x2') at 23 e32 (2.9e-6), gW of splitk in 'float32x3' at 12 e32 (2.4e-6), gW
      of the dense one-hot rows at 17 e32; the bias sums, which take no product, pass.  Old tests in 'float32x3': all pass.
  wgrad3_kernel<2, 1, 2>:  a_lo * b_hi dropped.  gW of splitk in 'float32x2' at 1043 e32 (relative L2 2.1e-4).  Half of the low
      pieces is no subtle loss: the old bars see it too -- test_conv1d_fwd_bwd[float32x2] (16 cases),
      test_conv1d_random_shapes_vs_oracle[float32x2] (13) and test_conv1d_contract[float32x2] (2) fail.
  cstack_bwd_kernel:  the h_{l-1} operand of the weight-gradient MFMA truncated to bf16.  Every gW[l] of all five
      test_convstack_call_accuracy rows at 9 000 .. 76 000 e32 (relative L2 3.1e-3 .. 3.5e-3); h, gx and gb pass.  Not subtle
      either: test_conv_stack_fused_vs_oracle (12 cases) and test_latent_fusions_contract (4) fail as well.
  xent_fwd_kernel:  the second class group's sum-exp truncated to bf16 before the four are combined.  lse of all five
      test_softmax_xent_call_accuracy rows at 2 800 .. 9 900 e32 (relative L2 1.1e-5 .. 2.4e-4), and the loss scalar at 2.5 .. 24
      times its model.  test_softmax_xent_contract fails at 7 of its 9 shapes and test_softmax_xent at 1: its 1e-5 bar sees most of it.
Nothing among the five escaped this file.  What it cannot see by construction: an error that the float32 reference shares (the
ill-conditioned mixture terms, hence the L2-only assertion there), and a scalar off by less than its loose model.
"""
import ctypes as C

import numpy as np
import pytest

import call_accuracy_ref as R
from test_gpu_abi_contract import UPS_BWD_CASES, _tables

pytestmark = pytest.mark.gpu


def _L():
    from vqvae_amd import _lib
    return _lib


class Judge(object):
    """Collects the lines of one test and asserts the bar once, with every miss in the message."""

    def __init__(self, row, mode):
        self.row, self.mode, self.lines, self.misses = row, mode, 0, []

    def __call__(self, entry, quantity, got, want64, want32, margin=(0.0, 0.0), l2_only=False):
        """margin: this quantity's own addition to the bar (l2, max), from an error model written where it is passed."""
        assert np.isfinite(np.asarray(got)).all(), '%s %s %s: non-finite' % (self.row, entry, quantity)
        err, e32 = R.metrics(got, want64), R.metrics(want32, want64)
        ratio = [e / max(r, 1e-30) for e, r in zip(err, e32)]
        line = 'CALL_ACC %s %s %s %s l2 %.3e %.3e %.2f max %.3e %.3e %.2f' % (
            self.row, self.mode, entry, quantity, err[0], e32[0], ratio[0], err[1], e32[1], ratio[1])
        print(line)
        self.lines += 1
        ok = [e <= R.bar(r) + m for e, r, m in zip(err, e32, margin)]
        if not (ok[0] if l2_only else all(ok)):
            self.misses.append(line + ('' if not any(margin) else ' (margin %.3e %.3e)' % tuple(margin)))

    def scalar(self, entry, quantity, got, want64, allowed):
        err = abs(float(got) - float(want64))
        line = 'CALL_ACC %s %s %s %s scalar err %.3e allowed %.3e ratio %.2f' % (self.row, self.mode, entry, quantity, err, allowed,
                                                                                err / max(allowed, 1e-300))
        print(line)
        self.lines += 1
        if not (np.isfinite(float(got)) and err <= allowed):
            self.misses.append(line)

    def finish(self):
        assert not self.misses, '%d of %d quantities miss their bar (err <= 3 e32 + 1e-7; scalars: their model):\n%s' % (
            len(self.misses), self.lines, '\n'.join(self.misses))


class Dev(object):
    """The few lines of plumbing every test here needs: uploads, NaN-filled outputs, exactly sized workspaces, calls."""

    def __init__(self, gpu):
        self.gpu, self.L = gpu, _L()
        self.lib = self.L.load()

    def up(self, a):
        return self.gpu.to_device(np.ascontiguousarray(a))

    def out(self, shape, dtype=np.float32):
        return self.gpu.to_device(np.full(shape, np.nan, dtype) if dtype == np.float32 else np.full(shape, -1, dtype))

    def ws(self, nbytes):
        return self.gpu.to_device(np.full((nbytes // 4 + 1,), np.nan, np.float32))

    def call(self, name, *args):
        self.L.call(name, *(args + (self.gpu.stream(),)))

    def ptrs(self, arrays):
        return (C.c_void_p * len(arrays))(*[a.ptr for a in arrays])


# ---------------------------------------------------------------------------------------------------------------------------
# the generic conv
# ---------------------------------------------------------------------------------------------------------------------------
_REFS = {}


def _conv_refs(name):
    """The inputs and both references of a row, computed once and shared by the three modes (never written to)."""
    if name not in _REFS:
        inp = R.conv_inputs(name)
        _REFS[name] = (inp, R.conv_refs(name, inp, np.float64), R.conv_refs(name, inp, np.float32))
    return _REFS[name]


@pytest.mark.parametrize('name', [r[0] for r in R.CONV_ROWS])
def test_conv_call_accuracy(gpu, matmul_mode, name):
    D = Dev(gpu)
    _, row, opt = R.CONV_BY_NAME[name]
    d = R.desc_of(row)
    B, Cin, Tin, Cout, Tout, K, stride, pad, dil = d
    desc = lambda relu: D.L.Conv1dDesc(B, Cin, Tin, Cout, Tout, K, stride, pad, dil, relu)
    forms = {w: D.lib.vqvae_conv1d_forms(C.byref(desc(0)), w) for w in (0, 1, 2)}
    for w in (0, 1, 2):
        assert forms[w] == R.expected_forms(d, w, matmul_mode), '%s %s which %d: the library runs "%s", the predicates say "%s"' % (
            name, matmul_mode, w, R.describe(forms[w]), R.describe(R.expected_forms(d, w, matmul_mode)))
    R.check_row_forms(name, matmul_mode, lambda w: forms[w])
    inp, r64, r32 = _conv_refs(name)
    only = opt.get('only', (0, 1, 2))
    judge = Judge(name, matmul_mode)
    ws_bytes = D.lib.vqvae_conv1d_workspace_bytes(C.byref(desc(0)))
    ws = D.ws(ws_bytes)
    x, W, b, gy = D.up(inp['x']), D.up(inp['W']), D.up(inp['b']), D.up(inp['gy'])
    if 0 in only:
        y = D.out((B, Cout, Tout))
        D.call('vqvae_conv1d_fwd', C.byref(desc(0)), x.ptr, W.ptr, b.ptr, y.ptr, ws.ptr, ws_bytes)
        judge('vqvae_conv1d_fwd', 'y', y.get(), r64['y'], r32['y'])
        if opt.get('relu'):
            assert D.lib.vqvae_conv1d_forms(C.byref(desc(1)), 0) == R.expected_forms(d, 0, matmul_mode, relu=1)
            y = D.out((B, Cout, Tout))
            D.call('vqvae_conv1d_fwd', C.byref(desc(1)), x.ptr, W.ptr, b.ptr, y.ptr, ws.ptr, ws_bytes)
            judge('vqvae_conv1d_fwd', 'y_relu', y.get(), r64['y_relu'], r32['y_relu'])
    if 1 in only:
        gx = D.out((B, Cin, Tin))
        D.call('vqvae_conv1d_bwd_data', C.byref(desc(0)), W.ptr, gy.ptr, gx.ptr, 0, ws.ptr, ws_bytes)
        judge('vqvae_conv1d_bwd_data', 'gx', gx.get(), r64['gx'], r32['gx'])
        if opt.get('acc'):
            gx = D.up(inp['ax'])
            D.call('vqvae_conv1d_bwd_data', C.byref(desc(0)), W.ptr, gy.ptr, gx.ptr, 1, ws.ptr, ws_bytes)
            assert r32['gx+'].dtype == np.float32
            judge('vqvae_conv1d_bwd_data', 'gx+addend', gx.get(), r64['gx+'], r32['gx+'])
        if opt.get('relu'):
            gx, xr = D.out((B, Cin, Tin)), D.up(np.maximum(inp['x'], 0))
            D.call('vqvae_conv1d_bwd_data_relu', C.byref(desc(0)), W.ptr, gy.ptr, xr.ptr, gx.ptr, ws.ptr, ws_bytes, None)
            judge('vqvae_conv1d_bwd_data_relu', 'gx_relu', gx.get(), r64['gx_relu'], r32['gx_relu'])
    if 2 in only:
        gW, gb = D.out((Cout, Cin, K)), D.out((Cout,))
        D.call('vqvae_conv1d_bwd_weight', C.byref(desc(0)), x.ptr, gy.ptr, gW.ptr, gb.ptr, 0, ws.ptr, ws_bytes)
        judge('vqvae_conv1d_bwd_weight', 'gW', gW.get(), r64['gW'], r32['gW'])
        judge('vqvae_conv1d_bwd_weight', 'gb', gb.get(), r64['gb'], r32['gb'])
        if opt.get('acc'):
            gW, gb = D.up(inp['aW']), D.up(inp['ab'])
            D.call('vqvae_conv1d_bwd_weight', C.byref(desc(0)), x.ptr, gy.ptr, gW.ptr, gb.ptr, 1, ws.ptr, ws_bytes)
            judge('vqvae_conv1d_bwd_weight', 'gW+addend', gW.get(), r64['gW+'], r32['gW+'])
            judge('vqvae_conv1d_bwd_weight', 'gb+addend', gb.get(), r64['gb+'], r32['gb+'])
    judge.finish()


# ---------------------------------------------------------------------------------------------------------------------------
# the fused latent kernels (fp32 MFMA in every matmul mode: run once)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', R.STACK_ROWS, ids=lambda r: 'B%d_C%d_T%d_L%d' % (r[0], r[1], r[2], len(r[3])))
def test_convstack_call_accuracy(gpu, row):
    D = Dev(gpu)
    B, Cc, T, dils = row
    nl = len(dils)
    cd = (C.c_int * nl)(*dils)
    assert D.lib.vqvae_convstack_supported(nl, Cc, T, cd) == 1
    inp = R.stack_inputs(row)
    judge = Judge('stack_B%d_C%d_T%d_L%d' % (B, Cc, T, nl), '-')
    x, gy = D.up(inp['x']), D.up(inp['gy'])
    Ws, bs, hs = [D.up(a) for a in inp['W']], [D.up(a) for a in inp['b']], [D.out((B, Cc, T)) for _ in dils]
    D.call('vqvae_convstack_fwd', nl, B, Cc, T, cd, x.ptr, D.ptrs(Ws), D.ptrs(bs), D.ptrs(hs))
    h = [a.get() for a in hs]
    # STACK MARGIN (max metric only).  cstack_fwd_kernel and the backward-data half of cstack_bwd_kernel keep a whole output
    # in ONE fp32 accumulator over the 3 C terms of the contraction (tap-major, channel-minor, v_mfma_f32_32x32x2_f32: one
    # rounding per term, the arithmetic seq_error states): rms relative error seq_error(3 C), 3.4e-7 at C = 64, where NumPy's
    # float32 matmul of a (C, C) by (C, T <= 128) block -- SIMD partial sums -- stays at 5e-8 .. 1.1e-7.  The tensor's peak error
    # stands to that rms as its largest value stands to its rms, so the model is added to the max bar as it is.  The L2 bar
    # stays plain.
    seq = (0.0, R.seq_error(3 * Cc))
    for l in range(nl):                                       # every layer from the h_{l-1} it was handed
        prev = inp['x'] if l == 0 else h[l - 1]
        judge('vqvae_convstack_fwd', 'h[%d]' % l, h[l], R.convstack_layer(prev, inp['W'][l], inp['b'][l], dils[l]),
              R.convstack_layer(prev, inp['W'][l], inp['b'][l], dils[l], np.float32), seq)
    ws_bytes = D.lib.vqvae_convstack_workspace_bytes(nl, B, Cc)
    ws = D.ws(ws_bytes)
    gx, gWs, gbs = D.out((B, Cc, T)), [D.out((Cc, Cc, 3)) for _ in dils], [D.out((Cc,)) for _ in dils]
    D.call('vqvae_convstack_bwd', nl, B, Cc, T, cd, x.ptr, D.ptrs(Ws), D.ptrs(hs), gy.ptr, gx.ptr, D.ptrs(gWs), D.ptrs(gbs), 0, ws.ptr, ws_bytes)
    b64, b32 = (R.convstack_bwd(inp['x'], inp['W'], h, dils, inp['gy'], dt) for dt in (np.float64, np.float32))
    judge('vqvae_convstack_bwd', 'gx', gx.get(), b64[0], b32[0], seq)
    for l in range(nl):
        judge('vqvae_convstack_bwd', 'gW[%d]' % l, gWs[l].get(), b64[1][l], b32[1][l])
        judge('vqvae_convstack_bwd', 'gb[%d]' % l, gbs[l].get(), b64[2][l], b32[2][l])
    judge.finish()


@pytest.mark.parametrize('row', R.S2_ROWS, ids=lambda r: 'B%d_T%d_mask%d' % r)
def test_conv_s2_bwd_call_accuracy(gpu, row):
    D = Dev(gpu)
    B, Tin, mask = row
    Cc = 64
    inp = R.s2_inputs(row)
    Tout = inp['Tout']
    assert D.lib.vqvae_conv_s2_bwd_supported(Cc, Cc, 4, 2, 1, 1, Tin, Tout) == 1
    ws_bytes = D.lib.vqvae_conv_s2_bwd_workspace_bytes(B, Cc, Tin)
    ws = D.ws(ws_bytes)
    x, W, gy = D.up(inp['x']), D.up(inp['W']), D.up(inp['gy'])
    gx, gW, gb = D.out((B, Cc, Tin)), D.out((Cc, Cc, 4)), D.out((Cc,))
    D.call('vqvae_conv_s2_bwd', B, Cc, Tin, Tout, x.ptr, W.ptr, gy.ptr, mask, gx.ptr, gW.ptr, gb.ptr, 0, ws.ptr, ws_bytes)
    b64, b32 = (R.conv_s2_bwd(inp['x'], inp['W'], inp['gy'], mask, dt) for dt in (np.float64, np.float32))
    judge = Judge('s2_B%d_T%d_mask%d' % row, '-')
    for q, got, w64, w32 in zip(('gx', 'gW', 'gb'), (gx, gW, gb), b64, b32):
        judge('vqvae_conv_s2_bwd', q, got.get(), w64, w32)
    judge.finish()


# ---------------------------------------------------------------------------------------------------------------------------
# the one-hot embed conv: gather / bincount forms (one-hot input) and the dense conv (any other input)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', R.ONEHOT_KINDS)
@pytest.mark.parametrize('row', R.ONEHOT_ROWS, ids=lambda r: 'B%d_Co%d_q%d_K%d_T%d' % r)
def test_embed_onehot_call_accuracy(gpu, matmul_mode, row, kind):
    D = Dev(gpu)
    B, Cout, q, K, T = row
    inp = R.onehot_inputs(row, kind)
    ws_bytes = D.lib.vqvae_embed_onehot_workspace_bytes(B, Cout, q, K, T)
    ws = D.ws(ws_bytes)
    x, W, b, gy = D.up(inp['x']), D.up(inp['W']), D.up(inp['b']), D.up(inp['gy'])
    y, idx, flag = D.out((B, Cout, T)), D.out((B, T), np.int32), D.out((1,), np.int32)
    D.call('vqvae_embed_onehot_fwd', x.ptr, W.ptr, b.ptr, B, Cout, q, K, T, y.ptr, idx.ptr, flag.ptr, ws.ptr, ws_bytes)
    assert int(flag.get()[0]) == int(kind != 'dense')
    if kind != 'dense':
        np.testing.assert_array_equal(idx.get(), inp['idx'])
    judge = Judge('onehot_B%d_Co%d_q%d_K%d_T%d_%s' % (row + (kind,)), matmul_mode)
    judge('vqvae_embed_onehot_fwd', 'y', y.get(), R.embed_fwd(inp['x'], inp['W'], inp['b']), R.embed_fwd(inp['x'], inp['W'], inp['b'], np.float32))
    gW, gb = D.out((Cout, q, K)), D.out((Cout,))
    D.call('vqvae_embed_onehot_wgrad', x.ptr, idx.ptr, flag.ptr, gy.ptr, B, Cout, q, K, T, gW.ptr, gb.ptr, 0, ws.ptr, ws_bytes)
    g64, g32 = (R.embed_wgrad(inp['x'], inp['gy'], K, dt) for dt in (np.float64, np.float32))
    judge('vqvae_embed_onehot_wgrad', 'gW', gW.get(), g64[0], g32[0])
    judge('vqvae_embed_onehot_wgrad', 'gb', gb.get(), g64[1], g32[1])
    judge.finish()


# ---------------------------------------------------------------------------------------------------------------------------
# the losses
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', R.XENT_ROWS, ids=lambda r: 'q%d_B%d_T%d' % r)
def test_softmax_xent_call_accuracy(gpu, row):
    D = Dev(gpu)
    q, B, T = row
    N = B * T
    inp = R.xent_inputs(row)
    ws_bytes = D.lib.vqvae_softmax_xent_workspace_bytes(B, q, T)
    ws = D.ws(ws_bytes)
    y, t = D.up(inp['y']), D.up(inp['t'])
    lse, loss = D.out((B, T)), D.out((1,))
    D.call('vqvae_softmax_xent_fwd', y.ptr, t.ptr, B, q, T, lse.ptr, loss.ptr, ws.ptr, ws_bytes)
    r64, r32 = R.xent(inp['y'], inp['t'], R.XENT_GLOSS), R.xent(inp['y'], inp['t'], R.XENT_GLOSS, dtype=np.float32)
    judge = Judge('xent_q%d_B%d_T%d' % row, '-')
    judge('vqvae_softmax_xent_fwd', 'lse', lse.get(), r64['lse'], r32['lse'])
    # the loss: the mean of the N terms lse - y[t], the two-stage sum of xent_fwd_kernel (64 term-carrying lanes per workgroup)
    # + sum_stage2, over terms that carry lse's own error: what lse's bar allows for every term (the max metric, times its
    # scale) and the rounding of the subtraction
    terms = r64['lse'] - np.take_along_axis(inp['y'].astype(np.float64), inp['t'][:, None, :].astype(np.int64), 1)[:, 0, :]
    mass = np.abs(terms).sum() / N
    e32_lse = R.metrics(r32['lse'], r64['lse'])[1]
    allowed = R.scalar_model(N, lanes=64) * mass + R.bar(e32_lse) * np.abs(r64['lse']).max() + 2.0 ** -24 * mass
    judge.scalar('vqvae_softmax_xent_fwd', 'loss', loss.get()[0], r64['loss'], allowed)
    # the gradient from the lse the backward is handed: the device's own
    lse_dev = lse.get()
    gl, gyd = D.up(np.array([R.XENT_GLOSS], np.float32)), D.out((B, q, T))
    D.call('vqvae_softmax_xent_bwd', y.ptr, t.ptr, lse.ptr, gl.ptr, B, q, T, gyd.ptr)
    g64 = R.xent(inp['y'], inp['t'], R.XENT_GLOSS, lse_in=lse_dev)['gy']
    g32 = R.xent(inp['y'], inp['t'], R.XENT_GLOSS, lse_in=lse_dev, dtype=np.float32)['gy']
    judge('vqvae_softmax_xent_bwd', 'gy', gyd.get(), g64, g32)
    judge.finish()


@pytest.mark.parametrize('row', R.MOL_ROWS, ids=lambda r: 'nm%d_B%d_T%d' % r)
def test_mol_nll_call_accuracy(gpu, row):
    D = Dev(gpu)
    nm, B, T = row
    N = B * T
    inp = R.mol_inputs(row)
    y, t = D.up(inp['y']), D.up(inp['t'])
    ws, loss = D.ws(4096 * 4), D.out((1,))
    D.call('vqvae_mol_nll_fwd', y.ptr, t.ptr, B, nm, T, 256, -40.0, loss.ptr, ws.ptr, 4096 * 4)
    judge = Judge('mol_nm%d_B%d_T%d' % row, '-')
    # the loss: the mean of N per-position terms through mol_kernel<0>'s grid-stride chains + sum_stage2, over terms with the
    # error of the ill-conditioned per-position evaluation: what the bar allows the float32 reference's own per-position error
    t64, t32 = R.mol_terms(inp['y'], inp['t']), R.mol_terms(inp['y'], inp['t'], np.float32)
    mass = np.abs(t64).sum() / N
    allowed = R.scalar_model(N) * mass + R.bar(R.metrics(t32, t64)[1]) * np.abs(t64).max()
    judge.scalar('vqvae_mol_nll_fwd', 'loss', loss.get()[0], t64.mean(), allowed)
    gl, gyd = D.up(np.array([1.0], np.float32)), D.out((B, 3 * nm, T))
    D.call('vqvae_mol_nll_bwd', y.ptr, t.ptr, gl.ptr, B, nm, T, 256, -40.0, gyd.ptr)
    got = gyd.get()
    g64, g32 = R.mol(inp['y'], inp['t'])['gy'], R.mol(inp['y'], inp['t'], dtype=np.float32)['gy']
    for i, part in enumerate(('logits', 'means', 'log-scales')):
        s = slice(i * nm, (i + 1) * nm)
        judge('vqvae_mol_nll_bwd', 'gy ' + part, got[:, s], g64[:, s], g32[:, s], l2_only=True)
    judge.finish()


@pytest.mark.parametrize('n', R.SCALAR_N)
def test_scalar_reduce_call_accuracy(gpu, n):
    D = Dev(gpu)
    inp = R.scalar_inputs(n)
    ws, out = D.ws(4096 * 4), D.out((1,))
    judge = Judge('scalar_n%d' % n, '-')
    x64 = inp['x'].astype(np.float64)
    x, a, b = D.up(inp['x']), D.up(inp['a']), D.up(inp['b'])
    D.call('vqvae_sum', x.ptr, n, 0.5, out.ptr, ws.ptr, 4096 * 4)
    judge.scalar('vqvae_sum', 'sum', out.get()[0], 0.5 * x64.sum(), R.scalar_model(n) * 0.5 * np.abs(x64).sum())
    # mean((a - b)^2): the terms carry two roundings of their own (the subtraction, the square): 2 x 2^-24 of each term
    d64 = (inp['a'].astype(np.float64) - inp['b'].astype(np.float64)) ** 2
    D.call('vqvae_sqdiff_mean', a.ptr, b.ptr, n, out.ptr, ws.ptr, 4096 * 4)
    judge.scalar('vqvae_sqdiff_mean', 'mean', out.get()[0], d64.mean(), (R.scalar_model(n) + 3 * 2.0 ** -24) * d64.mean())
    judge.finish()


# ---------------------------------------------------------------------------------------------------------------------------
# small related quantities on the same bar
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', UPS_BWD_CASES, ids=lambda c: 'B%d_C%d_%dto%d_pad%d_%d_shift%d' % c)
def test_upsample_bwd_call_accuracy(gpu, case):
    """Every road of vqvae_upsample_linear_bwd accumulates in float64 and rounds once: it should sit under e32."""
    D = Dev(gpu)
    B, Cc, Tin, Tout, gpad, xpad, shift = case
    rs = R._rs('upsb', case)
    tab = _tables(Tin, Tout)
    gyb, gxb = Cc * Tout + gpad, Cc * Tin + xpad
    assert shift % 4 == 0
    host = R._f32(rs.standard_normal(B * gyb + shift // 4))      # the padding holds finite junk the kernel must not sum
    gy = host[shift // 4:].reshape(B, gyb)[:, :Cc * Tout].reshape(B, Cc, Tout)
    gyd, gx = D.up(host), D.out((B, gxb))
    tb = dict((k, D.up(tab[k])) for k in ('w0', 'w1', 'lo0', 'hi0', 'lo1', 'hi1'))
    D.call('vqvae_upsample_linear_bwd', gyd.ptr + shift, gyb, B, Cc, Tin, Tout, tb['w0'].ptr, tb['w1'].ptr, tb['lo0'].ptr, tb['hi0'].ptr,
           tb['lo1'].ptr, tb['hi1'].ptr, gx.ptr, gxb)
    got = gx.get()[:, :Cc * Tin].reshape(B, Cc, Tin)
    judge = Judge('ups_B%d_C%d_%dto%d_pad%d_%d_shift%d' % case, '-')
    judge('vqvae_upsample_linear_bwd', 'gx', got, R.upsample_bwd(gy, tab, Tin), R.upsample_bwd(gy, tab, Tin, np.float32))
    judge.finish()


@pytest.mark.parametrize('B,Cc,Tout,G', [(1, 1, 5, 1), (3, 5, 961, 7), (2, 24, 7680, 10)])
def test_embed_broadcast_bwd_call_accuracy(gpu, B, Cc, Tout, G):
    """The speaker slice of the (B, C + G, Tout) condition gradient, as test_upsample_fwd_and_embed_broadcast_contract hands it."""
    D = Dev(gpu)
    rs = R._rs('bcast', B, Cc, Tout, G)
    n_id = 6
    ids = rs.randint(0, n_id, B).astype(np.int32)
    gy = R._f32(rs.standard_normal((B, Cc + G, Tout)))
    add = R._f32(rs.standard_normal((n_id, G)))
    gyd, idd, ws = D.up(gy), D.up(ids), D.ws(B * G * 4)
    judge = Judge('bcast_B%d_C%d_T%d_G%d' % (B, Cc, Tout, G), '-')
    for acc in (0, 1):
        gE = D.up(add) if acc else D.out((n_id, G))
        D.call('vqvae_embed_broadcast_bwd', gyd.ptr + 4 * Cc * Tout, (Cc + G) * Tout, idd.ptr, B, G, Tout, n_id, gE.ptr, acc, ws.ptr, B * G * 4)
        a = add if acc else None
        judge('vqvae_embed_broadcast_bwd', 'gE' + ('+addend' if acc else ''), gE.get(), R.embed_broadcast_bwd(gy[:, Cc:], ids, n_id, a),
              R.embed_broadcast_bwd(gy[:, Cc:], ids, n_id, a, np.float32))
    judge.finish()
