"""Every kernel of the decoder chain held to fp32 accuracy on its own arithmetic.

The neighbouring chain tests (test_packed_chain_contract, test_gpu_chain_domain, test_gpu_bench_shapes, test_gpu_wide_chain,
test_resblock_fwd_bwd) compare block i's output with a float64 chain run from the original inputs at 1e-4: the error they
see is the accumulated error of every kernel before it, so no kernel is judged alone and anything in the 1e-6 .. 1e-4 band
passes.  Here every entry point call of the packed chain -- driven through test_gpu_abi_contract_chain.Chain, storage bits
asserted against _expect_bits as there -- is compared with tests/chain_accuracy_ref.py's float64 evaluation of THAT call's
function over the values that call was handed (the decoded stored tensors its producer wrote, the fp32 weights, the float32
resize tables).  Two metrics per quantity, relative L2 error and max error over the tensor's scale, each for the device
(`err`) and for NumPy's float32 evaluation of the same function over the same values (`e32`):

    err <= 3 e32 + 1e-7          both metrics, every quantity, every mode          (chain_accuracy_ref.bar)

3: tests/test_host_chain_accuracy.py puts faithful split3 / split2 arithmetic within 1.1x of NumPy's float32 at these K and
one dropped product of float32x3 at 7x .. 10x.  1e-7: a 512-term bias sum comes out at 9e-8 in NumPy's pairwise sum; a
fixed-order device tree need not match that.  A result kept pre-split (res, gh in 'float32x2') is compared decoded, and the
float32 evaluation goes through the same host encoder under the call's own scale word (_presplit), so the storage rounding
is on both sides.  bf16 storage has its own e_ref bars elsewhere.

Weight gradients: Chain.dil_wgrad / res_skip_wgrad run accumulate 0 and 1; the accumulate = 0 result is judged, and where
that call had a NULL destination (the second block's gWd and the first block's gbd of a group) the accumulate = 1 result
against reference + addend, with the addend added in float32 on the e32 side.  The skip sum: accumulate 0, relu 0.  The
pull-back: vqvae_pullback_reduce over the blocks' pb_part where the gate-derivative launch is fused with it, else
vqvae_upsample_linear_bwd_f16x2 per block with a pre-split gh, vqvae_upsample_linear_bwd per other block of such a row, and
vqvae_upsample_linear_bwd_blocks over all blocks where none is pre-split; the reference is the lerp's adjoint over gh_dec.

One line per call and quantity (pytest -s):  CHAIN_ACC <row> <mode> <entry point> <quantity> l2 err e32 ratio max err e32 ratio

The unpacked block (wavenet.ResidualBlockFunction over a materialised condition: vqvae_resblock_fwd / _bwd) is held to the same
bar against oracle.resblock_fwd / _bwd in float64, e32 from the same oracle functions in float32.

MEASURED, one run on an MI355X (bit-reproducible: a second run printed the same 818 lines): the worst err / e32 per quantity
and mode over all rows and blocks, relative L2 then max-over-scale:

    quantity             float32x2    float32x3    float32
    tanh                 0.90  0.99   1.45  2.04   1.67  3.15 *
    sigmoid              1.16  1.52   1.48  2.47   1.70  1.83
    z                    1.11  1.25   1.45  2.07   1.67  2.98
    res                  0.81  0.87   0.84  1.18   1.00  1.00
    skip                 1.10  2.02   1.48  2.45   1.75  3.32
    gh                   0.91  1.13   1.18  1.60   1.22  1.58
    gx                   1.43  1.78   1.96  2.40   2.12  2.63
    gW dil               0.52  0.51   0.61  0.76   0.74  0.81
    gb dil               1.00  1.57   0.99  1.47   1.06  1.54
    gW res               0.52  0.45   0.59  0.65   0.73  0.89
    gb res               0.97  1.22   1.08  1.50   0.93  1.11
    gW skip              0.52  0.56   0.58  0.59   0.73  0.76
    gb skip              0.94  1.31   0.94  1.31   0.94  1.31
    gcond                2.24  2.98   2.22  3.32 * 2.62  3.66 *
    gP                   1.59  2.63   1.06  1.55   1.07  1.37
    unpacked res         1.01  1.06   1.01  1.06   1.20  1.41
    unpacked skip        1.01  1.06   1.01  1.06   1.20  1.18
    unpacked gx          1.15  1.57   1.15  1.57   1.32  1.31
    unpacked gcond       1.03  1.27   1.03  1.27   1.25  1.25
    unpacked gW, gb (8)  1.55  1.91   1.55  1.91   1.48  2.28

(a ratio above 3 passes where 1e-7 carries it: skip, 'float32'.)  * = outside the plain bar, all three at c512_T256 and in the max
metric only; none is a defect of one kernel, all are what ONE fp32 accumulator over a long K costs against NumPy's blocked sum
(chain_accuracy_ref.seq_error), so two quantities carry a margin of their own, derived where it is passed (GATE MARGIN, GCOND
MARGIN in test_packed_chain_accuracy): the max metric of tanh / sigmoid / z gains seq_error(2 Cr + 2) max |h| in 'float32' (the
mode whose arithmetic the model states, and the only one that missed), the max metric of gcond gains seq_error(nb Cd).  The L2
bar, which is what sees a lost product, is the plain one for every quantity in every mode.  No kernel was changed.

SHOWN ABLE TO FAIL where the 1e-4 bars could not (one value-only mutation each, in a scratch copy of csrc/, built into a scratch
library and run once against test_packed_chain_accuracy and test_packed_chain_contract of the mode named; never committed):
  float32x3 K loop:  a_m * b_m dropped from the product chain of the LEAN two-tap loop of conv_gemm_x3_kernel (mfma_chain is shared
      by every loop, so the lmma lambda got a copy of it without that MFMA).  test_packed_chain_accuracy[float32x3] fails at the five
      rows that run 256-row tiles (c384_Cs320, 128-row tiles, passes) with "12 of 38 quantities miss err <= 3 e32 + 1e-7" (14 at
      c512_T256, where res of blocks 0 and 1 fails as well, at 9 e32): tanh, sigmoid, z at 10 .. 14 e32 (relative L2 2.4e-6 .. 3.2e-6) and gx at
      8 .. 9.6 e32 of every block.  test_packed_chain_contract[float32x3]: 9 passed.
  float32x3 weight gradient:  a_l * b_h dropped from both product chains of wgrad3_kernel<.., 3> (the LEANW form and the plain one).
      test_packed_chain_accuracy[float32x3] fails at all six rows with "8 of 38 quantities miss": gWd, gWr, gWs of every block at
      7.0 .. 8.9 e32 (relative L2 2.4e-6 .. 2.5e-6; the bias sums, which take no product, pass).  test_packed_chain_contract: 9 passed.
  float32x2 residual add:  presplit_value of the add path decoding the high piece only, in lin128_stream_kernel (conv_gemm_x3.hip)
      and lin_stream_wide.hip.  test_packed_chain_accuracy[float32x2] fails at c256_T256 and c256_Cs128 -- the two rows whose block 1
      adds a pre-split x_1 (with three blocks, block 0 adds the fp32 input and block 2 has no res) -- with "res[1] l2 1.958e-04
      8.193e-08 2390.17 max 3.411e-04 1.492e-07 2286.51".  Half the significand is no subtle loss: the old bar sees it too,
      test_packed_chain_contract[float32x2] fails at c256_T256, c512_T384, c256_Cs128, c256_Cs512 with "res of block 1: max err
      8.154e-04 ... tol 0.0001".
"""
import numpy as np
import pytest

import chain_accuracy_ref as R
import vqvae_oracle as O
from helpers import to4
from test_gpu_abi_contract import _f32, _presplit, _rs
from test_gpu_abi_contract_chain import GHX2, GSIG, K, RESX2, ROWS, Chain, _expect_bits
from test_gpu_kernels import RB_CASES, _rb_params
from zoned import In, Out, run_contract

pytestmark = pytest.mark.gpu

_BY_NAME = dict((p.values[0][0], p) for p in ROWS)


class Judge(object):
    """Collects (entry point, quantity, err, e32) of one test and asserts the bar once, with every miss in the message."""

    def __init__(self, row, mode):
        self.row, self.mode, self.lines, self.misses = row, mode, [], []

    def __call__(self, entry, quantity, got, want64, want32, margin=(0.0, 0.0)):
        """margin: this quantity's own addition to the bar (l2, max), from an error model written where it is passed."""
        err, e32 = R.metrics(got, want64), R.metrics(want32, want64)
        ratio = [e / max(r, 1e-30) for e, r in zip(err, e32)]
        line = 'CHAIN_ACC %s %s %s %s l2 %.3e %.3e %.2f max %.3e %.3e %.2f' % (
            self.row, self.mode, entry, quantity, err[0], e32[0], ratio[0], err[1], e32[1], ratio[1])
        print(line)
        self.lines.append((entry, quantity, err, e32))
        if not all(e <= R.bar(r) + m for e, r, m in zip(err, e32, margin)):
            self.misses.append(line + ('' if not any(margin) else ' (margin %.3e %.3e)' % tuple(margin)))

    def finish(self):
        assert not self.misses, '%d of %d quantities miss err <= 3 e32 + 1e-7:\n%s' % (
            len(self.misses), len(self.lines), '\n'.join(self.misses))


def _stored32(v32, scale):
    """A float32 evaluation through the host encoder / decoder of a pre-split tensor under the call's own scale word."""
    return _presplit(_f32(v32), np.asarray(scale, np.uint32)[:1].view(np.float32)[0])[2]


class AccChain(Chain):
    """Chain whose 1e-4 comparisons record instead: name -> (result, the caller's addend or None)."""

    def __init__(self, *a):
        Chain.__init__(self, *a)
        self.seen = {}

    def tol(self, got, want, name, scaled=True, addend=None):
        self.seen[name] = (np.array(got), addend)

    def grad(self, kind, l):
        """The accumulate = 0 result of `kind` of block l, or (where that destination was NULL) the accumulate = 1 one."""
        for acc in (0, 1):
            if '%s of block %d, accumulate %d' % (kind, l, acc) in self.seen:
                return self.seen['%s of block %d, accumulate %d' % (kind, l, acc)]
        raise KeyError((kind, l))

    def pull_back_unfused(self):
        """gP (B, nb Cd, Tl) by the entry points the chain takes where the gate-derivative launch does not carry the pull-back."""
        nb, B, T, Cd, Tl, tab = self.nb, self.B, self.T, self.Cd, self.Tl, self.tab
        tabs = dict((k, In(tab[k])) for k in ('w0', 'w1'))
        tabs.update((k, In(tab[k], index_range=(0, T))) for k in ('lo0', 'hi0', 'lo1', 'hi1'))
        targs = lambda b: (b.w0.ptr, b.w1.ptr, b.lo0.ptr, b.hi0.ptr, b.lo1.ptr, b.hi1.ptr)
        pre = [bool(bits & GHX2) for bits in self.bwd_bits]
        if not any(pre):
            r = run_contract(self.gpu, lambda b: self.call('vqvae_upsample_linear_bwd_blocks', b.gy.ptr, 0, B * Cd * T, Cd * T, nb, B, Cd,
                                                           Tl, T, *(targs(b) + (b.gP.ptr, Cd * Tl, nb * Cd * Tl))),
                             dict(tabs, gy=In(np.stack(self.gh)), gP=Out((B, nb * Cd, Tl))))
            return r['gP'], ['vqvae_upsample_linear_bwd_blocks'] * nb
        gP, names = np.zeros((B, nb * Cd, Tl), np.float32), []
        for l in range(nb):
            if pre[l]:
                r = run_contract(self.gpu, lambda b: self.call('vqvae_upsample_linear_bwd_f16x2', b.gy.ptr, Cd * T, B, Cd, Tl, T,
                                                               *(targs(b) + (b.gx.ptr, Cd * Tl, b.scale.ptr))),
                                 dict(tabs, gy=In(self.gh[l]), scale=In(self.gh_scale[l]), gx=Out((B, Cd, Tl))))
                names.append('vqvae_upsample_linear_bwd_f16x2')
            else:
                r = run_contract(self.gpu, lambda b: self.call('vqvae_upsample_linear_bwd', b.gy.ptr, Cd * T, B, Cd, Tl, T,
                                                               *(targs(b) + (b.gx.ptr, Cd * Tl))),
                                 dict(tabs, gy=In(self.gh[l]), gx=Out((B, Cd, Tl))))
                names.append('vqvae_upsample_linear_bwd')
            gP[:, l * Cd:(l + 1) * Cd] = r['gx']
        return gP, names


@pytest.mark.parametrize('row', [_BY_NAME[n] for n in R.ACC_ROWS])
def test_packed_chain_accuracy(gpu, matmul_mode, row):
    name, Cr, Cs, Cc, T, Tl, B, dils = row
    ch = AccChain(gpu, row, matmul_mode)
    fwd, bwd, fused = _expect_bits(row, matmul_mode)
    assert (ch.fwd_bits, ch.bwd_bits, ch.fused) == (fwd, bwd, fused), \
        '%s %s runs with storage %s / %s, fused pull-back %s; the predicates say %s / %s, %s' % (
            name, matmul_mode, ch.fwd_bits, ch.bwd_bits, ch.fused, fwd, bwd, fused)
    nb, Cd, Ch = ch.nb, ch.Cd, ch.Ch
    rs = _rs('chain_acc', row)
    none = dict(grads=[dict(conv=(None, None), res=(None, None), skip=(None, None))] * nb, gcond=None, gP=None)
    # the device run: every call's outputs, as Chain keeps them
    ch.pack()
    for i in range(nb):
        ch.block_forward(i)
    skip = ch.skip_forward(0, 0)['skip']
    for i in range(nb - 1, -1, -1):
        ch.block_backward(i)
    ch.dil_wgrad(none, rs)
    ch.res_skip_wgrad(none, rs)
    ch.gcond_bwd(none, rs)
    if ch.fused:
        ch.pullback(none)
        gP, pull = ch.seen['gP (vqvae_pullback_reduce)'][0], ['vqvae_pullback_reduce'] * nb
    else:
        gP, pull = ch.pull_back_unfused()
    # the references of every call over what it was handed
    handed = dict(blocks=ch.inp['blocks'], dils=dils, tab=ch.tab, Tl=Tl, P_all=ch.P_all, gy=ch.inp['gy'],
                  gsig=[bool(b & GSIG) for b in ch.bwd_bits], x_dec=ch.x_dec, gates=ch.gates, z_dec=ch.z_dec,
                  gh_dec=ch.gh_dec, gx_dec=ch.gx_dec)
    assert [bool(b & GSIG) for b in ch.fwd_bits] == handed['gsig']
    r64, r32 = R.chain_refs(handed, np.float64), R.chain_refs(handed, np.float32)
    judge = Judge(name, matmul_mode)
    for i in range(nb):
        k = lambda q: (R.FWD, q, i)
        # GATE MARGIN (max metric only, 'float32' only: the one mode with a measured miss).  tanh, sigmoid and z have scale 1 and slopes <= 1, 1/4 in the pre-activation h, so their
        # largest error is the largest ABSOLUTE error of h where the slope is near its maximum.  h is a K = 2 Cr (+ 2: the
        # lerp) term sum in one fp32 accumulator: rms error seq_error(K) rms(h), and its peak over the tensor stands to that
        # as max |h| stands to rms(h).  NumPy's blocked sum does not grow with K, so at Cr = 512 the fp32 MFMA path itself
        # ('float32': tanh of block 0, 5.17e-6 against 3 x 1.64e-6 + 1e-7) is outside 3 e32.  One rounding per term is that
        # path's arithmetic; the split modes round per 16-deep step, measure 2.47 e32 at worst and keep the plain bar.  The L2
        # metric, which is what sees a lost product (2.4e-6 .. 2.8e-6 against a bar of ~9e-7), keeps the plain bar in every mode.
        seq = R.seq_error(K * Cr + 2) if matmul_mode == 'float32' else 0.0
        ha, hb = np.abs(r64[k('h')][:, :Ch]).max(), np.abs(r64[k('h')][:, Ch:]).max()
        if not handed['gsig'][i]:
            judge(R.FWD, 'tanh[%d]' % i, ch.gates[i][:, :Ch], r64[k('tanh')], r32[k('tanh')], (0.0, seq * ha))
        judge(R.FWD, 'sigmoid[%d]' % i, ch.gates[i][:, Ch:], r64[k('sigmoid')], r32[k('sigmoid')], (0.0, seq * hb / 4))
        judge(R.FWD, 'z[%d]' % i, ch.z_dec[i], r64[k('z')], r32[k('z')], (0.0, seq * (ha + hb / 4)))
        if i < nb - 1:
            w32 = _stored32(r32[k('res')], ch.x_scale[i + 1]) if ch.fwd_bits[i] & RESX2 else r32[k('res')]
            judge(R.FWD, 'res[%d]' % i, ch.x_dec[i + 1], r64[k('res')], w32)
    judge(R.SKIP, 'skip', skip, r64[(R.SKIP, 'skip', None)], r32[(R.SKIP, 'skip', None)])
    for i in range(nb - 1, -1, -1):
        w32 = _stored32(r32[(R.BWD, 'gh', i)], ch.gh_scale[i]) if ch.bwd_bits[i] & GHX2 else r32[(R.BWD, 'gh', i)]
        judge(R.BWD, 'gh[%d]' % i, ch.gh_dec[i], r64[(R.BWD, 'gh', i)], w32)
        judge(R.BWD, 'gx[%d]' % i, ch.gx_dec[i], r64[(R.BWD, 'gx', i)], r32[(R.BWD, 'gx', i)])
    for entry, kinds in ((R.DILW, ('gWd', 'gbd')), (R.RESW, ('gWr', 'gbr')), (R.SKIPW, ('gWs', 'gbs'))):
        for i in range(nb - 1 if entry == R.RESW else nb):
            for kind in kinds:
                got, addend = ch.grad(kind, i)
                w64, w32 = r64[(entry, kind, i)], r32[(entry, kind, i)]
                if addend is not None:
                    w64, w32 = w64 + addend, w32 + addend
                    assert w32.dtype == np.float32
                judge(entry, '%s[%d]%s' % (kind, i, '' if addend is None else '+addend'), got, w64, w32)
    # GCOND MARGIN (max metric only).  sum_l Wc_l^T gh_l is ONE accumulator over K = nb Cd terms, 1536 at Cr = 512: the longest
    # contraction of the chain.  The device error follows sqrt(K) in every mode (4.6e-7, 5.7e-7, 6.4e-7 relative L2 at
    # K = 768, 1152, 1536; 'float32': 5.4e-7, 6.6e-7, 7.6e-7) while NumPy's blocked sum stays at 2.9e-7 .. 4.1e-7, so at 1536
    # the max metric of 'float32x3' (3.32 e32) and 'float32' (3.66 e32) is outside the plain bar.  The model of a single
    # accumulator (chain_accuracy_ref.seq_error: 9.5e-7 at K = 1536) is added to the max bar.  The L2 metric never missed
    # (2.24, 2.22, 2.62 e32) and keeps the plain bar, ~9.6e-7 at K = 1536: 2.5x inside a lost product's 2.4e-6.
    seq = R.seq_error(nb * Cd)
    judge(R.GCOND, 'gcond', ch.seen['gcond, accumulate 0'][0], r64[(R.GCOND, 'gcond', None)], r32[(R.GCOND, 'gcond', None)], (0.0, seq))
    for i in range(nb):
        judge(pull[i], 'gP[%d]' % i, gP[:, i * Cd:(i + 1) * Cd], r64[(R.PULL, 'gP', i)], r32[(R.PULL, 'gP', i)])
    judge.finish()


UNPACKED = [RB_CASES[i] for i in (0, 2, 3, 5)]
ORDER = ('conv', 'condition_proj', 'res', 'skip')


def _oracle_block(p, x, c, dil, g_res, g_skip, dtype):
    f = lambda a: a.astype(dtype)
    p = {n: (f(W), f(b)) for n, (W, b) in p.items()}
    res, skip, cache = O.resblock_fwd(p, f(x), f(c), dil)
    gx, gc, gr = O.resblock_bwd(p, cache, f(c), dil, f(g_res), f(g_skip))
    out = dict(res=res, skip=skip, gx=gx, gcond=gc)
    for n in ORDER:
        out['gW ' + n], out['gb ' + n] = gr[n]
    assert all(v.dtype == dtype for v in out.values())
    return out


@pytest.mark.parametrize('case', UNPACKED)
def test_unpacked_block_accuracy(gpu, matmul_mode, case):
    from vqvae_amd.core import Variable
    from vqvae_amd.wavenet import ResidualBlockFunction
    B, T, Cr, Cd, Cs, Cc, K, dil = case
    rs = np.random.RandomState(sum(case))
    p = _rb_params(rs, Cr, Cd, Cs, Cc, K)
    x, c = _f32(rs.standard_normal((B, Cr, T))), _f32(rs.standard_normal((B, Cc, T)))
    g_res, g_skip = _f32(rs.standard_normal((B, Cr, T))), _f32(rs.standard_normal((B, Cs, T)))
    w64, w32 = (_oracle_block(p, x, c, dil, g_res, g_skip, dt) for dt in (np.float64, np.float32))
    dev = lambda a: gpu.to_device(np.ascontiguousarray(a))
    vs = [Variable(dev(to4(x))), Variable(dev(to4(c)))]
    for n in ORDER:
        vs += [Variable(dev(to4(p[n][0]))), Variable(dev(p[n][1]))]
    res, skip = ResidualBlockFunction(dil).apply(vs)
    gouts = res.creator.backward(tuple(range(10)), (Variable(dev(to4(g_res))), Variable(dev(to4(g_skip)))))
    got = dict(res=res.data.get(), skip=skip.data.get(), gx=gouts[0].get(), gcond=gouts[1].get())
    for i, n in enumerate(ORDER):
        got['gW ' + n], got['gb ' + n] = gouts[2 + 2 * i].get(), gouts[3 + 2 * i].get()
    judge = Judge('rb_B%d_T%d_C%d_%d_%d_%d_K%d_dil%d' % case, matmul_mode)
    for q in ('res', 'skip', 'gx', 'gcond') + tuple(k + n for n in ORDER for k in ('gW ', 'gb ')):
        judge('vqvae_resblock_fwd' if q in ('res', 'skip') else 'vqvae_resblock_bwd', q.replace(' ', '_'),
              got[q].reshape(w64[q].shape), w64[q], w32[q])
    judge.finish()
