"""Every arithmetic form of a generation step held to fp32 accuracy: err <= 3 e32 + 1e-7 (chain_accuracy_ref.bar) against
the float64 evaluation of tests/gen_accuracy_ref.py, in relative L2 and in max-over-scale, where e32 is the error of NumPy's
own float32 evaluation of the same function over the same values.  The neighbouring generation tests (test_gpu_generate*.py,
test_gpu_sampling.py) assert 1e-4 absolute on logits of scale 1.5 .. 3.4, a bar at least 100 times wider.

(a) test_one_step_from_a_handed_state: vqvae_wavenet_gen_step through ctypes, ONE call from a caller-made state (rings
    N(0, 1), one-hot or scalar inputs, step = 5 so that the blocks meet different ring slots), every state buffer sized for
    exactly n between NaN red zones and NaN-filled where the call must write it.  n <= 4 runs gen_conv_kernel / gen_dense_kernel
    (matrix-vector), n >= 5 ls_gemm_body (lockstep); the test asserts which.  Judged: every block's pushed input (the ring
    slot it wrote), the last residual output, the last z, skip_acc, s1, logits.  Exact: step + 1, the other ring slots, the
    embed-queue shift, the copy of the last block's input, the zones (nothing for a sequence >= n).
(b) test_persistent_run: WaveNet.generate_sequence(persistent=True), 12 teacher-forced steps with one all-zero input, the
    four instantiations of gen_mega_kernel<MegaNarrow> and the wide class; the test asserts the persistent road, a non-zero
    workspace, the restated width class and status word 0.  Judged: logits_out as a whole and every step on its own (the
    worst one is printed).  test_persistent_chunk_seam: two launches give the bits of one.

One line per row and quantity (pytest -s):  GEN_ACC <row> <form> <quantity> l2 err e32 ratio max err e32 ratio

MARGINS.  None: every quantity of every row meets the plain bar in both metrics, so no error model was needed.

MEASURED, one run on an MI355X (143 lines; a second run printed the same lines): the worst err / e32 per form and quantity
over its rows, relative L2 then max-over-scale, and the same as a fraction of the bar 3 e32 + 1e-7:

    form                    quantity             err / e32      err / bar
    matrix-vector  n 1..4   push[l]              1.22  1.67     0.29  0.42
                            h_final              1.04  1.20     0.26  0.31
                            z                    1.05  1.24     0.27  0.34
                            skip_acc             1.13  1.36     0.30  0.35
                            s1                   1.11  1.01     0.31  0.27
                            logits               1.14  1.36     0.32  0.38
    lockstep  n 5..128      push[l]              1.28  1.49     0.36  0.43
                            h_final              1.27  1.41     0.37  0.40
                            z                    1.41  1.73     0.41  0.52
                            skip_acc             1.30  1.39     0.38  0.41
                            s1                   1.32  1.38     0.37  0.38
                            logits               1.29  1.21     0.36  0.34
    persistent <= 256       logits, run          1.20  2.37     0.33  0.67
                            logits, worst step   2.12  3.72     0.57  0.97
    persistent <= 512       logits, run          0.86  0.82     0.25  0.24
                            logits, worst step   1.06  1.05     0.30  0.30

push[0], the embed of a one-hot input, is 1.00 everywhere (one product per tap).  The persistent kernel's reordering and its
hardware exp / rcp cost nothing measurable in L2: the device's runs sit at 0.22 .. 0.33 of the bar, the NumPy runs of the same
order with NumPy's exp (tests/test_host_gen_accuracy.py) at 0.22 .. 0.35 on the same rows.  The one figure near the bar is step 10 of pn_mol (60 numbers: max error 4.34e-7 against
3 x 1.16e-7 + 1e-7, that step's e32 being the lowest of its run, 1.83e-7 over the run); it is no defect and no kernel was changed.

SHOWN ABLE TO FAIL.  Value-only mutations (a rounding; no address, bound, barrier, tag or launch geometry, nothing of the spin
protocol) in a scratch copy of csrc/, built into scratch libraries and run once against this file and once against the old 1e-4
tests of the same forms (test_gpu_generate.py, _wide.py, _lockstep.py, _refill.py and
test_gpu_sampling.py::test_generate_sequence_teacher_forced_with_controls: 58 tests); never committed.
  Library A, to half precision:  (1) gen_dense_kernel: lane 5's partial before the butterfly sum; (2) ls_gemm_body: wave 3's
      partial tile of the gate product before the LDS sum; (3) gen_mega_pack_kernel: cb.  This file: 21 of 22 fail (the chunk seam,
      a bit identity, passes).  (1) every matrix-vector row, first miss in data-flow order push[1]: 70 .. 740 e32 over the quantities;
      (2) every lockstep row, from push[1] on: 310 .. 1630 e32; (3) every persistent row: 68 .. 154 e32 (<= 256), 44 .. 87 (<= 512).
      push[0] stays at 1.00 in both step forms.  Half precision is not subtle at the old tests' sample counts: 26 of the 58 notice
      (1.1e-4 .. 1.5e-3 against 1e-4); test_generate_sequence_teacher_forced[True], the narrow persistent class, passes (3).
  Library C, the same three values cut to 16 significand bits (a 32 times smaller rounding):  this file: the same 21 of 22 fail --
      matrix-vector 3.6 .. 46 e32, lockstep 19 .. 105, persistent 3.7 .. 10.7 (<= 256) and 2.6 .. 5.1 (<= 512: at most 1.49 times
      the bar, the narrowest misses).  Old tests: 56 of 58 pass; the two that notice are test_gpu_generate_wide's 1e-5 comparisons of
      the persistent kernel with the per-step kernels (1.06e-5 and 1.59e-5), none of the 1e-4 assertions against the oracle.
  Library B, (4) the persistent chain wave: lane 7's first product of the shadow term u = Wc1_{l+1} x_l to half precision.  All
      nine persistent rows fail: 15 .. 198 e32 (<= 256), 4.2 .. 26 (<= 512).  Old tests of the persistent forms (27): 23 pass;
      test_mol_generation_matches_oracle[True] (2.3e-4) and the same 1e-5 comparisons of test_gpu_generate_wide (1.2e-5 .. 3.2e-5) notice.
Nothing escaped this file.  What it cannot see by construction: an error that NumPy's float32 evaluation shares; which of a
block's two launches is wrong when the first miss is push[l + 1] (z_l of an inner block is overwritten before the call
returns; the last z is judged); the persistent kernel's inner quantities, of which only logits_out reaches caller memory; the
samplers and the slots / latent-condition / RNG entry points, which other files tie bit for bit to these kernels.
"""
import ctypes as C

import numpy as np
import pytest

import chain_accuracy_ref as A
import gen_accuracy_ref as R
import helpers as H
from test_gpu_generate_wide import _took_persistent_road, _workspace_bytes
from zoned import ZonedArray

pytestmark = pytest.mark.gpu

_INT_MAX = 2 ** 31 - 1


class Judge(object):
    """Collects the lines of one test and asserts the bar once, with every miss in the message."""

    def __init__(self, row, form):
        self.row, self.form, self.lines, self.misses = row, form, 0, []

    def measure(self, got, want64, want32):
        err, e32 = A.metrics(got, want64), A.metrics(want32, want64)
        return err, e32, max(e / A.bar(r) for e, r in zip(err, e32))

    def __call__(self, quantity, got, want64, want32, margin=(0.0, 0.0), show=True):
        """margin: this quantity's own addition to the bar (l2, max), from an error model written where it is passed."""
        assert np.isfinite(np.asarray(got)).all(), '%s %s %s: non-finite' % (self.row, self.form, quantity)
        assert np.asarray(want32).dtype == np.float32 and np.asarray(want64).dtype == np.float64
        err, e32, _ = self.measure(got, want64, want32)
        ratio = [e / max(r, 1e-30) for e, r in zip(err, e32)]
        line = 'GEN_ACC %s %s %s l2 %.3e %.3e %.2f max %.3e %.3e %.2f' % (
            self.row, self.form, quantity, err[0], e32[0], ratio[0], err[1], e32[1], ratio[1])
        if show:
            print(line)
            self.lines += 1
        if not all(e <= A.bar(r) + m for e, r, m in zip(err, e32, margin)):
            self.misses.append(line + ('' if not any(margin) else ' (margin %.3e %.3e)' % tuple(margin)))

    def finish(self):
        assert not self.misses, '%d quantities miss their bar (err <= 3 e32 + 1e-7), %d lines printed:\n%s' % (
            len(self.misses), self.lines, '\n'.join(self.misses))


_DEC = {}


def _decoder(name):
    """The device decoder of a row next to the parameters gen_accuracy_ref made for it."""
    if name not in _DEC:
        _, _, _, cfg, _, mol, seed = R.BY_NAME[name]
        P, model = H.build_model(cfg, seed=seed, use_logistic=mol, tweak=R.bias_tweak(seed + 1))
        p = R.params(name)
        for key in ('embed', 'proj1', 'proj2'):
            for a, b in zip(P['decoder'][key], p[key]):
                np.testing.assert_array_equal(a, b)
        for ba, bb in zip(P['decoder']['blocks'], p['blocks']):
            for key in bb:
                for a, b in zip(ba[key], bb[key]):
                    np.testing.assert_array_equal(a, b)
        model.to_gpu()
        _DEC[name] = model.decoder
    return R.params(name), _DEC[name]


def _ids(cases):
    return ['%s-n%d' % c for c in cases]


# ---------------------------------------------------------------------------------------------------------------------------
# (a) one step from a handed state: the matrix-vector and the lockstep form
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.STEP_CASES, ids=_ids(R.STEP_CASES))
def test_one_step_from_a_handed_state(gpu, case):
    from vqvae_amd import _lib
    from vqvae_amd.generation import LockstepState
    name, n = case
    form = R.BY_NAME[name][2]
    assert (n <= _lib.GEN_MAX_N) == (form == 'mv') and (n > _lib.GEN_MAX_N) == (form == 'ls'), 'the row is in the suite for another form'
    p, dec = _decoder(name)
    inp = R.inputs(name, n)
    t, dils, L = inp['t'], R.dilations(name), len(p['blocks'])
    st = LockstepState(dec, n)
    assert [b.dilation for b in st._blocks] == dils and st.desc.n == n

    f32 = np.float32
    half = st.dilated // 2
    z = dict(step=ZonedArray(gpu, host=np.array([t], np.int32), name='step'),
             x_cur=ZonedArray(gpu, host=inp['x_cur'], name='x_cur'), x_prev=ZonedArray(gpu, host=inp['x_prev'], name='x_prev'),
             cond=ZonedArray(gpu, host=inp['cond'], name='cond'))
    for key, width in (('h0', st.residual), ('h1', st.residual), ('z', half), ('skip_acc', st.skip), ('s1', st.skip),
                       ('logits', st.out_dim)):
        z[key] = ZonedArray(gpu, shape=(n, width), dtype=f32, fill='poison', name=key)          # NaN where the call must write
    for l, ring in enumerate(inp['rings']):
        z['ring%d' % l] = ZonedArray(gpu, host=ring, name='ring%d' % l)

    d = st.desc
    for key in ('step', 'x_cur', 'x_prev', 'h0', 'h1', 'z', 'skip_acc', 's1', 'logits'):
        setattr(d, key, z[key].ptr)
    for l, blk in enumerate(st._blocks):
        blk.ring = z['ring%d' % l].ptr
    d.sample_mode = _lib.GEN_NONE
    d.cond, d.cond_bstride, d.cond_cstride, d.cond_follows_step = z['cond'].ptr, st.cond_dim, 1, 0
    d.uniforms, d.n_uniform, d.forced_next = None, 1, None
    d.out, d.out_bstride, d.logits_out, d.max_steps = None, 0, None, _INT_MAX
    _lib.call('vqvae_wavenet_gen_step', C.byref(d), gpu.stream())
    gpu.synchronize()

    # ---- exact ----
    problems = [str(c) for a in z.values() for c in a.corruption()]
    assert not problems, 'write outside a buffer sized for n = %d:\n%s' % (n, '\n'.join(problems))
    got = dict((k, a.get()) for k, a in z.items())
    assert int(got['step'][0]) == t + 1
    H._same(got['x_cur'], inp['x_cur'], 'x_cur (GEN_NONE feeds nothing back)')
    H._same(got['x_prev'], inp['x_cur'], 'the embed queue shift')
    H._same(got['cond'], inp['cond'], 'cond')
    for l, (ring, dil) in enumerate(zip(inp['rings'], dils)):
        keep = np.arange(dil) != t % dil
        H._same(got['ring%d' % l][keep], ring[keep], 'ring %d: the slots the step does not push to' % l)
    final, other = ('h0', 'h1') if L % 2 == 0 else ('h1', 'h0')
    H._same(got[other], got['ring%d' % (L - 1)][t % dils[-1]], 'the last block\'s input is what its ring got')

    # ---- judged ----
    state = dict(rings=inp['rings'], x_prev=inp['x_prev'])
    r64, r32 = (R.step(p, state, inp['x_cur'], inp['cond'], t, dt) for dt in (np.float64, np.float32))
    judge = Judge('%s-n%d' % case, form)
    for l in range(L):
        judge('push[%d]' % l, got['ring%d' % l][t % dils[l]], r64['push'][l], r32['push'][l])
    judge('h_final', got[final], r64['h_final'], r32['h_final'])
    for key in ('z', 'skip_acc', 's1', 'logits'):
        judge(key, got[key], r64[key], r32[key])
    judge.finish()


# ---------------------------------------------------------------------------------------------------------------------------
# (b) a whole teacher-forced run: the persistent forms
# ---------------------------------------------------------------------------------------------------------------------------
def _persistent_logits(gpu, name, n, chunk=None):
    from vqvae_amd import _lib
    _, _, form, cfg, _, mol, _ = R.BY_NAME[name]
    p, dec = _decoder(name)
    inp = R.inputs(name, n)
    cond = gpu.to_device(inp['cond'])
    if chunk is None:
        _, logits = dec.generate_sequence(cond, inp['u'], forced=inp['forced'], return_logits=True, persistent=True)
    else:
        dec.initialize(n)
        _, logits = dec._gen.run(cond, inp['u'], _lib.GEN_MOL if mol else _lib.GEN_SOFTMAX, forced=inp['forced'],
                                 return_logits=True, persistent=True, chunk=chunk)
    # which form ran: a silent fall-back to the per-step kernels would otherwise pass as the persistent kernel
    assert _took_persistent_road(dec), '%s n=%d ran on the per-step kernels' % (name, n)
    assert _workspace_bytes(dec) > 0
    assert int(dec._gen._last_ws.flat_view(0, 1).get()[0]) == 0, 'status word'
    assert R.mega_class(p, cfg['local_dim'] + cfg['global_dim'])[0] == dict(pn=4, pw=8)[form], 'the row is in the suite for the other width class'
    got = logits.get()
    assert got.shape == (inp['T'] - 1, n, cfg['out_dim']) and got.dtype == np.float32
    return got


@pytest.mark.parametrize('case', R.RUN_CASES, ids=_ids(R.RUN_CASES))
def test_persistent_run(gpu, case):
    name, n = case
    form = R.BY_NAME[name][2]
    got = _persistent_logits(gpu, name, n)
    w64, w32 = R.reference(case, np.float64), R.reference(case, np.float32)
    judge = Judge('%s-n%d' % case, form)
    judge('logits', got, w64, w32)
    worst = max(range(got.shape[0]), key=lambda t: judge.measure(got[t], w64[t], w32[t])[2])
    for t in range(got.shape[0]):
        judge('logits@t%d' % t, got[t], w64[t], w32[t], show=t == worst)
    judge.finish()


def test_persistent_chunk_seam(gpu):
    """pn_small at n = 1 in launches of 5 + 5 + 1 steps: queues, mailboxes and feedback survive the seams bit for bit."""
    H._same(_persistent_logits(gpu, 'pn_small', 1, chunk=5), _persistent_logits(gpu, 'pn_small', 1), 'chunked vs one launch')
