"""CPU checks of lockstep generation with refill (include/vqvae_gen_slots.h, csrc/generate_slots.hip,
vqvae_amd/generation.py): the host replay of the device scheduler on hand-worked cases and against its bounds, the header
against the table Python binds, the compiled kernels' resource budget, run_lockstep_refill on a stub in place of the
device, and the argument validation of the two exports."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from vqvae_amd import _lib
from vqvae_amd.generation import plan_lockstep, plan_refill, refill_queue, refill_slots, run_lockstep_refill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the scheduler's rule on the host -------------------------------------------------------------------------------
def test_plan_refill_hand_worked():
    """steps 5 1 3 3 2 4 1 in 5 slots.  Queue (longest first, ties in the caller's order): 0 5 2 3 4 | 1 6.
    tick 0: slots 0..4 hold 0 5 2 3 4.  Sequence 4 (2 steps) ends with tick 1: slot 4 takes 1 at tick 2.  With tick 2
    end 2 and 3 (3 steps, slots 2 and 3) and 1 (1 step, slot 4): the free slots in slot order are 2 3 4 and one sequence
    waits, so slot 2 takes 6 at tick 3 and slots 3 and 4 go idle.  Tick 3 is the last of 5 (4 steps) and of 6 (1 step),
    tick 4 the last of 0: 5 ticks."""
    ticks, where = plan_refill([5, 1, 3, 3, 2, 4, 1], 5)
    assert ticks == 5
    assert where.tolist() == [[0, 0], [4, 2], [2, 0], [3, 0], [4, 0], [1, 0], [2, 3]]
    assert refill_queue([5, 1, 3, 3, 2, 4, 1]).tolist() == [0, 5, 2, 3, 4, 1, 6]


def test_plan_refill_leaves_zero_step_sequences_out_and_slots_idle():
    ticks, where = plan_refill([0, 3, 0, 1, 0], 5)                       # lengths 1 4 1 2 1
    assert refill_queue([0, 3, 0, 1, 0]).tolist() == [1, 3]
    assert ticks == 3 and where.tolist() == [[-1, -1], [0, 0], [-1, -1], [1, 0], [-1, -1]]
    ticks, where = plan_refill([2, 7, 4], 5)                             # fewer sequences than slots: slots 3 and 4 idle
    assert ticks == 7 and where.tolist() == [[2, 0], [0, 0], [1, 0]]
    assert plan_refill([0, 0], 5)[0] == 0 and plan_refill([], 5)[0] == 0
    assert refill_slots(3) == 5 and refill_slots(300) == 128 and refill_slots(300, 21) == 21 and refill_slots(9, 21) == 9
    for bad in (4, 129):
        with pytest.raises(ValueError):
            refill_slots(10, bad)
    with pytest.raises(ValueError):
        plan_refill([3, -1], 5)


def test_plan_refill_between_the_lower_bound_and_sorted_groups():
    rs = np.random.RandomState(7)
    gain = []
    for case in range(20):
        N = int(rs.randint(1, 400))
        S = int(rs.choice([5, 16, 37, 128]))
        T = 400
        lengths = np.clip(rs.gamma(2.0, 60.0, N), 1, T).astype(np.int64)
        steps, groups = plan_lockstep(N, T, lengths, group=S)
        ticks, where = plan_refill(steps, refill_slots((steps > 0).sum(), S))
        assert ticks >= max(int(steps.max()), -(-int(steps.sum()) // S)), case
        assert ticks <= sum(g for _, g in groups), case
        gain.append(sum(g for _, g in groups) / max(ticks, 1))
        # every queued sequence has a place, no two share a slot at a tick, and all end by `ticks`
        run = where[:, 0] >= 0
        assert (run == (steps > 0)).all()
        busy = np.zeros((S, max(ticks, 1)), np.int32)
        for i in np.flatnonzero(run):
            busy[where[i, 0], where[i, 1]:where[i, 1] + steps[i]] += 1
            assert where[i, 1] + steps[i] <= ticks
        assert busy.max(initial=0) <= 1
    assert max(gain) > 1.2                                               # the point of the feature shows in the plan


# ---- the header, the table, the library -----------------------------------------------------------------------------
def test_header_exports_are_the_bound_table_and_versions_stand():
    """The header, the library, the versions and vqvae_gen_slots' layout: tests/test_host_abi.py, for every header."""
    assert set(_lib.HEADERS['vqvae_gen_slots.h'].prototypes) == {'vqvae_gen_slots_abi_version', 'vqvae_gen_slots_init',
                                                                 'vqvae_wavenet_gen_step_slots'}
    assert 'generate_slots.hip' in open(os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'Makefile')).read()


def test_c_side_validation_needs_no_device():
    lib = _lib.load()
    fake = 0x10000                                                      # never dereferenced: every call below is rejected first

    def table(**kw):
        t = _lib.GenSlots()
        t.n_seq, t.n_queue = 8, 8
        for name in ('steps', 'queue', 'next', 'slot_seq', 'slot_t', 'live'):
            setattr(t, name, fake)
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    d = _lib.GenDesc()
    d.n, d.step = 5, fake
    step = lib.vqvae_wavenet_gen_step_slots
    init = lib.vqvae_gen_slots_init

    def rejected(fn, what, *args):
        assert fn(*args) == -1, what
        assert what.encode() in lib.vqvae_last_error_string(), (what, lib.vqvae_last_error_string())

    for fn, who, tail in ((init, 'gen_slots_init', (None,)), (step, 'gen_step_slots', (None, None))):
        rejected(fn, who, None, C.byref(table()), *tail)
        rejected(fn, who, C.byref(d), None, *tail)
        for n in (0, 4, 129):
            d.n = n
            rejected(fn, '5..128', C.byref(d), C.byref(table()), *tail)
        d.n = 5
        for member in ('steps', 'queue', 'next', 'slot_seq', 'slot_t', 'live'):
            rejected(fn, 'null slot table member', C.byref(d), C.byref(table(**{member: None})), *tail)
        rejected(fn, 'n_queue', C.byref(d), C.byref(table(n_queue=9)), *tail)
        rejected(fn, 'n_queue', C.byref(d), C.byref(table(n_queue=-1)), *tail)
        d.step = None
        rejected(fn, 'null tick', C.byref(d), C.byref(table()), *tail)
        d.step = fake
    # a table that is one, a descriptor that is not: vqvae_wavenet_gen_step's own checks
    rejected(step, 'gen_step: no residual blocks', C.byref(d), C.byref(table()), None, None)
    # ... and one that passes them but asks for nothing, or for controls the sampler does not take
    blocks = (_lib.GenBlock * 1)()
    d.n_blocks, d.blocks = 1, blocks
    d.input_dim, d.residual, d.dilated, d.skip, d.out_dim, d.cond_dim = 4, 16, 16, 16, 30, 0
    for name in ('embed_W', 'embed_b', 'proj1_W', 'proj1_b', 'proj2_W', 'proj2_b', 'x_cur', 'x_prev', 'h0', 'h1', 'z',
                 'skip_acc', 's1', 'logits'):
        setattr(d, name, fake)
    d.sample_mode = _lib.GEN_NONE
    rejected(step, 'needs logits_out', C.byref(d), C.byref(table()), None, None)
    d.logits_out = fake
    rejected(step, 'sampling controls need', C.byref(d), C.byref(table()), C.byref(_lib.GenSampling(fake, None, None)), None)
    d.sample_mode, d.uniforms, d.n_uniform = _lib.GEN_MOL, fake, 10
    rejected(step, 'top_k', C.byref(d), C.byref(table()), C.byref(_lib.GenSampling(None, fake, None)), None)
    rejected(step, 'block 0 incomplete', C.byref(d), C.byref(table()), None, None)      # before the first launch
    d.sample_mode, d.out_dim = _lib.GEN_SOFTMAX, 1025
    rejected(step, 'at most 1024 classes', C.byref(d), C.byref(table()), None, None)


# ---- run_lockstep_refill around a stub ------------------------------------------------------------------------------
class _StubNet(object):
    class proj2(object):
        class W(object):
            shape = (8, 4)


def test_run_lockstep_refill_keeps_the_callers_order_and_cuts_tails():
    """A stub in place of the device whose 'sample' of sequence i at step t is 1000 * i + t + 1, which writes past a
    sequence's end (the device does not): rows come back where the caller put them, tails and zero-step rows are 0."""
    N, T = 13, 20
    rs = np.random.RandomState(0)
    lengths = rs.randint(1, T + 1, N)
    lengths[4], lengths[7] = T, 1
    cond = np.zeros((N, 3, T), np.float32)
    u = rs.random_sample((T, N))
    forced = rs.randint(0, 4, (T, N)).astype(np.int32)
    seen = []

    def stub(steps, ug, fg, sampling):
        seen.append(sampling)
        np.testing.assert_array_equal(steps, lengths - 1)
        assert ug.shape == (T - 1, N, 1) and fg.shape[1] == N
        np.testing.assert_array_equal(ug[:, :, 0], u[:T - 1])
        np.testing.assert_array_equal(fg[:T - 1], forced[:T - 1])
        o = (1000 * np.arange(N)[:, None] + np.arange(T)[None, :] + 1).astype(np.int32)
        lg = np.zeros((T - 1, N, 8), np.float32)
        lg[:] = (np.arange(N)[None, :, None] + 1) * (np.arange(T - 1)[:, None, None] + 1)
        return o, lg

    out, logits = run_lockstep_refill(_StubNet(), cond, u, _lib.GEN_SOFTMAX, lengths=lengths, forced=forced,
                                      return_logits=True, group=5, _run=stub)
    assert out.shape == (N, T) and out.dtype == np.int32 and logits.shape == (T - 1, N, 8)
    for i, L in enumerate(lengths):
        np.testing.assert_array_equal(out[i, :L - 1], 1000 * i + np.arange(L - 1) + 1)
        assert (out[i, L - 1:] == 0).all() and (logits[L - 1:, i] == 0).all()
        np.testing.assert_array_equal(logits[:L - 1, i, 0], (i + 1) * (np.arange(L - 1) + 1))
    controls = (np.arange(N, dtype=np.float32), None, None)

    def capped(steps, ug, fg, sampling):                                 # n_steps caps every sequence; no lengths: all run
        seen.append(sampling)
        assert (steps == 3).all() and ug.shape == (3, N, 1)
        return np.ones((N, T), np.int32), None

    out = run_lockstep_refill(_StubNet(), cond, u, _lib.GEN_SOFTMAX, n_steps=3, forced=forced, group=5, _run=capped,
                              sampling=controls)
    assert (out[:, :3] == 1).all() and not out[:, 3:].any()
    assert seen[0] is None and seen[-1] is controls                      # the controls go through whole: they are read at [seq]
    # nothing to run: the device is not asked
    out = run_lockstep_refill(_StubNet(), cond, u, _lib.GEN_SOFTMAX, lengths=np.ones(N, int), _run=None)
    assert out.shape == (N, T) and not out.any()
    for bad in (dict(uniforms=u[:5]), dict(uniforms=u[:, :5]), dict(lengths=lengths[:-1]), dict(lengths=np.full(N, T + 1)),
                dict(group=4), dict(group=129), dict(forced=forced[:3]), dict(n_steps=T + 1, lengths=None)):
        kw = dict(uniforms=u, lengths=lengths, _run=stub)
        kw.update(bad)
        with pytest.raises(ValueError):
            run_lockstep_refill(_StubNet(), cond, kw.pop('uniforms'), _lib.GEN_SOFTMAX, **kw)


def test_refill_is_an_argument_of_generate_lockstep_and_synthesize_many_is_exported():
    import inspect
    import vqvae_amd
    from vqvae_amd.wavenet import WaveNet
    sig = inspect.signature(WaveNet.generate_lockstep)
    assert sig.parameters['refill'].default is False
    assert list(sig.parameters)[:12] == ['self', 'condition', 'uniforms', 'n_steps', 'lengths', 'forced', 'return_logits',
                                         'graph_steps', 'group', 'temperature', 'top_k', 'top_p']
    sig = inspect.signature(vqvae_amd.synthesize_many)
    assert sig.parameters['refill'].default is True and sig.parameters['rng'].default is None
    dec = WaveNet(1, 2, 2, 16, 8, 8, 8, 256, False, 16, -40, 8, 0)
    with pytest.raises(ValueError, match='generate_lockstep'):           # refused before a device is needed
        dec.generate_lockstep(np.zeros((2, 8, 10), np.float32), np.zeros((10, 2)), refill=True, temperature=-1.0)


# ---- the compiled kernels -------------------------------------------------------------------------------------------
def test_slot_kernels_compile_within_the_lockstep_budget(tmp_path, record_property):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    src = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'generate_slots.hip')
    out = str(tmp_path / 'generate_slots.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', src, '-o', out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = {}
    for m in re.finditer(r'\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+)'
                         r'.*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)', text, re.S):
        meta[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    names = ('gen_slots_gemm_kernel', 'gen_slots_finish_kernel', 'gen_slots_sampled_finish_kernel', 'gen_slots_init_kernel',
             'gen_slots_schedule_kernel')
    assert len(meta) == len(names), sorted(meta)
    for name in names:
        hits = [v for k, v in meta.items() if name + 'E' in k]
        assert len(hits) == 1, '%s is not in the compiled module' % name
        record_property(name, '%(vgpr)d VGPRs, %(lds)d B LDS' % hits[0])
        assert (hits[0]['scratch'], hits[0]['spill']) == (0, 0), (name, hits[0])
        assert hits[0]['vgpr'] <= 128, (name, hits[0])
    gemm = [v for k, v in meta.items() if 'gen_slots_gemm_kernel' in k][0]
    assert gemm['lds'] <= 40 * 1024, gemm
    assert 'v_mfma_f32_16x16x4_f32' in text, 'the product is not on the matrix pipe'
    assert 'atomic' not in text and 'ds_add' not in text, 'the K reduction and the scheduler must be free of atomics'
