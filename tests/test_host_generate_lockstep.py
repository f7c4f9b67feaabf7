"""CPU checks of lockstep generation: the kernels of csrc/generate_lockstep.hip compile for gfx950 without scratch,
the header's limits and prototypes are the ones Python binds, and run_lockstep's grouping / sorting / un-sorting is right
on a stub in place of the device."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-vq-vae_amd'))


@pytest.fixture(scope='module')
def lockstep_meta(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    src = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'generate_lockstep.hip')
    out = str(tmp_path_factory.mktemp('gen') / 'generate_lockstep.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', src, '-o', out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = {}
    for m in re.finditer(r'\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+)'
                         r'.*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)', text, re.S):
        meta[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    return meta, text


def test_lockstep_kernels_compile_without_scratch(lockstep_meta, record_property):
    meta, text = lockstep_meta
    for name in ('gen_lockstep_gemm_kernel', 'gen_lockstep_finish_kernel', 'gen_lockstep_advance_kernel'):
        hits = [v for k, v in meta.items() if name in k]
        assert len(hits) == 1, '%s is not in the compiled module' % name
        m = hits[0]
        record_property(name, '%(vgpr)d VGPRs, %(lds)d B LDS' % m)
        assert (m['scratch'], m['spill']) == (0, 0), (name, m)
    gemm = [v for k, v in meta.items() if 'gen_lockstep_gemm_kernel' in k][0]
    # eight waves per workgroup, two workgroups per CU: at most 128 registers per lane and a quarter of the LDS
    assert gemm['vgpr'] <= 128 and gemm['lds'] <= 40 * 1024, gemm
    assert 'v_mfma_f32_16x16x4_f32' in text, 'the product is not on the matrix pipe'
    assert 'global_atomic' not in text and 'ds_add' not in text, 'the K reduction must be a fixed-order sum'


def test_header_limits_and_prototypes():
    from vqvae_amd import _lib
    assert _lib.GEN_MAX_LOCKSTEP == 128 and _lib.GEN_MAX_N == 4          # against the header: tests/test_host_abi.py
    assert _lib.ABI_VERSION == 5                                        # no struct change, no new export
    # the feature adds no export: generation still has exactly these entry points
    assert sorted(n for n in _lib.PROTOTYPES if 'wavenet_gen' in n) == [
        'vqvae_wavenet_gen_run', 'vqvae_wavenet_gen_run_concurrency', 'vqvae_wavenet_gen_run_workspace_bytes',
        'vqvae_wavenet_gen_step']


def test_plan_lockstep_groups():
    from vqvae_amd.generation import plan_lockstep
    steps, groups = plan_lockstep(300, 50)
    assert (steps == 49).all() and [len(i) for i, _ in groups] == [128, 128, 44] and all(s == 49 for _, s in groups)
    np.testing.assert_array_equal(np.concatenate([i for i, _ in groups]), np.arange(300))
    steps, groups = plan_lockstep(7, 10, lengths=[3, 10, 5, 5, 1, 2, 9], group=5)
    np.testing.assert_array_equal(steps, [2, 9, 4, 4, 0, 1, 8])
    np.testing.assert_array_equal(groups[0][0], [1, 6, 2, 3, 0])         # longest first, ties in the caller's order
    assert groups[0][1] == 9
    np.testing.assert_array_equal(groups[1][0], [5, 4, 4, 4, 4])         # filled up to 5 with its last member
    assert groups[1][1] == 1
    steps, groups = plan_lockstep(3, 10, n_steps=4)
    np.testing.assert_array_equal(groups[0][0], [0, 1, 2, 2, 2])
    assert groups[0][1] == 4
    steps, _ = plan_lockstep(3, 10, lengths=[10, 2, 6], n_steps=4)
    np.testing.assert_array_equal(steps, [4, 1, 4])
    for bad in (dict(group=4), dict(group=129), dict(n_steps=11), dict(lengths=[1, 2]), dict(lengths=[0, 1, 2]),
                dict(lengths=[1, 2, 11])):
        with pytest.raises(ValueError):
            plan_lockstep(3, 10, **bad)


class _StubNet(object):
    class proj2(object):
        class W(object):
            shape = (8, 4)


def test_run_lockstep_sorts_groups_and_restores_the_callers_order():
    """A stub group runner whose 'sample' of sequence i at step t is 1000 * i + t + 1 and which keeps running past
    a member's end, as the device does: tails are cut, rows come back where the caller put them."""
    from vqvae_amd import _lib
    from vqvae_amd.generation import run_lockstep
    N, T = 13, 20
    rs = np.random.RandomState(0)
    lengths = rs.randint(1, T + 1, N)
    lengths[4] = T
    cond = np.zeros((N, 3, T), np.float32)
    u = rs.random_sample((T, N))
    forced = rs.randint(0, 4, (T, N)).astype(np.int32)
    calls = []

    def stub(idx, ug, fg, gsteps):
        calls.append((np.array(idx), gsteps))
        assert ug.shape == (max(gsteps, 1), len(idx), 1) and fg.shape == (gsteps, len(idx))
        np.testing.assert_array_equal(ug[:gsteps, :, 0], u[:gsteps, idx])
        np.testing.assert_array_equal(fg, forced[:gsteps, idx])
        o = np.zeros((len(idx), T), np.int32)
        o[:, :gsteps] = 1000 * np.asarray(idx)[:, None] + np.arange(gsteps)[None, :] + 1
        lg = np.zeros((gsteps, len(idx), 8), np.float32)
        lg[:] = (np.asarray(idx)[None, :, None] + 1) * (np.arange(gsteps)[:, None, None] + 1)
        return o, lg

    out, logits = run_lockstep(_StubNet(), cond, u, _lib.GEN_SOFTMAX, lengths=lengths, forced=forced,
                               return_logits=True, group=5, _run_group=stub)
    assert [len(i) for i, _ in calls] == [5, 5, 5]                     # 13 = 5 + 5 + 3 (filled up to 5)
    flat = np.concatenate([i for i, _ in calls])[:N]
    assert sorted(flat) == list(range(N))
    assert all(np.diff(lengths[i][:len(set(i))]).max(initial=0) <= 0 for i, _ in calls)   # longest first inside a group
    assert [s for _, s in calls] == [int(lengths[i].max()) - 1 for i, _ in calls]
    assert calls[0][1] == T - 1 and calls[0][1] >= calls[1][1] >= calls[2][1]
    assert out.shape == (N, T) and logits.shape == (T - 1, N, 8)
    for i, L in enumerate(lengths):
        np.testing.assert_array_equal(out[i, :L - 1], 1000 * i + np.arange(L - 1) + 1)
        assert (out[i, L - 1:] == 0).all() and (logits[L - 1:, i] == 0).all()
        np.testing.assert_array_equal(logits[:L - 1, i, 0], (i + 1) * (np.arange(L - 1) + 1))
    # without lengths: consecutive slices, every sequence T - 1 steps
    del calls[:]
    out = run_lockstep(_StubNet(), cond, u, _lib.GEN_SOFTMAX, forced=forced, group=8, _run_group=stub)
    np.testing.assert_array_equal(calls[0][0], np.arange(8))
    np.testing.assert_array_equal(calls[1][0], np.arange(8, 13))
    np.testing.assert_array_equal(out[:, :T - 1], 1000 * np.arange(N)[:, None] + np.arange(T - 1)[None, :] + 1)
    assert (out[:, T - 1] == 0).all()
    with pytest.raises(ValueError):
        run_lockstep(_StubNet(), cond, u[:5], _lib.GEN_SOFTMAX, _run_group=stub)
    with pytest.raises(ValueError):
        run_lockstep(_StubNet(), cond, u[:, :5], _lib.GEN_SOFTMAX, _run_group=stub)
