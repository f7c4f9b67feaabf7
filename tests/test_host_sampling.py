"""CPU checks of the sampling controls (include/vqvae_sampling.h, csrc/sampling.hip, vqvae_amd/generation.py): the NumPy
restatement tests/sampling_ref.py against the oracle and against its own stated properties, the header against the
table Python binds, argument validation on both sides of the C ABI, and the compiled kernel's resource budget."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sampling_ref as R
import vqvae_oracle as O
from vqvae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (0.1, 1.5, 3.0, 80.0)


def _logits(rs, n_cls, scale):
    return (scale * rs.standard_normal(n_cls)).astype(np.float32)


def test_neutral_controls_are_the_oracles_draw():
    rs = np.random.RandomState(0)
    for case in range(1000):
        n_cls = int(rs.choice([3, 30, 64, 65, 256, 1000]))
        l = _logits(rs, n_cls, SCALES[case % 4])
        u = rs.random_sample()
        want_p = O.softmax_axis1(l[None])[0]
        p, kept, mass = R.filtered(l)
        assert kept.all() and mass is None
        np.testing.assert_array_equal(p.view(np.uint32), want_p.view(np.uint32))
        assert R.sample(l, u) == O.choice_from_uniform(want_p, u)
        assert R.sample(l, u, 1.0, n_cls, 1.0) == R.sample(l, u, 1.0, n_cls + 7, 1.5) == R.sample(l, u)


def test_greedy_top1_and_a_tiny_nucleus_are_argmax_with_the_lowest_index_on_ties():
    rs = np.random.RandomState(1)
    for case in range(200):
        l = _logits(rs, 64, SCALES[case % 4])
        if case % 2:
            l[rs.choice(64, 5, replace=False)] = l.max()           # five-way tie at the top
        first = int(np.flatnonzero(l == l.max())[0])
        for u in (0.0, rs.random_sample(), np.nextafter(1.0, 0.0)):
            assert R.sample(l, u, temperature=0.0) == first
            assert R.sample(l, u, top_k=1) == first
            assert R.sample(l, u, top_p=1e-30) == first
        for kw in (dict(temperature=0.0), dict(top_k=1), dict(top_p=1e-30)):
            p, kept, _ = R.filtered(l, **kw)
            assert kept.sum() == 1 and kept[first] and p[first] > 0 and (np.delete(p, first) == 0).all()
            pr = R.probs(l, **kw)                                      # the nucleus is renormalised by the draw's own division
            assert pr[first] == 1.0 and pr.sum() == 1.0
    l = np.array([0.0, -0.0, -1.0], np.float32)                       # -0 ties with +0 and loses on the index
    assert R.sample(l, 0.9, temperature=0.0) == 0 and list(R.rank_order(l)) == [0, 1, 2]
    l = np.array([-0.0, 0.0, -1.0], np.float32)
    assert R.sample(l, 0.9, temperature=0.0) == 0


def test_all_equal_logits_keep_the_lowest_indices():
    l = np.full(40, 0.25, np.float32)
    p, kept, _ = R.filtered(l, top_k=5)
    assert list(np.flatnonzero(kept)) == [0, 1, 2, 3, 4]
    np.testing.assert_array_equal(p[:5], np.float32(0.2))
    assert (p[5:] == 0).all()
    p, kept, mass = R.filtered(l, top_k=5, top_p=0.5)                 # masses .2 .4 .6: the first reaching .5 is rank 2
    assert list(np.flatnonzero(kept)) == [0, 1, 2]
    # duplicated values straddling the top_k boundary: the lower indices of the tied group are the ones kept
    l = np.array([1, 3, 2, 2, 2, 2, 0], np.float32)
    _, kept, _ = R.filtered(l, top_k=3)
    assert list(np.flatnonzero(kept)) == [1, 2, 3]


@pytest.mark.parametrize('setting', [(1.0, 0, 1.0), (0.7, 0, 1.0), (1.0, 16, 1.0), (1.0, 0, 0.9), (0.8, 32, 0.95),
                                     (0.05, 0, 1.0), (0.0, 0, 1.0), (1.0, 1, 1.0), (2.0, 5, 0.3)])
def test_the_draw_stays_inside_the_kept_set(setting):
    T, k, tp = setting
    rs = np.random.RandomState(2)
    for case in range(120):
        l = _logits(rs, int(rs.choice([3, 65, 256])), SCALES[case % 4])
        p, kept, _ = R.filtered(l, T, k, tp)
        assert kept.any() and kept[R.rank_order(l)[0]]
        assert ((p > 0) <= kept).all()                                # p > 0 only inside (an underflow may leave a kept 0)
        for u in (0.0, np.nextafter(1.0, 0.0), rs.random_sample(), rs.random_sample()):
            c = R.sample(l, u, T, k, tp)
            assert kept[c] and (T == 0 or p[c] > 0), (case, u, c)
        pr = R.probs(l, T, k, tp)
        assert pr.dtype == np.float32 and ((pr > 0) == (p > 0)).all() and abs(float(pr.astype(np.float64).sum()) - 1) < 1e-5


def test_the_kept_set_grows_with_top_k_and_with_top_p():
    rs = np.random.RandomState(3)
    for case in range(40):
        l = _logits(rs, 100, SCALES[case % 4])
        l[rs.choice(100, 10)] = l[rs.choice(100, 10)]                 # some ties
        T = float(rs.choice([0.5, 1.0, 1.7]))
        prev = np.zeros(100, bool)
        for k in list(range(1, 101)) + [0]:                           # 0 = off = all
            _, kept, _ = R.filtered(l, T, top_k=k)
            assert kept.sum() == (k or 100) and (prev <= kept).all()
            prev = kept
        prev = np.zeros(100, bool)
        for tp in np.concatenate([np.linspace(1e-4, 0.9999, 57), [1.0]]):
            _, kept, _ = R.filtered(l, T, top_k=40, top_p=tp)
            assert (prev <= kept).all() and kept.sum() <= 40
            prev = kept
        assert prev.sum() == 40


def test_mol_restatement_at_temperature_one_is_the_oracle():
    rs = np.random.RandomState(4)
    out = rs.standard_normal((6, 30)).astype(np.float32)
    u = rs.uniform(0.02, 0.98, (6, 10))
    np.testing.assert_array_equal(R.mol_sample(out, u, 1.0), O.mol_sample_from_uniform(out, u))
    cold = R.mol_sample(out, u, np.full(6, 1e-3, np.float32))         # -> the mean of the heaviest component
    best = out[np.arange(6), 10 + out[:, :10].argmax(axis=1)]
    np.testing.assert_allclose(cold, np.clip(best / 127.5, -1, 1), atol=1e-4)


# ---- the header, the table, the library ---------------------------------------------------------------------------
def test_header_exports_are_the_bound_table_and_versions_stand():
    """The header, the library, the versions and vqvae_gen_sampling's layout: tests/test_host_abi.py, for every header."""
    assert set(_lib.HEADERS['vqvae_sampling.h'].prototypes) == {'vqvae_sampling_abi_version', 'vqvae_wavenet_gen_step_sampled',
                                                                'vqvae_sample_logits'}
    assert _lib.SAMPLING_MAX_CLASSES == 1024


def test_c_side_validation_needs_no_device():
    lib = _lib.load()
    fake = 0x10000                                                    # never dereferenced: every call below is rejected first
    smp_k = _lib.GenSampling(None, fake, None)
    smp_p = _lib.GenSampling(None, None, fake)
    smp_t = _lib.GenSampling(fake, None, None)

    def call(logits=fake, n=2, out_dim=256, mode=_lib.GEN_SOFTMAX, u=fake, n_uniform=1, s=None, out=fake, probs=None):
        return lib.vqvae_sample_logits(logits, n, out_dim, mode, -40.0, u, n_uniform, None if s is None else C.byref(s),
                                       out, probs, None)

    bad = [dict(logits=None), dict(u=None), dict(out=None), dict(n=0), dict(out_dim=0), dict(out_dim=1025),
           dict(mode=_lib.GEN_NONE), dict(mode=7), dict(n_uniform=0),
           dict(mode=_lib.GEN_MOL, out_dim=31, n_uniform=10), dict(mode=_lib.GEN_MOL, out_dim=30, n_uniform=9),
           dict(mode=_lib.GEN_MOL, out_dim=30, n_uniform=10, s=smp_k), dict(mode=_lib.GEN_MOL, out_dim=30, n_uniform=10, s=smp_p),
           dict(mode=_lib.GEN_MOL, out_dim=30, n_uniform=10, s=smp_t, probs=fake)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b'sample_logits' in lib.vqvae_last_error_string(), kw
    # the step: controls without a sampler, truncation with the mixture output, and (through vqvae_wavenet_gen_step's own
    # checks) a descriptor that is not one
    d = _lib.GenDesc()
    d.sample_mode = _lib.GEN_NONE
    assert lib.vqvae_wavenet_gen_step_sampled(C.byref(d), C.byref(smp_t), None) == -1
    assert b'gen_step_sampled' in lib.vqvae_last_error_string()
    d.sample_mode = _lib.GEN_MOL
    assert lib.vqvae_wavenet_gen_step_sampled(C.byref(d), C.byref(smp_k), None) == -1
    assert b'top_k' in lib.vqvae_last_error_string()
    assert lib.vqvae_wavenet_gen_step_sampled(C.byref(d), C.byref(smp_t), None) == -1      # n = 0
    assert lib.vqvae_wavenet_gen_step_sampled(None, C.byref(smp_t), None) == -1
    assert lib.vqvae_wavenet_gen_step_sampled(None, None, None) == -1                      # = vqvae_wavenet_gen_step(NULL)
    assert lib.vqvae_wavenet_gen_step_sampled(C.byref(d), C.byref(_lib.GenSampling()), None) == -1


# ---- Python argument errors ---------------------------------------------------------------------------------------
def test_sampling_controls_values():
    from vqvae_amd.generation import sampling_controls
    assert sampling_controls(3) is None
    t, k, p = sampling_controls(3, temperature=0.5)
    assert t.dtype == np.float32 and t.tolist() == [0.5] * 3 and k is None and p is None
    t, k, p = sampling_controls(3, top_k=[0, 4, 999], top_p=np.array([1.0, 0.5, 1e-6]))
    assert t is None and k.dtype == np.int32 and k.tolist() == [0, 4, 999] and p.dtype == np.float32
    t, k, p = sampling_controls(2, temperature=[0, 2], top_k=3.0, top_p=1)
    assert t.tolist() == [0, 2] and k.tolist() == [3, 3] and p.tolist() == [1, 1]
    assert sampling_controls(2, temperature=[0.5, 1.0], use_logistic=True)[0].tolist() == [0.5, 1.0]
    for bad in (dict(temperature=-0.1), dict(temperature=float('nan')), dict(temperature=float('inf')),
                dict(temperature=[1.0, 1.0]), dict(temperature=[[1.0] * 3]), dict(temperature='warm'),
                dict(top_k=-1), dict(top_k=2.5), dict(top_k=[1, 2, 3, 4]), dict(top_k=2 ** 31),
                dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.01), dict(top_p=float('nan')), dict(top_p=[0.5] * 2),
                dict(top_k=4, use_logistic=True), dict(top_p=0.9, use_logistic=True),
                dict(temperature=0.0, use_logistic=True), dict(temperature=[1.0, 0.5, 0.0], use_logistic=True)):
        with pytest.raises(ValueError):
            sampling_controls(3, **bad)


def test_wavenet_calls_refuse_bad_controls_before_they_need_a_device():
    from vqvae_amd.wavenet import WaveNet
    from vqvae_amd import synthesis
    import inspect
    cond = np.zeros((2, 8, 10), np.float32)                           # a host array: a valid call would stop at require_device
    u = np.zeros((10, 2))
    for use_logistic, out_dim in ((False, 16), (True, 30)):
        dec = WaveNet(1, 2, 2, 16, 8, 8, 8, 256, use_logistic, out_dim, -40, 8, 0)
        for call in (dec.generate_sequence, dec.generate_lockstep):
            for bad in (dict(temperature=-1.0), dict(top_k=-2), dict(top_p=0.0), dict(top_p=1.5), dict(temperature=[1.0] * 3)):
                with pytest.raises(ValueError, match=call.__name__):
                    call(cond, u, **bad)
        for kw in (dict(temperature=0.8), dict(top_k=4), dict(top_p=0.9)):
            with pytest.raises(ValueError, match='generate_lockstep'):
                dec.generate_batch(cond, u, **kw)
    for kw in (dict(top_k=4), dict(top_p=0.9), dict(temperature=0.0)):  # dec is the mixture-of-logistics decoder here
        with pytest.raises(ValueError, match='mixture of logistics'):
            dec.generate_sequence(cond, u, **kw)
        with pytest.raises(ValueError, match='mixture of logistics'):
            dec.generate_lockstep(cond, u, **kw)
    for fn in (WaveNet.generate_sequence, WaveNet.generate_lockstep, synthesis.synthesize):
        sig = inspect.signature(fn)
        assert all(sig.parameters[n].default is None for n in ('temperature', 'top_k', 'top_p')), fn


def test_run_lockstep_gathers_the_controls_with_the_groups_indices():
    """The stub group runner of tests/test_host_generate_lockstep.py with a fifth argument: every group sees its members'
    values, repeats of the last member included; without controls the runner is called as before."""
    from vqvae_amd.generation import run_lockstep, sampling_controls

    class StubNet(object):
        class proj2(object):
            class W(object):
                shape = (8, 4)

    N, T = 8, 6
    cond = np.zeros((N, 3, T), np.float32)
    u = np.random.RandomState(0).random_sample((T, N))
    sampling = sampling_controls(N, temperature=np.arange(N) / 4.0, top_k=None, top_p=np.linspace(0.2, 1.0, N))
    seen = []

    def stub(idx, ug, fg, gsteps, *rest):
        seen.append((np.array(idx), rest))
        return np.zeros((len(idx), T), np.int32), None

    run_lockstep(StubNet(), cond, u, _lib.GEN_SOFTMAX, lengths=[6, 5, 4, 3, 2, 2, 6, 1], group=5, _run_group=stub,
                 sampling=sampling)
    assert [len(i) for i, _ in seen] == [5, 5] and list(seen[1][0][2:]) == [seen[1][0][2]] * 3     # 8 = 5 + 3 (+ 2 repeats)
    for idx, rest in seen:
        (t, k, p), = rest
        assert k is None
        np.testing.assert_array_equal(t, sampling[0][idx])
        np.testing.assert_array_equal(p, sampling[2][idx])
    del seen[:]
    run_lockstep(StubNet(), cond, u, _lib.GEN_SOFTMAX, group=5, _run_group=stub)
    assert all(rest == () for _, rest in seen)


# ---- the compiled kernel ------------------------------------------------------------------------------------------
def test_sampling_kernels_compile_without_scratch(tmp_path, record_property):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    src = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'sampling.hip')
    out = str(tmp_path / 'sampling.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', src, '-o', out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = {}
    for m in re.finditer(r'\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+)'
                         r'.*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)', text, re.S):
        meta[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    for name in ('gen_sampled_finish_kernel', 'gen_sampled_advance_kernel'):
        hits = [v for k, v in meta.items() if name in k]
        assert len(hits) == 1, '%s is not in the compiled module' % name
        record_property(name, '%(vgpr)d VGPRs, %(lds)d B LDS' % hits[0])
        assert (hits[0]['scratch'], hits[0]['spill']) == (0, 0), (name, hits[0])
    finish = [v for k, v in meta.items() if 'gen_sampled_finish_kernel' in k][0]
    # 1024 keys (8 KB) + 1024 cdf entries (8 KB) + 1024 probabilities (4 KB) + 1024 keep flags (1 KB) + a few words
    assert 21 * 1024 <= finish['lds'] <= 22 * 1024 and finish['vgpr'] <= 128, finish
